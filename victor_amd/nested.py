"""Nested sampling of the data vector and of every realisation, stepped on the GPU: ``CCFFit.nested_sampling``,
``Realisations.nested_sampling`` (``paired_model=True`` included), ``JointFit.nested_sampling`` and
``JointRealisations.nested_sampling`` (``"name@q"`` parameters included).  The evidence is relative to the NORMALISED uniform prior
over the box of the cobaya ``params`` block, in any dimension up to 10, and the posterior sample depends on no start point.

**A Python loop is the definition and the device loop reproduces it** (``device=False`` / ``device=True``, as
:mod:`victor_amd.chains`).  R problems (the data vector: R = 1; or R realisations, one problem each), L live points per problem
(``n_live``), K of them replaced per iteration (``batch``; K divides L, K <= L / 2) by K walkers that take S constrained
random-walk steps each (``steps``), d <= 10 sampled parameters.

**Random numbers** are drawn on the host from three generators, in blocks of ``BLOCK`` = 8 iterations, whatever the lengths of the
calls that consume them:

* ``np.random.default_rng([seed, 0]).random((L, d))``: the start, ONE draw for every problem (two problems against the same data
  start from the same bytes and part at the first iteration);
* ``np.random.default_rng([seed, 1]).random((8, R, K))`` per block: the survivor picks;
* ``np.random.default_rng([seed, 2]).standard_normal((8, S, R, K, d))`` per block: the step increments.

**Start.**  ``x[r][i] = lo + u[i] * (hi - lo)`` (one product, one sum, then clamped to the box), evaluated in L / K launches of R K rows: row ``r K + k`` of
pass p is live point ``p K + k`` of problem r.  Every launch of a run has exactly R K rows in this order.  A NaN lnL is stored as
-inf.

**Iteration t, per problem** (``vk_nested_step.h`` states the same rules in C++):

1. ``range_j = max_i x_ij - min_i x_ij`` over the L live points.
2. The K live points smallest in (lnL, index) - ties go to the smaller index - are the dead points (t, 0 .. K - 1) in that order;
   ``L*`` is the lnL of dead point K - 1.  Their lnL, chi2 and (``keep_dead``) x enter the dead record.
3. Walker k starts at survivor ``min(floor(pick[t][r][k] * (L - K)), L - K - 1)`` of the L - K others in increasing index.
4. S steps: ``prop = y + (scale * range_j) * dz_j``, each product and the sum rounded on its own; a proposal outside the box is
   evaluated at the walker's current position and discarded (the chains' rule); accept when the proposal is inside the box and
   ``lnL' > L*`` - strict, a NaN rejects.
5. Walker k's (y, lnL, chi2) replaces dead point k in its slot.  ``n_accept`` and ``n_steps`` count per problem; a walker that
   never moved leaves a duplicate of its survivor, counted in ``n_stuck``.

**Read-out** (host, ``np.longdouble``, both routes alike; :func:`read_out`).  ``ln X`` falls by ``1 / (L - k)`` at dead point
(t, k); a dead point weighs ``w = X_prev - X``, the final live points ``X_end / L`` each; ``ln_evidence`` is the log-sum-exp of
``ln w + lnL``, ``information`` the Kullback-Leibler divergence H of the posterior from the prior, and ``ln_evidence_error =
sqrt(H / L)`` (Skilling 2006).

**Under a Gaussian prior** (``prior=``, :mod:`victor_amd.priors`) the run samples the uniform box as before - the start points are
the same bytes - and orders, kills and constrains on ``lnpost = lnL + lnprior``: ``lnprior`` is ``ResolvedPrior.lnprior`` at the
point's own sampled values and lnpost ONE rounded addition (``-inf + finite`` is ``-inf``; a NaN lnL is stored as -inf first).
Rule 2: the K live points smallest in (lnpost, index) die and ``L*`` is the lnpost of dead point K - 1; the dead record gains
``dead_lnprior`` while ``dead_lnl`` and ``dead_chi2`` keep holding lnL and chi2.  Rule 3: a walker takes its survivor's x, lnL,
chi2 and lnprior.  Rule 4: accept when the proposal is inside the box and ``lnL' + lnprior(prop) > L*`` - strict, a NaN rejects -,
lnprior taken at exactly the values the proposal arithmetic produces and rule 5 commits.  Rule 5: the walker's lnprior goes into
the slot with the rest.  The random-number protocol does not change.  In the read-out lnpost takes the place of lnL - terms,
stop, weights, moments, ``NO_FINITE`` -, the log-sum is ``ln_evidence_unnormalised = ln((1 / V) integral_box L exp(lnprior))``
and ``information`` is the divergence of the posterior from the UNIFORM BOX, which is what sets the shrinkage error.  The
prior's normalisation ``ln_prior_norm = ln((1 / V) integral_box exp(lnprior))``, the same for every problem, is the closed form
of independent priors (``prior_norm="exact"``, error 0; :func:`exact_prior_norm`) or the prior's own problem run through this
same loop on the host (``"nested"``: R = 1, lnL = 0, the call's ``n_live``, ``batch``, ``steps``, ``scale``, ``tol`` and
``max_iter``, the generators ``[seed, 3]``, ``[seed, 4]``, ``[seed, 5]`` in the roles of ``[seed, 0 .. 2]``, no theory evaluation;
:func:`nested_prior_norm`; ``extend`` does not run it again); ``"auto"`` takes the closed form where there is one.  Then
``ln_evidence = ln_evidence_unnormalised - ln_prior_norm`` and ``ln_evidence_error = sqrt(H / L + ln_prior_norm_error^2)``.
Without a prior nothing changes, not a byte: the new attributes are None and ``ln_evidence_unnormalised`` is ``ln_evidence``.

**Stop.**  Blocks of at most 8 iterations are enqueued without synchronisation; after each the dead record and the live lnL come
home.  At every multiple of 8 iterations (over the life of the run) the run ends when every problem has
``ln(Z_live / (Z_dead + Z_live)) < ln(tol)``, or at ``max_iter``; ``n_iter=`` runs a fixed count instead.  Nothing depends on how a
run is cut into blocks or :meth:`NestedSampling.extend` calls.

With epsilon fixed both routes launch the same bytes and return the same bytes.  With epsilon sampled the device forms the
Alcock-Paczynski factors with its own ``pow``: the log-likelihoods agree to rounding, and a decision ``lnL' > L*`` (or an order of
two live points) within that margin could fall the other way - ``decision_margin`` of the definition route says how close the
closest one was.
"""

import ctypes as C
import math

import numpy as np

from . import _native as N
from .fitting import _Sampled
from .utils import InputError

BLOCK = 8
MAX_ROWS = 65536
MAX_LIVE = 4096
OK, MAX_ITER, NO_FINITE = 0, 1, 2
STATUS = {OK: "OK", MAX_ITER: "MAX_ITER", NO_FINITE: "NO_FINITE"}
DEFAULT_LIVE, DEFAULT_BATCH, DEFAULT_STEPS = 256, 32, 16
_ld = np.longdouble


def _logsumexp(a, axis):
    """log sum exp of extended-precision ``a`` along ``axis``; -inf where every term is -inf (no NaN)."""
    m = a.max(axis=axis, keepdims=True)
    safe = np.where(np.isfinite(m), m, _ld(0))
    with np.errstate(divide="ignore"):
        return np.log(np.exp(a - safe).sum(axis=axis)) + np.squeeze(safe, axis=axis)


def shrinkage(n_iter, n_live, batch):
    """``ln X`` (extended precision, (n_iter * batch,)) behind every dead point in order: it falls by ``1 / (L - k)`` at (t, k)."""
    step = -1 / (_ld(n_live) - np.arange(batch).astype(_ld))
    return np.cumsum(np.tile(step, n_iter))


def log_weights(ln_x, n_live):
    """``ln w`` of the dead points (``w = X_prev - X``) and of one final live point (``X_end / L``) from their ``ln X`` (..., n)."""
    prev = np.concatenate([np.zeros(ln_x.shape[:-1] + (1,), dtype=_ld), ln_x[..., :-1]], axis=-1)
    with np.errstate(divide="ignore"):
        ln_w = prev + np.log(-np.expm1(ln_x - prev))
    end = ln_x[..., -1] if ln_x.shape[-1] else np.zeros(ln_x.shape[:-1], dtype=_ld)
    return ln_w, end - np.log(_ld(n_live))


def read_out(dead_lnl, live_lnl, n_live, batch, ln_x=None, dead_lnprior=None, live_lnprior=None):
    """The evidence of R problems from their dead record ``dead_lnl`` (T, R, K) and final live ``live_lnl`` (R, L), in extended
    precision: dict of ``ln_evidence``, ``information``, ``ln_evidence_error`` (R,), ``log_weights`` (R, T K + L: the dead points
    in order, then the live points; normalised, -inf where lnL is), ``ln_z_dead``, ``ln_z_live`` (R,) and ``no_finite`` (R,).
    ``ln_x`` (T K,) or (R, T K): the shrinkage to use instead of the expected one.

    With ``dead_lnprior`` (T, R, K) and ``live_lnprior`` (R, L) - a run under a Gaussian prior - lnpost = lnL + ln prior (one
    rounded float64 addition, the run's own) takes the place of lnL everywhere: ``ln_evidence`` is then the UNNORMALISED
    ln((1 / V) integral over the box of L exp(ln prior)), ``no_finite`` says that no lnpost was finite, and ``information`` is
    the Kullback-Leibler divergence of the posterior from the UNIFORM BOX - the prior the run samples and compresses, hence what
    sets the shrinkage error ``sqrt(H / L)`` -, not from the Gaussian prior."""
    if dead_lnprior is not None:
        dead_lnl = np.asarray(dead_lnl, dtype=float) + np.asarray(dead_lnprior, dtype=float)
        live_lnl = np.asarray(live_lnl, dtype=float) + np.asarray(live_lnprior, dtype=float)
    dead = np.asarray(dead_lnl, dtype=_ld)
    T, R, K = dead.shape
    L = int(n_live)
    dead = np.moveaxis(dead, 1, 0).reshape(R, T * K)
    live = np.asarray(live_lnl, dtype=_ld)
    if ln_x is None:
        ln_x = shrinkage(T, L, batch)
    ln_x = np.broadcast_to(np.asarray(ln_x, dtype=_ld), (R, T * K))
    ln_w, ln_w_live = log_weights(ln_x, L)
    terms = np.concatenate([ln_w + dead, ln_w_live[:, None] + live], axis=1)           # (-inf lnL: -inf, never NaN: ln w is finite)
    ln_z_dead = _logsumexp(terms[:, :T * K], 1) if T else np.full(R, -np.inf, dtype=_ld)
    ln_z_live = _logsumexp(terms[:, T * K:], 1)
    ln_z = _logsumexp(terms, 1)
    none = ~np.isfinite(ln_z)
    lnl_all = np.concatenate([dead, live], axis=1)
    with np.errstate(invalid="ignore"):
        logp = np.where(none[:, None], -np.inf, terms - np.where(none, 0, ln_z)[:, None])
        p = np.exp(logp)
        info = np.where(p > 0, p * np.where(p > 0, lnl_all, 0), 0).sum(axis=1) - np.where(none, 0, ln_z)
    info = np.where(none, 0, np.maximum(info, 0))
    return {"ln_evidence": ln_z.astype(float), "information": info.astype(float),
            "ln_evidence_error": np.sqrt(info / L).astype(float), "log_weights": logp, "ln_z_dead": ln_z_dead, "ln_z_live": ln_z_live,
            "no_finite": none}


class NestedSampling:
    """R nested-sampling runs and what they have produced so far.

    ``names``; ``n_live``, ``batch``, ``steps``, ``scale``; ``n_iter``: iterations done; ``status`` (R,): ``OK`` (0), ``MAX_ITER``
    (1: the stop was not reached; also what a fixed ``n_iter`` leaves when the criterion does not hold) or ``NO_FINITE`` (2:
    every lnL was -inf; the evidence is -inf), ``status_names``; ``ln_evidence``, ``information``, ``ln_evidence_error`` (R,);
    ``remaining`` (R,): ``ln(Z_live / (Z_dead + Z_live))``; ``dead_lnl``, ``dead_chi2`` (n_iter, R, K), ``dead_x``
    (n_iter, R, K, d; None without ``keep_dead``); ``x`` (R, L, d), ``lnl``, ``chi2`` (R, L): the final live points;
    ``n_accept``, ``n_steps``, ``n_stuck`` (R,), ``acceptance`` (R,).  With ``keep_dead``: ``samples`` (R, n, d) - the dead points in
    order, then the live points -, ``weights`` (R, n) normalised, ``mean`` (R, d), ``cov`` (R, d, d), ``sigma`` (R, d).
    Diagnostic of the definition route only (None on the device route): ``decision_margin``, the smallest ``|lnL' - L*|`` over the
    decisions taken inside the box with a finite difference and the smallest gap between two unequal neighbours among the K + 1
    lowest live lnL of an iteration (equal values are copies of one evaluation and stay equal).  :meth:`extend` continues the same runs.

    Under a prior (None otherwise): ``prior`` (the :class:`victor_amd.priors.ResolvedPrior`), ``dead_lnprior`` (n_iter, R, K),
    ``lnprior`` (R, L), ``ln_prior_norm``, ``ln_prior_norm_error`` (floats), ``prior_norm`` ("exact" or "nested");
    ``ln_evidence_unnormalised`` (R,) is the log-sum before the normalisation (without a prior: ``ln_evidence`` itself),
    ``information`` the divergence from the uniform box, and the margins, the stop and the weights are those of lnL + ln prior."""

    def __init__(self, names, lo, hi, fixed, R, n_live, batch, steps, scale, seed, tol, keep_dead, evaluator, device_handle, which,
                 prior=None, streams=(0, 1, 2)):
        self.names = list(names)
        self.fixed = fixed
        self._lo, self._hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        self.R, self.n_live, self.batch, self.steps, self.scale = int(R), int(n_live), int(batch), int(steps), float(scale)
        self.seed, self.tol, self.keep_dead = seed, float(tol), bool(keep_dead)
        self._evaluate, self._dev, self._which = evaluator, device_handle, which
        self._refresh = self._fit = None
        self.prior = prior                                   # a ResolvedPrior, or None
        self._streams = tuple(streams)                       # the generators [seed, i] of the start, the picks, the increments
        self._rng_pick, self._rng_dz = np.random.default_rng([seed, streams[1]]), np.random.default_rng([seed, streams[2]])
        self._block, self._at = None, BLOCK
        self._cut = BLOCK                                    # iterations per call of the device route (tests cut runs differently)
        self.n_iter = 0
        self._dead = ([], [], [])
        self._dead_lp = []                                   # the dead record's ln prior (under a prior)
        self._live_lnl = self._live_lp = None
        self.ln_prior_norm = self.ln_prior_norm_error = self.prior_norm = None
        self.decision_margin = None
        self._trace = None                                   # a list: the definition route appends every iteration's steps to it

    # ------------------------------------------------------------------ random numbers ------------------------------------
    def start_points(self):
        """(R, L, d): one draw of the prior for every problem."""
        u = np.random.default_rng([self.seed, self._streams[0]]).random((self.n_live, len(self.names)))
        x = self._lo + u * (self._hi - self._lo)
        x = np.minimum(np.maximum(x, self._lo), self._hi)    # (lo + u (hi - lo) may round past hi by an ulp)
        return np.ascontiguousarray(np.broadcast_to(x, (self.R,) + x.shape))

    def _draw_block(self):
        R, K, S, d = self.R, self.batch, self.steps, len(self.names)
        return self._rng_pick.random((BLOCK, R, K)), self._rng_dz.standard_normal((BLOCK, S, R, K, d))

    def _piece(self, remaining, ahead=None):
        """The next piece of the current block of random numbers (a new block when it is used up): (pick [n, R, K],
        dz [n, S, R, K, d]), n <= remaining and n <= the cut."""
        if self._at >= BLOCK:
            self._block = ahead if ahead is not None else self._draw_block()
            self._at = 0
        n = min(BLOCK - self._at, remaining, self._cut)
        t = self._at
        self._at = t + n
        return tuple(a[t:t + n] for a in self._block)

    # ------------------------------------------------------------------ the definition -----------------------------------
    def _start_host(self, x0):
        R, L, K, d = self.R, self.n_live, self.batch, len(self.names)
        self._x = x0.copy()
        self._lnl, self._chi2 = np.empty((R, L)), np.empty((R, L))
        for p in range(L // K):
            lnl, chi2 = self._evaluate(x0[:, p * K:(p + 1) * K].reshape(R * K, d), self._which)
            self._lnl[:, p * K:(p + 1) * K] = np.where(np.isnan(lnl), -np.inf, lnl).reshape(R, K)
            self._chi2[:, p * K:(p + 1) * K] = np.asarray(chi2, dtype=float).reshape(R, K)
        self._n_accept, self._n_steps, self._n_stuck = (np.zeros(R, dtype=np.int64) for _ in range(3))
        self.decision_margin = np.inf
        self._live_lnl = self._lnl
        if self.prior is not None:
            self._lnprior = self.prior.lnprior(x0)
            self._live_lp = self._lnprior

    def _iterate_host(self, pick, dz):
        """One iteration of every problem: ``pick`` (R, K), ``dz`` (S, R, K, d).  Returns the dead record (lnl, chi2, x)."""
        R, L, K, S = self.R, self.n_live, self.batch, self.steps
        lo, hi = self._lo, self._hi
        x, lnl, chi2 = self._x, self._lnl, self._chi2
        prior = self.prior
        lp = self._lnprior if prior is not None else None
        key = lnl if prior is None else lnl + lp                                  # lnpost: one rounded addition
        rows_of = np.arange(R)[:, None]
        span = x.max(axis=1) - x.min(axis=1)                                      # (R, d)
        order = np.argsort(key, axis=1, kind="stable")                           # (lnL, index): ties go to the smaller index
        dead = order[:, :K]
        lstar = key[np.arange(R), dead[:, K - 1]]
        record = (lnl[rows_of, dead].copy(), chi2[rows_of, dead].copy(), x[rows_of, dead].copy())
        if prior is not None:
            self._dead_lp.append(lp[rows_of, dead].copy()[None])
        with np.errstate(invalid="ignore"):                                        # how close the order of the dead points was
            gaps = np.diff(key[rows_of, order[:, :K + 1]], axis=1)
        gaps = gaps[np.isfinite(gaps) & (gaps > 0)]
        if gaps.size:
            self.decision_margin = min(self.decision_margin, float(gaps.min()))
        survivors = np.sort(order[:, K:], axis=1)
        q = np.minimum(np.floor(pick * float(L - K)).astype(np.int64), L - K - 1)
        src = survivors[rows_of, q]
        y, yl, yc = x[rows_of, src].copy(), lnl[rows_of, src].copy(), chi2[rows_of, src].copy()
        ylp = lp[rows_of, src].copy() if prior is not None else None
        moved = np.zeros((R, K), dtype=np.int64)
        width = (self.scale * span)[:, None, :]
        trace = None if self._trace is None else {"dead": dead.copy(), "lstar": lstar.copy(), "range": span.copy(), "from": src.copy(), "steps": []}
        for s in range(S):
            prop = y + width * dz[s]
            inside = ((prop >= lo) & (prop <= hi)).all(axis=2)
            rows = np.where(inside[:, :, None], prop, y)                          # outside: the current position, result discarded
            lnl_p, chi2_p = self._evaluate(rows.reshape(R * K, -1), self._which)
            lnl_p = np.where(inside, np.asarray(lnl_p, dtype=float).reshape(R, K), -np.inf)
            chi2_p = np.asarray(chi2_p, dtype=float).reshape(R, K)
            if prior is not None:
                lp_p = prior.lnprior(prop)                                         # at the proposal, the values an acceptance stores
            with np.errstate(invalid="ignore"):
                key_p = lnl_p if prior is None else lnl_p + lp_p
                accept = inside & (key_p > lstar[:, None])                        # NaN: False
                margin = np.abs(key_p - lstar[:, None])[inside]
            margin = margin[np.isfinite(margin)]
            if margin.size:
                self.decision_margin = min(self.decision_margin, float(margin.min()))
            y[accept], yl[accept], yc[accept] = prop[accept], lnl_p[accept], chi2_p[accept]
            if prior is not None:
                ylp[accept] = lp_p[accept]
            moved += accept
            if trace is not None:
                trace["steps"].append((accept.copy(), y.copy(), yl.copy(), yc.copy(), inside.copy()) + (() if prior is None else (ylp.copy(),)))
        x[rows_of, dead], lnl[rows_of, dead], chi2[rows_of, dead] = y, yl, yc
        if prior is not None:
            lp[rows_of, dead] = ylp
        self._n_accept += moved.sum(axis=1)
        self._n_steps += S * K
        self._n_stuck += (moved == 0).sum(axis=1)
        if trace is not None:
            trace.update(x=x.copy(), lnl=lnl.copy(), chi2=chi2.copy())
            if prior is not None:
                trace.update(lnprior=lp.copy())
            self._trace.append(trace)
        return record

    def _run_host(self, n):
        done = 0
        while done < n:
            pick, dz = self._piece(n - done)
            for t in range(len(pick)):
                rec = self._iterate_host(pick[t], dz[t])
                for store, a in zip(self._dead, rec if self.keep_dead else rec[:2]):
                    store.append(a[None])
            done += len(pick)
            self.n_iter += len(pick)

    # ------------------------------------------------------------------ the device route ---------------------------------
    def _check(self, rc, what):
        if rc != 0:
            lib, h = self._dev
            msg = (lib.vk_nested_last_error(h) or b"").decode() or f"{what} failed ({rc})"
            raise (InputError if rc == -1 else N.NativeError)(msg)

    def _run_device(self, n):
        lib, h = self._dev
        R, L, K, d = self.R, self.n_live, self.batch, len(self.names)
        done, ahead = 0, None
        while done < n:
            pick, dz = (np.ascontiguousarray(a) for a in self._piece(n - done, ahead))
            ahead = None
            m = len(pick)
            self._check(lib.vk_nested_begin(h, m, N.as_dp(pick), N.as_dp(dz), self.n_iter, 1 if self.keep_dead else 0), "vk_nested_begin")
            try:
                if self._at >= BLOCK and done + m < n:               # the next block's numbers, drawn while this one runs
                    ahead = self._draw_block()
            finally:
                dl, dc, live = np.empty((m, R, K)), np.empty((m, R, K)), np.empty((R, L))
                dx = np.empty((m, R, K, d)) if self.keep_dead else None
                self._check(lib.vk_nested_finish(h, N.as_dp(dl), N.as_dp(dc), None if dx is None else N.as_dp(dx), N.as_dp(live)),
                            "vk_nested_finish")
            for store, a in zip(self._dead, (dl, dc, dx) if self.keep_dead else (dl, dc)):
                store.append(a)
            self._live_lnl = live
            if self.prior is not None:
                dp, live_lp = np.empty((m, R, K)), np.empty((R, L))
                self._check(lib.vk_nprior_record(h, m, N.as_dp(dp), N.as_dp(live_lp)), "vk_nprior_record")
                self._dead_lp.append(dp)
                self._live_lp = live_lp
            self.n_iter += m
            done += m

    def _read_device(self):
        lib, h = self._dev
        R, L, d = self.R, self.n_live, len(self.names)

        def i64(a):
            return a.ctypes.data_as(C.POINTER(C.c_int64))
        self._x, self._lnl, self._chi2 = np.empty((R, L, d)), np.empty((R, L)), np.empty((R, L))
        self._n_accept, self._n_steps, self._n_stuck = (np.empty(R, dtype=np.int64) for _ in range(3))
        self._check(lib.vk_nested_state(h, N.as_dp(self._x), N.as_dp(self._lnl), N.as_dp(self._chi2), i64(self._n_accept),
                                        i64(self._n_steps), i64(self._n_stuck)), "vk_nested_state")
        self._live_lnl = self._lnl
        if self.prior is not None:
            self._lnprior = np.empty((R, L))
            self._check(lib.vk_nprior_record(h, 0, None, N.as_dp(self._lnprior)), "vk_nprior_record")
            self._live_lp = self._lnprior

    def __del__(self):
        dev = getattr(self, "_dev", None)
        if dev:
            try:
                dev[0].vk_nested_destroy(dev[1])
            except Exception:
                pass
            self._dev = None

    # ------------------------------------------------------------------ public ------------------------------------------
    def _dead_arrays(self):
        R, K, d = self.R, self.batch, len(self.names)
        shapes = ((0, R, K), (0, R, K), (0, R, K, d))
        out = []
        for i, store in enumerate(self._dead):
            if len(store) > 1:
                store[:] = [np.concatenate(store)]
            out.append(store[0] if store else np.empty(shapes[i]))
        return out

    def _dead_lnprior(self):
        """(n_iter, R, K): the dead record's ln prior; None without a prior."""
        if self.prior is None:
            return None
        if len(self._dead_lp) > 1:
            self._dead_lp[:] = [np.concatenate(self._dead_lp)]
        return self._dead_lp[0] if self._dead_lp else np.empty((0, self.R, self.batch))

    def _remaining(self):
        """``ln(Z_live / (Z_dead + Z_live))`` (R,) of the runs as they stand (NaN for a problem without a finite lnL)."""
        ro = read_out(self._dead_arrays()[0], self._live_lnl, self.n_live, self.batch, dead_lnprior=self._dead_lnprior(),
                      live_lnprior=self._live_lp)
        with np.errstate(invalid="ignore"):
            return (ro["ln_z_live"] - np.logaddexp(ro["ln_z_dead"], ro["ln_z_live"])).astype(float)

    def _converged(self):
        rem = self._remaining()
        return np.isnan(rem) | (rem < np.log(self.tol))

    def _advance(self, n):
        if n:
            (self._run_device if self._dev else self._run_host)(n)

    def run(self, max_iter):
        """Iterate until every problem meets the stop (checked at every multiple of 8 iterations) or ``max_iter`` is reached."""
        if self._dev and self._refresh is not None:
            self._refresh()
        while self.n_iter < max_iter:
            if self.n_iter % BLOCK == 0 and self.n_iter and np.all(self._converged()):
                break
            self._advance(min(BLOCK - self.n_iter % BLOCK, max_iter - self.n_iter))
        return self._publish()

    def extend(self, n_iter):
        """Continue the same runs for ``n_iter`` more iterations: the same generators, the same blocks of random numbers - the
        runs of one longer call."""
        n_iter = int(n_iter)
        if n_iter < 0:
            raise InputError("nested_sampling: n_iter must be >= 0")
        if self._dev and self._refresh is not None:
            self._refresh()                                   # another object's realisations may have been set on the engine since
        self._advance(n_iter)
        return self._publish()

    def _publish(self):
        if self._dev:
            self._read_device()
        R, L, K, d = self.R, self.n_live, self.batch, len(self.names)
        dead = self._dead_arrays()
        self.dead_lnl, self.dead_chi2 = dead[0], dead[1]
        self.dead_x = dead[2] if self.keep_dead else None
        self.x, self.lnl, self.chi2 = self._x.copy(), self._lnl.copy(), self._chi2.copy()
        self.n_accept, self.n_steps, self.n_stuck = self._n_accept.copy(), self._n_steps.copy(), self._n_stuck.copy()
        self.acceptance = self.n_accept / np.maximum(1, self.n_steps)
        self.dead_lnprior = self._dead_lnprior()
        self.lnprior = None if self.prior is None else self._lnprior.copy()
        ro = read_out(self.dead_lnl, self.lnl, L, K, dead_lnprior=self.dead_lnprior, live_lnprior=self.lnprior)
        self.ln_evidence, self.information, self.ln_evidence_error = ro["ln_evidence"], ro["information"], ro["ln_evidence_error"]
        self.ln_evidence_unnormalised = self.ln_evidence
        if self.prior is not None:
            self.ln_evidence = self.ln_evidence_unnormalised - self.ln_prior_norm
            self.ln_evidence_error = np.sqrt(ro["information"] / L + self.ln_prior_norm_error ** 2)
        with np.errstate(invalid="ignore"):
            self.remaining = (ro["ln_z_live"] - np.logaddexp(ro["ln_z_dead"], ro["ln_z_live"])).astype(float)
            done = self.remaining < np.log(self.tol)
        self.status = np.where(ro["no_finite"], NO_FINITE, np.where(done, OK, MAX_ITER)).astype(np.int32)
        self.status_names = [STATUS[int(s)] for s in self.status]
        self.samples = self.weights = self.mean = self.cov = self.sigma = None
        if self.keep_dead:
            self.samples = np.concatenate([np.moveaxis(self.dead_x, 1, 0).reshape(R, -1, d), self.x], axis=1)
            w = np.exp(ro["log_weights"])
            self.weights = w.astype(float)
            s = self.samples.astype(_ld)
            with np.errstate(invalid="ignore"):
                mean = (w[:, :, None] * s).sum(axis=1)
                dev = s - mean[:, None, :]
                cov = (w[:, :, None, None] * dev[:, :, :, None] * dev[:, :, None, :]).sum(axis=1)
            mean[ro["no_finite"]] = np.nan
            cov[ro["no_finite"]] = np.nan
            self.mean, self.cov = mean.astype(float), cov.astype(float)
            self.sigma = np.sqrt(np.einsum("rjj->rj", self.cov))
        return self

    def ln_evidence_samples(self, n, seed=0):
        """(n, R) evidences under redrawn shrinkage factors: ``t ~ Beta(L - k, 1)`` at dead point (t, k), i.e.
        ``ln t = ln(u) / (L - k)`` - the scatter the evidence has from the unknown volumes (not from the finite walks)."""
        T, R, K = self.dead_lnl.shape
        rng = np.random.default_rng(seed)
        out = np.empty((int(n), R))
        live = _ld(self.n_live) - np.tile(np.arange(K), T).astype(_ld)
        for i in range(int(n)):
            ln_t = np.log(rng.random((R, T * K))).astype(_ld) / live
            out[i] = read_out(self.dead_lnl, self.lnl, self.n_live, K, ln_x=np.cumsum(ln_t, axis=1), dead_lnprior=self.dead_lnprior,
                              live_lnprior=self.lnprior)["ln_evidence"]
        if self.prior is not None:
            out -= self.ln_prior_norm
        return out

    def equal_weight_samples(self, n, seed=0):
        """(R, n, d): ``n`` draws (with replacement) of every problem's posterior sample by its weights (NaN rows for a problem
        without a finite lnL)."""
        if not self.keep_dead:
            raise InputError("nested_sampling: equal_weight_samples needs the dead record (keep_dead=True)")
        rng = np.random.default_rng(seed)
        out = np.full((self.R, int(n), len(self.names)), np.nan)
        for r in range(self.R):
            w = self.weights[r]
            if w.sum() > 0:
                out[r] = self.samples[r][rng.choice(len(w), size=int(n), p=w / w.sum())]
        return out


def exact_prior_norm(prior, lo, hi):
    """``ln((1 / V) integral over the box of exp(ln prior))`` of a :class:`victor_amd.priors.ResolvedPrior` whose priors are all
    independent (``sigma=`` or a diagonal ``cov``): the sum over the named parameters of
    ``ln(sigma sqrt(pi / 2) [erf((hi - mu) / (sigma sqrt 2)) - erf((lo - mu) / (sigma sqrt 2))] / (hi - lo))``.  None for a
    correlated prior."""
    if prior.sigma is None:
        return None
    total = 0.0
    for j in range(prior.d):
        sg = float(prior.sigma[j])
        if math.isnan(sg):                                   # (no prior names this parameter: its factor is 1)
            continue
        mu, a, b = float(prior.mu[j]), float(lo[j]), float(hi[j])
        total += math.log(sg * math.sqrt(math.pi / 2.0) * (math.erf((b - mu) / (sg * math.sqrt(2.0))) - math.erf((a - mu) / (sg * math.sqrt(2.0))))
                          / (b - a))
    return total


def nested_prior_norm(prior, names, lo, hi, n_live, batch, steps, scale, seed, tol, max_iter):
    """(value, error) of the prior's normalisation over the box by the route's own method: the definition loop on the prior's own
    problem - R = 1, lnL = 0 - with the generators ``[seed, 3]``, ``[seed, 4]``, ``[seed, 5]`` in the roles of ``[seed, 0 .. 2]``.
    On the host, without a theory evaluation."""
    def zero(x, rows_which=None):
        z = np.zeros(len(x))
        return z, z.copy()
    ns = NestedSampling(names, lo, hi, {}, 1, n_live, batch, steps, scale, seed, tol, False, zero, None, None, prior=prior, streams=(3, 4, 5))
    ns.ln_prior_norm = ns.ln_prior_norm_error = 0.0          # (the prior's own problem: its evidence IS the normalisation)
    ns._start_host(ns.start_points())
    ns.run(max_iter)
    return float(ns.ln_evidence_unnormalised[0]), float(np.sqrt(ns.information[0] / n_live))


def nested_sampling(fit, params, n_live=DEFAULT_LIVE, batch=DEFAULT_BATCH, steps=DEFAULT_STEPS, scale=None, seed=0, fixed=None,
                    tol=1e-3, max_iter=None, n_iter=None, keep_dead=True, device=True, evaluate=None, kwargs=None, realisations=None,
                    prior=None, prior_norm="auto"):
    """The work of the ``nested_sampling`` methods (``realisations=None``: the fit's data vector, R = 1); see the module docstring.
    With ``evaluate`` - a callable taking a dict of ``(n,)`` arrays (sampled and fixed parameters) and returning ``lnL (n,)`` or
    ``(lnL, chi2)`` - in place of ``fit`` only the definition route (``device=False``) is possible, R = 1 and no GPU is needed.

    ``params``: the cobaya block, whose uniform priors are the box; ``fixed``: name -> scalar overrides; ``scale``: the step
    width in units of the live range, default ``0.5 / sqrt(d)``; ``tol``, ``max_iter`` (default ``128 n_live / batch``): the stop;
    ``n_iter``: a fixed number of iterations instead; ``keep_dead``: keep the dead points' positions (the posterior sample).
    ``prior``: a :class:`victor_amd.priors.GaussianPrior` or a list of them, multiplied onto the box (with ``evaluate``: over the
    block's names); the run then orders, kills and constrains on lnL + ln prior, and the evidence is under the Gaussian
    normalised over the box.  ``prior_norm``: how that normalisation is had - ``"exact"`` (the closed form of independent
    priors; refused on a correlated one), ``"nested"`` (the prior's own run of the definition loop, on the host) or ``"auto"``
    (exact where possible).
    Every argument is checked before the first device call.  Returns a :class:`NestedSampling`."""
    from .priors import GaussianPrior
    kwargs = dict(kwargs or {})
    who = "nested_sampling"
    prior = kwargs.pop("prior", prior)
    if prior is not None and not isinstance(prior, GaussianPrior) and not (
            isinstance(prior, (list, tuple)) and len(prior) and all(isinstance(p, GaussianPrior) for p in prior)):
        raise InputError(f"{who}: prior= is not accepted: it must be a GaussianPrior or a list of them")
    if prior_norm not in ("auto", "exact", "nested"):
        raise InputError(f"{who}: prior_norm must be 'auto', 'exact' or 'nested'")
    n_live, batch, steps = int(n_live), int(batch), int(steps)
    if n_live < 2 or n_live > MAX_LIVE:
        raise InputError(f"{who}: need 2 <= n_live <= {MAX_LIVE}")
    if batch < 1 or n_live % batch or batch > n_live // 2:
        raise InputError(f"{who}: batch must divide n_live and be at most n_live / 2 (n_live = {n_live}, batch = {batch})")
    if steps < 1:
        raise InputError(f"{who}: steps must be >= 1")
    if steps > 1024:
        raise InputError(f"{who}: steps must be <= 1024")
    if not tol > 0:
        raise InputError(f"{who}: tol must be > 0")
    if n_iter is not None and int(n_iter) < 0:
        raise InputError(f"{who}: n_iter must be >= 0")
    if evaluate is not None and device:
        raise InputError(f"{who}: an evaluate callable runs the definition route only (device=False)")
    if evaluate is None and fit is None:
        raise InputError(f"{who}: a fit or an evaluate callable is needed")
    q = _Sampled(who, "sampled", params, fixed)
    names, fixed_all, lo, hi, d = q.names, q.fixed_all, q.lo, q.hi, len(q.names)
    arrays = sorted(k for k, v in fixed_all.items() if np.ndim(v) > 0)
    if evaluate is None:
        q.check_columns(fit)
    if d > 10:
        raise InputError(f"{who}: at most 10 sampled parameters")
    if evaluate is None:
        q.check_alpha()
    if arrays:
        raise InputError(f"{who}: fixed values must be scalars ({arrays} are not)")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise InputError(f"{who}: every sampled parameter needs a finite prior box")
    scale = 0.5 / np.sqrt(d) if scale is None else float(scale)
    if not (np.isfinite(scale) and scale > 0):
        raise InputError(f"{who}: scale must be finite and > 0")
    if evaluate is None:
        fit_options = q.fit_options(fit, kwargs)
    prior = q.prior(list(prior) if isinstance(prior, tuple) else prior, fit)
    if prior is not None and prior_norm == "exact" and prior.sigma is None:
        raise InputError(f"{who}: prior_norm='exact' needs independent priors (sigma=, or a diagonal cov); a correlated prior is "
                         "normalised by prior_norm='nested'")
    R = len(realisations) if realisations is not None else 1
    if R * batch > MAX_ROWS:
        raise InputError(f"{who}: {R} problems x batch {batch} = {R * batch} rows: at most {MAX_ROWS}")
    max_iter = 128 * (n_live // batch) if max_iter is None else int(max_iter)
    if max_iter < 0:
        raise InputError(f"{who}: max_iter must be >= 0")
    which = np.repeat(np.arange(R, dtype=np.int32), batch)
    fixed_out = {k: float(v) for k, v in fixed_all.items()}

    def batch_of(x):
        b = dict(fixed_out)
        b.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names)})
        return b

    ns = NestedSampling(names, lo, hi, fixed_out, R, n_live, batch, steps, scale, seed, tol, keep_dead, None, None, which, prior=prior)
    x0 = ns.start_points()
    if prior is not None:
        if prior_norm == "exact" or (prior_norm == "auto" and prior.sigma is not None):
            ns.prior_norm, ns.ln_prior_norm, ns.ln_prior_norm_error = "exact", exact_prior_norm(prior, lo, hi), 0.0
        else:
            ns.prior_norm = "nested"
            ns.ln_prior_norm, ns.ln_prior_norm_error = nested_prior_norm(prior, names, lo, hi, n_live, batch, steps, scale, seed, tol, max_iter)
    if evaluate is not None:
        def evaluator(x, rows_which=None):
            out = evaluate(batch_of(x))
            if isinstance(out, tuple):
                return np.asarray(out[0], dtype=float), np.asarray(out[1], dtype=float)
            lnl = np.asarray(out, dtype=float)
            return lnl, -2.0 * lnl
    elif not device:
        if realisations is not None:
            def evaluator(x, rows_which=None):
                return realisations.log_likelihood_pairs(batch_of(x), which if rows_which is None else rows_which, **kwargs)
        else:
            def evaluator(x, rows_which=None):
                return fit.log_likelihood_batch(batch_of(x), **kwargs)
    else:
        evaluator = None
        lib, h, refresh = q.create("vk_nested_create", fit, realisations, kwargs, fit_options, batch_of(x0[:, :batch].reshape(R * batch, d)),
                                   which, shape=(n_live, batch, steps, scale))
        ns._dev, ns._refresh, ns._fit = (lib, h), refresh, fit
    ns._evaluate = evaluator
    if ns._dev and prior is not None:
        ns._check(ns._dev[0].vk_nprior_set(ns._dev[1], N.as_dp(prior.mu), N.as_dp(prior.pp)), "vk_nprior_set")
    if ns._dev:
        ns._check(ns._dev[0].vk_nested_start(ns._dev[1], N.as_dp(N.f64(x0))), "vk_nested_start")
        ns._live_lnl = None
    else:
        ns._start_host(x0)
    if n_iter is not None:
        return ns.extend(int(n_iter))
    return ns.run(max_iter)


def run_definition(params, evaluate, **options):
    """The definition route on an ``evaluate`` callable (no fit, no GPU): ``nested_sampling(None, params, device=False, ...)``."""
    return nested_sampling(None, params, device=False, evaluate=evaluate, **options)
