"""The best-fit search of ``vk_fit_run`` restated in NumPy, slot for slot: the definition route the device loop has to reproduce.

Every other device loop of the sampled layer has a host route (``device=False``) that it reproduces byte for byte; the
Nelder-Mead search behind ``best_fit`` (``victor_amd/fitting.py``) has this module.  Two layers:

* :class:`State`, :func:`start` and :func:`transition` restate ``vkfit::State`` / ``start`` / ``lay_start`` / ``lay_candidates`` /
  ``lay_shrink`` / ``decide`` / ``transition`` of ``victor_amd/csrc/vk_fit_simplex.h`` INCLUDING the slot layout: a problem owns
  ``S = max(4, d + 1)`` row slots; ``live[slot]`` says whether the search uses the slot's value; a dead slot (a spare slot of an
  init or shrink launch, a candidate outside the box) carries a copy of ``v[0]``; all four candidates r, e, oc, ic travel in one
  launch (speculation) and ``n_evals`` counts what a one-point-at-a-time search would have evaluated.  The association is the
  header's: the centroid a running sum from 0.0 divided by d, ``c + g``, ``c + 2 g``, ``c + 0.5 g``, ``c - 0.5 g``, the shrink
  ``v0 + 0.5 (vi - v0)`` - IEEE doubles on both sides, no product but by 2 and 1/2, so the bits agree.
* :func:`run` restates ``fit_loop`` of ``victor_amd/csrc/vk_sampled.hip``: every iteration evaluates ONE batch of
  ``n_active * S`` rows, problems in active-list order and slots in slot order; every ``FIT_CHECK`` iterations the finished
  problems are dropped from the list and the rows laid out again; until then a finished problem's last rows stay in the launch
  (their values are read by nobody).  Which rows share a launch therefore depends only on the problems' own histories
  ("Compaction").  Under a prior a live slot's value is ``lnL + prior.lnprior(pt[slot])`` before the
  transition and chi2 stays the row's (the statement of ``vk_fit_step_kernel``).

:func:`best_fit` drives :func:`run` through the public calls the chains' definition routes use (``log_likelihood_batch`` /
``log_likelihood_pairs`` of a fit, its realisations, a joint fit, its realisations), with the start simplex, steps and tolerances
formed by the ``_Sampled`` helpers ``fitting.best_fit`` itself calls.  No GPU import at module level; :func:`run` with an analytic
``evaluate`` needs none at all (``tests/test_best_fit.py``).
"""

import math

import numpy as np

INF = math.inf
FIT_CHECK = 8                  # kFitCheck of victor_amd/csrc/vk_sampled.hip: iterations between two looks at the status words
INIT, CAND, SHRINK, DONE = 0, 1, 2, 3                                                     # phases (vk_fit_simplex.h)
R_, E_, OC, IC = 0, 1, 2, 3                                                               # candidate slots
VERTICES, EXPAND, REFLECT, OUTSIDE, INSIDE, SHRUNK, RESTART, CONVERGED, MAX_ITER, NO_FINITE_START = range(10)   # vkfit::Decision
ST_CONVERGED, ST_MAX_ITER, ST_NO_FINITE_START = 0, 1, 2                                   # VK_FIT_* of include/victor_hip.h


def slots(d):
    return d + 1 if d + 1 > 4 else 4


class Params:
    """``vkfit::Params``: what every problem of a run shares."""

    def __init__(self, lo, hi, step, xtol, ftol, max_iter, restarts):
        self.lo, self.hi, self.step, self.xtol = (np.array(a, dtype=np.float64) for a in (lo, hi, step, xtol))
        self.d = len(self.lo)
        self.S = slots(self.d)
        self.ftol, self.max_iter, self.restarts = float(ftol), int(max_iter), int(restarts)


class State:
    """``vkfit::State`` of one problem, and what the checks read beside it: the decisions taken, the smallest margin of a
    comparison, the dead candidate slots seen."""

    def __init__(self, q):
        d, S = q.d, q.S
        self.phase, self.status, self.iter, self.restarts_left, self.n_evals = INIT, -1, 0, 0, 0
        self.live = [0] * S
        self.f = np.full(d + 1, INF)
        self.chi = np.full(d + 1, INF)
        self.v = np.zeros((d + 1, d))
        self.pt = np.zeros((S, d))
        self.x0 = np.zeros(d)
        self.decisions = []
        self.margin = INF
        self.n_dead_candidates = 0

    def compare(self, a, b):
        """Note how far apart two values the search is about to compare are (a difference that is not finite could not fall the
        other way for a rounding's sake)."""
        m = abs(a - b) if math.isfinite(a) and math.isfinite(b) else INF
        if m < self.margin:
            self.margin = m


def in_box(q, x):
    return bool(np.all((x >= q.lo) & (x <= q.hi)))                  # (a NaN is outside)


def _put(s, q, slot, x):
    inside = in_box(q, x)
    s.live[slot] = 1 if inside else 0
    s.pt[slot] = x if inside else s.v[0]


def lay_start(s, q):
    s.phase = INIT
    d = q.d
    for i in range(1, d + 1):
        j = i - 1
        s.v[i] = s.v[0]
        v0 = s.v[0, j]
        up, down = v0 + q.step[j], v0 - q.step[j]
        s.v[i, j] = up if up <= q.hi[j] else (down if down >= q.lo[j] else (q.hi[j] if q.hi[j] - v0 >= v0 - q.lo[j] else q.lo[j]))
    for i in range(q.S):
        _put(s, q, i, s.v[i if i <= d else 0])
    for i in range(d + 1, q.S):
        s.live[i] = 0                                               # spare slots repeat the start


def start(q, x0):
    s = State(q)
    s.restarts_left = q.restarts
    s.x0[:] = x0
    s.v[0] = x0
    lay_start(s, q)
    return s


def f_of(lnl):
    return -lnl if math.isfinite(lnl) else INF                      # -inf / NaN / +inf lnL: failed


def _sort(s, q):
    """Insertion sort of the d + 1 vertices by f; equal values keep their order."""
    for i in range(1, q.d + 1):
        k = i
        while k > 0:
            s.compare(s.f[k], s.f[k - 1])
            if not s.f[k] < s.f[k - 1]:
                break
            s.f[[k, k - 1]] = s.f[[k - 1, k]]
            s.chi[[k, k - 1]] = s.chi[[k - 1, k]]
            s.v[[k, k - 1]] = s.v[[k - 1, k]]
            k -= 1


def _converged(s, q):
    ok = True
    for i in range(1, q.d + 1):
        diff = s.f[i] - s.f[0]
        s.compare(diff, q.ftol)
        ok = ok and bool(diff <= q.ftol)
        ok = ok and bool(np.all(np.abs(s.v[i] - s.v[0]) <= q.xtol))
    return ok


def lay_candidates(s, q):
    s.phase = CAND
    d = q.d
    c = np.zeros(d)
    for i in range(d):
        c = c + s.v[i]
    c = c / d
    g = c - s.v[d]
    s.pt[R_] = c + g
    s.pt[E_] = c + 2.0 * g
    s.pt[OC] = c + 0.5 * g
    s.pt[IC] = c - 0.5 * g
    for k in range(4):
        inside = in_box(q, s.pt[k])
        s.live[k] = 1 if inside else 0
        if not inside:
            s.pt[k] = s.v[0]
            s.n_dead_candidates += 1
    for i in range(4, q.S):
        s.live[i] = 0
        s.pt[i] = s.v[0]


def lay_shrink(s, q):
    s.phase = SHRINK
    d = q.d
    for i in range(1, d + 1):
        s.v[i] = s.v[0] + 0.5 * (s.v[i] - s.v[0])
    for i in range(q.S):
        _put(s, q, i, s.v[i + 1 if i < d else 0])
    for i in range(d, q.S):
        s.live[i] = 0


def _take(s, q, slot, f, chi):
    s.v[q.d] = s.pt[slot]
    s.f[q.d] = f
    s.chi[q.d] = chi


def decide(s, q, fc, cc):
    d = q.d
    fr = fc[R_]
    s.compare(fr, s.f[0])
    if fr < s.f[0]:
        s.compare(fc[E_], fr)
        if fc[E_] < fr:
            _take(s, q, E_, fc[E_], cc[E_])
            return EXPAND
        _take(s, q, R_, fr, cc[R_])
        return REFLECT
    s.compare(fr, s.f[d - 1])
    if fr < s.f[d - 1]:
        _take(s, q, R_, fr, cc[R_])
        return REFLECT
    s.compare(fr, s.f[d])
    if fr < s.f[d]:
        s.compare(fc[OC], fr)
        if fc[OC] <= fr:
            _take(s, q, OC, fc[OC], cc[OC])
            return OUTSIDE
        return SHRUNK
    s.compare(fc[IC], s.f[d])
    if fc[IC] < s.f[d]:
        _take(s, q, IC, fc[IC], cc[IC])
        return INSIDE
    return SHRUNK


def transition(s, q, lnl, chi2):
    """One transition: the values ``lnl`` / ``chi2`` (S,) of the pending launch's slots -> the next launch's slots, or the end.
    Returns the decision and appends it to ``s.decisions``."""
    dec = _transition(s, q, [float(a) for a in lnl], [float(a) for a in chi2])
    s.decisions.append(dec)
    return dec


def _transition(s, q, lnl, chi2):
    d = q.d
    s.iter += 1
    dec = VERTICES
    if s.phase == INIT:
        for i in range(d + 1):
            s.f[i] = f_of(lnl[i]) if s.live[i] else INF
            s.chi[i] = chi2[i] if s.live[i] else INF
            s.n_evals += s.live[i]
        if not np.any(s.f < INF):
            s.v[0] = s.x0
            s.f[0] = s.chi[0] = INF
            s.status, s.phase = ST_NO_FINITE_START, DONE
            return NO_FINITE_START
    elif s.phase == CAND:
        fc = [f_of(lnl[k]) if s.live[k] else INF for k in range(4)]
        cc = [chi2[k] if s.live[k] else INF for k in range(4)]
        s.n_evals += s.live[R_]
        if fc[R_] < s.f[0]:
            s.n_evals += s.live[E_]
        elif not fc[R_] < s.f[d - 1]:
            s.n_evals += s.live[OC] if fc[R_] < s.f[d] else s.live[IC]
        dec = decide(s, q, fc, cc)
        if dec == SHRUNK:
            if s.iter >= q.max_iter:
                s.status, s.phase = ST_MAX_ITER, DONE
                return MAX_ITER
            lay_shrink(s, q)
            return SHRUNK
    else:                                                           # SHRINK: slots 0 .. d - 1 hold v_1 .. v_d
        for i in range(1, d + 1):
            s.f[i] = f_of(lnl[i - 1]) if s.live[i - 1] else INF
            s.chi[i] = chi2[i - 1] if s.live[i - 1] else INF
            s.n_evals += s.live[i - 1]
    _sort(s, q)
    if _converged(s, q):
        if s.restarts_left > 0 and s.iter < q.max_iter:
            s.restarts_left -= 1
            lay_start(s, q)
            return RESTART
        s.status, s.phase = ST_CONVERGED, DONE
        return CONVERGED
    if s.iter >= q.max_iter:
        s.status, s.phase = ST_MAX_ITER, DONE
        return MAX_ITER
    lay_candidates(s, q)
    return dec


class Result:
    """What :func:`run` returns: ``x`` (R, d), ``lnl`` (under a prior: lnL + ln prior, ``lnpost``), ``chi2``, ``status``,
    ``n_iter``, ``n_evals`` as ``vk_fit_run`` returns them; ``decisions``: per problem, the decision of each of its launches;
    ``margin`` (R,): the smallest ``|f_a - f_b|`` over the comparisons the problem's search took - the ``<`` / ``<=`` tests of
    ``decide``, the ftol test, and the sort's (which order the vertices the next centroid is formed from); ``launches``: the
    rows of every evaluation; ``n_active``: the length of the active list at every look at the status words (its first entry
    R); ``n_dead_candidates`` (R,): candidate slots that fell outside the box; ``trace`` (with ``trace=True``): per problem,
    ``(phase, live, pt)`` of every launch."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.lnpost = self.lnl

    @property
    def compactions(self):
        return sum(1 for a, b in zip(self.n_active, self.n_active[1:]) if 0 < b < a)


def run(evaluate, x0, lo, hi, step, xtol, ftol, max_iter, restarts, prior=None, trace=False):
    """``fit_loop``: ``evaluate(points (m, d), problem (m,)) -> (lnL (m,), chi2 (m,))`` is called once per iteration with the
    ``n_active * S`` pending rows."""
    x0 = np.array(x0, dtype=np.float64)
    R, d = x0.shape
    q = Params(lo, hi, step, xtol, ftol, max_iter, restarts)
    S = q.S
    for p in range(R):
        if not in_box(q, x0[p]):
            raise ValueError(f"the start of problem {p} is outside the box")
    states = [start(q, x0[p]) for p in range(R)]
    traces = [[] for _ in range(R)]
    rows = np.empty((R * S, d))
    row_problem = np.empty(R * S, dtype=np.int32)

    def emit(p, k):                                                 # fit_emit: problem p's pending rows at launch position k
        rows[k * S:(k + 1) * S] = states[p].pt
        row_problem[k * S:(k + 1) * S] = p
        if trace:
            s = states[p]
            traces[p].append((s.phase, tuple(s.live), s.pt.copy()))

    act = list(range(R))
    for p in act:
        emit(p, p)
    launches, n_active = [], [R]
    while True:
        for _ in range(FIT_CHECK):
            if all(states[p].phase == DONE for p in act):
                break                                               # (the device evaluates on: nobody reads those values)
            m = len(act) * S
            lnl, chi2 = evaluate(rows[:m].copy(), row_problem[:m].copy())
            lnl, chi2 = np.array(lnl, dtype=np.float64), np.array(chi2, dtype=np.float64)
            launches.append(m)
            for k, p in enumerate(act):
                s = states[p]
                if s.phase == DONE:
                    continue
                sl = slice(k * S, (k + 1) * S)
                if prior is not None:
                    for slot in range(S):
                        if s.live[slot]:
                            lnl[k * S + slot] = lnl[k * S + slot] + prior.lnprior(s.pt[slot])
                transition(s, q, lnl[sl], chi2[sl])
                if s.phase != DONE:
                    emit(p, k)
        nxt = [p for p in act if states[p].phase != DONE]
        n_active.append(len(nxt))
        if not nxt:
            break
        if len(nxt) < len(act):
            act = nxt
            for k, p in enumerate(act):
                if trace:
                    traces[p].pop()                                 # (the same pending launch, laid out again)
                emit(p, k)
    return Result(x=np.array([s.v[0] for s in states]), lnl=np.array([-s.f[0] for s in states]),
                  chi2=np.array([s.chi[0] for s in states]), status=np.array([s.status for s in states], dtype=np.int32),
                  n_iter=np.array([s.iter for s in states], dtype=np.int32), n_evals=np.array([s.n_evals for s in states], dtype=np.int64),
                  decisions=[s.decisions for s in states], margin=np.array([s.margin for s in states]), launches=launches,
                  n_active=n_active, n_dead_candidates=np.array([s.n_dead_candidates for s in states]), trace=traces if trace else None)


def best_fit(target, params, fixed=None, start=None, step=None, xtol=None, ftol=1e-6, max_iter=None, restarts=1, prior=None, **kwargs):
    """:func:`run` with the arguments of ``best_fit`` of ``target`` - a ``CCFFit``, a ``Realisations``, a ``JointFit`` or a
    ``JointRealisations`` - evaluated through ``log_likelihood_batch`` / ``log_likelihood_pairs``, the fixed values merged as
    ``victor_amd/chains.py`` merges them (an array in ``fixed``: problem p's value in problem p's rows).  The start, the steps and
    xtol are those ``victor_amd.fitting.best_fit`` forms, by the same helpers.  The result also carries ``names`` and, under a
    prior, ``lnprior`` (the host's, at ``x``)."""
    from victor_amd.fitting import _Sampled
    if hasattr(target, "joint"):
        fit, realisations = target.joint, target
    elif hasattr(target, "numbers") and hasattr(target, "fit"):
        fit, realisations = target.fit, target
    else:
        fit, realisations = target, None
    q = _Sampled("best_fit", "fitted", params, fixed)
    names, fixed_all, d = q.names, q.fixed_all, len(q.names)
    q.check_columns(fit)
    arrays = {k: np.atleast_1d(np.asarray(v, dtype=float)) for k, v in fixed_all.items() if np.ndim(v) > 0}
    R = len(realisations) if realisations is not None else (len(next(iter(arrays.values()))) if arrays else 1)
    q.check_alpha()
    resolved = q.prior(prior, fit)
    x0 = q.starts(start, R)
    steps = q.per_param("step", step, [s.proposal for s in q.specs])
    xtols = q.per_param("xtol", xtol, 1e-4 * steps)
    max_iter = 200 * d if max_iter is None else int(max_iter)
    scalars = {k: float(v) for k, v in fixed_all.items() if k not in arrays}

    def evaluate(x, problem):
        batch = dict(scalars)
        batch.update({k: np.ascontiguousarray(v[problem]) for k, v in arrays.items()})
        batch.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names)})
        if realisations is not None:
            return realisations.log_likelihood_pairs(batch, problem, **kwargs)
        return fit.log_likelihood_batch(batch, **kwargs)

    out = run(evaluate, x0, q.lo, q.hi, steps, xtols, ftol, max_iter, int(restarts), resolved)
    out.names = list(names)
    out.lnprior = np.zeros(R) if resolved is None else resolved.lnprior(out.x)
    return out
