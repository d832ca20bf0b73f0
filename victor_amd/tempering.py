"""Replica exchange (parallel tempering) of the Metropolis chains of :mod:`victor_amd.chains`, and the evidence by thermodynamic
integration: ``sample_chains(..., temper=...)``.  This module is the NumPy statement of ``victor_amd/csrc/vk_temper_step.h`` - the
definition the device route (``vk_chain_begin_tempered``, ``include/victor_hip.h``) reproduces bit for bit - and what reads the
result.

K copies of every problem are sampled at inverse temperatures 1 = beta_0 > beta_1 > ... > beta_(K-1) >= 0; the copy at beta samples
``L**beta * prior`` (the prior: the box, times the Gaussian ``prior=`` if any).  Chain ``c = (r K + k) W + w`` is problem r, rung
k, walker w, so the ``group = W`` features of the chains (moment sums pooled per problem, marginals, autocorr) see every (r, k)
as a problem and the host slices out k = 0, the cold rung: the posterior itself.

**The tempered step.**  ``post' = beta * lnL' (+ lp')`` and ``post = beta * lnL (+ lp)``, every product and sum rounded on its own;
accept when the proposal is inside the box and ``logu < post' - post`` (a NaN rejects).  ``1 * v == v``, so at beta = 1 this is
the plain chains' decision bit for bit.  At beta = 0 without a prior every proposal inside the box with a finite lnL' is accepted;
``0 * -inf`` is NaN, so a row that failed is never moved onto - and, the one dead end, a chain whose STORED lnL is -inf at beta = 0
never moves by a step (a swap can carry the state to a colder rung).  State, history and chi2 keep the log-likelihood.

**The energy sums.**  At every kept step, after the decision and before any swap, a chain whose stored lnL is finite counts it:
``n_e += 1``; the first such value becomes ``pivot_e``; ``a = lnL - pivot_e``; ``e1 += a``; ``e2 += a * a``.

**The swap.**  A swap event follows the step with life-long index s when ``(s + 1) % swap_every == 0`` (``swap_every = 0``:
never); event ``e = (s + 1) / swap_every - 1`` has parity ``e % 2`` and pairs (k, w) with (k + 1, w) of the same problem for every
k = parity (mod 2) with k + 1 < K.  Accept when ``logs < (beta_k - beta_(k+1)) * (lnL_(k+1) - lnL_k)`` (a NaN rejects), ``logs``
the entry of the lower rung's chain; on accept x, lnL and chi2 are exchanged (the untempered prior cancels in the ratio) while
temperatures, pivots, sums and counters stay with the rung.  The W ladders of a problem never interact, so ``rhat`` over the cold
rung's W chains stays meaningful.

**Random numbers.**  ``dz`` and ``logu`` are the plain chains' for C = R K W chains; ``logs`` comes from a second generator,
``np.random.default_rng([seed, 1])``: ``log(random((64, C)))`` per block of 64 steps - so ``temper={"betas": [1.0]}`` consumes the
plain chains' stream and reproduces them bit for bit.

**The evidence.**  ``ln Z = int_0^1 <lnL>_beta dbeta`` relative to the NORMALISED prior (the beta = 0 rung samples the prior itself),
from the rungs' pooled means E_k and variances V_k of lnL (``d<lnL>/dbeta = Var(lnL)``):
``ln_evidence_trapezoid = sum_k (dbeta_k / 2) (E_k + E_(k+1))`` and ``ln_evidence = ln_evidence_trapezoid - sum_k (dbeta_k**2 / 12)
(V_k - V_(k+1))`` with ``dbeta_k = beta_k - beta_(k+1)``.  Both are NaN for a ladder that does not reach beta = 0.
"""

import numpy as np

from .utils import InputError

BLOCK = 64
DEFAULT_RUNGS, DEFAULT_POWER, DEFAULT_SWAP_EVERY = 16, 5.0, 4


def power_ladder(rungs, power):
    """``beta_k = ((K - 1 - k) / (K - 1))**p``, k = 0 .. K - 1: from 1 down to 0 (Friel & Pettitt 2008 use p = 5); [1] for K = 1."""
    K = int(rungs)
    if K == 1:
        return np.array([1.0])
    return ((K - 1 - np.arange(K)) / (K - 1.0)) ** float(power)


class Ladder:
    """The ``temper=`` argument resolved: ``betas`` (K,), ``K``, ``swap_every`` and ``scales`` (K,), the factor on the proposal
    widths (and on a Laplace proposal's factors) of each rung."""

    def __init__(self, betas, swap_every, scales):
        self.betas = np.ascontiguousarray(betas, dtype=np.float64)
        self.K = len(self.betas)
        self.swap_every = int(swap_every)
        self.scales = np.ascontiguousarray(scales, dtype=np.float64)


def default_scales(betas, width, lo, hi):
    """``scale_k = min(1 / sqrt(beta_k), min_j (hi_j - lo_j) / (2 width_j))``, 1 / sqrt(0) read as infinity: a hot rung proposes as
    widely as its flattened density asks for, up to half the box."""
    cap = float(np.min((np.asarray(hi) - np.asarray(lo)) / (2.0 * np.asarray(width))))
    with np.errstate(divide="ignore"):
        return np.minimum(1.0 / np.sqrt(betas), cap)


def resolve_temper(temper, who, width, lo, hi):
    """The :class:`Ladder` of a ``temper=`` argument (None for None or False); every refusal is an ``InputError``."""
    if temper is None or temper is False:
        return None
    opts = {} if temper is True else temper
    if not isinstance(opts, dict):
        raise InputError(f"{who}: temper must be None, True or a dict")
    unknown = sorted(set(opts) - {"rungs", "power", "betas", "swap_every", "scales"})
    if unknown:
        raise InputError(f"{who}: temper has no option {unknown} (rungs, power, betas, swap_every, scales)")
    if "betas" in opts:
        if "rungs" in opts or "power" in opts:
            raise InputError(f"{who}: temper takes an explicit ladder (betas) or a power ladder (rungs, power), not both")
        betas = np.atleast_1d(np.asarray(opts["betas"], dtype=np.float64))
        if betas.ndim != 1 or betas.size < 1:
            raise InputError(f"{who}: temper betas must be a list of at least one inverse temperature")
    else:
        rungs, power = int(opts.get("rungs", DEFAULT_RUNGS)), float(opts.get("power", DEFAULT_POWER))
        if rungs < 1:
            raise InputError(f"{who}: temper needs rungs >= 1")
        if not (np.isfinite(power) and power > 0):
            raise InputError(f"{who}: temper needs power > 0")
        betas = power_ladder(rungs, power)
    if not np.all(np.isfinite(betas)) or np.any(betas < 0):
        raise InputError(f"{who}: every inverse temperature of the ladder must be finite and >= 0 ({betas.tolist()})")
    if betas[0] != 1.0:
        raise InputError(f"{who}: rung 0 of the ladder is the posterior itself: betas[0] must be 1, not {betas[0]}")
    if np.any(~(np.diff(betas) < 0)):
        raise InputError(f"{who}: the inverse temperatures must decrease strictly from rung to rung ({betas.tolist()})")
    swap_every = int(opts.get("swap_every", DEFAULT_SWAP_EVERY))
    if swap_every < 0:
        raise InputError(f"{who}: temper needs swap_every >= 0 (0: never)")
    if opts.get("scales") is None:
        scales = default_scales(betas, width, lo, hi)
    else:
        scales = np.atleast_1d(np.asarray(opts["scales"], dtype=np.float64))
        if scales.shape != betas.shape or not np.all(np.isfinite(scales)) or np.any(~(scales > 0)):
            raise InputError(f"{who}: temper scales must be one finite factor > 0 per rung ({len(betas)})")
    return Ladder(betas, swap_every, scales)


# ---------------------------------------------------------------------- the definition ---------------------------------------
def gain(beta, lnl_prop, lnl, lp_prop=None, lp=None):
    """``post' - post`` of the tempered decision, elementwise: ``beta * lnL'`` and ``beta * lnL`` rounded, the priors added when
    given, one subtraction.  (NaN where 0 * inf or inf - inf occur: the caller's comparison rejects.)"""
    post_prop, post = beta * lnl_prop, beta * lnl
    if lp_prop is not None:
        post_prop, post = post_prop + lp_prop, post + lp
    return post_prop - post


def is_swap(step, swap_every):
    return swap_every > 0 and (step + 1) % swap_every == 0


def swap_parity(step, swap_every):
    return ((step + 1) // swap_every - 1) % 2


class TemperState:
    """The rungs' side of C = R K W tempered chains: ``beta`` (C,) of each chain, the energy sums ``pivot_e``, ``e1``, ``e2``,
    ``n_e`` and the swap counters ``n_swap_try``, ``n_swap_acc`` (C,; counted on the lower chain of a pair), and the generator
    of the swap levels."""

    def __init__(self, ladder, R, W, seed):
        self.ladder, self.R, self.K, self.W = ladder, int(R), ladder.K, int(W)
        self.C = self.R * self.K * self.W
        self.rung = (np.arange(self.C) // self.W) % self.K
        self.beta = ladder.betas[self.rung]
        self.scale = ladder.scales[self.rung]
        self.pivot_e, self.e1, self.e2 = np.zeros(self.C), np.zeros(self.C), np.zeros(self.C)
        self.n_e = np.zeros(self.C, dtype=np.int64)
        self.n_swap_try, self.n_swap_acc = np.zeros(self.C, dtype=np.int64), np.zeros(self.C, dtype=np.int64)
        self._rng = np.random.default_rng([seed, 1])

    def draw_logs(self):
        """The swap levels of the next block of 64 steps."""
        return np.log(self._rng.random((BLOCK, self.C)))

    def energy_add(self, lnl):
        """A kept step: the stored lnL (C,) after the decision, before any swap."""
        fin = np.isfinite(lnl)
        first = fin & (self.n_e == 0)
        self.pivot_e[first] = lnl[first]
        self.n_e[fin] += 1
        a = lnl[fin] - self.pivot_e[fin]
        self.e1[fin] = self.e1[fin] + a
        self.e2[fin] = self.e2[fin] + a * a

    def pairs(self, parity):
        """The lower chains (R * pairs * W,) of an event's candidate pairs; the upper chain of each is W further on."""
        R, K, W = self.R, self.K, self.W
        ks = np.arange(parity, K - 1, 2)
        lo = (np.arange(R)[:, None, None] * K + ks[None, :, None]) * W + np.arange(W)[None, None, :]
        return lo.ravel(), np.broadcast_to(ks[None, :, None], lo.shape).ravel()

    def swap(self, step, x, lnl, chi2, logs):
        """The swap event behind the step with life-long index ``step``, if one follows it: exchanges rows of ``x`` (C, d), ``lnl``,
        ``chi2`` (C,) in place; ``logs`` (C,) are the step's swap levels."""
        if not is_swap(step, self.ladder.swap_every):
            return
        lo, k = self.pairs(swap_parity(step, self.ladder.swap_every))
        if not lo.size:
            return
        hi = lo + self.W
        betas = self.ladder.betas
        with np.errstate(invalid="ignore"):
            g = (betas[k] - betas[k + 1]) * (lnl[hi] - lnl[lo])
            acc = logs[lo] < g                                # NaN: False
        self.n_swap_try[lo] += 1
        self.n_swap_acc[lo] += acc
        a, b = lo[acc], hi[acc]
        for arr in (x, lnl, chi2):
            t = arr[a].copy()
            arr[a] = arr[b]
            arr[b] = t


# ---------------------------------------------------------------------- the result -------------------------------------------
def energy_moments(n_e, pivot_e, e1, e2):
    """(mean (R, K), var (R, K), walker_mean (R, K, W)) of lnL from the per-chain sums (R, K, W), pooled over the W walkers of a
    rung, in extended precision (as :func:`victor_amd.chains.pooled_moments` reads its sums); NaN where a rung counted fewer than
    one (mean) or two (var) values."""
    ld = np.longdouble
    n, p, s1, s2 = (np.asarray(a, dtype=ld) for a in (n_e, pivot_e, e1, e2))
    tot = n.sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (n * p + s1).sum(axis=2) / tot
        delta = p - mean[:, :, None]
        m2 = (s2 + 2 * s1 * delta + n * delta * delta).sum(axis=2)
        var = m2 / (tot - 1)
        walker = p + s1 / n
    mean, var, walker = mean.astype(float), var.astype(float), walker.astype(float)
    mean[np.asarray(tot < 1)] = np.nan
    var[np.asarray(tot < 2)] = np.nan
    return mean, var, walker


def trapezoid_weights(betas):
    """c_k with ``sum_k c_k E_k`` the trapezoid rule of ``int E dbeta`` over the ladder's range."""
    db = betas[:-1] - betas[1:]
    c = np.zeros(len(betas))
    c[:-1] += 0.5 * db
    c[1:] += 0.5 * db
    return c


class Tempering:
    """What ``Chains.tempering`` holds.  ``betas`` (K,), ``scales`` (K,), ``swap_every``; ``mean_lnl``, ``var_lnl`` (R, K): the
    rungs' mean and variance (ddof = 1) of the kept finite lnL, pooled over the W walkers; ``n_not_finite`` (R, K): kept values
    that were -inf and entered neither; ``acceptance`` (R, K): of the Metropolis steps; ``swap_acceptance`` (R, K - 1): of the
    swaps between rung k and rung k + 1 (NaN before the first attempt); ``x`` (R, K, W, d), ``lnl``, ``chi2`` (R, K, W): the
    all-rung state; ``chain`` (n_kept, R, K, W, d), ``lnl_chain``, ``chi2_chain`` (n_kept, R, K, W): the all-rung history (None
    without ``keep_chain``); ``ln_evidence_trapezoid``, ``ln_evidence``, ``ln_evidence_error`` (R,) (module docstring; the error
    is the standard error propagated through the trapezoid weights from the scatter of the W per-walker means of each rung, NaN
    for W = 1); and the raw per-chain arrays ``pivot_e``, ``e1``, ``e2``, ``n_e``, ``n_swap_try``, ``n_swap_acc`` (R, K, W) as the
    route that ran the chains returns them."""

    def __init__(self, state, n_accept, n_steps, n_kept, x, lnl, chi2, hist):
        R, K, W = state.R, state.K, state.W
        lad = state.ladder
        self.betas, self.scales, self.swap_every = lad.betas.copy(), lad.scales.copy(), lad.swap_every
        shape = (R, K, W)
        for name in ("pivot_e", "e1", "e2", "n_e", "n_swap_try", "n_swap_acc"):
            setattr(self, name, getattr(state, name).reshape(shape).copy())
        self.x, self.lnl, self.chi2 = x.reshape(R, K, W, x.shape[-1]).copy(), lnl.reshape(shape).copy(), chi2.reshape(shape).copy()
        self.chain = self.lnl_chain = self.chi2_chain = None
        if hist is not None:
            hx, hl, hc = hist
            self.chain = hx.reshape(len(hx), R, K, W, x.shape[-1])
            self.lnl_chain, self.chi2_chain = hl.reshape(len(hl), R, K, W), hc.reshape(len(hc), R, K, W)
        self.acceptance = n_accept.reshape(shape).sum(axis=2) / max(1, n_steps * W)
        tries, wins = self.n_swap_try[:, :-1].sum(axis=2), self.n_swap_acc[:, :-1].sum(axis=2)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.swap_acceptance = np.where(tries > 0, wins / tries, np.nan)
        self.n_not_finite = (n_kept.reshape(shape) - self.n_e).sum(axis=2)
        self.mean_lnl, self.var_lnl, walker = energy_moments(self.n_e, self.pivot_e, self.e1, self.e2)
        b = self.betas
        db = b[:-1] - b[1:]
        E, V = self.mean_lnl, self.var_lnl
        self.ln_evidence_trapezoid = (0.5 * db * (E[:, :-1] + E[:, 1:])).sum(axis=1)
        self.ln_evidence = self.ln_evidence_trapezoid - (db * db / 12.0 * (V[:, :-1] - V[:, 1:])).sum(axis=1)
        if W > 1:
            with np.errstate(invalid="ignore"):
                s2 = walker.var(axis=2, ddof=1)
            self.ln_evidence_error = np.sqrt((trapezoid_weights(b) ** 2 * s2 / W).sum(axis=1))
        else:
            self.ln_evidence_error = np.full(R, np.nan)
        if b[-1] != 0.0:                                      # the integral needs the prior's own rung
            self.ln_evidence_trapezoid = np.full(R, np.nan)
            self.ln_evidence = np.full(R, np.nan)
            self.ln_evidence_error = np.full(R, np.nan)
