"""Posterior-predictive model vectors and the deviance information criterion from the chains of ``sample_chains``: the
``predictive=`` keyword (``CCFFit`` and ``Realisations``; both moves, both routes).

A void-galaxy fit is judged by one picture: the multipoles of the data with the posterior band of the model drawn through them.
The band needs the theory vector at every kept position, which a run with ``keep_chain=False`` no longer has and a run with a
history would have to evaluate a second time.  The theory vector of every proposal exists where its step is decided, so the sums
are taken there: on the device by two small kernels behind the step kernel (``vk_chain_set_predictive``,
``victor_amd/csrc/vk_predictive.h``), on the definition route by :class:`PredictiveState` below - the NumPy statement of the same
rules, which is the definition.  Chain ``c = r W + w`` is walker w of problem r; N is the length of the data vector.

**Hold.**  ``held[c]`` is the theory vector at chain c's CURRENT position, ``seen[c]`` the chain's accept count when it was taken.
After the start's evaluation every chain takes its row.  After every decision, kept or not, a chain with ``n_accept[c] !=
seen[c]`` takes its row of the launch just decided (row c of a Metropolis launch; row i of a stretch half-step serves the moving
walker ``(2 (i // h) + side) h + i % h``, h = W / 2) and ``seen[c] = n_accept[c]``.  A rejected proposal, and one outside the box
(whose row carries the current position and is never accepted), leaves ``held[c]`` alone.

**Pivot.**  At the start ``pivot_t[r] = held[r W]`` where finite, else 0; ``pivot_chi2[r]``, ``pivot_lnl[r]`` likewise from the
start of chain r W.

**Accumulate**, on a kept step - a kept sweep after its second half, the moment the series of :mod:`victor_amd.autocorr` is taken.
For w = 0 .. W - 1 in that order: if ``chi2[c]`` and ``lnl[c]`` are both finite, ``v = held[c] - pivot_t[r]``, ``sum_t[r] += v``,
``sum_tt[r] += v v``, the four deviance sums likewise about their pivots, ``n[r] += 1``; otherwise ``n_skipped[r] += 1`` and
nothing is summed.  Plain double sums in (step, walker) order, so a run does not depend on how it is cut; the device may contract
``v v`` into the sum (an fma), so the two routes agree to rounding, not bit for bit.

**The read-out** (:class:`Predictive`) forms the moments from pivot and sums in extended precision: ``mean = pivot + sum / n``,
``var = (sum2 - sum^2 / n) / (n - 1)``.  With the deviance D = -2 lnL: ``p_d = mean_D - D(mean position)``, ``p_v = var_D / 2``,
``dic = mean_D + p_d``.  The state costs (C + 3 R) N doubles: 87 MB at 8192 problems of 8 walkers and N = 120.
"""

import numpy as np

from .utils import InputError

DEVIANCE = ("pivot_chi2", "pivot_lnl", "s_chi2", "s_chi2sq", "s_lnl", "s_lnlsq")
FIELDS = ("pivot_t", "sum_t", "sum_tt", "deviance", "n", "n_skipped", "held")


class PredictiveError(InputError, ValueError):
    """A ``predictive=`` argument that cannot be honoured (an :class:`victor_amd.InputError` that is also a ``ValueError``)."""


def resolve_predictive(predictive, who, joint=False, tempered=False, has_fit=True):
    """True for ``predictive=True``, False for None; every refusal is a :class:`PredictiveError`, raised before any evaluation
    and any device call."""
    if predictive is None:
        return False
    if predictive is not True:
        raise PredictiveError(f"{who}: predictive must be None or True, not {predictive!r}")
    if joint:
        raise PredictiveError(f"{who}: predictive is not provided for joint fits (the theory workspace of a joint handle is laid out "
                              "by the route that evaluates it, not as one vector per row)")
    if tempered:
        raise PredictiveError(f"{who}: predictive is not provided with temper= (a swap moves states between chains without touching "
                              "the accept counters the held theory vectors follow)")
    if not has_fit:
        raise PredictiveError(f"{who}: predictive needs a fit (an evaluate callable returns no theory vectors)")
    return True


def resolve_sample_predictive(predictive, who, has_fit=True):
    """The ``predictive=`` of ``importance_posterior`` (:mod:`victor_amd.importance`): True for True, False for None.  A shared
    sample holds a weight per (point, problem) and every point's theory vector, so joint fits are served; what is refused - a
    :class:`PredictiveError`, before any evaluation and any device call - is any other value and a call without a fit."""
    if predictive is None:
        return False
    if predictive is not True:
        raise PredictiveError(f"{who}: predictive must be None or True, not {predictive!r}")
    if not has_fit:
        raise PredictiveError(f"{who}: predictive needs a fit (an evaluate callable returns no theory vectors)")
    return True


def stretch_chains(M, half, side):
    """The chain each of the M rows of half-step ``side`` serves: row i is member i % half of the moving half of ensemble
    i // half."""
    i = np.arange(M)
    return (2 * (i // half) + side) * half + i % half


class PredictiveState:
    """The running state of R problems of W chains with theory vectors of N entries - the NumPy definition of what
    ``vk_chain_hold_kernel`` and ``vk_chain_predict_kernel`` keep (module docstring): ``pivot_t``, ``sum_t``, ``sum_tt`` (R, N),
    ``deviance`` (R, 6) in the order of ``DEVIANCE``, ``n``, ``n_skipped`` (R,), ``held`` (R W, N), ``seen`` (R W,)."""

    def __init__(self, R, W, N):
        self.R, self.W, self.N = int(R), int(W), int(N)
        self.reset()

    def reset(self):
        R, C_, N = self.R, self.R * self.W, self.N
        self.pivot_t, self.sum_t, self.sum_tt = np.zeros((R, N)), np.zeros((R, N)), np.zeros((R, N))
        self.deviance = np.zeros((R, 6))
        self.n, self.n_skipped = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
        self.held, self.seen = np.zeros((C_, N)), np.zeros(C_, dtype=np.int64)

    def changed(self, chains, n_accept):
        """Which of ``chains`` (the chains the rows of the launch just decided serve) take their row."""
        return np.asarray(n_accept)[chains] != self.seen[chains]

    def hold(self, chains, theory, n_accept):
        """``chains`` (m,) take the theory vectors ``theory`` (m, N): the caller hands the changed ones (or all, at the start)."""
        self.held[chains] = theory
        self.seen[chains] = np.asarray(n_accept)[chains]

    def start(self, theory, n_accept, chi2, lnl):
        """Fresh sums; every chain holds its start's theory vector (C, N); the pivots."""
        self.reset()
        self.hold(np.arange(self.R * self.W), theory, n_accept)
        first = np.arange(self.R) * self.W

        def pivot(v):
            return np.where(np.isfinite(v), v, 0.0)
        self.pivot_t[...] = pivot(self.held[first])
        self.deviance[:, 0] = pivot(np.asarray(chi2, dtype=float)[first])
        self.deviance[:, 1] = pivot(np.asarray(lnl, dtype=float)[first])

    def add(self, chi2, lnl):
        """One kept step (one kept sweep): the chains' chi2 and lnl (C,), walker after walker."""
        chi2, lnl = np.asarray(chi2, dtype=float).reshape(self.R, self.W), np.asarray(lnl, dtype=float).reshape(self.R, self.W)
        held = self.held.reshape(self.R, self.W, self.N)
        dev = self.deviance
        for w in range(self.W):
            ok = np.isfinite(chi2[:, w]) & np.isfinite(lnl[:, w])
            with np.errstate(invalid="ignore", over="ignore"):
                v = held[:, w] - self.pivot_t
                a, b = chi2[:, w] - dev[:, 0], lnl[:, w] - dev[:, 1]
                self.sum_t[ok] = self.sum_t[ok] + v[ok]
                self.sum_tt[ok] = self.sum_tt[ok] + v[ok] * v[ok]
                dev[ok, 2] = dev[ok, 2] + a[ok]
                dev[ok, 3] = dev[ok, 3] + a[ok] * a[ok]
                dev[ok, 4] = dev[ok, 4] + b[ok]
                dev[ok, 5] = dev[ok, 5] + b[ok] * b[ok]
            self.n += ok
            self.n_skipped += ~ok
        return self

    def arrays(self):
        return {k: getattr(self, k).copy() for k in FIELDS}


def moments(n, pivot, s1, s2):
    """(mean, variance with ddof = 1) from a pivot and the sums about it, formed in ``np.longdouble``; ``n`` (R,) broadcasts over
    trailing axes.  NaN where n < 1 (mean) or n < 2 (variance)."""
    ld = np.longdouble
    n = np.asarray(n)
    shape = n.shape + (1,) * (np.ndim(s1) - n.ndim)
    nn = n.astype(ld).reshape(shape)
    p, a, b = (np.asarray(v, dtype=ld) for v in (pivot, s1, s2))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = p + a / nn
        var = (b - a * a / nn) / (nn - 1)
    mean, var = mean.astype(float), var.astype(float)
    few1, few2 = np.broadcast_to((n < 1).reshape(shape), mean.shape), np.broadcast_to((n < 2).reshape(shape), var.shape)
    mean[few1] = np.nan
    var[few2] = np.nan
    return mean, var


class Predictive:
    """What ``Chains.predictive`` holds, per problem: ``n``, ``n_skipped`` (R,): the kept samples summed and those skipped because
    their chi2 or lnL was not finite; ``mean``, ``std`` (R, N): the posterior mean and ddof = 1 scatter of the theory vector;
    ``multipoles``: ``{ell: (mean (R, n_s), std (R, n_s))}`` in the fit's ``poles_s`` / ``s`` order; ``mean_chi2``, ``var_chi2``,
    ``mean_lnl``, ``var_lnl`` (R,); ``chi2_at_mean``, ``lnl_at_mean`` (R,): the likelihood at the pooled mean position
    (``Chains.mean``; NaN where there is none); with D = -2 lnL, ``p_d = mean_D - D(mean position)``, ``p_v = var_D / 2`` and
    ``dic = mean_D + p_d``; ``state``: the raw arrays ``pivot_t``, ``sum_t``, ``sum_tt`` (R, N), ``deviance`` (R, 6) - pivot_chi2,
    pivot_lnl, s_chi2, s_chi2sq, s_lnl, s_lnlsq -, ``n``, ``n_skipped`` (R,) and ``held`` (R W, N) as the route that ran the chains
    returns them."""

    def __init__(self, state, poles=None, n_s=None, chi2_at_mean=None, lnl_at_mean=None):
        self.state = {k: np.array(state[k]) for k in FIELDS}
        q = self.state
        self.n, self.n_skipped = q["n"].astype(np.int64), q["n_skipped"].astype(np.int64)
        R = len(self.n)
        self.mean, var = moments(self.n, q["pivot_t"], q["sum_t"], q["sum_tt"])
        with np.errstate(invalid="ignore"):
            self.std = np.sqrt(np.maximum(var, 0.0))                   # (a variance below zero is rounding about a constant entry)
        self.std[np.isnan(var)] = np.nan
        dev = q["deviance"]
        self.mean_chi2, self.var_chi2 = moments(self.n, dev[:, 0], dev[:, 2], dev[:, 3])
        self.mean_lnl, self.var_lnl = moments(self.n, dev[:, 1], dev[:, 4], dev[:, 5])
        self.chi2_at_mean = np.full(R, np.nan) if chi2_at_mean is None else np.array(chi2_at_mean, dtype=float)
        self.lnl_at_mean = np.full(R, np.nan) if lnl_at_mean is None else np.array(lnl_at_mean, dtype=float)
        mean_d = -2.0 * self.mean_lnl
        self.p_d = mean_d - (-2.0 * self.lnl_at_mean)
        self.p_v = (4.0 * self.var_lnl) / 2.0
        self.dic = mean_d + self.p_d
        self.multipoles = {}
        if poles is not None:
            for i, ell in enumerate(np.atleast_1d(poles)):
                cut = slice(i * n_s, (i + 1) * n_s)
                self.multipoles[int(ell)] = (self.mean[:, cut], self.std[:, cut])
