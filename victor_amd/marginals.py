"""Marginal histograms of the chains of ``sample_chains`` and what is read from them: the ``marginals=`` keyword (``CCFFit``,
``Realisations``, ``JointFit``, ``JointRealisations`` and the ``evaluate=`` route), medians and equal-tailed credible intervals.

With ``keep_chain=False`` a run keeps no history, and the pooled ``mean`` and ``cov`` are a Gaussian read of a posterior that is
cut by the prior box and kinked in beta.  Counting where the chains have been needs no history: every KEPT position (the ones
that enter the moment sums) adds one to a 1-D histogram of every sampled parameter and to the 2-D histograms of chosen pairs, per
problem (the W chains of a problem pool), in 64-bit integers - where the chains run: the step kernels on the device
(``vk_chain_set_marginals``), the NumPy loop on the definition route.  Integer adds commute, so both routes give the same counts.

**The binning rule (one rule, three compilers).**  Parameter j has a range ``[a_j, b_j]`` (default: its prior box) and ``n``
bins; ``inv_j = n / (b_j - a_j)`` is one IEEE division, made once.  A value ``v < a_j`` counts "below" (slot 0), ``v > b_j``
"above" (slot n + 1), any other goes to slot ``1 + min(n - 1, int((v - a_j) * inv_j))``: ``v == b_j`` lands in the last bin.
One subtraction, one multiplication, one truncation - nothing a compiler could fuse -, so :func:`slots` here,
``victor_amd/csrc/vk_marginals.h`` under hipcc (the step kernels) and under g++ (the CPU tests) choose the same slot from the same
bits.  A sample enters the 2-D histogram of a pair only when it lies inside BOTH ranges, in the cell of its two bins by the same
rule with ``bins2d`` bins (:func:`cells`).
"""

import numpy as np

from .utils import InputError

MAX_BINS, MAX_BINS_2D, MAX_PAIRS = 1024, 128, 45
DEFAULT_BINS, DEFAULT_BINS_2D = 128, 32


def inverse_width(n, a, b):
    """``n / (b - a)``: the one division of a range."""
    return float(n) / (np.asarray(b, dtype=np.float64) - np.asarray(a, dtype=np.float64))


def bins(v, a, inv, n):
    """The bin, in 0 .. n - 1, of values inside ``[a, b]``."""
    t = (np.asarray(v, dtype=np.float64) - a) * inv
    with np.errstate(invalid="ignore"):
        return np.minimum(n - 1, t.astype(np.int64))


def slots(v, a, b, n, inv=None):
    """The slot of every value of ``v`` among the n + 2 slots of a 1-D histogram over ``[a, b]`` (module docstring)."""
    v = np.asarray(v, dtype=np.float64)
    inv = inverse_width(n, a, b) if inv is None else inv
    below, above = v < a, ~(v <= b)
    inner = 1 + bins(np.where(below | above, a, v), a, inv, n)
    return np.where(below, 0, np.where(above, n + 1, inner))


def cells(vj, aj, bj, vk, ak, bk, n, invj=None, invk=None):
    """The cell ``bin_j * n + bin_k`` of every sample ``(vj, vk)`` in a pair's n x n histogram, -1 outside either range."""
    vj, vk = np.asarray(vj, dtype=np.float64), np.asarray(vk, dtype=np.float64)
    invj = inverse_width(n, aj, bj) if invj is None else invj
    invk = inverse_width(n, ak, bk) if invk is None else invk
    inside = ~(vj < aj) & (vj <= bj) & ~(vk < ak) & (vk <= bk)
    at = bins(np.where(inside, vj, aj), aj, invj, n) * n + bins(np.where(inside, vk, ak), ak, invk, n)
    return np.where(inside, at, -1)


class Binning:
    """The ``marginals=`` argument resolved against the sampled parameters: ``names``, ``n_bins``, ``a``, ``b`` (d,), ``inv``,
    ``inv2`` (d,), ``pairs`` (n_pairs, 2) indices with j < k, ``pair_names`` as the caller named them and ``n_bins2``."""

    def __init__(self, names, n_bins, a, b, pairs, pair_names, n_bins2):
        self.names, self.n_bins, self.n_bins2 = list(names), int(n_bins), int(n_bins2)
        self.a, self.b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        self.inv, self.inv2 = inverse_width(self.n_bins, self.a, self.b), inverse_width(self.n_bins2, self.a, self.b)
        self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        self.pair_names = list(pair_names)

    def zeros(self, R):
        """Empty histograms of R problems: ``h1`` (R, d, n_bins + 2), ``h2`` (R, n_pairs, n_bins2, n_bins2)."""
        return (np.zeros((R, len(self.names), self.n_bins + 2), dtype=np.int64),
                np.zeros((R, len(self.pairs), self.n_bins2, self.n_bins2), dtype=np.int64))

    def add(self, h1, h2, x, W):
        """Count the positions ``x`` (C, d) of C = R W chains, chain c in problem c // W: the rule in NumPy."""
        C_ = len(x)
        problem = np.arange(C_) // W
        for j in range(len(self.names)):
            np.add.at(h1[:, j], (problem, slots(x[:, j], self.a[j], self.b[j], self.n_bins, self.inv[j])), 1)
        flat = h2.reshape(h2.shape[0], h2.shape[1], self.n_bins2 * self.n_bins2)       # (a view: h2 is contiguous)
        for p, (j, k) in enumerate(self.pairs):
            at = cells(x[:, j], self.a[j], self.b[j], x[:, k], self.a[k], self.b[k], self.n_bins2, self.inv2[j], self.inv2[k])
            ok = at >= 0
            np.add.at(flat[:, p], (problem[ok], at[ok]), 1)


def resolve_marginals(marginals, who, names, lo, hi):
    """The :class:`Binning` of a ``marginals=`` argument (None for None or False) against the sampled ``names`` with box ``lo``,
    ``hi``; every refusal is an :class:`InputError`, raised before any evaluation."""
    if marginals is None or marginals is False:
        return None
    names = list(names)
    if marginals is True:
        marginals = {}
    if not isinstance(marginals, dict):
        raise InputError(f"{who}: marginals must be None, True or a dict with the keys bins, range, pairs, bins2d")
    opt = dict(marginals)
    n_bins, n_bins2 = opt.pop("bins", DEFAULT_BINS), opt.pop("bins2d", DEFAULT_BINS_2D)
    ranges, pairs = opt.pop("range", None) or {}, opt.pop("pairs", None) or []
    if opt:
        raise InputError(f"{who}: marginals has unknown keys {sorted(opt)} (bins, range, pairs, bins2d)")

    def count(value, what, most):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= most:
            raise InputError(f"{who}: marginals {what} must be an integer in 1..{most}, not {value!r}")
        return int(value)
    n_bins, n_bins2 = count(n_bins, "bins", MAX_BINS), count(n_bins2, "bins2d", MAX_BINS_2D)
    if not isinstance(ranges, dict):
        raise InputError(f"{who}: marginals range must be a dict name -> (a, b)")
    unknown = sorted(n for n in ranges if n not in names)
    if unknown:
        raise InputError(f"{who}: marginals range names parameters that are not sampled: {unknown}")
    a, b = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    for n, r in ranges.items():
        try:
            ra, rb = (float(v) for v in r)
        except (TypeError, ValueError):
            raise InputError(f"{who}: marginals range of {n} must be a pair (a, b)") from None
        a[names.index(n)], b[names.index(n)] = ra, rb
    with np.errstate(over="ignore", invalid="ignore"):
        bad = ~(np.isfinite(a) & np.isfinite(b) & (a < b) & np.isfinite(b - a))
    if np.any(bad):
        j = int(np.argmax(bad))
        raise InputError(f"{who}: marginals range of {names[j]} ({a[j]}, {b[j]}) must be finite with a < b")
    if isinstance(pairs, str):
        if pairs != "all":
            raise InputError(f"{who}: marginals pairs must be a list of (name, name) or 'all', not {pairs!r}")
        pairs = [(names[j], names[k]) for j in range(len(names)) for k in range(j + 1, len(names))]
    index, pair_names = [], []
    for pair in pairs:
        try:
            n1, n2 = pair
        except (TypeError, ValueError):
            raise InputError(f"{who}: marginals pairs must be a list of (name, name), not {pair!r}") from None
        missing = sorted(n for n in (n1, n2) if n not in names)
        if missing:
            raise InputError(f"{who}: marginals pairs names parameters that are not sampled: {missing}")
        j, k = names.index(n1), names.index(n2)
        if j == k:
            raise InputError(f"{who}: marginals pair ({n1}, {n2}) names one parameter twice")
        if (min(j, k), max(j, k)) in index:
            raise InputError(f"{who}: marginals pair ({n1}, {n2}) is given twice")
        index.append((min(j, k), max(j, k)))
        pair_names.append((n1, n2))
    if len(index) > MAX_PAIRS:
        raise InputError(f"{who}: marginals takes at most {MAX_PAIRS} pairs, not {len(index)}")
    return Binning(names, n_bins, a, b, index, pair_names, n_bins2)


class Marginals:
    """The marginal histograms of R problems' chains (``Chains.marginals``).

    ``names``; ``edges[name]`` (n_bins + 1,); ``counts[name]`` (R, n_bins) int64; ``below[name]``, ``above[name]`` (R,): the kept
    samples outside the range; ``counts2d[(n1, n2)]`` (R, bins2d, bins2d), axis 1 along ``n1``, of the samples inside both
    ranges (``edges2d[name]`` (bins2d + 1,)); ``n`` (R,): the kept samples of each problem, all its chains together."""

    def __init__(self, binning, h1, h2, n):
        q = binning
        self.names = list(q.names)
        self.n = np.asarray(n, dtype=np.int64).copy()
        self.edges = {m: np.linspace(q.a[j], q.b[j], q.n_bins + 1) for j, m in enumerate(q.names)}
        self.edges2d = {m: np.linspace(q.a[j], q.b[j], q.n_bins2 + 1) for j, m in enumerate(q.names)}
        self.counts = {m: h1[:, j, 1:-1].copy() for j, m in enumerate(q.names)}
        self.below = {m: h1[:, j, 0].copy() for j, m in enumerate(q.names)}
        self.above = {m: h1[:, j, -1].copy() for j, m in enumerate(q.names)}
        self.counts2d = {}
        for p, ((j, k), (n1, n2)) in enumerate(zip(q.pairs, q.pair_names)):
            self.counts2d[(n1, n2)] = (h2[:, p] if q.names[j] == n1 else np.swapaxes(h2[:, p], 1, 2)).copy()

    def _name(self, name):
        if name not in self.counts:
            raise InputError(f"Marginals: {name} has no histogram ({self.names})")
        return name

    def quantile(self, name, q):
        """(R,) the q-quantile of ``name`` read from its histogram.  With ``t = q n`` and ``cum_k = below + sum_{i<k} counts_i``,
        the first bin k with ``counts_k > 0`` and ``cum_k + counts_k >= t`` holds it, at ``edges[k] + (t - cum_k) / counts_k *
        width``: linear inside the bin, within one bin width of the sample quantile.  NaN when ``t`` falls into the mass below
        or above the range, or when nothing was kept: the result never extrapolates."""
        name, q = self._name(name), float(q)
        if not 0.0 <= q <= 1.0:
            raise InputError(f"Marginals.quantile: q must lie in [0, 1], not {q}")
        counts, below, edges = self.counts[name], self.below[name], self.edges[name]
        out = np.full(len(self.n), np.nan)
        for r in range(len(self.n)):
            t = q * float(self.n[r])
            if self.n[r] == 0 or (below[r] > 0 and t <= below[r]):
                continue
            cum = below[r] + np.concatenate([[0], np.cumsum(counts[r])])
            hit = np.flatnonzero((counts[r] > 0) & (cum[1:] >= t))
            if hit.size:
                k = int(hit[0])
                out[r] = edges[k] + (t - cum[k]) / counts[r, k] * (edges[k + 1] - edges[k])
        return out

    def interval(self, name, level=0.68):
        """The equal-tailed interval: the two quantiles at ``(1 -+ level) / 2``, each (R,)."""
        level = float(level)
        if not 0.0 < level < 1.0:
            raise InputError(f"Marginals.interval: level must lie in (0, 1), not {level}")
        return self.quantile(name, (1.0 - level) / 2.0), self.quantile(name, (1.0 + level) / 2.0)

    def median(self, name):
        return self.quantile(name, 0.5)

    def density(self, name):
        """(R, n_bins) the counts normalised to unit integral over the range (NaN where no sample fell inside it)."""
        name = self._name(name)
        counts, width = self.counts[name], np.diff(self.edges[name])
        total = counts.sum(axis=1, keepdims=True).astype(float)
        with np.errstate(invalid="ignore", divide="ignore"):
            return counts / (total * width)
