"""Grid posteriors: ``CCFFit.grid_posterior`` and ``Realisations.grid_posterior`` - exact marginals, profile likelihoods and the
evidence of the data vector (R = 1) or of EVERY realisation (R = ``len(rs)``) over one shared regular grid of the sampled
parameters, reduced where the likelihoods are produced (``vk_grid_run``, ``include/victor_hip.h``).

The fits have two to four sampled parameters.  In so few dimensions a grid has no burn-in, no R-hat, no autocorrelation time and
no ladder bias: it is the yardstick for the chains, the histograms counted from them, Laplace / Fisher and the
thermodynamic-integration evidence.  Against mocks it is also the cheapest product: a grid point's theory vector is computed once
and compared with every realisation (the cross mode of ``Realisations.log_likelihood``), so R mocks cost G theory evaluations.

**The grid.**  The sampled parameters of the cobaya block are the axes, in sampled order; axis j has ``n_j`` cells over ``(a_j,
b_j)`` (the prior box, or ``ranges[name]`` inside it) and its nodes are the cell midpoints, formed ONCE on the host as ``a + (k +
0.5) * ((b - a) / n)``: the host arrays are the definition, the device looks nodes up.  Flat index g decodes row-major (the last
sampled parameter varies fastest).

**The definition** (:func:`run_definition`; ``device=False`` runs it over ``log_likelihood_batch`` /
``Realisations.log_likelihood`` or an ``evaluate`` callable, ``device=True`` reproduces it in kernels).  The grid goes through in
chunks ``[c chunk, min((c + 1) chunk, G))``, in order.  For chunk c and problem r, with M the running maximum (-inf at first):

1. ``lnpost[g] = lnl[g][r] + lnprior[g]``, one addition (without a prior ``lnl`` itself); a value that is not finite counts as
   -inf (the evaluators report a failed point as -inf).
2. ``M' = max(M, max_g lnpost[g])``; ``arg_max`` moves only on a strict increase, to the smallest such g of the chunk.  If ``M'``
   is -inf nothing else happens.
3. If ``M' > M`` every accumulator of r (``total``, ``m1``, ``m2``) is multiplied by ``exp(M - M')`` (0 stays 0; ``M = -inf``
   multiplies by 0), then ``M = M'``.
4. Every accumulator cell adds ``exp(lnpost[g] - M)`` for the chunk's g that belong to it, IN INCREASING g, one at a time,
   starting from the accumulator's value.  No pairwise or tree sums: the order is the definition.
5. ``p1``, ``p2`` take maxima of lnpost; ``n_finite`` counts.

So maxima, arg max and counts do not depend on ``chunk``, sums depend on it through rounding only, and for a given ``chunk`` the
bytes depend on nothing else.  With a prior the Gaussian's own midpoint sum over the same grid (``lnpost = lnprior``) goes through
the same steps as one more problem: it normalises the prior over the grid's range in ``ln_evidence``.

:class:`GridPosterior` derives everything else on the host, for both routes alike.
"""

import ctypes as C

import numpy as np

from . import _native as N
from .fitting import _Sampled, blend_opts
from .utils import InputError

MAX_AXES = 10
MAX_BINS = 1024          # vkgrid::kMaxBins
MAX_BINS2 = 128          # ... of an axis of a pair
MAX_PAIRS = 45
MAX_POINTS = 1 << 40
MAX_CHUNK = 65536
VALUE_BYTES = 256 << 20  # device-memory budget of the two [chunk][R] arrays of a handle behind the default chunk


class Grid:
    """The axes of a call: ``names``; ``a``, ``b``, ``lo``, ``hi`` (d,) the ranges and the prior box; ``shape``; ``axes[j]``
    the nodes and ``edges[j]`` the cell edges of axis j; ``pairs`` the (ja < jb) index pairs of the 2-D products and
    ``pair_names`` as the caller wrote them; ``G`` the number of points (a Python int)."""

    def __init__(self, names, shape, a, b, lo, hi, pairs, pair_names):
        self.names, self.shape = list(names), tuple(int(n) for n in shape)
        self.a, self.b, self.lo, self.hi = (np.asarray(v, dtype=np.float64) for v in (a, b, lo, hi))
        self.axes = [self.a[j] + (np.arange(n) + 0.5) * ((self.b[j] - self.a[j]) / n) for j, n in enumerate(self.shape)]
        self.edges = [np.linspace(self.a[j], self.b[j], n + 1) for j, n in enumerate(self.shape)]
        self.pairs, self.pair_names = list(pairs), list(pair_names)
        self.G = 1
        for n in self.shape:
            self.G *= n
        self.axis_off = np.concatenate([[0], np.cumsum(self.shape)]).astype(int)
        self.pair_off = np.concatenate([[0], np.cumsum([self.shape[i] * self.shape[j] for i, j in self.pairs])]).astype(int)

    @property
    def d(self):
        return len(self.names)

    @property
    def n1(self):
        return int(self.axis_off[-1])

    @property
    def n2(self):
        return int(self.pair_off[-1])

    def decode(self, g):
        """(len(g), d) node indices of the flat indices ``g``: row-major."""
        return np.stack(np.unravel_index(np.asarray(g, dtype=np.int64), self.shape), axis=-1)

    def points(self, g):
        """(len(g), d) the node values at the flat indices ``g``: looked up, never recomputed."""
        k = self.decode(g)
        return np.stack([self.axes[j][k[:, j]] for j in range(self.d)], axis=-1)


def resolve_grid(who, names, lo, hi, bins, ranges, pairs):
    """The :class:`Grid` of the arguments ``bins``, ``ranges``, ``pairs`` against the sampled ``names`` with box ``lo``, ``hi``;
    every refusal an ``InputError``."""
    names = list(names)
    d = len(names)
    if d > MAX_AXES:
        raise InputError(f"{who}: at most {MAX_AXES} axes ({d} parameters are sampled)")
    given = dict(bins) if isinstance(bins, dict) else {n: bins for n in names}
    unknown = sorted(set(given) - set(names))
    if unknown or set(given) != set(names):
        raise InputError(f"{who}: bins names {unknown or sorted(set(names) - set(given))}: a dict gives every axis, and only axes, "
                         f"a count ({names})")
    shape = []
    for n in names:
        v = given[n]
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= MAX_BINS:
            raise InputError(f"{who}: bins of {n} must be an integer in 1 .. {MAX_BINS}, not {v!r}")
        shape.append(int(v))
    G = 1
    for n in shape:
        G *= n                                                   # (a Python int: no overflow)
    if G > MAX_POINTS:
        raise InputError(f"{who}: the grid has {G} points: at most 2^40")
    a, b = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    ranges = dict(ranges or {})
    for n, r in ranges.items():
        if n not in names:
            raise InputError(f"{who}: ranges names {n}, which is not an axis ({names})")
        j = names.index(n)
        try:
            ra, rb = float(r[0]), float(r[1])
        except (TypeError, ValueError, IndexError):
            raise InputError(f"{who}: the range of {n} must be a pair (a, b)") from None
        if not (np.isfinite(ra) and np.isfinite(rb) and ra < rb):
            raise InputError(f"{who}: the range of {n} needs finite a < b, not ({ra}, {rb})")
        if ra < lo[j] or rb > hi[j]:
            raise InputError(f"{who}: the range of {n} ({ra}, {rb}) leaves its prior box [{lo[j]}, {hi[j]}]")
        a[j], b[j] = ra, rb
    index, pair_names = [], []
    for p in pairs or []:
        try:
            n1, n2 = p
        except (TypeError, ValueError):
            raise InputError(f"{who}: pairs must be a list of name pairs") from None
        if n1 not in names or n2 not in names or n1 == n2:
            raise InputError(f"{who}: the pair ({n1}, {n2}) must name two different axes ({names})")
        j, k = sorted((names.index(n1), names.index(n2)))
        if (j, k) in index:
            raise InputError(f"{who}: the pair ({n1}, {n2}) is given twice")
        if shape[j] > MAX_BINS2 or shape[k] > MAX_BINS2:
            raise InputError(f"{who}: an axis of a pair has at most {MAX_BINS2} bins (({n1}, {n2}): {shape[j]}, {shape[k]})")
        index.append((j, k))
        pair_names.append((n1, n2))
    if len(index) > MAX_PAIRS:
        raise InputError(f"{who}: at most {MAX_PAIRS} pairs, not {len(index)}")
    return Grid(names, shape, a, b, lo, hi, index, pair_names)


def default_chunk(R, G):
    """Grid points per launch when the caller names none: what keeps the two ``[chunk][R]`` arrays of a handle inside
    ``VALUE_BYTES``, at most ``MAX_CHUNK`` and at most the grid."""
    return int(max(1, min(MAX_CHUNK, VALUE_BYTES // (16 * max(int(R), 1)), G)))


class Accumulators:
    """What a run returns per problem (the arrays of ``vk_grid_result``): ``ln_max``, ``arg_max``, ``total``, ``n_finite`` (R,);
    ``m1``, ``p1`` (R, sum n_j); ``m2``, ``p2`` (R, sum_pairs n_a n_b)."""

    def __init__(self, grid, R):
        self.ln_max = np.full(R, -np.inf)
        self.arg_max = np.full(R, -1, dtype=np.int64)
        self.total = np.zeros(R)
        self.n_finite = np.zeros(R, dtype=np.int64)
        self.m1, self.p1 = np.zeros((R, grid.n1)), np.full((R, grid.n1), -np.inf)
        self.m2, self.p2 = np.zeros((R, grid.n2)), np.full((R, grid.n2), -np.inf)


def step_definition(grid, acc, g0, lnpost):
    """Steps 1 - 5 of the module docstring for one chunk: ``lnpost`` (n, R) of the flat indices ``g0 .. g0 + n - 1`` into the
    :class:`Accumulators` ``acc``, in place."""
    lnpost = np.asarray(lnpost, dtype=np.float64)
    lnpost = np.where(np.isfinite(lnpost), lnpost, -np.inf)
    n = len(lnpost)
    acc.n_finite += np.count_nonzero(lnpost > -np.inf, axis=0)
    cmax = lnpost.max(axis=0)
    carg = g0 + np.argmax(lnpost, axis=0)                        # (the first of equal maxima)
    up = cmax > acc.ln_max
    with np.errstate(invalid="ignore"):
        factor = np.where(up, np.exp(acc.ln_max - cmax), 1.0)
    acc.arg_max = np.where(up, carg, acc.arg_max)
    acc.ln_max = np.where(up, cmax, acc.ln_max)
    acc.total = acc.total * factor                               # (a factor of 1.0 changes no bit)
    acc.m1 = acc.m1 * factor[:, None]
    acc.m2 = acc.m2 * factor[:, None]
    live = acc.ln_max > -np.inf
    with np.errstate(invalid="ignore"):
        w = np.where(live, np.exp(lnpost - acc.ln_max), 0.0)
    k = grid.decode(g0 + np.arange(n))
    for i in range(n):                                           # one addition at a time, in increasing g
        wi, vi = w[i], lnpost[i]
        acc.total = acc.total + wi
        for j in range(grid.d):
            c = grid.axis_off[j] + k[i, j]
            acc.m1[:, c] = acc.m1[:, c] + wi
            acc.p1[:, c] = np.maximum(acc.p1[:, c], vi)
        for q, (ja, jb) in enumerate(grid.pairs):
            c = grid.pair_off[q] + k[i, ja] * grid.shape[jb] + k[i, jb]
            acc.m2[:, c] = acc.m2[:, c] + wi
            acc.p2[:, c] = np.maximum(acc.p2[:, c], vi)


def run_definition(grid, R, chunk, values, prior=None):
    """The definition: ``values(x)`` gives lnL ``(n, R)`` (or ``(n,)``: R = 1) at the points ``x`` (n, d) of a chunk; ``R``
    None: whatever the first chunk returns.  Returns ``(Accumulators, prior Accumulators or None)``."""
    acc = None
    pacc = Accumulators(grid, 1) if prior is not None else None
    for g0 in range(0, grid.G, chunk):
        g = np.arange(g0, min(g0 + chunk, grid.G))
        x = grid.points(g)
        lnl = np.asarray(values(x), dtype=np.float64)
        lnl = lnl.reshape(len(g), -1 if R is None else R)
        if acc is None:
            R = lnl.shape[1]
            acc = Accumulators(grid, R)
        if prior is not None:
            lp = prior.lnprior(x)
            lnl = lnl + lp[:, None]
            step_definition(grid, pacc, g0, lp[:, None])
        step_definition(grid, acc, g0, lnl)
    return acc, pacc


class GridPosterior:
    """The posterior of R problems on one grid.

    ``names``; ``axes[name]`` the nodes and ``edges[name]`` the cell edges; ``shape``; ``n_problems``; ``chunk``, ``n_chunks``
    (what the sums' rounding depends on); ``ln_max`` (R,) the largest lnpost and ``best[name]`` (R,) the node attaining it (the
    smallest flat index, ``arg_max``; NaN without a finite node); ``n_finite`` (R,); ``status`` (R,): ``OK`` or ``NO_FINITE``
    (every node failed: ``ln_evidence`` -inf, marginals zeros, profiles -inf, moments NaN-free zeros).  ``raw``: the
    :class:`Accumulators`.

    ``ln_evidence`` (R,): without a prior ``ln_max + log(total) + sum_j log((b_j - a_j) / n_j) - sum_j log(hi_j - lo_j)``, the
    evidence under the block's normalised uniform prior - what ``Laplace.ln_evidence`` and the tempered chains estimate; a
    sub-range integrates only its share of the box.  With a Gaussian prior: ``(ln_max + log(total)) - (prior_ln_max +
    log(prior_total))``, the prior normalised by the same midpoint sum on the same grid."""

    OK, NO_FINITE = 0, 1

    def __init__(self, grid, acc, pacc, chunk):
        self._grid, self.raw = grid, acc
        self.names = list(grid.names)
        self.axes = dict(zip(self.names, grid.axes))
        self.edges = dict(zip(self.names, grid.edges))
        self.shape = grid.shape
        self.n_problems = R = len(acc.ln_max)
        self.chunk, self.n_chunks = int(chunk), -(-grid.G // int(chunk))
        self.ln_max, self.arg_max, self.n_finite = acc.ln_max, acc.arg_max, acc.n_finite
        self.status = np.where(acc.n_finite > 0, self.OK, self.NO_FINITE).astype(np.int32)
        ok = self.status == self.OK
        self._total = np.where(ok, acc.total, 1.0)               # (never divided by zero)
        self._ok = ok
        self._h = (grid.b - grid.a) / np.array(grid.shape)
        k = grid.decode(np.where(ok, acc.arg_max, 0))
        self.best = {n: np.where(ok, grid.axes[j][k[:, j]], np.nan) for j, n in enumerate(self.names)}
        with np.errstate(divide="ignore"):
            ln_sum = np.where(ok, np.where(ok, acc.ln_max, 0.0) + np.log(self._total), -np.inf)
        if pacc is None:
            self.ln_evidence = ln_sum + np.sum(np.log(self._h)) - np.sum(np.log(grid.hi - grid.lo))
        else:
            self.prior_ln_max, self.prior_total = float(pacc.ln_max[0]), float(pacc.total[0])
            self.ln_evidence = ln_sum - (self.prior_ln_max + np.log(self.prior_total))
        self.ln_evidence = np.where(ok, self.ln_evidence, -np.inf)
        w1 = [self._m1(j) / self._total[:, None] for j in range(grid.d)]
        self.mean = np.stack([w1[j] @ grid.axes[j] for j in range(grid.d)], axis=1)
        self.sigma = np.stack([np.sqrt(np.sum(w1[j] * (grid.axes[j][None, :] - self.mean[:, j, None]) ** 2, axis=1))
                               for j in range(grid.d)], axis=1)
        self.edge_mass = np.stack([np.stack([w1[j][:, 0], w1[j][:, -1]], axis=1) for j in range(grid.d)], axis=1)
        self._reader = None

    def __len__(self):
        return self.n_problems

    def _axis(self, name):
        if name not in self.names:
            raise InputError(f"GridPosterior: {name} is not an axis ({self.names})")
        return self.names.index(name)

    def _m1(self, j):
        return self.raw.m1[:, self._grid.axis_off[j]:self._grid.axis_off[j + 1]]

    def _pair(self, a, b, what):
        """(slot, transposed) of the pair (a, b) among the requested ones."""
        j, k = self._axis(a), self._axis(b)
        key = tuple(sorted((j, k)))
        if j == k or key not in self._grid.pairs:
            raise InputError(f"GridPosterior.{what}: the pair ({a}, {b}) was not requested (pairs={self._grid.pair_names})")
        return self._grid.pairs.index(key), j > k

    def _cells2(self, arr, q, swap):
        ja, jb = self._grid.pairs[q]
        out = arr[:, self._grid.pair_off[q]:self._grid.pair_off[q + 1]].reshape(-1, self.shape[ja], self.shape[jb])
        return np.swapaxes(out, 1, 2) if swap else out

    def marginal(self, name):
        """(R, n_j) the marginal posterior density of ``name`` at its nodes: unit integral over the axis' range."""
        j = self._axis(name)
        return self._m1(j) / (self._total[:, None] * self._h[j])

    def marginal2d(self, a, b):
        """(R, n_a, n_b) the joint marginal density of a requested pair, axis 1 along ``a``."""
        q, swap = self._pair(a, b, "marginal2d")
        ja, jb = self._grid.pairs[q]
        return self._cells2(self.raw.m2, q, swap) / (self._total[:, None, None] * (self._h[ja] * self._h[jb]))

    def _minus_max(self, p):
        shape = (-1,) + (1,) * (p.ndim - 1)
        with np.errstate(invalid="ignore"):
            return np.where(self._ok.reshape(shape), p - np.where(self._ok, self.ln_max, 0.0).reshape(shape), -np.inf)

    def profile(self, name):
        """(R, n_j) the profile of ``name``: max of lnpost over the other axes at each node, minus ``ln_max`` (<= 0)."""
        j = self._axis(name)
        return self._minus_max(self.raw.p1[:, self._grid.axis_off[j]:self._grid.axis_off[j + 1]])

    def profile2d(self, a, b):
        q, swap = self._pair(a, b, "profile2d")
        return self._minus_max(self._cells2(self.raw.p2, q, swap))

    def cov_of(self, a, b):
        """(R,) the posterior covariance of a requested pair, from its 2-D marginal and the 1-D means."""
        q, swap = self._pair(a, b, "cov_of")
        ja, jb = self._grid.pairs[q]
        w = self._cells2(self.raw.m2, q, False) / self._total[:, None, None]
        da = self._grid.axes[ja][None, :] - self.mean[:, ja, None]
        db = self._grid.axes[jb][None, :] - self.mean[:, jb, None]
        return np.einsum("rab,ra,rb->r", w, da, db)

    def _marginals(self, name):
        """The 1-D marginals as the histogram reader of :mod:`victor_amd.marginals` takes them - weights for counts, nothing
        below or above the range - with ``n`` the sum of ``name``'s own cells (the axes' sums differ by rounding)."""
        if self._reader is None:
            from .marginals import Marginals
            m = object.__new__(Marginals)
            m.names = list(self.names)
            m.counts = {n: self._m1(j) for j, n in enumerate(self.names)}
            m.below = {n: np.zeros(self.n_problems) for n in self.names}
            m.above = {n: np.zeros(self.n_problems) for n in self.names}
            m.edges = dict(self.edges)
            self._reader = m
        self._reader.n = np.cumsum(self._m1(self._axis(name)), axis=1)[:, -1]     # (the reader's own running sum: q = 1 is inside)
        return self._reader

    def quantile(self, name, q):
        """(R,) the q-quantile of ``name``, read from its marginal the way ``Marginals.quantile`` reads a histogram (linear inside
        a cell; NaN for a problem without a finite node, as a histogram nothing was kept in)."""
        return self._marginals(name).quantile(name, q)

    def interval(self, name, level=0.68):
        """The equal-tailed interval of ``name``: two (R,) arrays."""
        return self._marginals(name).interval(name, level)

    def median(self, name):
        return self.quantile(name, 0.5)


def grid_posterior(fit, params, bins=32, ranges=None, fixed=None, prior=None, pairs=None, chunk=None, device=True, kwargs=None,
                   realisations=None, evaluate=None):
    """The work of ``CCFFit.grid_posterior`` (``realisations=None``: the fit's data vector, R = 1) and
    ``Realisations.grid_posterior`` (R = the realisations, one shared grid); see the module docstring.  With ``evaluate`` - a
    callable taking a dict of ``(n,)`` arrays (axes and fixed parameters) and returning lnL ``(n,)`` or ``(n, R)`` - in place of
    ``fit`` only the definition route (``device=False``) is possible and no GPU is needed.

    ``params``: the cobaya block, as ``best_fit`` takes it (sampled parameters are the axes, scalars and ``fixed`` values are
    fixed; ``fixed`` values must be scalars); ``bins``: an int or a dict name -> int, 1 .. 1024 each, at most 2^40 points;
    ``ranges``: name -> (a, b) inside the prior box (default the box); ``pairs``: name pairs for the 2-D products (each axis of a
    pair at most 128 bins); ``prior``: a :class:`victor_amd.priors.GaussianPrior` or a list of them; ``chunk``: grid points per
    launch, at most 65536 (default :func:`default_chunk`); ``device=False``: the NumPy definition.  Every argument is checked
    before the first device call.  Returns a :class:`GridPosterior`."""
    who = "grid_posterior"
    kwargs = kwargs or {}
    if evaluate is not None and device:
        raise InputError(f"{who}: an evaluate callable runs the definition route only (device=False)")
    if evaluate is None and fit is None:
        raise InputError(f"{who}: a fit or an evaluate callable is needed")
    from .joint import JointFit
    if isinstance(fit, JointFit):
        raise InputError(f"{who}: joint fits have no grid posterior")
    q = _Sampled(who, "gridded", params, fixed)
    names, fixed_all = q.names, q.fixed_all
    per_block = sorted(n for n in list(names) + list(fixed_all) if "@" in n)
    if per_block:
        raise InputError(f"{who}: per-block parameters ('name@block': {per_block}) have no grid posterior")
    if len(names) > MAX_AXES:
        raise InputError(f"{who}: at most {MAX_AXES} axes ({len(names)} parameters are sampled)")
    if evaluate is None:
        q.check_columns(fit)
        q.check_alpha()
    arrays = sorted(k for k, v in fixed_all.items() if np.ndim(v) > 0)
    if arrays:
        raise InputError(f"{who}: fixed values must be scalars ({arrays} are not)")
    grid = resolve_grid(who, names, q.lo, q.hi, bins, ranges, pairs)
    prior = q.prior(prior, fit)
    if realisations is not None and getattr(realisations, "paired_model", False):
        raise InputError(f"{who}: realisations(paired_model=True) have no cross mode (a point has one theory vector per "
                         "realisation): a grid evaluates every point once")
    if evaluate is None:
        fit_options = q.fit_options(fit, kwargs)
    R = len(realisations) if realisations is not None else 1
    if chunk is None:
        chunk = default_chunk(R, grid.G)
    if isinstance(chunk, bool) or int(chunk) != chunk or not 1 <= int(chunk) <= MAX_CHUNK:
        raise InputError(f"{who}: chunk must be an integer in 1 .. {MAX_CHUNK}, not {chunk!r}")
    chunk = int(chunk)
    fixed_out = {k: float(v) for k, v in fixed_all.items()}

    def batch_of(x):
        batch = dict(fixed_out)
        batch.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names)})
        return batch

    if not device:
        if evaluate is not None:
            R = None                                             # (as many problems as the callable returns columns)

            def values(x):
                return evaluate(batch_of(x))
        elif realisations is not None:
            def values(x):
                return getattr(realisations, "_cross", realisations.log_likelihood)(batch_of(x), **kwargs)[0]
        else:
            def values(x):
                return fit.log_likelihood_batch(batch_of(x), **kwargs)[0]
        acc, pacc = run_definition(grid, R, chunk, values, prior)
        return GridPosterior(grid, acc, pacc, chunk)

    # ---- device
    lib, h, refresh = create_handle(q, fit, realisations, kwargs, fit_options, grid, fixed_out, chunk)
    try:
        if prior is not None:
            rc = lib.vk_grid_set_prior(h, N.as_dp(prior.mu), N.as_dp(prior.pp))
            _check(lib, h, rc, "vk_grid_set_prior")
        if refresh is not None:
            refresh()
        _check(lib, h, lib.vk_grid_run(h, 0, grid.G), "vk_grid_run")
        acc, pacc = read_result(lib, h, grid, R, prior is not None)
    finally:
        lib.vk_grid_destroy(h)
    return GridPosterior(grid, acc, pacc, chunk)


def _check(lib, h, rc, entry):
    if rc != 0:
        msg = (lib.vk_grid_last_error(h) or b"").decode() or f"{entry} failed ({rc})"
        raise (InputError if rc == -1 else N.NativeError)(msg)


def create_handle(q, fit, realisations, kwargs, fit_options, grid, fixed_out, chunk):
    """``(lib, handle, refresh)`` of ``vk_grid_create`` for the grid: the base row from the fixed values (the axes' columns are
    overwritten per point), the nodes, and per epsilon node the host's own ``eps^(-2/3)`` (``vk_epsilon_to_ap``: libm's pow)."""
    model = fit._merged(kwargs)
    fit._check_supported(model)
    batch = dict(fixed_out)
    batch.update({n: np.array([grid.axes[j][0]]) for j, n in enumerate(grid.names)})
    base = np.ascontiguousarray(fit._fit_rows(batch, model), dtype=np.float64)
    cols = np.array([N.ROW_COLUMNS.get(n, N.VK_WALK_EPSILON) for n in grid.names], dtype=np.int32)
    refresh = None
    if realisations is None:
        eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
        opts = eng.make_opts(model, fit_options)
    else:
        _, _, eng, opts = realisations._plan(kwargs)

        def refresh():
            realisations._upload(eng)
    opts = blend_opts(fit, fit_options, opts)
    eps_pow = None
    if "epsilon" in grid.names:
        with np.errstate(invalid="ignore"):
            eps_pow = N.f64(N.epsilon_to_ap(N.f64(grid.axes[grid.names.index("epsilon")]), 1.0)[1])
    i32 = C.POINTER(C.c_int32)
    shape = np.array(grid.shape, dtype=np.int32)
    nodes = N.f64(np.concatenate(grid.axes))
    pairs = np.array(grid.pairs, dtype=np.int32).reshape(-1, 2)
    err = C.create_string_buffer(512)
    h = eng._lib.vk_grid_create(eng._ctx, C.byref(opts), grid.d, cols.ctypes.data_as(i32), shape.ctypes.data_as(i32), N.as_dp(nodes),
                                None if eps_pow is None else N.as_dp(eps_pow), N.as_dp(base), float(fixed_out.get("alpha", 1)),
                                0 if realisations is None else 1, len(pairs), pairs.ctypes.data_as(i32) if len(pairs) else None,
                                chunk, err, len(err))
    if not h:
        msg = err.value.decode()
        raise (N.NativeError if "device memory" in msg else InputError)(msg)
    return eng._lib, h, refresh


def read_result(lib, h, grid, R, with_prior):
    """``(Accumulators, prior Accumulators or None)`` of a completed run (``vk_grid_result``)."""
    acc = Accumulators(grid, R)
    i64 = C.POINTER(C.c_int64)
    pm, pt = C.c_double(0.0), C.c_double(0.0)
    rc = lib.vk_grid_result(h, N.as_dp(acc.ln_max), acc.arg_max.ctypes.data_as(i64), N.as_dp(acc.total),
                            acc.n_finite.ctypes.data_as(i64), N.as_dp(acc.m1), N.as_dp(acc.p1), N.as_dp(acc.m2), N.as_dp(acc.p2),
                            C.cast(C.byref(pm), C.POINTER(C.c_double)), C.cast(C.byref(pt), C.POINTER(C.c_double)))
    _check(lib, h, rc, "vk_grid_result")
    pacc = None
    if with_prior:
        pacc = Accumulators(grid, 1)
        pacc.ln_max[0], pacc.total[0] = pm.value, pt.value
    return acc, pacc
