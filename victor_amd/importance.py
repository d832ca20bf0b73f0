"""Importance-sampled posteriors: ``CCFFit.importance_posterior`` and ``Realisations.importance_posterior`` - the evidence, the
effective sample size, the moments and the marginal histograms of the data vector (R = 1) or of EVERY realisation (R =
``len(rs)``) from ONE shared sample of a proposal that covers every problem's posterior, reduced where the likelihoods are
produced (``vk_is_run``, ``include/victor_hip.h``).  Joint fits: ``JointRealisations.importance_posterior``
(every joint realisation, ``vk_is_create_joint``; with ``"name@q"`` parameters ``vk_is_create_joint_blocks``) and, for the joint
data vector, :func:`importance_posterior` itself with the ``JointFit`` for ``fit``.

A point's theory vector is computed once and compared with every realisation (the cross mode of ``Realisations.log_likelihood``),
so R mocks cost G theory evaluations - the grid's economy (:mod:`victor_amd.grid`) without its limit of two to four axes and
without its nodes where the posterior is empty.  Gaussian priors work in any dimension a handle allows (d <= 10); there is no
burn-in and no R-hat, and the effective sample size says directly how good the proposal - a Laplace covariance, say - is for
each mock.

**The definition** (:func:`run_definition` / :func:`step_definition`; ``device=False`` runs it over ``log_likelihood_batch`` /
``Realisations.log_likelihood`` or an ``evaluate`` callable, ``device=True`` reproduces it in kernels).

1. *The sample.*  ``z = default_rng([seed, 0]).standard_normal((n, d))`` and ``x = mean + z @ L.T``, ``L`` the Cholesky factor of
   the proposal covariance; with ``dof`` every row of ``z`` is first scaled by ``sqrt(dof / chi2)``, ``chi2 = default_rng([seed,
   1]).chisquare(dof, n)`` (a multivariate Student-t).  ``ln q`` is the closed form of the UNTRUNCATED density, in float64 on the
   host.  Points outside the prior box are dropped on the host, in order: ``n_drawn`` counts all of them, ``n_inside = G`` is what
   remains, and flat index g runs over the kept points.  No truncation constant of q is needed: a dropped point has weight 0 and
   still counts in ``n_drawn``.
2. *Host-side arrays, shared by every problem.*  ``lno[g] = ln prior(x_g) - ln q(x_g)``, with ``ln prior`` the resolved Gaussian
   prior's value (:mod:`victor_amd.priors`: no normalisation constant) or ``-sum_j log(hi_j - lo_j)`` without a prior; ``y = x -
   mean_q``, the centred coordinates the moments use; with epsilon sampled libm's ``eps^(-2/3)`` per point, so that device rows
   equal ``CCFFit._fit_rows`` rows bit for bit; the slot of every point in every 1-D histogram (``bins + 2`` slots: below the
   range, the bins, above it) and its cell in every pair's histogram, by :func:`victor_amd.marginals.slots` / ``cells`` - one
   binning rule, ranges default to the box, a pair has ``min(bins_a, bins_b, 128)`` bins per axis and holds the points inside
   both ranges; and per chunk and axis or pair the chunk's points LISTED BY CELL in increasing g, with the cells' offsets
   (:class:`Lists`).
3. *The step.*  The chunks ``[c chunk, min((c + 1) chunk, G))`` go through in order.  Per chunk and problem r the step is the
   grid's, with the same rounding rules (no fused multiply-add): ``lnpost = lnl + lno[g]``, one addition, a value that is not
   finite counts as -inf; the running maximum M, ``arg_max`` moving on a strict increase to the smallest g; when M rises every
   accumulator is multiplied by ``f = exp(M - M')`` - the sum of squares by f twice, each product rounded -; ``w = exp(lnpost -
   M)``; then the additions run ONE AT A TIME IN INCREASING g: ``total += w``, ``sq += w w``, ``s1[j] += w y_j``, ``s2[j][k] +=
   (w y_j) y_k`` for j <= k, and each histogram slot and pair cell ``+= w`` over its list.  So maxima, arg max and counts do
   not depend on ``chunk``, sums depend on it through rounding only, and two runs give the same bytes.
4. *The prior's own problem.*  Under a prior ``lnpost = lno[g]`` (its total only) rides along as problem R, as in the grid: it
   normalises the prior over the box, by the same sample.  ``ln_evidence = (ln_max + log total) - (prior_ln_max + log
   prior_total)`` with a prior, ``ln_max + log total - log n_drawn`` without one.
5. *The read-out* (:class:`ImportancePosterior`, host, both routes alike).  ``ess = total^2 / sq``; ``max_weight_share = 1 /
   total`` (the largest weight is 1); ``ln_evidence_error = sqrt(sq / total^2 - 1 / n_drawn)``; mean and covariance from ``s1``,
   ``s2`` and the centre; histograms through the reader of :mod:`victor_amd.marginals`; ``outside_mass`` from the below and above
   slots; ``status``: ``OK``, ``LOW_ESS`` (``ess < min_ess``), ``NO_FINITE`` (no point was finite: evidence -inf, no NaN in any
   sum).
6. *Predictive* (``predictive=True``; :class:`SamplePredictive`, ``ip.predictive``): the posterior mean and scatter of the THEORY
   VECTOR of every problem - the band drawn through the data multipoles - and the moments of its deviance, from the weights
   the step already forms and the theory vectors the evaluation already computes: no further theory evaluation, and R mocks
   share the G vectors.  T[g] is the theory vector of kept point g, N entries; of a joint fit the blocks' vectors concatenated
   in block order.  *Pivots*: ``pivot_t = T[0]`` where its entries are finite, else 0 - one vector for all problems -;
   ``pivot_chi2[r] = chi2[0][r]`` and ``pivot_lnl[r] = lnl[0][r]`` where finite, else 0.  *Per chunk*, after the step's own
   rescale and with its weights: every predictive accumulator is multiplied by the chunk's factor f ONCE (each term is linear
   in w); then every point with ``w > 0`` adds, with ``v = T - pivot_t``, ``a = chi2 - pivot_chi2[r]`` and ``b = lnl -
   pivot_lnl[r]``, the terms ``w v`` and ``(w v) v`` to ``pt[r]`` and ``ptt[r]`` (N entries each) and ``w a``, ``(w a) a``, ``w
   b``, ``(w b) b`` to the four deviance sums ``dev[r]`` - each difference and product rounded on its own.  A point with ``w ==
   0`` adds nothing, so no NaN of a failed point can enter a sum.  The prior's own problem keeps no such sums.  The definition
   adds in increasing g; the device adds in a fixed order of its own (``victor_amd/csrc/vk_is_predict.h``), so the two routes
   agree to rounding and each gives the same bytes twice.  The definition route takes its vectors from the batched theory call
   on the rows the likelihood call forms (``theory_vector_batch``; per block and concatenated for a joint fit -
   :func:`victor_amd.fisher.host_vectors`) and chi2 from the call that gives it lnL.  *The read-out*, in ``np.longdouble``:
   ``mean = pivot + pt / total``, ``var = ptt / total - (pt / total)^2`` (weighted, no ddof: as ``cov``); D = -2 lnL carries no
   prior term, the weights do; ``p_d = mean_D - D(mean position)``, ``p_v = var_D / 2``, ``dic = mean_D + p_d``, with the
   likelihood at ``ip.mean[r]`` from one pairs call after the run.  A ``NO_FINITE`` problem reads NaN throughout.
7. *The tail* (``tail=True`` or ``tail={"size": M}``; :class:`SampleTail`, ``ip.tail``): a generalised Pareto fit to every
   problem's M largest weights - its shape k says whether ``ess`` and ``ln_evidence_error``, which are the weights' second
   moment estimated from the same sample, can be believed - and the Pareto-smoothed estimates (PSIS: Vehtari, Simpson, Gelman,
   Yao, Gabry).  The default is ``M = min(floor(0.2 G), ceil(3 sqrt(G)), 4095)``; ``1 <= M <= min(G - 1, 4095)``.
   *Selection* (:class:`Held`; on the device ``vk_is_set_tail`` / ``vk_is_tail``, ``victor_amd/csrc/vk_is_tail.h``): with ``K =
   M + 1`` problem r holds the K largest finite ``lnpost[g][r]`` of the WHOLE sample with their g - rule 3's value: one
   addition, and a value that is not finite is never held.  The order is total: the larger lnpost first, between equal values
   the smaller g first; so the held set and its order are unique, do not depend on ``chunk``, and both routes give the same
   bytes.  ``count[r] = min(K, n_finite[r])``; the prior's own problem keeps no tail.
   *The read-out* (host, both routes alike; the corrected sums in ``np.longdouble``).  The cutoff is the LAST held entry and the
   tail the held entries whose lnpost is strictly above its value.  ``count < K``: ``SHORT``; no finite point: ``NO_FINITE``; a
   tail of fewer than 5 entries: ``k = inf`` - in each of the three the smoothed figures equal the raw ones.  Otherwise, with
   ``w = exp(lnpost - ln_max[r])`` (the largest is 1) and the cutoff's weight u, the excesses ``w - u`` in ascending order go
   to :func:`gpd_fit`, the Zhang-Stephens empirical-Bayes fit as PSIS uses it, regularised ``k = (n k + 5) / (n + 10)``; the
   tail's i-th smallest weight (i = 1 .. n) becomes ``min(u + scale expm1(-k log1p(-p_i)) / k, 1)``, ``p_i = (i - 0.5) / n``
   (``k = 0``: the limit ``-scale log1p(-p_i)``), the smoothed values assigned to the tail's points in their order by weight;
   and each of ``total``, ``sq``, ``s1``, ``s2`` of ``ip.raw`` is corrected by ``sum_tail (w'^p - w^p) (1, y_j, y_j y_k)``, p = 1
   (p = 2 for ``sq``), y of the held indices.  ``ess``, ``ln_evidence``, ``ln_evidence_error``, ``mean`` and ``cov`` follow from
   the corrected sums by rule 5's formulas (under a prior with the same prior normalisation), ``max_weight_share`` is the
   largest smoothed weight over the corrected total.  Histograms are not corrected.  ``k_threshold = min(1 - 1 / log10(n_drawn),
   0.7)``; ``HIGH_K``: ``k > k_threshold``.
8. *A proposal per problem* (``proposal`` a :class:`ProposalSet`; ``Realisations.importance_posterior`` alone, ``paired_model=True``
   included; on the device ``vk_is_create_own``, ``victor_amd/csrc/vk_kernel_is_own.h``): where one proposal cannot cover every
   problem's posterior - a mock flagged ``LOW_ESS`` or ``HIGH_K`` - problem r draws n points of its OWN from a proposal of its own,
   its best fit and Laplace covariance say (:meth:`ProposalSet.from_fits`), and is evaluated against realisation r alone: n R
   theory evaluations in pairs mode instead of G.
   *Common random numbers*: ``z`` (with ``dof`` scaled as in rule 1) is drawn ONCE for all problems, ``x[r] = mean_r + z @
   L_r.T``, and ``ln q[r][g]`` is rule 1's closed form with problem r's mean and Cholesky factor.
   *No point is dropped*: index g runs over all n drawn points of every problem and ``n_drawn = n``.  A point of problem r
   outside the box has ``lno[r][g] = -inf`` (rule 3 counts it as not finite), belongs to no histogram list, and is evaluated at
   the problem's centre ``mean_r`` in its place - the host substitutes it before anything travels, so no out-of-box row is ever
   evaluated; ``n_inside[r]`` counts the others.
   *Problem r's sums* are what rules 3 - 5 and 7 give for a one-problem run over its n points: ``y[r] = x[r] - mean_r``, its own
   lists (:class:`OwnLists`), ``lnpost = lnL + lno[r][g]`` and, under a prior, its own prior problem ``lnop[r][g] = lno[r][g]``
   (``prior_ln_max``, ``prior_total`` and ``prior_error`` are (R,) arrays).
   *Chunks*: a chunk holds ``chunk`` consecutive g of every problem; row ``i R + r`` of its evaluation is point ``g0 + i`` of
   problem r against realisation r, in one pairs call - ``Realisations.log_likelihood_pairs``, or the ``evaluate`` callable given
   the batch and, as a second argument, ``which``.  The default chunk is ``max(1, min(n, 65536 // R))``; ``chunk R <= 65536`` and
   ``n R <= 2^24``.  *The read-out* is rule 5's with the per-problem centre and prior normalisation, ``tail`` rule 7's with ``y``
   taken from the problem's own sample.  ``predictive=True``, joint fits and a caller's own ``sample`` are refused here.
"""

import ctypes as C
import math

import numpy as np

from . import _native as N
from .fitting import _Sampled, blend_opts
from .grid import MAX_CHUNK, default_chunk
from .marginals import Marginals, cells, slots
from .priors import resolve_prior, tri
from .utils import InputError

MAX_AXES = 10
MAX_BINS = 1024          # vkis::kMaxBins
MAX_BINS2 = 128          # ... of an axis of a pair
MAX_PAIRS = 45
MAX_POINTS = 1 << 24     # vkis::kMaxPoints
MAX_OFFSETS = 1 << 27    # vkis::kMaxOffsets


class GaussianProposal:
    """The shared proposal: a multivariate normal over ``names`` with ``mean`` (d,) and ``cov`` (d, d), or with ``dof=k`` the
    multivariate Student-t of k degrees of freedom with that location and scale matrix (heavier tails)."""

    def __init__(self, names, mean, cov, dof=None):
        if isinstance(names, str):
            names = [names]
        self.names = [str(n) for n in names]
        d = len(self.names)
        if d < 1 or len(set(self.names)) != d:
            raise InputError("GaussianProposal: names must be different parameters, at least one")
        self.mean = np.atleast_1d(np.asarray(mean, dtype=np.float64))
        self.cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
        if self.mean.shape != (d,) or not np.all(np.isfinite(self.mean)):
            raise InputError(f"GaussianProposal: mean must hold {d} finite values, one per name")
        if self.cov.shape != (d, d) or not np.all(np.isfinite(self.cov)) or not np.allclose(self.cov, self.cov.T, rtol=1e-12, atol=0.0):
            raise InputError(f"GaussianProposal: cov must be a finite symmetric ({d}, {d}) matrix")
        self.cov = 0.5 * (self.cov + self.cov.T)
        try:
            self.chol = np.linalg.cholesky(self.cov)
        except np.linalg.LinAlgError:
            raise InputError("GaussianProposal: cov is not positive definite") from None
        if dof is not None and (isinstance(dof, bool) or not np.isfinite(dof) or not dof > 0):
            raise InputError(f"GaussianProposal: dof must be None or a number > 0, not {dof!r}")
        self.dof = None if dof is None else float(dof)

    def __repr__(self):
        return f"GaussianProposal({self.names}, mean={self.mean.tolist()}, dof={self.dof})"

    @classmethod
    def from_fits(cls, bf, lap=None, inflate=2.0, dof=None):
        """The proposal pooled over the converged problems of a :class:`victor_amd.fitting.BestFit`: the mean of their best fits,
        and for covariance their scatter (if more than one) plus the mean of ``lap.cov`` over the same problems (a
        :class:`victor_amd.laplace.Laplace`, if given; its problems without a finite covariance are left out), times ``inflate``."""
        ok = np.asarray(bf.status) == bf.CONVERGED
        if not np.any(ok):
            raise InputError("GaussianProposal.from_fits: no problem of the best fit converged")
        if not np.isfinite(inflate) or not inflate > 0:
            raise InputError(f"GaussianProposal.from_fits: inflate must be > 0, not {inflate!r}")
        x = np.asarray(bf.x, dtype=np.float64)[ok]
        d = x.shape[1]
        cov = np.zeros((d, d))
        if len(x) > 1:
            cov = cov + np.atleast_2d(np.cov(x, rowvar=False))
        if lap is not None:
            if list(lap.names) != list(bf.names) or len(lap.cov) != len(bf.x):
                raise InputError("GaussianProposal.from_fits: lap must be the Laplace of the same best fit")
            c = np.asarray(lap.cov, dtype=np.float64)[ok]
            c = c[np.all(np.isfinite(c), axis=(1, 2))]
            if not len(c):
                raise InputError("GaussianProposal.from_fits: no converged problem has a finite Laplace covariance")
            cov = cov + c.mean(axis=0)
        if not np.any(cov):
            raise InputError("GaussianProposal.from_fits: one problem and no lap: nothing gives a covariance")
        return cls(bf.names, x.mean(axis=0), float(inflate) * cov, dof)

    def ordered(self, who, names):
        """``(mean, chol)`` in the order of the sampled ``names``: the proposal names exactly them."""
        if set(self.names) != set(names):
            raise InputError(f"{who}: the proposal names {self.names}, the sampled parameters are {list(names)}")
        at = [self.names.index(n) for n in names]
        cov = self.cov[np.ix_(at, at)]
        return self.mean[at], np.linalg.cholesky(cov)

    @staticmethod
    def standard(d, dof, n, seed):
        """(n, d) standard normal rows, with ``dof`` scaled to Student-t rows: the random numbers of rule 1."""
        z = np.random.default_rng([seed, 0]).standard_normal((n, d))
        if dof is not None:
            chi2 = np.random.default_rng([seed, 1]).chisquare(dof, n)
            z = z * np.sqrt(dof / chi2)[:, None]
        return z

    @staticmethod
    def draw(mean, chol, dof, n, seed):
        """(n, d) points: rule 1 of the module docstring."""
        return mean + GaussianProposal.standard(len(mean), dof, n, seed) @ chol.T

    @staticmethod
    def ln_density(x, mean, chol, dof):
        """(n,) ln q of the untruncated density at ``x`` (n, d)."""
        d = len(mean)
        z = np.linalg.solve(chol, (np.asarray(x, dtype=np.float64) - mean).T)
        q = np.sum(z * z, axis=0)
        ln_det = float(np.sum(np.log(np.diag(chol))))
        if dof is None:
            return -0.5 * q - ln_det - 0.5 * d * math.log(2.0 * math.pi)
        return (math.lgamma(0.5 * (dof + d)) - math.lgamma(0.5 * dof) - 0.5 * d * math.log(dof * math.pi) - ln_det
                - 0.5 * (dof + d) * np.log1p(q / dof))


class ProposalSet:
    """A proposal PER PROBLEM (rule 8 of the module docstring): over ``names`` problem r draws from the multivariate normal - with
    ``dof=k`` the multivariate Student-t - of mean ``mean[r]`` (``mean``: (R, d)) and covariance ``cov[r]`` (``cov``: (R, d, d)).
    ``len(qs)`` is R; ``qs.take(index)`` the sub-set of the listed problems; ``pooled`` (R,) bool: the problems whose proposal
    :meth:`from_fits` took from the pooled fit instead of their own."""

    def __init__(self, names, mean, cov, dof=None):
        if isinstance(names, str):
            names = [names]
        self.names = [str(n) for n in names]
        d = len(self.names)
        if d < 1 or len(set(self.names)) != d:
            raise InputError("ProposalSet: names must be different parameters, at least one")
        self.mean = np.array(mean, dtype=np.float64)
        self.cov = np.array(cov, dtype=np.float64)
        if self.mean.ndim != 2 or self.mean.shape[1] != d or not len(self.mean):
            raise InputError(f"ProposalSet: mean must be (R, {d}), one row per problem and one value per name")
        R = len(self.mean)
        if self.cov.shape != (R, d, d):
            raise InputError(f"ProposalSet: cov must be ({R}, {d}, {d}), one matrix per problem")
        self.chol = np.empty_like(self.cov)
        for r in range(R):
            if not np.all(np.isfinite(self.mean[r])):
                raise InputError(f"ProposalSet: the mean of problem {r} is not finite")
            if not np.all(np.isfinite(self.cov[r])):
                raise InputError(f"ProposalSet: the covariance of problem {r} is not finite")
            if not np.allclose(self.cov[r], self.cov[r].T, rtol=1e-12, atol=0.0):
                raise InputError(f"ProposalSet: the covariance of problem {r} is not symmetric")
            self.cov[r] = 0.5 * (self.cov[r] + self.cov[r].T)
            try:
                self.chol[r] = np.linalg.cholesky(self.cov[r])
            except np.linalg.LinAlgError:
                raise InputError(f"ProposalSet: the covariance of problem {r} is not positive definite") from None
        if dof is not None and (isinstance(dof, bool) or not np.isfinite(dof) or not dof > 0):
            raise InputError(f"ProposalSet: dof must be None or a number > 0, not {dof!r}")
        self.dof = None if dof is None else float(dof)
        self.pooled = np.zeros(R, dtype=bool)

    def __len__(self):
        return len(self.mean)

    def __repr__(self):
        return f"ProposalSet({self.names}, {len(self)} problems, dof={self.dof})"

    def take(self, index):
        """The proposals of the problems ``index`` (integers, or an (R,) bool mask), in that order: what goes with
        ``fit.realisations(numbers)`` when only some mocks are proposed again."""
        index = np.atleast_1d(np.asarray(index))
        if index.dtype == bool:
            if index.shape != (len(self),):
                raise InputError(f"ProposalSet.take: a mask must have one entry per problem ({len(self)})")
            index = np.flatnonzero(index)
        if index.ndim != 1 or not len(index) or not np.issubdtype(index.dtype, np.integer):
            raise InputError("ProposalSet.take: index must be a non-empty list of problem numbers, or a bool mask")
        if np.any(index < 0) or np.any(index >= len(self)):
            raise InputError(f"ProposalSet.take: problem numbers must lie in 0 .. {len(self) - 1}")
        out = ProposalSet(self.names, self.mean[index], self.cov[index], self.dof)
        out.pooled = self.pooled[index].copy()
        return out

    @classmethod
    def from_fits(cls, bf, lap, inflate=2.0, dof=None):
        """Problem r's own best fit and Laplace covariance: mean ``bf.x[r]``, covariance ``inflate * lap.cov[r]``.  A problem
        that did not converge, or whose Laplace covariance is not finite and positive definite, takes the pooled proposal
        ``GaussianProposal.from_fits(bf, lap, inflate, dof)`` instead and is marked in ``pooled``.  Refused, as the pooled
        proposal is, when no problem converged."""
        pool = GaussianProposal.from_fits(bf, lap, inflate, dof)
        if lap is None:
            raise InputError("ProposalSet.from_fits: lap, the Laplace of the best fit, gives the covariances")
        x = np.asarray(bf.x, dtype=np.float64)
        cov = float(inflate) * np.asarray(lap.cov, dtype=np.float64)
        bad = np.asarray(bf.status) != bf.CONVERGED
        bad |= ~np.all(np.isfinite(cov), axis=(1, 2)) | ~np.all(np.isfinite(x), axis=1)
        for r in np.flatnonzero(~bad):
            try:
                np.linalg.cholesky(0.5 * (cov[r] + cov[r].T))
            except np.linalg.LinAlgError:
                bad[r] = True
        mean, cov = x.copy(), 0.5 * (cov + np.swapaxes(cov, 1, 2))
        mean[bad], cov[bad] = pool.mean, pool.cov
        out = cls(bf.names, mean, cov, dof)
        out.pooled = bad
        return out

    def ordered(self, who, names):
        """``(mean (R, d), chol (R, d, d))`` in the order of the sampled ``names``: the set names exactly them."""
        if set(self.names) != set(names):
            raise InputError(f"{who}: the proposals name {self.names}, the sampled parameters are {list(names)}")
        at = [self.names.index(n) for n in names]
        cov = self.cov[:, at][:, :, at]
        return np.ascontiguousarray(self.mean[:, at]), np.linalg.cholesky(cov)


class Layout:
    """The histograms of a call: ``names``; ``n_bins`` (d,); ``a``, ``b`` the ranges and ``lo``, ``hi`` the prior box; ``edges[j]``;
    ``pairs`` the (ja < jb) index pairs, ``pair_names`` as the caller wrote them and ``pair_bins`` their bins per axis;
    ``cell_off`` (d + n_pairs + 1,): the first cell of every list - the axes (``n_bins + 2`` cells each), then the pairs."""

    def __init__(self, names, n_bins, a, b, lo, hi, pairs, pair_names):
        self.names, self.n_bins = list(names), [int(n) for n in n_bins]
        self.a, self.b, self.lo, self.hi = (np.asarray(v, dtype=np.float64) for v in (a, b, lo, hi))
        self.edges = [np.linspace(self.a[j], self.b[j], n + 1) for j, n in enumerate(self.n_bins)]
        self.pairs, self.pair_names = list(pairs), list(pair_names)
        self.pair_bins = [min(self.n_bins[i], self.n_bins[j], MAX_BINS2) for i, j in self.pairs]
        counts = [n + 2 for n in self.n_bins] + [m * m for m in self.pair_bins]
        self.cell_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    @property
    def d(self):
        return len(self.names)

    @property
    def n_lists(self):
        return self.d + len(self.pairs)

    @property
    def n1(self):
        return int(self.cell_off[self.d])

    @property
    def n2(self):
        return int(self.cell_off[-1] - self.cell_off[self.d])

    def cells_of(self, x):
        """(n_lists, n) the cell of every point of ``x`` (n, d) in every list: the slot 0 .. bins + 1 of an axis, the cell of a
        pair or -1 outside either of its ranges."""
        out = np.empty((self.n_lists, len(x)), dtype=np.int64)
        for j in range(self.d):
            out[j] = slots(x[:, j], self.a[j], self.b[j], self.n_bins[j])
        for q, (ja, jb) in enumerate(self.pairs):
            out[self.d + q] = cells(x[:, ja], self.a[ja], self.b[ja], x[:, jb], self.a[jb], self.b[jb], self.pair_bins[q])
        return out


def resolve_layout(who, names, lo, hi, bins, ranges, pairs):
    """The :class:`Layout` of the arguments ``bins``, ``ranges``, ``pairs`` against the sampled ``names`` with box ``lo``, ``hi``;
    every refusal an ``InputError``."""
    names = list(names)
    given = dict(bins) if isinstance(bins, dict) else {n: bins for n in names}
    if set(given) != set(names):
        raise InputError(f"{who}: bins names {sorted(set(given) ^ set(names))}: a dict gives every sampled parameter, and only those, "
                         f"a count ({names})")
    n_bins = []
    for n in names:
        v = given[n]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or not 1 <= int(v) <= MAX_BINS:
            raise InputError(f"{who}: bins of {n} must be an integer in 1 .. {MAX_BINS}, not {v!r}")
        n_bins.append(int(v))
    a, b = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    for n, r in dict(ranges or {}).items():
        if n not in names:
            raise InputError(f"{who}: ranges names {n}, which is not sampled ({names})")
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
            raise InputError(f"{who}: the pair ({n1}, {n2}) must name two different sampled parameters ({names})")
        j, k = sorted((names.index(n1), names.index(n2)))
        if (j, k) in index:
            raise InputError(f"{who}: the pair ({n1}, {n2}) is given twice")
        index.append((j, k))
        pair_names.append((n1, n2))
    if len(index) > MAX_PAIRS:
        raise InputError(f"{who}: at most {MAX_PAIRS} pairs, not {len(index)}")
    return Layout(names, n_bins, a, b, lo, hi, index, pair_names)


class Sample:
    """The kept points of a call and what every problem shares: ``x`` (G, d); ``centre`` (d,) and ``y = x - centre``; ``lno``
    (G,); ``lnop`` (G,) the prior's own lnpost, or None without a prior; ``n_drawn``; ``G = n_inside``."""

    def __init__(self, x, centre, lnq, n_drawn, lo, hi, prior):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.centre = np.asarray(centre, dtype=np.float64)
        self.y = np.ascontiguousarray(self.x - self.centre)
        self.n_drawn, self.G = int(n_drawn), len(self.x)
        lnq = np.asarray(lnq, dtype=np.float64)
        if prior is not None:
            self.lno = prior.lnprior(self.x) - lnq
            self.lnop = self.lno
        else:
            self.lno = -np.sum(np.log(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))) - lnq
            self.lnop = None
        self.lno = np.ascontiguousarray(self.lno)

    own = False

    @property
    def n_inside(self):
        return self.G

    def points(self, at):
        """(R, d) the points ``at`` (R,), one per problem."""
        return self.x[at]

    def held_y(self, index):
        """(R, K, d) the centred coordinates of the held points ``index`` (R, K)."""
        return self.y[index]

    def prior_error(self):
        """Rule 5's standard error of the prior's own normalisation."""
        b = np.exp(self.lnop - self.lnop.max())
        return float(np.sqrt(max(np.sum(b * b) / np.sum(b) ** 2 - 1.0 / self.n_drawn, 0.0)))


class OwnSample:
    """Rule 8's sample, n points per problem: ``x`` (n, R, d), a point outside the box replaced by its problem's centre;
    ``centre`` (R, d) and ``y = x - centre``; ``inside`` (n, R) and ``n_inside`` (R,); ``lno`` (n, R), -inf outside the box;
    ``lnop`` the same array under a prior, else None; ``n_drawn = G = n``."""

    own = True

    def __init__(self, x, centre, lnq, lo, hi, prior):
        x = np.asarray(x, dtype=np.float64)
        self.centre = np.ascontiguousarray(centre, dtype=np.float64)
        self.inside = np.all((x >= lo) & (x <= hi), axis=2)
        self.n_inside = np.count_nonzero(self.inside, axis=0).astype(np.int64)
        self.x = np.ascontiguousarray(np.where(self.inside[:, :, None], x, self.centre[None, :, :]))
        self.y = np.ascontiguousarray(self.x - self.centre[None, :, :])
        self.n_drawn = self.G = len(x)
        self.R = x.shape[1]
        lnq = np.asarray(lnq, dtype=np.float64)
        if prior is not None:
            lno = prior.lnprior(self.x) - lnq
        else:
            lno = -np.sum(np.log(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64))) - lnq
        lno[~self.inside] = -np.inf
        self.lno = np.ascontiguousarray(lno)
        self.lnop = self.lno if prior is not None else None

    def points(self, at):
        return self.x[at, np.arange(self.R)]

    def held_y(self, index):
        return self.y[index, np.arange(self.R)[:, None]]

    def prior_error(self):
        top = self.lnop.max(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            b = np.exp(self.lnop - np.where(np.isfinite(top), top, 0.0))
            out = np.sqrt(np.maximum(np.sum(b * b, axis=0) / np.sum(b, axis=0) ** 2 - 1.0 / self.n_drawn, 0.0))
        return np.where(np.isfinite(top), out, np.inf)


class Lists:
    """Rule 2's lists: ``entries`` (n_lists, G) int32 - list l's segment of chunk c starts at ``c chunk`` and names the chunk's
    points (g - c chunk) cell by cell, in increasing g inside a cell - and ``offsets`` (n_chunks, cells + n_lists) int32: per
    chunk, list after list, one offset more than the list has cells."""

    def __init__(self, layout, x, chunk):
        G = len(x)
        self.chunk, self.n_chunks = int(chunk), -(-G // int(chunk))
        per = int(layout.cell_off[-1]) + layout.n_lists
        if self.n_chunks * per > MAX_OFFSETS:
            raise InputError(f"importance_posterior: {self.n_chunks} chunks x {per} cell offsets are more than 2^27: take a larger "
                             "chunk or fewer bins and pairs")
        self.entries = np.zeros((layout.n_lists, G), dtype=np.int32)
        self.offsets = np.zeros((self.n_chunks, per), dtype=np.int32)
        where = layout.cells_of(x)
        for c in range(self.n_chunks):
            g0 = c * self.chunk
            for l in range(layout.n_lists):
                s = where[l, g0:g0 + self.chunk]
                inside = np.flatnonzero(s >= 0)
                order = inside[np.argsort(s[inside], kind="stable")]             # by cell, increasing g inside a cell
                self.entries[l, g0:g0 + len(order)] = order
                K = int(layout.cell_off[l + 1] - layout.cell_off[l])
                at = int(layout.cell_off[l]) + l
                self.offsets[c, at + 1:at + K + 1] = np.cumsum(np.bincount(s[inside], minlength=K))

    def members(self, layout, c, l):
        """``(entries of the chunk's segment, offsets of list l's cells)``."""
        at = int(layout.cell_off[l]) + l
        K = int(layout.cell_off[l + 1] - layout.cell_off[l])
        g0 = c * self.chunk
        return self.entries[l, g0:g0 + self.chunk], self.offsets[c, at:at + K + 1]


class OwnLists:
    """Rule 2's lists of every problem of an :class:`OwnSample`: ``entries`` (R, n_lists, G) int32 and ``offsets`` (n_chunks, R,
    cells + n_lists) int32, problem r's as :class:`Lists` holds one sample's; a point outside the box is in no list.  Built over
    all problems at once: per chunk and list one stable argsort along the point axis.  ``of(r)``: problem r's, as
    :func:`step_definition` asks for them."""

    def __init__(self, layout, sample, chunk):
        G, R = sample.G, sample.R
        self.chunk, self.n_chunks = int(chunk), -(-G // int(chunk))
        per = int(layout.cell_off[-1]) + layout.n_lists
        if self.n_chunks * R * per > MAX_OFFSETS:
            raise InputError(f"importance_posterior: {self.n_chunks} chunks x {R} problems x {per} cell offsets are more than 2^27: "
                             "take a larger chunk or fewer bins and pairs")
        self.entries = np.zeros((R, layout.n_lists, G), dtype=np.int32)
        self.offsets = np.zeros((self.n_chunks, R, per), dtype=np.int32)
        where = layout.cells_of(sample.x.reshape(G * R, layout.d)).reshape(layout.n_lists, G, R)
        where[:, ~sample.inside] = -1
        problem = np.arange(R)[None, :]
        for c in range(self.n_chunks):
            g0 = c * self.chunk
            for l in range(layout.n_lists):
                K = int(layout.cell_off[l + 1] - layout.cell_off[l])
                s = where[l, g0:g0 + self.chunk]                             # (n, R)
                key = np.where(s >= 0, s, K)                                 # (in no cell: behind every cell)
                order = np.argsort(key, axis=0, kind="stable")               # by cell, increasing g inside a cell
                listed = np.take_along_axis(key, order, axis=0) < K
                self.entries[:, l, g0:g0 + len(s)] = np.where(listed, order, 0).T
                counts = np.bincount((key + problem * (K + 1)).ravel(), minlength=R * (K + 1)).reshape(R, K + 1)[:, :K]
                at = int(layout.cell_off[l]) + l
                self.offsets[c, :, at + 1:at + K + 1] = np.cumsum(counts, axis=1)

    def of(self, r):
        return _ProblemLists(self, r)


class _ProblemLists:
    def __init__(self, lists, r):
        self.lists, self.r, self.chunk, self.n_chunks = lists, r, lists.chunk, lists.n_chunks

    def members(self, layout, c, l):
        at = int(layout.cell_off[l]) + l
        K = int(layout.cell_off[l + 1] - layout.cell_off[l])
        g0 = c * self.chunk
        return self.lists.entries[self.r, l, g0:g0 + self.chunk], self.lists.offsets[c, self.r, at:at + K + 1]


class Sums:
    """What a run returns per problem (the arrays of ``vk_is_result``): ``ln_max``, ``arg_max``, ``n_finite``, ``total``, ``sq``
    (R,); ``s1`` (R, d); ``s2`` (R, d (d + 1) / 2), the packed upper triangle; ``h1`` (R, sum (bins_j + 2)); ``h2`` (R, sum
    m_q^2).  With ``n_theory=N`` (rule 6; the arrays of ``vk_is_predictive``) also ``pivot_t`` (N,), ``pt``, ``ptt`` (R, N),
    ``pivots`` (2, R): pivot_chi2, pivot_lnl, and ``dev`` (4, R): sum w a, (w a) a, w b, (w b) b; without it no such attribute."""

    def __init__(self, layout, R, n_theory=None):
        d = layout.d
        if n_theory is not None:
            self.pivot_t = np.zeros(n_theory)
            self.pt, self.ptt = np.zeros((R, n_theory)), np.zeros((R, n_theory))
            self.pivots, self.dev = np.zeros((2, R)), np.zeros((4, R))
        self.ln_max = np.full(R, -np.inf)
        self.arg_max = np.full(R, -1, dtype=np.int64)
        self.n_finite = np.zeros(R, dtype=np.int64)
        self.total, self.sq = np.zeros(R), np.zeros(R)
        self.s1, self.s2 = np.zeros((R, d)), np.zeros((R, d * (d + 1) // 2))
        self.h1, self.h2 = np.zeros((R, layout.n1)), np.zeros((R, layout.n2))


def _add_in_order(acc, terms):
    """``acc`` (R,) plus the rows of ``terms`` (n, R), one addition at a time in the rows' order (``np.add.accumulate`` is that
    loop)."""
    if not len(terms):
        return acc
    return np.add.accumulate(np.concatenate([acc[None, :], terms], axis=0), axis=0)[-1]


def _pivot(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(np.isfinite(v), v, 0.0)


def _predictive_step(acc, g0, f, w, theory, chi2, lnl):
    """Rule 6 for one chunk: the factors ``f`` (R,) and weights ``w`` (n, R; None: nothing is live yet) of the step just made,
    the points' theory vectors (n, N), chi2 and lnL (n, R)."""
    theory, chi2, lnl = (np.asarray(v, dtype=np.float64) for v in (theory, chi2, lnl))
    if g0 == 0:
        acc.pivot_t = _pivot(theory[0])
        acc.pivots = np.stack([_pivot(chi2[0]), _pivot(lnl[0])])
    acc.pt, acc.ptt, acc.dev = acc.pt * f[:, None], acc.ptt * f[:, None], acc.dev * f[None, :]
    if w is None:
        return
    on = w > 0

    off = ~on

    def in_order(acc, terms):                                    # _add_in_order on an array of the caller's own: no copy
        terms[0] += acc
        return np.add.accumulate(terms, axis=0, out=terms)[-1].copy()

    def add(s1, s2, values, pivot):
        with np.errstate(invalid="ignore", over="ignore"):
            v = values - pivot
            wv = w * v
            wv[off] = 0.0                                        # (a point of weight 0 adds nothing, whatever it holds)
            wvv = wv * v
            wvv[off] = 0.0
        return in_order(s1, wv), in_order(s2, wvv)

    for k in range(theory.shape[1]):
        acc.pt[:, k], acc.ptt[:, k] = add(acc.pt[:, k], acc.ptt[:, k], theory[:, k, None], acc.pivot_t[k])
    acc.dev[0], acc.dev[1] = add(acc.dev[0], acc.dev[1], chi2, acc.pivots[0][None, :])
    acc.dev[2], acc.dev[3] = add(acc.dev[2], acc.dev[3], lnl, acc.pivots[1][None, :])


class Held:
    """Rule 7's selection: per problem the ``K`` largest finite lnpost seen so far and their points - ``lnpost`` (R, K), padded
    with -inf, ``index`` (R, K) int64, padded with -1, ``count`` (R,) - in the total order (larger lnpost first, between equal
    values the smaller g first)."""

    def __init__(self, R, K):
        self.K = int(K)
        self.lnpost = np.full((R, self.K), -np.inf)
        self.index = np.full((R, self.K), -1, dtype=np.int64)
        self.count = np.zeros(R, dtype=np.int64)

    def step(self, g0, lnpost):
        """The chunk's ``lnpost`` (n, R; not finite: -inf) of the points ``g0 .. g0 + n - 1`` joins the held entries.  The held
        entries are in order and belong to earlier points, the chunk's come in increasing g: a stable sort by value keeps
        equal values in increasing g."""
        n, R = lnpost.shape
        v = np.concatenate([self.lnpost, lnpost.T], axis=1)
        g = np.concatenate([self.index, np.broadcast_to(g0 + np.arange(n, dtype=np.int64), (R, n))], axis=1)
        order = np.argsort(-v, axis=1, kind="stable")[:, :self.K]
        self.lnpost = np.take_along_axis(v, order, axis=1)
        self.index = np.take_along_axis(g, order, axis=1)
        self.index[self.lnpost == -np.inf] = -1
        self.count = np.count_nonzero(self.lnpost > -np.inf, axis=1).astype(np.int64)


def step_definition(layout, lists, c, y, acc, g0, lnpost, total_only=False, predictive=None, tail=None):
    """Rule 3 of the module docstring for chunk ``c``: ``lnpost`` (n, R) of the points ``g0 .. g0 + n - 1``, whose centred
    coordinates are ``y`` (n, d), into the :class:`Sums` ``acc``, in place.  ``predictive``: ``(theory (n, N), chi2 (n, R), lnl
    (n, R))`` of the chunk's points, for rule 6 (``acc`` was made with ``n_theory=N``).  ``tail``: the :class:`Held` of rule 7,
    which takes the chunk's values as the step reads them."""
    lnpost = np.asarray(lnpost, dtype=np.float64)
    lnpost = np.where(np.isfinite(lnpost), lnpost, -np.inf)
    if tail is not None:
        tail.step(g0, lnpost)
    acc.n_finite += np.count_nonzero(lnpost > -np.inf, axis=0)
    cmax = lnpost.max(axis=0)
    carg = g0 + np.argmax(lnpost, axis=0)                        # (the first of equal maxima)
    up = cmax > acc.ln_max
    with np.errstate(invalid="ignore"):
        f = np.where(up, np.exp(acc.ln_max - cmax), 1.0)
    acc.arg_max = np.where(up, carg, acc.arg_max)
    acc.ln_max = np.where(up, cmax, acc.ln_max)
    acc.total = acc.total * f                                    # (a factor of 1.0 changes no bit)
    acc.sq = (acc.sq * f) * f
    acc.s1, acc.s2, acc.h1, acc.h2 = acc.s1 * f[:, None], acc.s2 * f[:, None], acc.h1 * f[:, None], acc.h2 * f[:, None]
    live = acc.ln_max > -np.inf
    if not np.any(live):
        if predictive is not None:
            _predictive_step(acc, g0, f, None, *predictive)
        return
    with np.errstate(invalid="ignore"):
        w = np.where(live, np.exp(lnpost - acc.ln_max), 0.0)
    if predictive is not None:
        _predictive_step(acc, g0, f, w, *predictive)
    acc.total = _add_in_order(acc.total, w)
    if total_only:
        return
    d = layout.d
    acc.sq = _add_in_order(acc.sq, w * w)
    for j in range(d):
        wy = w * y[:, j, None]
        acc.s1[:, j] = _add_in_order(acc.s1[:, j], wy)
        for k in range(j, d):
            acc.s2[:, tri(d, j, k)] = _add_in_order(acc.s2[:, tri(d, j, k)], wy * y[:, k, None])
    for l in range(layout.n_lists):
        entries, off = lists.members(layout, c, l)
        h, base = (acc.h1, int(layout.cell_off[l])) if l < d else (acc.h2, int(layout.cell_off[l]) - layout.n1)
        for k in np.flatnonzero(np.diff(off)):
            h[:, base + k] = _add_in_order(h[:, base + k], w[entries[off[k]:off[k + 1]]])


def run_definition(layout, sample, lists, R, values, theory=None, tail=None):
    """The definition: ``values(x)`` gives lnL ``(n, R)`` (or ``(n,)``: R = 1) at the points ``x`` (n, d) of a chunk; ``R`` None:
    whatever the first chunk returns.  Returns ``(Sums, the prior's own Sums or None)``.  With ``theory`` - ``theory(x)`` gives
    the points' theory vectors (n, N) - rule 6 runs along, and ``values(x)`` gives ``(lnL, chi2)``, both (n, R).  With ``tail=K``
    rule 7's selection runs along: the Sums carry the :class:`Held` as ``tail``."""
    acc = None
    pacc = Sums(layout, 1) if sample.lnop is not None else None
    chunk = lists.chunk
    for c in range(lists.n_chunks):
        g0 = c * chunk
        x, y, lno = sample.x[g0:g0 + chunk], sample.y[g0:g0 + chunk], sample.lno[g0:g0 + chunk]
        pred = None
        if theory is None:
            lnl = np.asarray(values(x), dtype=np.float64)
        else:
            lnl, chi2 = (np.asarray(v, dtype=np.float64) for v in values(x))
        lnl = lnl.reshape(len(x), -1 if R is None else R)
        if theory is not None:
            vectors = np.asarray(theory(x), dtype=np.float64).reshape(len(x), -1)
            pred = (vectors, chi2.reshape(lnl.shape), lnl)
        if acc is None:
            R = lnl.shape[1]
            acc = Sums(layout, R, None if pred is None else vectors.shape[1])
            if tail is not None:
                acc.tail = Held(R, tail)
        if pacc is not None:
            step_definition(layout, lists, c, y, pacc, g0, sample.lnop[g0:g0 + chunk, None], total_only=True)
        step_definition(layout, lists, c, y, acc, g0, lnl + lno[:, None], predictive=pred, tail=getattr(acc, "tail", None))
    return acc, pacc


def stack_sums(layout, parts):
    """The :class:`Sums` of R problems from their one-problem Sums, in order (with their :class:`Held`, if they carry one)."""
    acc = Sums(layout, len(parts))
    for name in ("ln_max", "arg_max", "n_finite", "total", "sq", "s1", "s2", "h1", "h2"):
        setattr(acc, name, np.concatenate([getattr(p, name) for p in parts], axis=0))
    if hasattr(parts[0], "tail"):
        acc.tail = held = Held(len(parts), parts[0].tail.K)
        for name in ("lnpost", "index", "count"):
            setattr(held, name, np.concatenate([getattr(p.tail, name) for p in parts], axis=0))
    return acc


def run_definition_own(layout, sample, lists, values, tail=None):
    """Rule 8's definition over an :class:`OwnSample` and its :class:`OwnLists`: ``values(x, which)`` gives lnL ``(m,)`` of the
    rows ``x`` (m, d) against the realisations ``which`` (m,) - a chunk's rows, row ``i R + r`` point ``g0 + i`` of problem r.
    Every problem then takes rule 3's step on its own column, points, lists and (under a prior) prior problem.  Returns ``(Sums,
    the prior problems' Sums or None)``, R problems each; with ``tail=K`` the Sums carry the :class:`Held`."""
    R, d, chunk = sample.R, layout.d, lists.chunk
    accs = [Sums(layout, 1) for _ in range(R)]
    paccs = [Sums(layout, 1) for _ in range(R)] if sample.lnop is not None else None
    if tail is not None:
        for a in accs:
            a.tail = Held(1, tail)
    for c in range(lists.n_chunks):
        g0 = c * chunk
        x = sample.x[g0:g0 + chunk]
        n = len(x)
        which = np.tile(np.arange(R, dtype=np.int32), n)
        lnl = np.asarray(values(x.reshape(n * R, d), which), dtype=np.float64).reshape(n, R)
        with np.errstate(invalid="ignore"):
            lnpost = lnl + sample.lno[g0:g0 + chunk]
        for r in range(R):
            mine = lists.of(r)
            y = sample.y[g0:g0 + chunk, r]
            if paccs is not None:
                step_definition(layout, mine, c, y, paccs[r], g0, sample.lnop[g0:g0 + chunk, r, None], total_only=True)
            step_definition(layout, mine, c, y, accs[r], g0, lnpost[:, r, None], tail=getattr(accs[r], "tail", None))
    return stack_sums(layout, accs), None if paccs is None else stack_sums(layout, paccs)


class SamplePredictive:
    """What ``ImportancePosterior.predictive`` holds (rule 6 of the module docstring), read the way ``Chains.predictive`` is.
    Per problem: ``mean``, ``std`` (R, N) the posterior mean and scatter (weighted, no ddof) of the theory vector, N the joint
    length for a joint fit; ``multipoles``: ``{ell: (mean (R, n_s), std (R, n_s))}`` in the fit's ``poles_s`` / ``s`` order - of
    a joint fit ``multipoles_of(q)`` gives block q's, and ``blocks`` the slices of the joint vector -; ``mean_chi2``,
    ``var_chi2``, ``mean_lnl``, ``var_lnl`` (R,); ``chi2_at_mean``, ``lnl_at_mean`` (R,): the likelihood of problem r at
    ``ip.mean[r]``; with D = -2 lnL (no prior term; the weights include the prior) ``p_d = mean_D - D(mean position)``, ``p_v =
    var_D / 2`` and ``dic = mean_D + p_d``; ``state``: the raw arrays ``pivot_t`` (N,), ``sum_t``, ``sum_tt`` (R, N), ``pivots``
    (2, R), ``deviance`` (4, R) and ``total`` (R,) as the route that ran the sample returns them.  A ``NO_FINITE`` problem reads
    NaN throughout."""

    def __init__(self, acc, ok, blocks, poles, chi2_at_mean=None, lnl_at_mean=None):
        ld = np.longdouble
        R = len(acc.total)
        ok = np.asarray(ok, dtype=bool)
        self.state = {"pivot_t": np.array(acc.pivot_t), "sum_t": np.array(acc.pt), "sum_tt": np.array(acc.ptt),
                      "pivots": np.array(acc.pivots), "deviance": np.array(acc.dev), "total": np.array(acc.total)}
        total = np.where(ok, acc.total, 1.0).astype(ld)

        def moments(pivot, s1, s2, t):
            m = np.asarray(s1, dtype=ld) / t
            var = np.asarray(s2, dtype=ld) / t - m * m
            return (np.asarray(pivot, dtype=ld) + m).astype(np.float64), var.astype(np.float64)

        def masked(v):
            v = np.array(v, dtype=np.float64)
            v[~ok] = np.nan
            return v

        mean, var = moments(acc.pivot_t[None, :], acc.pt, acc.ptt, total[:, None])
        self.mean = masked(mean)
        self.std = masked(np.sqrt(np.maximum(var, 0.0)))         # (a variance below zero is rounding about a constant entry)
        mean_chi2, var_chi2 = moments(acc.pivots[0], acc.dev[0], acc.dev[1], total)
        mean_lnl, var_lnl = moments(acc.pivots[1], acc.dev[2], acc.dev[3], total)
        self.mean_chi2, self.var_chi2, self.mean_lnl, self.var_lnl = (masked(v) for v in (mean_chi2, var_chi2, mean_lnl, var_lnl))
        self.chi2_at_mean = masked(np.full(R, np.nan) if chi2_at_mean is None else chi2_at_mean)
        self.lnl_at_mean = masked(np.full(R, np.nan) if lnl_at_mean is None else lnl_at_mean)
        mean_d = -2.0 * self.mean_lnl
        self.p_d = mean_d - (-2.0 * self.lnl_at_mean)
        self.p_v = (4.0 * self.var_lnl) / 2.0
        self.dic = mean_d + self.p_d
        self.blocks = list(blocks)
        self._poles = list(poles)
        self.multipoles = self.multipoles_of(0) if len(self.blocks) == 1 else None

    def multipoles_of(self, q):
        """``{ell: (mean (R, n_s), std (R, n_s))}`` of block ``q`` of a joint fit (block 0: a single fit's)."""
        if not 0 <= int(q) < len(self.blocks):
            raise InputError(f"SamplePredictive.multipoles_of: block {q!r} is outside 0 .. {len(self.blocks) - 1}")
        at, (poles, n_s) = self.blocks[int(q)].start, self._poles[int(q)]
        out = {}
        for i, ell in enumerate(np.atleast_1d(poles)):
            cut = slice(at + i * n_s, at + (i + 1) * n_s)
            out[int(ell)] = (self.mean[:, cut], self.std[:, cut])
        return out


MAX_TAIL = 4095          # vkist::kMaxK - 1: the tail without its cutoff
MIN_TAIL_FIT = 5         # entries a generalised Pareto fit needs


def default_tail_size(G):
    """Rule 7's default M for G kept points: ``min(floor(0.2 G), ceil(3 sqrt(G)), 4095)``."""
    return int(min(math.floor(0.2 * G), math.ceil(3.0 * math.sqrt(G)), MAX_TAIL))


def resolve_tail(tail, who, G):
    """The argument ``tail`` against G kept points: None (off) or the tail size M; every refusal an ``InputError``."""
    if tail is None:
        return None
    top = min(G - 1, MAX_TAIL)
    if tail is True:
        M = default_tail_size(G)
        if M < 1:
            raise InputError(f"{who}: tail=True needs at least 5 kept points ({G} are kept): the default tail is a fifth of them")
        return M
    if not isinstance(tail, dict) or set(tail) != {"size"}:
        raise InputError(f"{who}: tail must be None, True or {{'size': M}}, not {tail!r}")
    M = tail["size"]
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or not 1 <= int(M) <= top:
        raise InputError(f"{who}: the tail size must be an integer in 1 .. min(G - 1, {MAX_TAIL}) = {top}, not {M!r}")
    return int(M)


def gpd_fit(x):
    """``(k, scale)`` of the generalised Pareto distribution fitted to the n ascending excesses ``x`` (> 0 at the top): the
    Zhang-Stephens empirical-Bayes fit as PSIS uses it (rule 7), with the regularisation ``k = (n k + 5) / (n + 10)``.  ``x``
    (B, n) fits B samples of one length at once and returns two (B,) arrays - the same arithmetic per sample.  A sample whose
    largest or lower-quartile excess is not positive has no fit: ``(inf, nan)``."""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.ascontiguousarray(np.atleast_2d(x))
    B, n = x.shape
    k_out, scale_out = np.full(B, np.inf), np.full(B, np.nan)
    if n >= 1:
        quartile = x[:, int(math.floor(n / 4.0 + 0.5)) - 1]
        fit = (quartile > 0) & np.isfinite(x[:, -1])
        if np.any(fit):
            xs, quartile = x[fit], quartile[fit]
            m = 30 + int(math.floor(math.sqrt(n)))
            i = np.arange(1, m + 1, dtype=np.float64)
            b = 1.0 / xs[:, -1, None] + (1.0 - np.sqrt(m / (i - 0.5)))[None, :] / (3.0 * quartile[:, None])       # (F, m)
            k = np.mean(np.log1p(-b[:, :, None] * xs[:, None, :]), axis=2)
            L = n * (np.log(-b / k) - k - 1.0)
            with np.errstate(over="ignore"):                     # (a candidate far below the best: weight 0)
                weight = 1.0 / np.sum(np.exp(L[:, None, :] - L[:, :, None]), axis=2)
            weight = np.where(weight >= 10.0 * np.finfo(np.float64).eps, weight, 0.0)                             # dropped
            weight = weight / weight.sum(axis=1, keepdims=True)
            b_post = np.sum(b * weight, axis=1)
            k_post = np.mean(np.log1p(-b_post[:, None] * xs), axis=1)
            scale_out[fit] = -k_post / b_post
            k_out[fit] = (n * k_post + 5.0) / (n + 10.0)
    return (float(k_out[0]), float(scale_out[0])) if one else (k_out, scale_out)


def gpd_quantile(p, k, scale):
    """The quantile function of the generalised Pareto distribution of shape ``k`` and scale ``scale`` (location 0) at ``p``:
    ``scale expm1(-k log1p(-p)) / k``, at ``k = 0`` its limit ``-scale log1p(-p)``; the three broadcast."""
    k, scale = np.asarray(k, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    lp = np.log1p(-np.asarray(p, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        general = scale * np.expm1(-k * lp) / k
    return np.where(k == 0, -scale * lp, general)


def smooth_tail(w, u):
    """Rule 7 for one problem: ``w`` (n,) the tail's weights in DESCENDING order (the held order), ``u`` the cutoff's weight.
    Returns ``(k, scale, the smoothed weights in the same order)``; fewer than 5 entries, or no fit: ``k = inf`` and the weights
    as they are.  ``w`` (B, n) with ``u`` (B,): B problems with tails of one length at once, ``k`` and ``scale`` (B,)."""
    w = np.asarray(w, dtype=np.float64)
    one = w.ndim == 1
    w, u = np.atleast_2d(w), np.atleast_1d(np.asarray(u, dtype=np.float64))
    B, n = w.shape
    k, scale, out = np.full(B, np.inf), np.full(B, np.nan), w.copy()
    if n >= MIN_TAIL_FIT:
        k_fit, scale_fit = gpd_fit((w - u[:, None])[:, ::-1])
        good = np.isfinite(k_fit) & np.isfinite(scale_fit)
        p = (np.arange(1, n + 1, dtype=np.float64) - 0.5) / n
        smoothed = np.minimum(u[good, None] + gpd_quantile(p[None, :], k_fit[good, None], scale_fit[good, None]), 1.0)
        out[good] = smoothed[:, ::-1]                            # (ascending: the i-th smallest; handed out in the held order)
        k[good], scale[good] = k_fit[good], scale_fit[good]
    return (float(k[0]), float(scale[0]), out[0]) if one else (k, scale, out)


class SampleTail:
    """What ``ImportancePosterior.tail`` holds (rule 7 of the module docstring).  ``size`` M; ``count`` (R,) the entries held
    (at most M + 1: the tail and its cutoff); ``lnpost`` (R, M + 1) the held values, largest first, padded with -inf, and
    ``index`` (R, M + 1) int64 their points g, padded with -1; ``n_tail`` (R,) the entries strictly above the cutoff; ``k``,
    ``scale`` (R,) the fitted generalised Pareto shape and scale (``k = inf``: no fit; NaN without a finite point) and
    ``k_threshold`` the limit above which ``k`` is flagged; ``weight``, ``smoothed_weight`` (R, M + 1) the held entries' weights
    ``exp(lnpost - ln_max)`` and what replaces them (0 in the padding; the cutoff and an unfitted tail keep theirs);
    ``ln_evidence``, ``ln_evidence_error``, ``ess``, ``max_weight_share`` (R,), ``mean`` (R, d), ``cov`` (R, d, d), ``sigma`` (R,
    d) the smoothed estimates, from ``sums``: the corrected ``total``, ``sq`` (R,), ``s1`` (R, d) and ``s2`` (R, d (d + 1) / 2);
    ``status`` (R,): ``OK``, ``HIGH_K`` (``k > k_threshold``: the variance of the estimate cannot be trusted), ``SHORT`` (fewer
    than M + 1 finite points: nothing to fit) or ``NO_FINITE``.  Where nothing is fitted the smoothed figures equal the raw
    ones."""

    OK, HIGH_K, SHORT, NO_FINITE = 0, 1, 2, 3

    def __init__(self, ip, held, pacc=None):
        ld = np.longdouble
        acc, sample = ip.raw, ip._sample
        R, d = ip.n_problems, len(ip.names)
        K = held.K
        self.size = K - 1
        self.count = np.array(held.count, dtype=np.int64)
        self.lnpost, self.index = np.array(held.lnpost), np.array(held.index, dtype=np.int64)
        with np.errstate(divide="ignore"):
            self.k_threshold = float(min(1.0 - 1.0 / np.log10(float(ip.n_drawn)), 0.7)) if ip.n_drawn > 1 else -np.inf
        self.k, self.scale = np.full(R, np.inf), np.full(R, np.nan)
        self.n_tail = np.zeros(R, dtype=np.int64)
        self.status = np.zeros(R, dtype=np.int32)
        ok = acc.n_finite > 0
        with np.errstate(invalid="ignore"):
            self.weight = np.exp(self.lnpost - np.where(ok, acc.ln_max, 0.0)[:, None])    # (the padding, -inf, reads 0)
        self.smoothed_weight = self.weight.copy()
        full = ok & (self.count == K)
        self.status[~ok], self.k[~ok] = self.NO_FINITE, np.nan
        self.status[ok & ~full] = self.SHORT
        self.n_tail[full] = np.count_nonzero(self.lnpost[full] > self.lnpost[full, K - 1:K], axis=1)
        # the fits: the problems whose tails have one length together, in blocks whose (block, m, n) temporaries stay in cache
        for n in np.unique(self.n_tail[full]):
            rows = np.flatnonzero(full & (self.n_tail == n))
            block = max(1, (1 << 18) // (max(int(n), 1) * (30 + int(math.sqrt(max(int(n), 1))))))
            for at in range(0, len(rows), block):
                r = rows[at:at + block]
                self.k[r], self.scale[r], self.smoothed_weight[r, :n] = smooth_tail(self.weight[r, :n], self.weight[r, K - 1])
        self.status[full] = np.where(self.k[full] > self.k_threshold, self.HIGH_K, self.OK)
        top = np.where(ok, self.smoothed_weight[:, 0], 1.0)      # the largest weight after smoothing (unsmoothed: 1)
        # the corrections, all problems at once: the entries that were not smoothed add exact zeros
        new, old = self.smoothed_weight.astype(ld), self.weight.astype(ld)
        dw = new - old                                           # (R, K)
        y = sample.held_y(np.maximum(self.index, 0)).astype(ld)  # (R, K, d); the padding reads point 0 with dw = 0
        total = np.array(acc.total, dtype=ld) + dw.sum(axis=1)
        sq = np.array(acc.sq, dtype=ld) + (new * new - old * old).sum(axis=1)
        s1, s2 = np.array(acc.s1, dtype=ld), np.array(acc.s2, dtype=ld)
        for j in range(d):
            wy = dw * y[:, :, j]
            s1[:, j] += wy.sum(axis=1)
            for j2 in range(j, d):
                s2[:, tri(d, j, j2)] += (wy * y[:, :, j2]).sum(axis=1)
        self.sums = {"total": total.astype(np.float64), "sq": sq.astype(np.float64), "s1": s1.astype(np.float64),
                     "s2": s2.astype(np.float64)}
        # rule 5's formulas on the corrected sums
        t = np.where(ok, self.sums["total"], 1.0)
        q = np.where(ok, self.sums["sq"], 1.0)
        with np.errstate(divide="ignore"):
            ln_sum = np.where(ok, acc.ln_max, 0.0) + np.log(t)
        if pacc is None:
            norm = np.log(float(ip.n_drawn))
        elif sample.own:                                         # (rule 8: every problem's own prior normalisation)
            with np.errstate(divide="ignore"):
                norm = pacc.ln_max + np.log(pacc.total)
        else:
            norm = float(pacc.ln_max[0]) + np.log(float(pacc.total[0]))
        self.ln_evidence = np.where(ok, ln_sum - norm, -np.inf)
        self.ess = np.where(ok, t * t / q, 0.0)
        self.max_weight_share = np.where(ok, top / t, 0.0)
        self.ln_evidence_error = np.where(ok, np.sqrt(np.maximum(q / (t * t) - 1.0 / ip.n_drawn, 0.0)), np.inf)
        m = self.sums["s1"] / t[:, None]
        self.mean = np.where(ok[:, None], np.atleast_2d(sample.centre) + m, np.nan)
        self.cov = np.empty((R, d, d))
        for j in range(d):
            for j2 in range(j, d):
                self.cov[:, j, j2] = self.cov[:, j2, j] = self.sums["s2"][:, tri(d, j, j2)] / t - m[:, j] * m[:, j2]
        self.cov[~ok] = np.nan
        with np.errstate(invalid="ignore"):
            self.sigma = np.sqrt(np.diagonal(self.cov, axis1=1, axis2=2))


class ImportancePosterior:
    """The posterior of R problems from one shared sample.

    ``names``; ``n_problems``; ``n_drawn``, ``n_inside`` (the points kept: inside the prior box) and ``n_finite`` (R,);
    ``chunk``, ``n_chunks`` (what the sums' rounding depends on); ``ln_max`` (R,) the largest lnpost = lnL + ln prior - ln q and
    ``best[name]`` (R,) the point attaining it (the first such point, ``arg_max``); ``ln_evidence`` (R,) under the block's
    normalised uniform prior, or under the Gaussian prior normalised over the box by the same sample, and
    ``ln_evidence_error`` (R,) its standard error, ``sqrt(1 / ess - 1 / n_drawn)`` - under a prior that of the numerator alone:
    ``prior_error`` is the same figure of the prior's own normalisation, which the same sample estimates (the proposal has to
    cover the prior inside the box as it covers the posterior), and the two do not add in any fixed way (they are correlated); ``ess`` (R,) the effective sample size
    ``total^2 / sq`` and ``max_weight_share`` (R,) the largest normalised weight; ``mean`` (R, d), ``cov`` (R, d, d), ``sigma``
    (R, d); ``outside_mass`` (R, d, 2) the posterior mass below and above every range; ``status`` (R,): ``OK``, ``LOW_ESS``
    (``ess < min_ess``: the proposal misses this problem's posterior) or ``NO_FINITE`` (no kept point had a finite lnpost:
    ``ln_evidence`` -inf, ``ess`` 0, the sums zeros, the moments and ``best`` NaN).  ``raw``: the :class:`Sums`.  ``predictive``: a
    :class:`SamplePredictive` with ``predictive=True`` - the band of the theory vector and the DIC per problem -, else None.
    ``tail``: a :class:`SampleTail` with ``tail=True`` or ``tail={"size": M}`` - the Pareto shape of every problem's largest
    weights and the smoothed estimates -, else None.  With a proposal per problem (rule 8): ``proposals`` the
    :class:`ProposalSet` (else None), ``n_inside`` an (R,) array, and under a prior ``prior_ln_max``, ``prior_total`` and
    ``prior_error`` (R,) arrays."""

    OK, LOW_ESS, NO_FINITE = 0, 1, 2

    def __init__(self, layout, sample, lists, acc, pacc, min_ess):
        self._layout, self._sample, self._lists, self.raw = layout, sample, lists, acc
        self.names = list(layout.names)
        self.edges = dict(zip(self.names, layout.edges))
        self.n_problems = R = len(acc.ln_max)
        self.n_drawn, self.n_inside = sample.n_drawn, sample.n_inside
        self.proposals = None                                    # the ProposalSet of a run with a proposal per problem (rule 8)
        self.chunk, self.n_chunks = lists.chunk, lists.n_chunks
        self.ln_max, self.arg_max, self.n_finite = acc.ln_max, acc.arg_max, acc.n_finite
        self.min_ess = float(min_ess)
        ok = self._ok = acc.n_finite > 0
        total = self._total = np.where(ok, acc.total, 1.0)       # (never divided by zero)
        d = layout.d
        with np.errstate(divide="ignore"):
            ln_sum = np.where(ok, acc.ln_max, 0.0) + np.log(total)
        if pacc is None:
            self.ln_evidence = ln_sum - np.log(float(self.n_drawn))
        else:
            if sample.own:                                       # (rule 8: (R,) arrays, every problem's own prior problem)
                self.prior_ln_max, self.prior_total = np.array(pacc.ln_max), np.array(pacc.total)
            else:
                self.prior_ln_max, self.prior_total = float(pacc.ln_max[0]), float(pacc.total[0])
            with np.errstate(divide="ignore"):
                self.ln_evidence = ln_sum - (self.prior_ln_max + np.log(self.prior_total))
            self.prior_error = sample.prior_error()
        self.ln_evidence = np.where(ok, self.ln_evidence, -np.inf)
        sq = np.where(ok, acc.sq, 1.0)
        self.ess = np.where(ok, total * total / sq, 0.0)
        self.max_weight_share = np.where(ok, 1.0 / total, 0.0)
        self.ln_evidence_error = np.where(ok, np.sqrt(np.maximum(sq / (total * total) - 1.0 / self.n_drawn, 0.0)), np.inf)
        m = acc.s1 / total[:, None]
        self.mean = np.where(ok[:, None], np.atleast_2d(sample.centre) + m, np.nan)
        self.cov = np.empty((R, d, d))
        for j in range(d):
            for k in range(j, d):
                self.cov[:, j, k] = self.cov[:, k, j] = acc.s2[:, tri(d, j, k)] / total - m[:, j] * m[:, k]
        self.cov[~ok] = np.nan
        with np.errstate(invalid="ignore"):
            self.sigma = np.sqrt(np.diagonal(self.cov, axis1=1, axis2=2))
        at = np.where(ok, acc.arg_max, 0)
        points = sample.points(at)
        self.best = {n: np.where(ok, points[:, j], np.nan) for j, n in enumerate(self.names)}
        self.outside_mass = np.stack([np.stack([self._h1(j)[:, 0], self._h1(j)[:, -1]], axis=1) for j in range(d)], axis=1) / total[:, None, None]
        self.status = np.where(ok, np.where(self.ess < self.min_ess, self.LOW_ESS, self.OK), self.NO_FINITE).astype(np.int32)
        self._reader = None
        self.predictive = None                                   # a SamplePredictive with predictive=True (rule 6)
        self.tail = None                                         # a SampleTail with tail=True or {"size": M} (rule 7)

    def __len__(self):
        return self.n_problems

    def _axis(self, name):
        if name not in self.names:
            raise InputError(f"ImportancePosterior: {name} is not a sampled parameter ({self.names})")
        return self.names.index(name)

    def _h1(self, j):
        return self.raw.h1[:, self._layout.cell_off[j]:self._layout.cell_off[j + 1]]

    def marginal(self, name):
        """(R, bins) the marginal posterior density of ``name`` over its range's bins: its integral is the mass inside the range."""
        j = self._axis(name)
        return self._h1(j)[:, 1:-1] / (self._total[:, None] * np.diff(self.edges[name])[None, :])

    def marginal2d(self, a, b):
        """(R, m, m) the joint marginal density of a requested pair, axis 1 along ``a``; ``edges2d(a, b)`` gives its edges."""
        q, swap = self._pair(a, b, "marginal2d")
        L = self._layout
        ja, jb = L.pairs[q]
        m = L.pair_bins[q]
        at = L.cell_off[L.d + q] - L.n1
        h = self.raw.h2[:, at:at + m * m].reshape(-1, m, m)
        area = ((L.b[ja] - L.a[ja]) / m) * ((L.b[jb] - L.a[jb]) / m)
        out = h / (self._total[:, None, None] * area)
        return np.swapaxes(out, 1, 2) if swap else out

    def edges2d(self, a, b):
        """The two edge arrays (m + 1,) of a requested pair's cells, in the order ``a``, ``b``."""
        q, _ = self._pair(a, b, "edges2d")
        L = self._layout
        return tuple(np.linspace(L.a[j], L.b[j], L.pair_bins[q] + 1) for j in (self._axis(a), self._axis(b)))

    def _pair(self, a, b, what):
        j, k = self._axis(a), self._axis(b)
        key = tuple(sorted((j, k)))
        if j == k or key not in self._layout.pairs:
            raise InputError(f"ImportancePosterior.{what}: the pair ({a}, {b}) was not requested (pairs={self._layout.pair_names})")
        return self._layout.pairs.index(key), j > k

    def _marginals(self, name):
        """The 1-D histograms as the reader of :mod:`victor_amd.marginals` takes them - weights for counts - with ``n`` the
        running sum of ``name``'s own slots (the axes' sums differ by rounding)."""
        if self._reader is None:
            m = object.__new__(Marginals)
            m.names = list(self.names)
            m.counts = {n: self._h1(j)[:, 1:-1] for j, n in enumerate(self.names)}
            m.below = {n: self._h1(j)[:, 0] for j, n in enumerate(self.names)}
            m.above = {n: self._h1(j)[:, -1] for j, n in enumerate(self.names)}
            m.edges = dict(self.edges)
            self._reader = m
        self._reader.n = np.cumsum(self._h1(self._axis(name)), axis=1)[:, -1]
        return self._reader

    def quantile(self, name, q):
        """(R,) the q-quantile of ``name``, read from its histogram as ``Marginals.quantile`` reads one (linear inside a bin; NaN
        in the mass outside the range, or without a finite point)."""
        return self._marginals(name).quantile(name, q)

    def interval(self, name, level=0.68):
        """The equal-tailed interval of ``name``: two (R,) arrays."""
        return self._marginals(name).interval(name, level)

    def median(self, name):
        return self.quantile(name, 0.5)


def importance_posterior(fit, params, proposal=None, n=16384, seed=0, fixed=None, prior=None, bins=64, ranges=None, pairs=None,
                         chunk=None, min_ess=50.0, device=True, evaluate=None, sample=None, ln_proposal=None, kwargs=None,
                         realisations=None, n_blocks=None, predictive=None, tail=None):
    """The work of ``CCFFit.importance_posterior`` (``realisations=None``: the fit's data vector, R = 1) and
    ``Realisations.importance_posterior`` (R = the realisations, one shared sample); see the module docstring.  With ``evaluate``
    - a callable taking a dict of ``(n,)`` arrays (sampled and fixed parameters) and returning lnL ``(n,)`` or ``(n, R)`` - in
    place of ``fit`` only the definition route (``device=False``) is possible and no GPU is needed.

    Joint fits: ``fit`` may be a :class:`victor_amd.joint.JointFit` - with ``realisations`` a ``JointRealisations`` this is the
    work of ``JointRealisations.importance_posterior`` (problem i: joint realisation i), without them the posterior of the JOINT
    DATA VECTOR (R = 1).  This function is the only way to the latter: ``JointFit`` has no ``importance_posterior`` method, by
    design (call ``victor_amd.importance.importance_posterior(joint, params, ...)``).  ``"name@q"`` parameters
    (:func:`victor_amd.joint.per_block`) may then be sampled or fixed under the rules of the other joint loops; a sampled
    ``epsilon@q`` is refused (a point carries one host ``eps^(-2/3)``), a fixed one is fine.  Without a joint fit a per-block
    name has nothing to refer to and is refused - except with ``evaluate=`` and ``n_blocks=B`` (``device=False``), the
    definition route for per-block parameters: the ``@`` names are then checked against B blocks and the callable receives the
    batch with the ``@`` names as keys.

    ``params``: the cobaya block, as ``best_fit`` takes it (``fixed`` values must be scalars); ``proposal``: a
    :class:`GaussianProposal` naming exactly the sampled parameters, drawn ``n`` times with ``seed``; or ``sample`` (G, d) with
    ``ln_proposal`` (G,): the caller's own points, columns in sampled order, and ln of their normalised density; or, with
    ``realisations`` (plain or ``paired_model=True``) or an ``evaluate(batch, which)`` callable, a :class:`ProposalSet` of one
    proposal per problem, each drawn ``n`` times (rule 8 of the module docstring); ``prior``: a
    :class:`victor_amd.priors.GaussianPrior` or a list of them; ``bins``: an int or a dict name -> int, 1 .. 1024; ``ranges``:
    name -> (a, b) inside the prior box (default the box); ``pairs``: name pairs for the 2-D histograms; ``chunk``: points per
    launch, at most 65536 (default :func:`victor_amd.grid.default_chunk`); ``min_ess``: below it a problem is ``LOW_ESS``;
    ``device=False``: the NumPy definition.  ``predictive``: None (off) or True for the posterior mean and scatter of the theory
    vector, the moments of chi2 and lnL and ``p_d``, ``p_v``, ``dic`` of every problem (``ip.predictive``, a
    :class:`SamplePredictive`; rule 6 of the module docstring) - joint fits, covariances and ``@`` parameters included; refused
    (a :class:`victor_amd.predictive.PredictiveError`) for any other value, with an ``evaluate`` callable in place of a fit, and
    with ``paired_model`` realisations.  ``tail``: None (off), True or ``{"size": M}`` for the Pareto tail diagnostic and the
    smoothed estimates of every problem (``ip.tail``, a :class:`SampleTail`; rule 7 of the module docstring) - on either route,
    with an ``evaluate`` callable, a prior, ``predictive=True`` or the caller's own sample; any other value is refused.  Every
    argument is checked before the first device call.  Returns an :class:`ImportancePosterior`."""
    who = "importance_posterior"
    kwargs = kwargs or {}
    from .predictive import PredictiveError, resolve_sample_predictive
    predictive = resolve_sample_predictive(predictive, who, has_fit=evaluate is None and fit is not None)
    if evaluate is not None and device:
        raise InputError(f"{who}: an evaluate callable runs the definition route only (device=False)")
    if evaluate is None and fit is None:
        raise InputError(f"{who}: a fit or an evaluate callable is needed")
    from .joint import JointFit, check_block_names, split_name
    joint = fit if isinstance(fit, JointFit) else None
    own = isinstance(proposal, ProposalSet)                       # rule 8: a proposal per problem
    if own:
        if predictive:
            raise PredictiveError(f"{who}: predictive=True needs one shared sample (a point's theory vector serves every problem); "
                                  "with a ProposalSet every problem has points of its own")
        if sample is not None or ln_proposal is not None:
            raise InputError(f"{who}: sample and ln_proposal come in place of the proposal, not beside a ProposalSet")
        if joint is not None or n_blocks is not None:
            raise InputError(f"{who}: a ProposalSet is not supported for joint fits (one proposal for all problems is)")
        if realisations is None and evaluate is None:
            raise InputError(f"{who}: a ProposalSet needs realisations (one problem per proposal) or an evaluate callable")
        if realisations is not None and len(proposal) != len(realisations):
            raise InputError(f"{who}: the ProposalSet holds {len(proposal)} proposals, there are {len(realisations)} realisations")
    if n_blocks is not None:
        if fit is not None or evaluate is None:
            raise InputError(f"{who}: n_blocks goes with an evaluate callable in place of a fit (a joint fit knows its blocks)")
        if isinstance(n_blocks, bool) or not isinstance(n_blocks, (int, np.integer)) or n_blocks < 1:
            raise InputError(f"{who}: n_blocks must be an integer >= 1, not {n_blocks!r}")
    q = _Sampled(who, "sampled", params, fixed)
    names, fixed_all = q.names, q.fixed_all
    d = len(names)
    per_block = sorted(n for n in list(names) + list(fixed_all) if "@" in n)
    if per_block and joint is None:
        # a per-block name needs blocks to refer to: a joint fit's, or the caller's word for them beside an evaluate callable
        if n_blocks is None:
            raise InputError(f"{who}: per-block parameters ('name@block': {per_block}) need a joint fit to refer to (or, beside "
                             "an evaluate callable, n_blocks)")
        check_block_names(per_block, int(n_blocks), who=who)
    if joint is not None and evaluate is not None:
        joint._check_block_names(per_block, who)
    eps_own = sorted(n for n in names if "@" in n and split_name(n)[0] == "epsilon")
    if eps_own:
        raise InputError(f"{who}: epsilon cannot be sampled per block ({eps_own}): a point of the sample carries one eps^(-2/3); "
                         "fix the per-block epsilons, or sample one epsilon for all blocks")
    if d > MAX_AXES:
        raise InputError(f"{who}: at most {MAX_AXES} sampled parameters ({d} are sampled)")
    if evaluate is None:
        q.check_columns(fit)
        q.check_alpha()
    arrays = sorted(k for k, v in fixed_all.items() if np.ndim(v) > 0)
    if arrays:
        raise InputError(f"{who}: fixed values must be scalars ({arrays} are not)")
    layout = resolve_layout(who, names, q.lo, q.hi, bins, ranges, pairs)
    prior = resolve_prior(prior, who, names, q.lo, q.hi, fixed_all, joint is not None or n_blocks is not None)
    if realisations is not None and getattr(realisations, "paired_model", False) and not own:
        raise (PredictiveError if predictive else InputError)(
            f"{who}: realisations(paired_model=True) have no cross mode (a point has one theory vector per "
            "realisation): a shared sample evaluates every point once")
    if evaluate is None:
        fit_options = q.fit_options(fit, kwargs, "predictive=True" if predictive else None)
    if joint is not None and evaluate is None and len({f._device for f in joint.fits}) != 1:
        raise InputError(f"{who}: every block of a joint fit must live on the same device")
    if not np.isfinite(min_ess) or min_ess < 0:
        raise InputError(f"{who}: min_ess must be a number >= 0, not {min_ess!r}")

    if own:
        return _own_posterior(who, q, fit, realisations, kwargs, layout, prior, proposal, n, seed, chunk, min_ess, device, evaluate, tail,
                              fixed_all)

    # ---- rule 1: the sample
    if sample is not None or ln_proposal is not None:
        if sample is None or ln_proposal is None or proposal is not None:
            raise InputError(f"{who}: sample and ln_proposal come together, in place of the proposal")
        x = np.asarray(sample, dtype=np.float64)
        lnq = np.asarray(ln_proposal, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != d or lnq.shape != (len(x),) or not len(x):
            raise InputError(f"{who}: sample must be (G, {d}) in the order {names} and ln_proposal (G,)")
        if not np.all(np.isfinite(x)) or not np.all(np.isfinite(lnq)):
            raise InputError(f"{who}: sample and ln_proposal must be finite")
        centre = None
    else:
        if not isinstance(proposal, GaussianProposal):
            raise InputError(f"{who}: a GaussianProposal is needed (or sample= and ln_proposal=)")
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_POINTS:
            raise InputError(f"{who}: n must be an integer in 1 .. 2^24, not {n!r}")
        if isinstance(seed, bool) or int(seed) != seed or int(seed) < 0:
            raise InputError(f"{who}: seed must be an integer >= 0, not {seed!r}")
        centre, chol = proposal.ordered(who, names)
        x = GaussianProposal.draw(centre, chol, proposal.dof, int(n), int(seed))
        lnq = GaussianProposal.ln_density(x, centre, chol, proposal.dof)
    if len(x) > MAX_POINTS:
        raise InputError(f"{who}: at most 2^24 points, not {len(x)}")
    inside = np.all((x >= q.lo) & (x <= q.hi), axis=1)
    if not np.any(inside):
        raise InputError(f"{who}: no point of the sample lies inside the prior box ({len(x)} drawn)")
    kept = x[inside]
    smp = Sample(kept, kept.mean(axis=0) if centre is None else centre, lnq[inside], len(x), q.lo, q.hi, prior)

    tail = resolve_tail(tail, who, smp.G)                         # M, or None

    R = len(realisations) if realisations is not None else 1
    if chunk is None:
        chunk = default_chunk(R, smp.G)
    if isinstance(chunk, bool) or int(chunk) != chunk or not 1 <= int(chunk) <= MAX_CHUNK:
        raise InputError(f"{who}: chunk must be an integer in 1 .. {MAX_CHUNK}, not {chunk!r}")
    chunk = int(chunk)
    lists = Lists(layout, smp.x, chunk)                           # rule 2
    fixed_out = {k: float(v) for k, v in fixed_all.items()}

    def batch_of(x):
        batch = dict(fixed_out)
        batch.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names)})
        return batch

    def finish(acc, pacc):
        ip = ImportancePosterior(layout, smp, lists, acc, pacc, min_ess)
        if predictive:
            ip.predictive = read_predictive(ip, fit, realisations, batch_of, kwargs)
        if tail is not None:
            ip.tail = SampleTail(ip, acc.tail, pacc)
        return ip

    if not device:
        both = (lambda v: v) if predictive else (lambda v: v[0])  # (rule 6 takes chi2 from the call that gives lnL)
        theory = None
        if evaluate is not None:
            R = None                                             # (as many problems as the callable returns columns)

            def values(x):
                return evaluate(batch_of(x))
        elif realisations is not None:
            def values(x):
                return both(getattr(realisations, "_cross", realisations.log_likelihood)(batch_of(x), **kwargs))
        else:
            def values(x):
                return both(fit.log_likelihood_batch(batch_of(x), **kwargs))
        if predictive:
            from .fisher import host_vectors

            def theory(x):
                return host_vectors(fit, batch_of(x), kwargs)
        return finish(*run_definition(layout, smp, lists, R, values, theory, None if tail is None else tail + 1))

    # ---- device
    lib, h, refresh = create_handle(q, fit, realisations, kwargs, fit_options, layout, smp, lists, fixed_out)
    try:
        if refresh is not None:
            refresh()
        if predictive:
            _check(lib, h, lib.vk_is_set_predictive(h, 1), "vk_is_set_predictive")
        if tail is not None:
            _check(lib, h, lib.vk_is_set_tail(h, tail + 1), "vk_is_set_tail")
        _check(lib, h, lib.vk_is_run(h, 0, smp.G), "vk_is_run")
        acc, pacc = read_result(lib, h, layout, R, smp.lnop is not None, theory_entries(fit) if predictive else None,
                                None if tail is None else tail + 1)
    finally:
        lib.vk_is_destroy(h)
    return finish(acc, pacc)


def draw_own(centre, chol, dof, n, seed):
    """Rule 8.1, common random numbers: ONE ``z`` (n, d) for all problems, ``x[:, r] = centre[r] + z @ chol[r].T`` and its ln q.
    Returns ``(x (n, R, d), centre, ln q (n, R))``, the first arguments of :class:`OwnSample`."""
    R, d = centre.shape
    z = GaussianProposal.standard(d, dof, n, seed)
    x, lnq = np.empty((n, R, d)), np.empty((n, R))
    for r in range(R):
        x[:, r] = centre[r] + z @ chol[r].T
        lnq[:, r] = GaussianProposal.ln_density(x[:, r], centre[r], chol[r], dof)
    return x, centre, lnq


def _own_posterior(who, q, fit, realisations, kwargs, layout, prior, proposals, n, seed, chunk, min_ess, device, evaluate, tail,
                   fixed_all):
    """Rule 8 behind :func:`importance_posterior`, whose checks have run: the sample of every problem from its own proposal,
    its lists, then the definition (``device=False``) or ``vk_is_create_own``."""
    names, d, R = layout.names, layout.d, len(proposals)
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= MAX_POINTS:
        raise InputError(f"{who}: n must be an integer in 1 .. 2^24, not {n!r}")
    if isinstance(seed, bool) or int(seed) != seed or int(seed) < 0:
        raise InputError(f"{who}: seed must be an integer >= 0, not {seed!r}")
    n = int(n)
    if n * R > MAX_POINTS:
        raise InputError(f"{who}: n x problems = {n} x {R} is more than 2^24 points: take fewer points or fewer problems at once")
    if chunk is None:
        chunk = max(1, min(n, MAX_CHUNK // R))
    if isinstance(chunk, bool) or int(chunk) != chunk or not 1 <= int(chunk) <= MAX_CHUNK:
        raise InputError(f"{who}: chunk must be an integer in 1 .. {MAX_CHUNK}, not {chunk!r}")
    chunk = int(chunk)
    if chunk * R > MAX_CHUNK:
        raise InputError(f"{who}: chunk x problems = {chunk} x {R} is more than {MAX_CHUNK} rows of one launch: take a smaller chunk")
    centre, chol = proposals.ordered(who, names)
    outside = np.flatnonzero(np.any((centre < q.lo) | (centre > q.hi), axis=1))
    if len(outside):
        raise InputError(f"{who}: the proposal of problem {int(outside[0])} has its mean {centre[outside[0]].tolist()} outside the "
                         f"prior box of {names}")
    smp = OwnSample(*draw_own(centre, chol, proposals.dof, n, int(seed)), q.lo, q.hi, prior)
    tail = resolve_tail(tail, who, n)
    lists = OwnLists(layout, smp, chunk)
    fixed_out = {k: float(v) for k, v in fixed_all.items()}

    def batch_of(x):
        batch = dict(fixed_out)
        batch.update({name: np.ascontiguousarray(x[:, j]) for j, name in enumerate(names)})
        return batch

    def finish(acc, pacc):
        ip = ImportancePosterior(layout, smp, lists, acc, pacc, min_ess)
        ip.proposals = proposals
        if tail is not None:
            ip.tail = SampleTail(ip, acc.tail, pacc)
        return ip

    K = None if tail is None else tail + 1
    if not device:
        if evaluate is not None:
            def values(x, which):
                return evaluate(batch_of(x), which)
        else:
            def values(x, which):
                return realisations.log_likelihood_pairs(batch_of(x), which, **kwargs)[0]
        return finish(*run_definition_own(layout, smp, lists, values, K))

    lib, h = create_own_handle(fit, realisations, kwargs, layout, smp, lists, fixed_out)
    try:
        if tail is not None:
            _check(lib, h, lib.vk_is_set_tail(h, K), "vk_is_set_tail")
        _check(lib, h, lib.vk_is_run(h, 0, n), "vk_is_run")
        acc, pacc = read_result(lib, h, layout, R, smp.lnop is not None, None, K, own=True)
    finally:
        lib.vk_is_destroy(h)
    return finish(acc, pacc)


def create_own_handle(fit, realisations, kwargs, layout, smp, lists, fixed_out, which=None):
    """``(lib, handle)`` of ``vk_is_create_own`` for an :class:`OwnSample` and its :class:`OwnLists` on the realisations' engine
    (``paired_model``: its table sets are uploaded with the data's): the base row from the fixed values, the sample's arrays and
    per point the host's own ``eps^(-2/3)``, as :func:`create_handle`.  ``which``: the realisation of every problem (default
    problem r: realisation r)."""
    names, d, n, R, chunk = layout.names, layout.d, smp.G, smp.R, lists.chunk
    i32 = C.POINTER(C.c_int32)
    batch = dict(fixed_out)
    batch.update({name: np.array([smp.x[0, 0, j]]) for j, name in enumerate(names)})
    model, own_options, eng, opts = realisations._plan(kwargs)
    opts = blend_opts(fit, own_options, opts)
    base = np.ascontiguousarray(fit._fit_rows(batch, model), dtype=np.float64)
    cols = np.array([N.ROW_COLUMNS.get(name, N.VK_WALK_EPSILON) for name in names], dtype=np.int32)
    eps_pow = None
    if "epsilon" in names:
        with np.errstate(invalid="ignore"):
            eps_pow = N.f64(N.epsilon_to_ap(N.f64(smp.x[:, :, names.index("epsilon")].ravel()), 1.0)[1])
    n_bins = np.array(layout.n_bins, dtype=np.int32)
    pair_bins = np.array(layout.pair_bins, dtype=np.int32)
    which = np.arange(R, dtype=np.int32) if which is None else np.ascontiguousarray(which, dtype=np.int32)
    err = C.create_string_buffer(512)
    lib = eng._lib
    h = lib.vk_is_create_own(eng._ctx, C.byref(opts), d, cols.ctypes.data_as(i32), n, R, which.ctypes.data_as(i32), N.as_dp(smp.x),
                             N.as_dp(smp.y), None if eps_pow is None else N.as_dp(eps_pow), N.as_dp(smp.lno),
                             None if smp.lnop is None else N.as_dp(smp.lnop), n_bins.ctypes.data_as(i32), len(pair_bins),
                             pair_bins.ctypes.data_as(i32) if len(pair_bins) else None, lists.entries.ctypes.data_as(i32),
                             lists.offsets.ctypes.data_as(i32), N.as_dp(base), float(fixed_out.get("alpha", 1)), chunk, err, len(err))
    if not h:
        msg = err.value.decode()
        raise (N.NativeError if "device memory" in msg else InputError)(msg)
    return lib, h


def _blocks_of(fit):
    from .joint import JointFit
    return list(fit.fits) if isinstance(fit, JointFit) else [fit]


def theory_entries(fit):
    """N: the entries of a point's theory vector - of a joint fit the blocks' vectors in block order."""
    return sum(len(f.s) * len(np.atleast_1d(f.poles_s)) for f in _blocks_of(fit))


def read_predictive(ip, fit, realisations, batch_of, kwargs):
    """The :class:`SamplePredictive` of a completed run whose :class:`Sums` carry rule 6's arrays: one pairs call gives the
    likelihood of problem r at ``ip.mean[r]`` (the problems without a mean read NaN)."""
    R = ip.n_problems
    lnl_at, chi2_at = np.full(R, np.nan), np.full(R, np.nan)
    has = np.flatnonzero(ip._ok & np.all(np.isfinite(ip.mean), axis=1))
    if len(has):
        batch = batch_of(ip.mean[has])
        if realisations is not None:
            lnl_at[has], chi2_at[has] = realisations.log_likelihood_pairs(batch, has.astype(np.int32), **kwargs)
        else:
            lnl_at[has], chi2_at[has] = fit.log_likelihood_batch(batch, **kwargs)
    blocks, poles, at = [], [], 0
    for f in _blocks_of(fit):
        n = len(f.s) * len(np.atleast_1d(f.poles_s))
        blocks.append(slice(at, at + n))
        poles.append((np.atleast_1d(f.poles_s), len(f.s)))
        at += n
    return SamplePredictive(ip.raw, ip._ok, blocks, poles, chi2_at, lnl_at)


def _check(lib, h, rc, entry):
    if rc != 0:
        msg = (lib.vk_is_last_error(h) or b"").decode() or f"{entry} failed ({rc})"
        raise (InputError if rc == -1 else N.NativeError)(msg)


def create_handle(q, fit, realisations, kwargs, fit_options, layout, smp, lists, fixed_out):
    """``(lib, handle, refresh)`` of ``vk_is_create`` for the sample: the base row from the fixed values (the sampled columns are
    overwritten per point), the sample's arrays, and per point the host's own ``eps^(-2/3)`` (``vk_epsilon_to_ap``: libm's pow).
    Of a :class:`victor_amd.joint.JointFit`: ``vk_is_create_joint`` over the engines, option block, covariance handle and
    realisation upload every joint device loop uses (``JointFit._sampled_plan`` / ``_sampled_rows`` / ``_sampled_device``); with
    ``@`` names among the sampled or fixed parameters its ``_blocks`` form, a base row per block."""
    from .joint import JointFit
    batch = dict(fixed_out)
    batch.update({n: np.array([smp.x[0, j]]) for j, n in enumerate(layout.names)})
    i32 = C.POINTER(C.c_int32)
    extra = ()
    if isinstance(fit, JointFit):
        engines, opts, kw = fit._sampled_plan(q.who, kwargs)
        base, cols, param_block, _ = fit._sampled_rows(layout.names, batch, kw)
        entry = "vk_is_create_joint"
        if param_block is not None:
            extra = (param_block.ctypes.data_as(i32),)
            entry += "_blocks"
        lib, ctxs, cov, refresh = fit._sampled_device(engines, realisations)
        head = (ctxs, len(engines), cov, C.byref(opts))
    else:
        model = fit._merged(kwargs)
        fit._check_supported(model)
        base = np.ascontiguousarray(fit._fit_rows(batch, model), dtype=np.float64)
        cols = np.array([N.ROW_COLUMNS.get(n, N.VK_WALK_EPSILON) for n in layout.names], dtype=np.int32)
        refresh = None
        if realisations is None:
            eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
            opts = eng.make_opts(model, fit_options)
        else:
            _, _, eng, opts = realisations._plan(kwargs)

            def refresh():
                realisations._upload(eng)
        opts = blend_opts(fit, fit_options, opts)
        lib, entry, head = eng._lib, "vk_is_create", (eng._ctx, C.byref(opts))
    eps_pow = None
    if "epsilon" in layout.names:
        with np.errstate(invalid="ignore"):
            eps_pow = N.f64(N.epsilon_to_ap(N.f64(smp.x[:, layout.names.index("epsilon")]), 1.0)[1])
    n_bins = np.array(layout.n_bins, dtype=np.int32)
    pair_bins = np.array(layout.pair_bins, dtype=np.int32)
    err = C.create_string_buffer(512)
    h = getattr(lib, entry)(*head, layout.d, cols.ctypes.data_as(i32), *extra, smp.G, N.as_dp(smp.x), N.as_dp(smp.y),
                            None if eps_pow is None else N.as_dp(eps_pow), N.as_dp(smp.lno),
                            None if smp.lnop is None else N.as_dp(smp.lnop), n_bins.ctypes.data_as(i32), len(pair_bins),
                            pair_bins.ctypes.data_as(i32) if len(pair_bins) else None, lists.entries.ctypes.data_as(i32),
                            lists.offsets.ctypes.data_as(i32), N.as_dp(base), float(fixed_out.get("alpha", 1)),
                            0 if realisations is None else 1, lists.chunk, err, len(err))
    if not h:
        msg = err.value.decode()
        raise (N.NativeError if "device memory" in msg else InputError)(msg)
    return lib, h, refresh


def read_result(lib, h, layout, R, with_prior, n_theory=None, tail=None, own=False):
    """``(Sums, the prior's own Sums or None)`` of a completed run (``vk_is_result``; with ``n_theory`` rule 6's arrays through
    ``vk_is_predictive``, whose ``[N][R]`` sums are turned to (R, N); with ``tail=K`` rule 7's :class:`Held` through
    ``vk_is_tail``, as the Sums' ``tail``)."""
    acc = Sums(layout, R, n_theory)
    if tail is not None:
        acc.tail = held = Held(R, tail)
        to_i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        _check(lib, h, lib.vk_is_tail(h, N.as_dp(held.lnpost), to_i64(held.index), to_i64(held.count)), "vk_is_tail")
    if n_theory is not None:
        pt, ptt = np.empty((n_theory, R)), np.empty((n_theory, R))
        _check(lib, h, lib.vk_is_predictive(h, N.as_dp(acc.pivot_t), N.as_dp(pt), N.as_dp(ptt), N.as_dp(acc.pivots), N.as_dp(acc.dev)),
               "vk_is_predictive")
        acc.pt, acc.ptt = np.ascontiguousarray(pt.T), np.ascontiguousarray(ptt.T)
    i64 = C.POINTER(C.c_int64)
    if own:                                                      # (vk_is_create_own: R values each, a prior problem per problem)
        pacc = Sums(layout, R)
        rc = lib.vk_is_result(h, N.as_dp(acc.ln_max), acc.arg_max.ctypes.data_as(i64), acc.n_finite.ctypes.data_as(i64),
                              N.as_dp(acc.total), N.as_dp(acc.sq), N.as_dp(acc.s1), N.as_dp(acc.s2), N.as_dp(acc.h1), N.as_dp(acc.h2),
                              N.as_dp(pacc.ln_max), N.as_dp(pacc.total))
        _check(lib, h, rc, "vk_is_result")
        return acc, pacc if with_prior else None
    pm, pt = C.c_double(0.0), C.c_double(0.0)
    rc = lib.vk_is_result(h, N.as_dp(acc.ln_max), acc.arg_max.ctypes.data_as(i64), acc.n_finite.ctypes.data_as(i64), N.as_dp(acc.total),
                          N.as_dp(acc.sq), N.as_dp(acc.s1), N.as_dp(acc.s2), N.as_dp(acc.h1), N.as_dp(acc.h2),
                          C.cast(C.byref(pm), C.POINTER(C.c_double)), C.cast(C.byref(pt), C.POINTER(C.c_double)))
    _check(lib, h, rc, "vk_is_result")
    pacc = None
    if with_prior:
        pacc = Sums(layout, 1)
        pacc.ln_max[0], pacc.total[0] = pm.value, pt.value
    return acc, pacc
