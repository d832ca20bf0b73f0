"""Gaussian priors on the sampled parameters of best fits, Metropolis chains and stretch-move ensembles: the ``prior=`` keyword
of ``best_fit`` and ``sample_chains`` (``CCFFit``, ``Realisations``, ``JointFit``, ``JointRealisations``).

The cobaya ``params`` block keeps its meaning: it defines the uniform box, the ``ref`` start and the proposal widths (``dist:
norm`` inside the block stays refused: the block's prior IS the box every device loop is bounded by, and a second way to state a
Gaussian would have to agree with this one).  A :class:`GaussianPrior` is multiplied onto that box, so the density it gives is a
Gaussian TRUNCATED by the box.

**The definition (one routine, three compilers).**  ln prior = -1/2 (x - mu)^T P (x - mu), with no normalisation constant: a
constant changes no accept / reject decision and no maximum, and the normalisation of the truncated density is not computed.  P
is the inverse covariance of the named parameters, embedded in the d x d matrix of the sampled parameters in sampled order (zero
rows for parameters without a prior); its upper triangle is packed row by row (``vkchain::tri`` order) with every off-diagonal
entry doubled - doubling is exact.  The arithmetic order is part of the definition::

    q = 0
    for j in 0 .. d-1:  dj = x[j] - mu[j]
        for k in j .. d-1:  t = pp[tri(d, j, k)] * dj;  t = t * (x[k] - mu[k]);  q = q + t
    lnprior = -0.5 * q

:meth:`ResolvedPrior.lnprior` states it in NumPy, elementwise over the rows; ``victor_amd/csrc/vk_prior.h`` states it in C++ for
hipcc (the step kernels) and g++ (the CPU tests), with the fused multiply-add forbidden.  The three agree bit for bit.
"""

import numpy as np

from .utils import InputError

MAX_PARAMS = 10


def tri(d, j, k):
    """Position of (j, k), j <= k, in the packed upper triangle of a d x d matrix, row by row (``vkchain::tri``)."""
    return j * d - j * (j - 1) // 2 + (k - j)


class GaussianPrior:
    """A Gaussian prior over some of the sampled parameters, independent or correlated.

    ``GaussianPrior(names, mean, cov=None, sigma=None)``: ``names`` are sampled parameters (``"sigma_v@2"`` on a joint fit),
    ``mean`` their k means; exactly one of ``cov``, a ``(k, k)`` symmetric positive-definite covariance matrix, and ``sigma``, k
    standard deviations > 0.  Several priors may be passed as a list when their names are disjoint.

    ln prior = -1/2 (x - mean)^T cov^-1 (x - mean), without a normalisation constant (it changes no decision and no maximum).
    The prior is multiplied onto the uniform box of the cobaya ``params`` block: what is sampled and maximised is the Gaussian
    truncated by the box.  A mean outside its parameter's box is refused."""

    def __init__(self, names, mean, cov=None, sigma=None):
        if isinstance(names, str):
            names = [names]
        self.names = [str(n) for n in names]
        k = len(self.names)
        if k < 1:
            raise InputError("GaussianPrior: no parameter is named")
        twice = sorted({n for n in self.names if self.names.count(n) > 1})
        if twice:
            raise InputError(f"GaussianPrior: {twice} named twice")
        self.mean = np.atleast_1d(np.asarray(mean, dtype=float))
        if self.mean.shape != (k,) or not np.all(np.isfinite(self.mean)):
            raise InputError(f"GaussianPrior: mean must hold {k} finite values, one per name")
        if (cov is None) == (sigma is None):
            raise InputError("GaussianPrior: give exactly one of cov and sigma")
        if sigma is not None:
            self.sigma = np.atleast_1d(np.asarray(sigma, dtype=float))
            if self.sigma.shape != (k,) or not np.all(np.isfinite(self.sigma)) or not np.all(self.sigma > 0):
                raise InputError(f"GaussianPrior: sigma must hold {k} finite standard deviations > 0")
            self.cov = np.diag(self.sigma * self.sigma)
        else:
            self.sigma = None
            self.cov = np.asarray(cov, dtype=float)
            if self.cov.shape != (k, k) or not np.all(np.isfinite(self.cov)):
                raise InputError(f"GaussianPrior: cov must be a finite ({k}, {k}) matrix")
            if not np.allclose(self.cov, self.cov.T, rtol=1e-12, atol=0.0):
                raise InputError("GaussianPrior: cov is not symmetric")
            self.cov = 0.5 * (self.cov + self.cov.T)
            try:
                np.linalg.cholesky(self.cov)
            except np.linalg.LinAlgError:
                raise InputError("GaussianPrior: cov is not positive definite") from None

    def __repr__(self):
        return f"GaussianPrior({self.names}, mean={self.mean.tolist()})"


class ResolvedPrior:
    """The priors of one call against its d sampled parameters: ``mu`` (d,) and ``pp`` (d (d + 1) / 2,), the packed triangle of
    the module docstring - what ``vk_fit_set_prior`` / ``vk_chain_set_prior`` take - and the NumPy statement of ln prior."""

    def __init__(self, names, mu, precision, sigma=None):
        self.names = list(names)
        self.sigma = sigma                                  # (d,) standard deviations (NaN: no prior) when every prior is independent
        d = self.d = len(self.names)
        self.mu = np.ascontiguousarray(mu, dtype=np.float64)
        self.precision = precision
        self.pp = np.zeros(d * (d + 1) // 2)
        for j in range(d):
            for k in range(j, d):
                self.pp[tri(d, j, k)] = precision[j, k] if j == k else 2.0 * precision[j, k]

    def lnprior(self, x):
        """ln prior of the points ``x`` (..., d): the definition, elementwise over the leading axes."""
        x = np.asarray(x, dtype=np.float64)
        d, mu, pp = self.d, self.mu, self.pp
        if x.shape[-1] != d:
            raise InputError(f"lnprior: points of {d} sampled parameters are needed")
        q = np.zeros(x.shape[:-1])
        for j in range(d):
            dj = x[..., j] - mu[j]
            for k in range(j, d):
                t = pp[tri(d, j, k)] * dj
                t = t * (x[..., k] - mu[k])
                q = q + t
        return -0.5 * q


def resolve_prior(prior, who, names, lo, hi, fixed=(), joint=True):
    """The :class:`ResolvedPrior` of ``prior`` (None, a :class:`GaussianPrior` or a list of them with disjoint names) against
    the sampled parameters ``names`` with box ``lo``, ``hi``; None for None.  ``fixed``: the names the call holds fixed (for the
    text of a refusal); ``joint``: the fit is a ``JointFit`` (``"name@q"`` means something).  Every refusal is an ``InputError``,
    raised before any device call."""
    if prior is None:
        return None
    priors = [prior] if isinstance(prior, GaussianPrior) else list(prior)
    if not priors or not all(isinstance(p, GaussianPrior) for p in priors):
        raise InputError(f"{who}: prior must be a GaussianPrior or a list of them")
    names = list(names)
    d = len(names)
    if d > MAX_PARAMS:
        raise InputError(f"{who}: at most {MAX_PARAMS} sampled parameters")
    seen = set()
    mu, precision = np.zeros(d), np.zeros((d, d))
    sigma = np.full(d, np.nan)                              # ... of independent priors; None once one is correlated
    for p in priors:
        for n in p.names:
            if "@" in n and not joint:
                raise InputError(f"{who}: prior on a per-block parameter ('name@block': {n}) needs a JointFit")
            if n in seen:
                raise InputError(f"{who}: {n} is named by two priors")
            seen.add(n)
            if n not in names:
                why = "it is fixed" if n in fixed else "it is not in the params block"
                raise InputError(f"{who}: prior names {n}, which is not sampled ({why}); sampled: {names}")
        # the named subset in SAMPLED order before it is inverted: the packed triangle does not depend on the order of `names`
        order = sorted(range(len(p.names)), key=lambda i: names.index(p.names[i]))
        at = [names.index(p.names[i]) for i in order]
        mean = p.mean[order]
        for i, j in enumerate(at):
            if not lo[j] <= mean[i] <= hi[j]:
                raise InputError(f"{who}: the prior mean of {names[j]} ({mean[i]}) is outside its box [{lo[j]}, {hi[j]}] (the "
                                 "Gaussian is truncated by the box)")
        if p.sigma is not None:
            sub = np.diag(1.0 / (p.sigma[order] * p.sigma[order]))
        else:
            sub = np.linalg.inv(p.cov[np.ix_(order, order)])
            sub = 0.5 * (sub + sub.T)
        if not np.all(np.isfinite(sub)):
            raise InputError(f"{who}: the inverse of the prior covariance of {p.names} is not finite")
        mu[at] = mean
        precision[np.ix_(at, at)] = sub
        if sigma is not None:
            if p.sigma is not None:
                sigma[at] = p.sigma[order]
            elif not np.any(p.cov - np.diag(np.diag(p.cov))):
                sigma[at] = np.sqrt(np.diag(p.cov))[order]
            else:
                sigma = None
    return ResolvedPrior(names, mu, precision, sigma)
