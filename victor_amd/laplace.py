"""Parameter covariances at best fits: the Hessian of lnL + ln prior on the GPU and the Laplace approximation from it -
``CCFFit.laplace``, ``Realisations.laplace``, ``JointFit.laplace`` and ``JointRealisations.laplace``, and
``best_fit(..., covariance=True)``.

``best_fit`` returns a point per problem; the local Gaussian approximation of the posterior around it is the cheap error bar: the
Hessian H of lnL + ln prior at the point and ``cov = (-H)^-1``.  For d sampled parameters that is one central-difference stencil
of ``M = 2 d^2 + 1`` evaluations per problem; ``vk_fit_hessian`` (``include/victor_hip.h``) forms the
R M rows on the device, evaluates them with the launches the search makes, and assembles A, the Hessian, the covariance and a
status per problem in one small kernel.

**The NumPy statement.**  :func:`stencil_points` and :func:`assemble` restate ``victor_amd/csrc/vk_hessian.h`` with the same
operations in the same order, elementwise over the problems, so the device, a g++ build of the header and this module agree bit
for bit (tests/test_hessian.py, tests/test_gpu_hessian.py):

* point ``m`` of a problem at ``x`` with steps ``h``: 0 is ``x``; ``1 + 2 j + s`` is ``x +- h_j e_j`` (``s = 0``: +);
  ``1 + 2 d + 4 q + c`` displaces ``x_j`` and ``x_k``, ``q`` the pair ``j < k`` in the order (0,1), (0,2), .., (1,2), .., ``c`` the
  signs (+,+), (+,-), (-,+), (-,-).  A displaced coordinate is the rounded sum.
* ``A = -H o (h h^T)``: ``A_jj = ((v0 + v0) - v(+j)) - v(-j)``, ``A_jk = 0.25 ((v(+-) - v(++)) + (v(-+) - v(--)))``.
* status, in this precedence: ``AT_BOUND`` (the stencil leaves the box, or ``x`` is outside it: every row of the problem is
  evaluated at ``x``), ``NOT_FINITE`` (a value is not finite), ``NOT_POSDEF`` (a Cholesky pivot fails ``> 0``), ``OK``.
* right-looking Cholesky ``A = L L^T``, ``W = L^-1`` by forward substitution, ``B = W^T W``; ``hess_jk = -A_jk / (h_j h_k)``,
  ``cov_jk = (h_j h_k) B_jk``.  NaN where the status leaves them undefined (``AT_BOUND``, ``NOT_FINITE``: A, hess, cov;
  ``NOT_POSDEF``: cov).

**At the faces of the box** the device only flags; the policy is the host's (:func:`face_steps`): a step is shrunk to 0.999 of
the distance to the nearer face while that distance is at least ``h / shrink``, and left alone - so that the device reports
``AT_BOUND`` - when the face is closer than that.  The default 1/8 is a condition, not a measurement: at ``h / 8`` the entries of A
fall by 64, which for scaled Hessians with eigenvalues of order 0.03 and more leaves them several orders above the rounding
of the values they are differences of.

**What it does not do.**  The Hessian of a likelihood that is kinked in a parameter (beta across a node of a tabulated
covariance: DESIGN.md section 7a) is whatever the stencil straddles - finite, and not flagged.  Fix that parameter or choose
the steps knowingly.  Under a :class:`victor_amd.priors.GaussianPrior` the evidence is not formed (the truncated Gaussian's
normalisation is out of scope): ``ln_evidence`` is None.
"""

import ctypes as C

import numpy as np

from . import _native as N
from .fitting import _per_problem, _Sampled
from .utils import InputError

OK, AT_BOUND, NOT_FINITE, NOT_POSDEF = N.VK_HESS_OK, N.VK_HESS_AT_BOUND, N.VK_HESS_NOT_FINITE, N.VK_HESS_NOT_POSDEF
MAX_PARAMS = 10
PROPOSAL_SCALE = 2.38          # the random-walk scale of Gelman, Roberts & Gilks (1996): 2.38 / sqrt(d) times the target's factor


# ---------------------------------------------------------------------- the NumPy statement of vk_hessian.h -----------------
def n_points(d):
    return 2 * d * d + 1


def pair_index(d, j, k):
    """Number of the pair ``j < k``."""
    return j * d - j * (j + 1) // 2 + (k - j - 1)


def at_axis(j, s):
    return 1 + 2 * j + s


def at_pair(d, j, k, c):
    return 1 + 2 * d + 4 * pair_index(d, j, k) + c


def decode(d, m):
    """``(j, k, sj, sk)`` of stencil point ``m``: coordinate j moves by ``sj h_j`` and k by ``sk h_k`` (-1: none)."""
    if m <= 0:
        return -1, -1, 0, 0
    if m < 1 + 2 * d:
        return (m - 1) // 2, -1, (-1 if (m - 1) % 2 else 1), 0
    t = m - 1 - 2 * d
    c, rem, j = t % 4, t // 4, 0
    while rem >= d - 1 - j:
        rem -= d - 1 - j
        j += 1
    return j, j + 1 + rem, (-1 if c // 2 else 1), (-1 if c % 2 else 1)


def at_bound(x, h, lo, hi):
    """``(R,)``: does the stencil of each problem leave the box (or is ``x`` outside it)?"""
    x, h = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_2d(np.asarray(h, dtype=float))
    return np.any(~(x >= lo) | ~(x <= hi) | (x - h < lo) | (x + h > hi), axis=1)


def stencil_points(x, h, lo=None, hi=None):
    """``(R, M, d)``: the stencil points of R problems at ``x`` (R, d) with steps ``h`` (R, d).  With a box, a problem whose
    stencil leaves it has every point at ``x`` - the rows the device evaluates."""
    x, h = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_2d(np.asarray(h, dtype=float))
    R, d = x.shape
    pts = np.repeat(x[:, None, :], n_points(d), axis=1)
    plus, minus = x + h, x - h
    for m in range(1, n_points(d)):
        j, k, sj, sk = decode(d, m)
        pts[:, m, j] = (plus if sj > 0 else minus)[:, j]
        if k >= 0:
            pts[:, m, k] = (plus if sk > 0 else minus)[:, k]
    if lo is not None:
        pts[at_bound(x, h, lo, hi)] = x[at_bound(x, h, lo, hi)][:, None, :]
    return pts


class Assembled:
    """What :func:`assemble` returns: ``a``, ``hess``, ``cov`` (R, d, d), ``status`` (R,) and the Cholesky factor ``chol`` and
    its inverse ``winv`` (lower triangles; meaningful where the status is ``OK``)."""

    def __init__(self, a, hess, cov, status, chol, winv):
        self.a, self.hess, self.cov, self.status, self.chol, self.winv = a, hess, cov, status, chol, winv


def assemble(values, x, h, lo, hi):
    """The statistic of ``vkhess::assemble``, elementwise over R problems: ``values`` (R, M), ``x``, ``h`` (R, d), the box."""
    v = np.atleast_2d(np.asarray(values, dtype=float))
    x, h = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_2d(np.asarray(h, dtype=float))
    R, d = x.shape
    if v.shape != (R, n_points(d)):
        raise InputError(f"assemble: {n_points(d)} values per problem are needed")
    status = np.zeros(R, dtype=np.int32)
    bound = at_bound(x, h, lo, hi)
    bad = ~np.all(np.isfinite(v), axis=1)
    A, S = np.zeros((R, d, d)), np.zeros((R, d, d))
    L, W, B = np.zeros((R, d, d)), np.zeros((R, d, d)), np.zeros((R, d, d))
    with np.errstate(all="ignore"):
        for j in range(d):
            A[:, j, j] = ((v[:, 0] + v[:, 0]) - v[:, at_axis(j, 0)]) - v[:, at_axis(j, 1)]
            for k in range(j):
                pp, pm, mp, mm = (v[:, at_pair(d, k, j, c)] for c in range(4))
                A[:, j, k] = A[:, k, j] = 0.25 * ((pm - pp) + (mp - mm))
        hh = h[:, :, None] * h[:, None, :]
        hess = -A / hh
        S[:] = A
        posdef = np.ones(R, dtype=bool)
        for c in range(d):
            posdef &= S[:, c, c] > 0.0
            L[:, c, c] = np.sqrt(S[:, c, c])
            for j in range(c + 1, d):
                L[:, j, c] = S[:, j, c] / L[:, c, c]
            for j in range(c + 1, d):
                for k in range(c + 1, j + 1):
                    t = L[:, j, c] * L[:, k, c]
                    S[:, j, k] = S[:, j, k] - t
        for c in range(d):
            W[:, c, c] = 1.0 / L[:, c, c]
            for j in range(c + 1, d):
                s = L[:, j, c] * W[:, c, c]
                for m in range(c + 1, j):
                    t = L[:, j, m] * W[:, m, c]
                    s = s + t
                W[:, j, c] = -s / L[:, j, j]
        for j in range(d):
            for k in range(j + 1):
                s = W[:, j, j] * W[:, j, k]
                for m in range(j + 1, d):
                    t = W[:, m, j] * W[:, m, k]
                    s = s + t
                B[:, j, k] = B[:, k, j] = s
        cov = hh * B
    status[~posdef] = NOT_POSDEF
    status[bad] = NOT_FINITE
    status[bound] = AT_BOUND
    none = bound | bad
    A[none], hess[none] = np.nan, np.nan
    cov[status != OK] = np.nan
    return Assembled(A, hess, cov, status, L, W)


def face_steps(x, step, lo, hi, shrink=8.0):
    """The steps the stencil uses, (R, d): ``min(h, 0.999 dist)`` where the distance ``dist`` of ``x`` to the nearer face is at
    least ``h / shrink``; ``h`` itself where the face is closer (the device then reports ``AT_BOUND``)."""
    x, step = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_2d(np.asarray(step, dtype=float))
    dist = np.minimum(x - lo, hi - x)
    return np.where(dist >= step / shrink, np.minimum(step, 0.999 * dist), step)


# ---------------------------------------------------------------------- the result ------------------------------------------
class Laplace:
    """The Laplace approximation of R posteriors at the points ``x``.

    ``names``: the sampled parameters; ``x`` (R, d): the points; ``step`` (R, d): the steps the stencil used (after the face
    policy and ``refine``); ``hessian`` (R, d, d): the Hessian of lnL + ln prior; ``cov`` (R, d, d) its negative inverse,
    ``sigma`` (R, d) the square roots of its diagonal and ``corr`` (R, d, d) the correlation matrix; ``status`` (R,):
    ``Laplace.OK``, ``AT_BOUND``, ``NOT_FINITE`` or ``NOT_POSDEF`` and ``ok = status == OK`` (NaN fills what a status leaves
    undefined); ``lnpost`` (R,): lnL + ln prior at ``x`` in the device's bits, ``lnprior`` the prior evaluated on the host
    (zeros without one), ``lnl = lnpost - lnprior``, ``chi2`` the chi-square at ``x``; ``a`` (R, d, d) the scaled negative
    Hessian the covariance was inverted from; ``values`` (R, M): the stencil's values (``keep_values=True``, else None);
    ``params``: name -> (R,) array of every sampled and fixed value.

    ``ln_evidence`` (R,): the Gaussian integral of the approximation over the whole space under the uniform prior of the
    box, ``lnpost + d/2 ln 2 pi - 1/2 ln det(-H) - sum_j ln(hi_j - lo_j)`` (NaN where the status is not ``OK``); None under a
    Gaussian prior, whose truncated normalisation the project leaves out of scope."""

    OK, AT_BOUND, NOT_FINITE, NOT_POSDEF = OK, AT_BOUND, NOT_FINITE, NOT_POSDEF

    def __init__(self, names, x, step, fixed, a, hess, cov, status, lnpost, chi2, lo, hi, lnprior=None, values=None):
        self.names = list(names)
        self.x, self.step, self.a, self.hessian, self.cov = x, step, a, hess, cov
        self.status = status
        self.ok = status == OK
        self.lnpost, self.chi2, self.values = lnpost, chi2, values
        self.lnprior = np.zeros(len(x)) if lnprior is None else lnprior
        self.lnl = lnpost if lnprior is None else lnpost - lnprior
        self.lo, self.hi = np.array(lo, dtype=float), np.array(hi, dtype=float)
        self.params = {name: x[:, j].copy() for j, name in enumerate(self.names)}
        self.params.update(fixed)
        d = len(self.names)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.sigma = np.sqrt(np.einsum("rjj->rj", cov))
            self.corr = cov / (self.sigma[:, :, None] * self.sigma[:, None, :])
        if lnprior is not None:
            self.ln_evidence = None
        else:
            self.ln_evidence = np.full(len(x), np.nan)
            if np.any(self.ok):
                sign, logdet = np.linalg.slogdet(-hess[self.ok])
                ev = lnpost[self.ok] + 0.5 * d * np.log(2.0 * np.pi) - 0.5 * logdet - np.sum(np.log(self.hi - self.lo))
                self.ln_evidence[self.ok] = np.where(sign > 0, ev, np.nan)

    def __len__(self):
        return len(self.x)

    def point(self, i):
        """The sampled and fixed values of problem ``i`` as the dict of scalars ``log_likelihood`` takes."""
        return {name: float(v[i]) for name, v in self.params.items()}

    def proposal_factors(self, width):
        """``(R, d, d)``: the factor F_r of a correlated Metropolis proposal ``dz = F_r normal(d)``:
        ``(2.38 / sqrt(d)) chol(cov_r)`` where the status is ``OK``, ``diag(width)`` elsewhere."""
        d = len(self.names)
        F = np.repeat(np.diag(np.asarray(width, dtype=float))[None], len(self), axis=0)
        for r in np.flatnonzero(self.ok):
            try:
                F[r] = PROPOSAL_SCALE / np.sqrt(d) * np.linalg.cholesky(self.cov[r])
            except np.linalg.LinAlgError:         # (cov is the rounded inverse of a positive definite matrix: keep the widths)
                pass
        return F


# ---------------------------------------------------------------------- the call --------------------------------------------
def check_policy(who, shrink, refine):
    try:
        shrink, n = float(shrink), int(refine)
    except (TypeError, ValueError):
        raise InputError(f"{who}: shrink must be a number and refine an integer") from None
    if not (np.isfinite(shrink) and shrink >= 1.0):
        raise InputError(f"{who}: shrink must be finite and >= 1 (a step is shrunk down to step / shrink at a face)")
    if n < 0 or n != refine:
        raise InputError(f"{who}: refine must be an integer >= 0")
    return shrink, n


def resolve_steps(q, step, R):
    """``(R, d)`` requested steps: ``step`` (name -> scalar or (R,)) over the block's proposal widths."""
    given = dict(step or {})
    out = np.empty((R, len(q.names)))
    for j, s in enumerate(q.specs):
        out[:, j] = _per_problem(f"step of {s.name}", given.pop(s.name, s.proposal), R, f"{q.who}: ")
    if given:
        raise InputError(f"{q.who}: step names parameters that are not {q.verb}: {sorted(given)}")
    if np.any(~(out > 0)) or not np.all(np.isfinite(out)):
        raise InputError(f"{q.who}: every step must be finite and > 0")
    return out


def resolve_points(q, at, R):
    """``(R, d)`` points from ``at``: a :class:`victor_amd.fitting.BestFit` (its fitted parameters must be the sampled ones) or
    a dict name -> scalar or (R,)."""
    if at is None:
        raise InputError(f"{q.who}: at= is needed: a BestFit or a dict name -> value")
    if hasattr(at, "params") and hasattr(at, "names"):
        if list(at.names) != list(q.names):
            raise InputError(f"{q.who}: at= holds the parameters {list(at.names)}, this call samples {list(q.names)}: pass the "
                             "same params block and the same fixed=")
        given = {n: at.params[n] for n in q.names}
    else:
        try:
            given = dict(at)
        except (TypeError, ValueError):
            raise InputError(f"{q.who}: at= must be a BestFit or a dict name -> value") from None
    x = np.empty((R, len(q.names)))
    for j, name in enumerate(q.names):
        if name not in given:
            raise InputError(f"{q.who}: at= gives no value of {name}")
        x[:, j] = _per_problem(f"at of {name}", given.pop(name), R, f"{q.who}: ")
    if given:
        raise InputError(f"{q.who}: at= names parameters that are not {q.verb}: {sorted(given)}")
    if not np.all(np.isfinite(x)):
        raise InputError(f"{q.who}: at= holds values that are not finite")
    bad = ~(x >= q.lo) | ~(x <= q.hi)
    if np.any(bad):
        p, j = np.argwhere(bad)[0]
        raise InputError(f"{q.who}: the point of {q.names[j]} ({x[p, j]}) of problem {p} is outside its prior [{q.lo[j]}, {q.hi[j]}]")
    return x


def run_passes(q, x, requested, shrink, refine, keep_values, prior, fixed_out, one_pass):
    """The passes of one call: ``one_pass(h) -> (values, a, hess, cov, lnpost, chi2, status)`` at the steps ``h`` (R, d), first
    at the requested steps under the face policy, then ``refine`` times at half the previous pass's sigma where it was OK."""
    for n in range(refine + 1):
        h = face_steps(x, requested, q.lo, q.hi, shrink)
        values, a, hess, cov, lnpost, chi2, status = one_pass(h)
        if n < refine:
            ok = status == OK
            with np.errstate(invalid="ignore"):
                sigma = np.sqrt(np.einsum("rjj->rj", cov))
            good = ok[:, None] & np.isfinite(sigma) & (sigma > 0)
            requested = np.where(good, 0.5 * sigma, requested)
    return Laplace(q.names, x, h, fixed_out, a, hess, cov, status, lnpost, chi2, q.lo, q.hi,
                   None if prior is None else prior.lnprior(x), values if keep_values else None)


def device_pass(lib, handle, x, R, d):
    """``one_pass`` of :func:`run_passes` on a ``vk_fit`` handle."""
    M = int(lib.vk_hessian_rows(d))
    xs = N.f64(x)

    def one_pass(h):
        values = np.empty((R, M))
        a, hess, cov = np.empty((R, d, d)), np.empty((R, d, d)), np.empty((R, d, d))
        lnpost, chi2, status = np.empty(R), np.empty(R), np.empty(R, dtype=np.int32)
        rc = lib.vk_fit_hessian(handle, N.as_dp(xs), N.as_dp(N.f64(h)), N.as_dp(values), N.as_dp(a), N.as_dp(hess), N.as_dp(cov),
                                N.as_dp(lnpost), N.as_dp(chi2), status.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            msg = (lib.vk_fit_last_error(handle) or b"").decode() or f"vk_fit_hessian failed ({rc})"
            raise (InputError if rc == -1 else N.NativeError)(msg)
        return values, a, hess, cov, lnpost, chi2, status
    return one_pass


def host_pass(q, evaluator, x, prior):
    """``one_pass`` of :func:`run_passes` on the host: the stencil's rows through ``evaluator(points (n, d), which (n,))``, the
    statistic by :func:`assemble` - the definition the device route is held to."""
    R, d = x.shape
    M = n_points(d)
    which = np.repeat(np.arange(R, dtype=np.int32), M)

    def one_pass(h):
        pts = stencil_points(x, h, q.lo, q.hi)
        lnl, chi2 = evaluator(pts.reshape(R * M, d), which)
        values = np.asarray(lnl, dtype=float).reshape(R, M)
        if prior is not None:
            values = values + prior.lnprior(pts)
        out = assemble(values, x, h, q.lo, q.hi)
        return values, out.a, out.hess, out.cov, values[:, 0].copy(), np.asarray(chi2, dtype=float).reshape(R, M)[:, 0].copy(), out.status
    return one_pass


def laplace(fit, params, at, step=None, fixed=None, prior=None, shrink=8, refine=0, keep_values=False, kwargs=None,
            realisations=None, device=True, evaluate=None):
    """The work of the four ``laplace`` methods (``realisations=None``: against the fit's data vector; a ``JointFit`` for ``fit``:
    the joint lnL).  ``params``: the cobaya block; ``at``: a :class:`victor_amd.fitting.BestFit` or a dict name -> scalar or
    ``(R,)``; ``step``: name -> scalar or ``(R,)``, default the block's proposal widths; ``fixed``: as ``best_fit``; ``prior``: a
    :class:`victor_amd.priors.GaussianPrior` or a list, added to lnL at every stencil point; ``shrink``, ``refine``: the module
    docstring.  ``device=False`` evaluates the same stencil on the host through ``log_likelihood_batch`` /
    ``log_likelihood_pairs`` and :func:`assemble`; with ``evaluate`` - a callable taking a dict of ``(n,)`` arrays and returning
    lnL or (lnL, chi2) - in place of ``fit`` only that route is possible and no GPU is needed.  Every argument is checked before
    the first device call.  Returns a :class:`Laplace`."""
    kwargs = kwargs or {}
    q = _Sampled("laplace", "sampled", params, fixed)
    names, fixed_all, d = q.names, q.fixed_all, len(q.names)
    if evaluate is not None and device:
        raise InputError("laplace: an evaluate callable runs the host route only (device=False)")
    if evaluate is None and fit is None:
        raise InputError("laplace: a fit or an evaluate callable is needed")
    if evaluate is None:
        q.check_columns(fit)
    if d > MAX_PARAMS:
        raise InputError(f"laplace: at most {MAX_PARAMS} sampled parameters")
    arrays = {k: v for k, v in fixed_all.items() if np.ndim(v) > 0}
    if realisations is not None:
        if arrays:
            raise InputError(f"laplace: fixed values must be scalars against realisations ({sorted(arrays)} are not)")
        R = len(realisations)
        if hasattr(at, "names") and hasattr(at, "x") and len(at.x) != R:
            raise InputError(f"laplace: at= holds {len(at.x)} problems, there are {R} realisations")
    else:
        lengths = {len(np.atleast_1d(v)) for v in arrays.values()}
        if hasattr(at, "names") and hasattr(at, "x"):
            lengths.add(len(at.x))
        elif isinstance(at, dict):
            lengths |= {len(np.atleast_1d(v)) for v in at.values() if np.ndim(v) > 0}
        if isinstance(step, dict):
            lengths |= {len(np.atleast_1d(v)) for v in step.values() if np.ndim(v) > 0}
        if len(lengths) > 1:
            raise InputError(f"laplace: at=, step= and fixed arrays have different lengths: {sorted(lengths)}")
        R = lengths.pop() if lengths else 1
    if evaluate is None:
        q.check_alpha()
    prior = q.prior(prior, fit)
    shrink, refine = check_policy("laplace", shrink, refine)
    if evaluate is None:
        fit_options = q.fit_options(fit, kwargs)
    x = resolve_points(q, at, R)
    requested = resolve_steps(q, step, R)
    fixed_out = {k: _per_problem(k, v, R) for k, v in fixed_all.items()}

    def batch_of(pts, rows=None):
        batch = {k: (v if rows is None or np.ndim(v) == 0 else np.asarray(v)[rows]) for k, v in fixed_all.items()}
        batch.update({n: np.ascontiguousarray(pts[:, j]) for j, n in enumerate(names)})
        return batch

    if not device:
        if evaluate is not None:
            def evaluator(pts, which):
                out = evaluate(batch_of(pts, which))
                if isinstance(out, tuple):
                    return np.asarray(out[0], dtype=float), np.asarray(out[1], dtype=float)
                lnl = np.asarray(out, dtype=float)
                return lnl, -2.0 * lnl
        elif realisations is not None:
            def evaluator(pts, which):
                return realisations.log_likelihood_pairs(batch_of(pts, which), which, **kwargs)
        else:
            def evaluator(pts, which):
                return fit.log_likelihood_batch(batch_of(pts, which), **kwargs)
        return run_passes(q, x, requested, shrink, refine, keep_values, prior, fixed_out, host_pass(q, evaluator, x, prior))

    # ---- device
    lib, h, _ = q.create("vk_fit_create", fit, realisations, kwargs, fit_options, batch_of(x), np.arange(R, dtype=np.int32))
    try:
        if prior is not None:
            q.set_prior("vk_fit_set_prior", lib, h, prior)
        return run_passes(q, x, requested, shrink, refine, keep_values, prior, fixed_out, device_pass(lib, h, x, R, d))
    finally:
        lib.vk_fit_destroy(h)


def resolve_covariance(covariance, q, R):
    """The ``covariance=`` argument of ``best_fit``: None / False (off), True or a dict ``{"step", "shrink", "refine",
    "keep_values"}`` -> None or ``(requested steps (R, d), shrink, refine, keep_values)``; refusals as ``InputError``."""
    if covariance is None or covariance is False:
        return None
    opts = {} if covariance is True else covariance
    if not isinstance(opts, dict):
        raise InputError(f"{q.who}: covariance must be True or a dict with the keys step, shrink, refine, keep_values")
    unknown = sorted(set(opts) - {"step", "shrink", "refine", "keep_values"})
    if unknown:
        raise InputError(f"{q.who}: covariance has unknown keys {unknown} (step, shrink, refine, keep_values)")
    shrink, refine = check_policy(q.who, opts.get("shrink", 8), opts.get("refine", 0))
    return resolve_steps(q, opts.get("step"), R), shrink, refine, bool(opts.get("keep_values", False))
