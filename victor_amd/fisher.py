"""Fisher matrices from model-vector Jacobians on the GPU: the errors a model, a binning and a covariance ALLOW -
``CCFFit.fisher``, ``Realisations.fisher``, ``JointFit.fisher`` and ``JointRealisations.fisher``.

``laplace`` answers what a data vector says about the parameters: it differentiates lnL twice, ``2 d^2 + 1`` rows per problem,
and noise in the data enters its curvature.  The forecast is the Fisher matrix ``F = J^T P J`` with
``J = d(theory vector)/d(theta)``: first differences of a vector, ``M = 2 d + 1`` rows per problem, positive semi-definite by
construction and independent of any data.  ``vk_fit_fisher`` (``include/victor_hip.h``) forms the R M rows
on the device, evaluates their theory vectors with the launches every evaluation makes, and assembles ``fisher``, ``a``, ``cov``
and a status per problem in one kernel, a workgroup per problem.  The Jacobian itself - the response ``d xi_ell(s)/d fsigma8``
and its siblings - comes back with ``keep_vectors=True``.

**The NumPy statement.**  :func:`stencil_points` and :func:`assemble` restate ``victor_amd/csrc/vk_fisher.h`` with the same
operations in the same order, elementwise over the problems, so the device, a g++ build of the header and this module agree bit
for bit on the same vectors (tests/test_fisher.py, tests/test_gpu_fisher.py):

* point ``m`` of a problem at ``x`` with steps ``h``: 0 is ``x``; ``1 + 2 j + s`` is ``x +- h_j e_j`` (``s = 0``: +) - the first
  ``2 d + 1`` points of the Hessian's stencil.
* ``D_ak = t_a(x + h_k e_k) - t_a(x - h_k e_k)``: the division by ``2 h`` is folded into the ``d x d`` scaling.
* ``P``: the precision the chi-square uses at the centre's beta - a fixed covariance's one slice; of a beta-gridded one, with
  the class's ``_bracket`` ``(lo, t)``, ``P_lo`` where ``t == 0``, else ``(1 - t) P_lo + t P_last``.  Block-diagonal over the
  blocks of a block-diagonal joint fit (each at the beta of its own row), one matrix under a joint covariance.
* ``G_ak = sum_b P_ab D_bk`` (ascending b through the block of a), ``S_jk = sum_a D_aj G_ak`` (ascending a, ``j >= k``,
  mirrored); every sum starts from its first term, each product rounded, then added.
* ``c = -2 dlnL/dchi2`` at ``chi2 = 0`` of the likelihood form (:func:`form_scale`): exact where data = model.
* ``fisher_jk = (0.25 c) S_jk / (h_j h_k)``; ``A_jk = (0.25 c) S_jk + Lambda_jk (h_j h_k)`` with ``Lambda`` the precision of the
  Gaussian prior (absent without one); Cholesky of A and ``B = A^-1`` as ``vk_hessian.h``; ``cov_jk = (h_j h_k) B_jk``.
* status, in this precedence: ``AT_BOUND`` (the stencil leaves the box: every row is formed at ``x``), ``NOT_FINITE`` (an entry
  of the M vectors is not finite), ``NOT_POSDEF`` (a Cholesky pivot fails ``> 0``: ``fisher`` and ``a`` given, ``cov`` NaN - a
  parameter the theory does not depend on has ``S_jj = 0`` exactly and reads this), ``OK``.

At the faces of the box the policy is ``laplace``'s (:func:`victor_amd.laplace.face_steps`, ``shrink``).

**What it does not do.**  The data vector's and the covariance's own beta-dependence is held at the centre: there is no
``d(data)/d(beta)``, no log-determinant term and no trace term.  No one-sided stencils at a face.  No prior per problem (one
``prior=`` for all of them).  No proposals for chains from a :class:`Fisher` (``sample_chains(proposal=...)`` takes widths or a
``Laplace``).  A block-diagonal joint fit whose blocks would scale their chi-squares differently (hartlap / percival with
blocks of different lengths) has no one ``c`` and is refused.
"""

import ctypes as C

import numpy as np

from . import _native as N
from .fitting import _per_problem, _Sampled
from .laplace import AT_BOUND, MAX_PARAMS, NOT_FINITE, NOT_POSDEF, OK, at_bound, check_policy, face_steps, resolve_points, resolve_steps
from .laplace import stencil_points as _hessian_points
from .utils import InputError


# ---------------------------------------------------------------------- the NumPy statement of vk_fisher.h ------------------
def n_rows(d):
    return 2 * d + 1


def stencil_points(x, h, lo=None, hi=None):
    """``(R, M, d)``: the ``M = 2 d + 1`` stencil points of R problems at ``x`` (R, d) with steps ``h`` (R, d) - the first
    ``2 d + 1`` of the Hessian's.  With a box, a problem whose stencil leaves it has every point at ``x``."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    return _hessian_points(x, h, lo, hi)[:, :n_rows(x.shape[1])]


def form_scale(form, nmocks=1.0, nparams=0.0, nd=0.0):
    """``c = -2 dlnL/dchi2`` at ``chi2 = 0``: ``form`` a name or a ``VK_LIKE_*`` code; ``nd`` the entries of the vector."""
    form = N.LIKE[form.lower()] if isinstance(form, str) else int(form)
    nm, npar, nd = float(nmocks), float(nparams), float(nd)
    if form == N.LIKE["sellentin"]:
        return nm / (nm - 1.0)
    if form == N.LIKE["hartlap"]:
        return (nm - nd - 2.0) / (nm - 1.0)
    if form == N.LIKE["percival"]:
        B = (nm - nd - 2.0) / ((nm - nd - 1.0) * (nm - nd - 4.0))
        m = npar + 2.0 + (nm - 1.0 + B * (nd - npar)) / (1.0 + B * (nd - npar))
        return m / (nm - 1.0)
    return 1.0


class Block:
    """One diagonal block of the precision: entries ``off .. off + n - 1`` of the vector meet ``p_lo`` ((n, n) or (R, n, n)),
    blended with ``p_last`` by the weights ``t`` (R,) where ``t != 0`` (``t=None``: one fixed slice)."""

    def __init__(self, off, p_lo, p_last=None, t=None):
        self.off, self.p_lo, self.p_last, self.t = int(off), np.asarray(p_lo, dtype=float), p_last, t
        self.n = self.p_lo.shape[-1]

    def precision(self, R):
        """``(R, n, n)``: ``P_lo`` where ``t == 0``, else ``(1 - t) P_lo + t P_last``, each product rounded, then the sum."""
        p_lo = np.broadcast_to(self.p_lo, (R, self.n, self.n))
        if self.t is None:
            return p_lo
        t = np.broadcast_to(np.asarray(self.t, dtype=float), (R,))[:, None, None]
        p_last = np.broadcast_to(np.asarray(self.p_last, dtype=float), (R, self.n, self.n))
        with np.errstate(all="ignore"):
            u = (1.0 - t) * p_lo
            v = t * p_last
            return np.where(t == 0.0, p_lo, u + v)


def lambda_matrix(pp, d):
    """``(d, d)`` precision of a prior from its packed triangle (off-diagonal entries doubled: halving is exact)."""
    from .priors import tri
    lam = np.zeros((d, d))
    for j in range(d):
        for k in range(j + 1):
            lam[j, k] = lam[k, j] = pp[tri(d, k, j)] if j == k else 0.5 * pp[tri(d, k, j)]
    return lam


class Assembled:
    """What :func:`assemble` returns: ``D``, ``G`` (R, N, d), ``S``, ``fisher``, ``a``, ``cov`` (R, d, d), ``status`` (R,) and
    the Cholesky factor ``chol`` and its inverse ``winv`` (lower triangles; meaningful where the status is ``OK``)."""

    def __init__(self, D, G, S, fisher, a, cov, status, chol, winv):
        self.D, self.G, self.S, self.fisher, self.a, self.cov = D, G, S, fisher, a, cov
        self.status, self.chol, self.winv = status, chol, winv


def assemble(vectors, x, h, lo, hi, blocks, scale=1.0, prior_pp=None):
    """The statistic of ``vkfisher::assemble``, elementwise over R problems: ``vectors`` (R, M, N), ``x``, ``h`` (R, d), the box,
    the precision's :class:`Block` list (or one (N, N) array), the scale ``c`` and the packed triangle of a prior."""
    v = np.asarray(vectors, dtype=float)
    x, h = np.atleast_2d(np.asarray(x, dtype=float)), np.atleast_2d(np.asarray(h, dtype=float))
    R, d = x.shape
    if v.ndim != 3 or v.shape[:2] != (R, n_rows(d)):
        raise InputError(f"assemble: {n_rows(d)} vectors per problem are needed")
    Nv = v.shape[2]
    if isinstance(blocks, np.ndarray):
        blocks = [Block(0, blocks)]
    status = np.zeros(R, dtype=np.int32)
    bound = at_bound(x, h, lo, hi)
    bad = ~np.all(np.isfinite(v), axis=(1, 2))
    G = np.zeros((R, Nv, d))
    L, W, B = np.zeros((R, d, d)), np.zeros((R, d, d)), np.zeros((R, d, d))
    with np.errstate(all="ignore"):
        D = np.moveaxis(v[:, 1:2 * d + 1:2] - v[:, 2:2 * d + 1:2], 1, 2).copy()      # (R, N, d)
        for b in blocks:
            P = b.precision(R)
            Db = D[:, b.off:b.off + b.n]
            s = P[:, :, 0, None] * Db[:, None, 0, :]
            for i in range(1, b.n):
                t = P[:, :, i, None] * Db[:, None, i, :]
                s = s + t
            G[:, b.off:b.off + b.n] = s
        S = D[:, 0, :, None] * G[:, 0, None, :]
        for a in range(1, Nv):
            t = D[:, a, :, None] * G[:, a, None, :]
            S = S + t
        S = np.where(np.tril(np.ones((d, d), dtype=bool)), S, np.swapaxes(S, 1, 2))       # (j >= k, mirrored: signed zeros kept)
        hh = h[:, :, None] * h[:, None, :]
        q = 0.25 * float(scale)
        u = q * S
        fisher = u / hh
        if prior_pp is None:
            A = u.copy()
        else:
            w = lambda_matrix(prior_pp, d)[None] * hh
            A = u + w
        T = A.copy()
        posdef = np.ones(R, dtype=bool)
        for c in range(d):
            posdef &= T[:, c, c] > 0.0
            L[:, c, c] = np.sqrt(T[:, c, c])
            for j in range(c + 1, d):
                L[:, j, c] = T[:, j, c] / L[:, c, c]
            for j in range(c + 1, d):
                for k in range(c + 1, j + 1):
                    t = L[:, j, c] * L[:, k, c]
                    T[:, j, k] = T[:, j, k] - t
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
    D[none], G[none], S[none], fisher[none], A[none] = np.nan, np.nan, np.nan, np.nan, np.nan
    cov[status != OK] = np.nan
    return Assembled(D, G, S, fisher, A, cov, status, L, W)


# ---------------------------------------------------------------------- the result ------------------------------------------
class Fisher:
    """The Fisher forecast of R problems at the points ``x``.

    ``names``: the sampled parameters; ``x`` (R, d): the points; ``step`` (R, d): the steps the stencil used (after the face
    policy); ``fisher`` (R, d, d): the likelihood's information ``c J^T P J``; ``a`` (R, d, d): ``(fisher + Lambda) o (h h^T)``,
    what was inverted; ``cov`` (R, d, d) the inverse of ``fisher + Lambda``, ``sigma`` (R, d) the square roots of its diagonal
    (the marginal errors) and ``corr`` the correlation matrix; ``conditional_sigma`` (R, d): ``1 / sqrt(diag(fisher + Lambda))``,
    the error of each parameter with the others held; ``status`` (R,): ``Fisher.OK``, ``AT_BOUND``, ``NOT_FINITE`` or
    ``NOT_POSDEF`` and ``ok = status == OK`` (NaN fills what a status leaves undefined); ``scale``: the ``c`` of the likelihood
    form; ``model`` (R, N): the theory vectors at the points; ``jacobian`` (R, N, d) ``= D / (2 h)`` and ``vectors`` (R, M, N), the
    stencil's theory vectors (both with ``keep_vectors=True``, else None); ``params``: name -> (R,) array of every sampled and
    fixed value."""

    OK, AT_BOUND, NOT_FINITE, NOT_POSDEF = OK, AT_BOUND, NOT_FINITE, NOT_POSDEF

    def __init__(self, names, x, step, fixed, fisher, a, cov, status, scale, model, lo, hi, prior_precision=None, vectors=None):
        self.names = list(names)
        self.x, self.step, self.fisher, self.a, self.cov = x, step, fisher, a, cov
        self.status = status
        self.ok = status == OK
        self.scale, self.model, self.vectors = float(scale), model, vectors
        self.lo, self.hi = np.array(lo, dtype=float), np.array(hi, dtype=float)
        self.params = {name: x[:, j].copy() for j, name in enumerate(self.names)}
        self.params.update(fixed)
        d = len(self.names)
        self.jacobian = None
        with np.errstate(invalid="ignore", divide="ignore"):
            self.sigma = np.sqrt(np.einsum("rjj->rj", cov))
            self.corr = cov / (self.sigma[:, :, None] * self.sigma[:, None, :])
            total = fisher if prior_precision is None else fisher + prior_precision[None]
            self.conditional_sigma = 1.0 / np.sqrt(np.einsum("rjj->rj", total))
            if vectors is not None:
                D = np.moveaxis(vectors[:, 1:2 * d + 1:2] - vectors[:, 2:2 * d + 1:2], 1, 2)
                self.jacobian = D / (2.0 * step[:, None, :])

    def __len__(self):
        return len(self.x)

    def point(self, i):
        """The sampled and fixed values of problem ``i`` as the dict of scalars ``log_likelihood`` takes."""
        return {name: float(v[i]) for name, v in self.params.items()}


# ---------------------------------------------------------------------- the call --------------------------------------------
def _like_scale(like, nd):
    form = str(like["form"]).lower()
    if form not in N.LIKE:
        raise InputError("Unrecognised likelihood form")
    return form_scale(form, like.get("nmocks", 1), like["nparams"] if form == "percival" else 0.0, nd)


def _n_data(fit):
    return len(fit.s) * len(fit.poles_s)


def resolve_scale(fit, kwargs):
    """``c`` of a fit's likelihood form under the call's options; of a block-diagonal joint fit the blocks' common value
    (``InputError`` where they differ)."""
    from .joint import JointFit
    if not isinstance(fit, JointFit):
        return _like_scale(fit._merged_fit(kwargs)["likelihood"], _n_data(fit))
    if fit.covariance is not None:
        return _like_scale(kwargs.get("likelihood", fit.likelihood), fit.n_data)
    scales = [_like_scale(f._merged_fit(kwargs)["likelihood"], _n_data(f)) for f in fit.fits]
    if any(s != scales[0] for s in scales):
        raise InputError("fisher: the blocks of a block-diagonal joint fit scale their chi-squares differently under this "
                         f"likelihood form ({scales}): there is no one scale")
    return scales[0]


def _bracketed(owner, beta, off, R):
    """The :class:`Block` of ``owner`` (a ``CCFFit`` or a ``JointFit`` under a covariance) at the centres' ``beta`` (R,)."""
    if owner.fixed_covmat:
        return Block(off, owner.icov)
    if beta is None:
        raise InputError("Need to supply a valid value of beta for interpolation")
    lo_t = [owner._bracket(float(b)) for b in beta]
    lo = np.array([p[0] for p in lo_t])
    return Block(off, np.asarray(owner.icov)[lo], np.asarray(owner.icov)[-1], np.array([p[1] for p in lo_t], dtype=float))


def host_vectors(fit, batch, kwargs):
    """The theory vectors (n, N) of a batch through ``theory_vector_batch`` - per block for a joint fit, concatenated in the
    joint's order."""
    from .joint import JointFit, block_params
    if not isinstance(fit, JointFit):
        return np.asarray(fit.theory_vector_batch(batch, **kwargs))
    kw = {k: v for k, v in kwargs.items() if k != "likelihood"} if fit.covariance is not None else kwargs
    return np.concatenate([np.asarray(f.theory_vector_batch(block_params(batch, b), **kw)) for b, f in enumerate(fit.fits)], axis=1)


def host_blocks(fit, centres, R):
    """The precision's :class:`Block` list at the centres (``centres``: name -> (R,) of every sampled and fixed value): a
    single fit's, a joint covariance's at block 0's beta, or a block-diagonal joint fit's blocks each at its own beta."""
    from .joint import JointFit, block_params
    if not isinstance(fit, JointFit):
        return [_bracketed(fit, centres.get("beta"), 0, R)]
    if fit.covariance is not None:
        return [_bracketed(fit, block_params(centres, 0).get("beta"), 0, R)]
    blocks, off = [], 0
    for b, f in enumerate(fit.fits):
        blocks.append(_bracketed(f, block_params(centres, b).get("beta"), off, R))
        off += _n_data(f)
    return blocks


def fisher(fit, params, at, step=None, fixed=None, prior=None, shrink=8, keep_vectors=False, kwargs=None, realisations=None,
           device=True, evaluate=None, precision=None):
    """The work of the four ``fisher`` methods (``realisations=None``: R from ``at=``, ``step=`` and ``fixed=``; with
    realisations: one problem per realisation, which supply R and nothing else - the forecast reads no data).  ``params``: the
    cobaya block; ``at``: a :class:`victor_amd.fitting.BestFit` or a dict name -> scalar or ``(R,)``; ``step``: name -> scalar or
    ``(R,)``, default the block's proposal widths; ``fixed``: as ``best_fit``; ``prior``: a
    :class:`victor_amd.priors.GaussianPrior` or a list, whose precision is added to the information; ``shrink``: the face policy
    of ``laplace``; ``keep_vectors``: return the stencil's vectors and the Jacobian.  ``device=False`` is the definition route:
    the stencil's vectors through ``theory_vector_batch`` (per block for a joint fit), the precision with the class's own
    ``_bracket``, then :func:`assemble`; with ``evaluate`` - a callable from a dict of ``(n,)`` arrays to ``(n, N)`` vectors - and
    ``precision``, an ``(N, N)`` array, in place of ``fit`` only that route is possible, the scale is 1 and no GPU is needed.
    Every argument is checked before the first device call.  Returns a :class:`Fisher`."""
    kwargs = kwargs or {}
    q = _Sampled("fisher", "sampled", params, fixed)
    names, fixed_all, d = q.names, q.fixed_all, len(q.names)
    if evaluate is not None and device:
        raise InputError("fisher: an evaluate callable runs the host route only (device=False)")
    if evaluate is None and fit is None:
        raise InputError("fisher: a fit or an evaluate callable is needed")
    if (evaluate is None) != (precision is None):
        raise InputError("fisher: evaluate= and precision= go together (the vectors and the (N, N) precision they meet)")
    if evaluate is None:
        q.check_columns(fit)
    if d > MAX_PARAMS:
        raise InputError(f"fisher: at most {MAX_PARAMS} sampled parameters")
    arrays = {k: v for k, v in fixed_all.items() if np.ndim(v) > 0}
    if realisations is not None:
        if arrays:
            raise InputError(f"fisher: fixed values must be scalars against realisations ({sorted(arrays)} are not)")
        R = len(realisations)
        if hasattr(at, "names") and hasattr(at, "x") and len(at.x) != R:
            raise InputError(f"fisher: at= holds {len(at.x)} problems, there are {R} realisations")
    else:
        lengths = {len(np.atleast_1d(v)) for v in arrays.values()}
        if hasattr(at, "names") and hasattr(at, "x"):
            lengths.add(len(at.x))
        elif isinstance(at, dict):
            lengths |= {len(np.atleast_1d(v)) for v in at.values() if np.ndim(v) > 0}
        if isinstance(step, dict):
            lengths |= {len(np.atleast_1d(v)) for v in step.values() if np.ndim(v) > 0}
        if len(lengths) > 1:
            raise InputError(f"fisher: at=, step= and fixed arrays have different lengths: {sorted(lengths)}")
        R = lengths.pop() if lengths else 1
    if evaluate is None:
        q.check_alpha()
    prior = q.prior(prior, fit)
    shrink, _ = check_policy("fisher", shrink, 0)
    keep_vectors = bool(keep_vectors)
    if evaluate is None:
        fit_options = q.fit_options(fit, kwargs, "a Fisher matrix (fisher, keep_vectors)")
        scale = resolve_scale(fit, kwargs)
    else:
        scale = 1.0
        precision = np.asarray(precision, dtype=float)
        if precision.ndim != 2 or precision.shape[0] != precision.shape[1]:
            raise InputError("fisher: precision= must be an (N, N) array")
    x = resolve_points(q, at, R)
    h = face_steps(x, resolve_steps(q, step, R), q.lo, q.hi, shrink)
    fixed_out = {k: _per_problem(k, v, R) for k, v in fixed_all.items()}
    lam = None if prior is None else lambda_matrix(prior.pp, d)
    M = n_rows(d)

    def batch_of(pts, rows=None):
        batch = {k: (v if rows is None or np.ndim(v) == 0 else np.asarray(v)[rows]) for k, v in fixed_all.items()}
        batch.update({n: np.ascontiguousarray(pts[:, j]) for j, n in enumerate(names)})
        return batch

    def result(out_fisher, a, cov, status, c, model, vectors):
        return Fisher(names, x, h, fixed_out, out_fisher, a, cov, status, c, model, q.lo, q.hi, lam, vectors if keep_vectors else None)

    # realisations(paired_model=True): the vectors depend on the problem's table set, which only the device route selects - the
    # centres come back with the stencil instead of through the fit's public route
    paired = getattr(realisations, "paired_model", False)
    if not device:
        if paired and evaluate is None:
            raise InputError("fisher: the definition route (device=False) takes its theory vectors from the fit's own tables; with "
                             "realisations(paired_model=True) use the device route")
        pts = stencil_points(x, h, q.lo, q.hi).reshape(R * M, d)
        which = np.repeat(np.arange(R), M)
        if evaluate is not None:
            vecs = np.asarray(evaluate(batch_of(pts, which)), dtype=float)
            if vecs.ndim != 2 or vecs.shape != (R * M, precision.shape[0]):
                raise InputError(f"fisher: evaluate must return ({R * M}, {precision.shape[0]}) vectors for {R * M} points")
            blocks = [Block(0, precision)]
        else:
            centres = dict(fixed_out)
            centres.update({n: x[:, j] for j, n in enumerate(names)})
            vecs, blocks = host_vectors(fit, batch_of(pts, which), kwargs), host_blocks(fit, centres, R)
        vecs = np.ascontiguousarray(vecs, dtype=float).reshape(R, M, -1)
        out = assemble(vecs, x, h, q.lo, q.hi, blocks, scale, None if prior is None else prior.pp)
        return result(out.fisher, out.a, out.cov, out.status, scale, vecs[:, 0].copy(), vecs)

    # ---- device
    lib, handle, _ = q.create("vk_fit_create", fit, realisations, kwargs, fit_options, batch_of(x), np.arange(R, dtype=np.int32))
    try:
        if prior is not None:
            q.set_prior("vk_fit_set_prior", lib, handle, prior)
        if int(lib.vk_fisher_rows(d)) != M:
            raise N.NativeError("vk_fisher_rows disagrees with the NumPy statement")
        out_fisher, a, cov = np.empty((R, d, d)), np.empty((R, d, d)), np.empty((R, d, d))
        status, c = np.empty(R, dtype=np.int32), C.c_double(0.0)
        vectors = None
        if keep_vectors or paired:
            n_entries = fit.n_data if hasattr(fit, "fits") else _n_data(fit)
            vectors = np.empty((R, M, n_entries))
        rc = lib.vk_fit_fisher(handle, N.as_dp(N.f64(x)), N.as_dp(N.f64(h)), None if vectors is None else N.as_dp(vectors),
                               N.as_dp(out_fisher), N.as_dp(a), N.as_dp(cov), C.byref(c), status.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            msg = (lib.vk_fit_last_error(handle) or b"").decode() or f"vk_fit_fisher failed ({rc})"
            raise (InputError if rc == -1 else N.NativeError)(msg)
    finally:
        lib.vk_fit_destroy(handle)
    # (without keep_vectors the stencil's vectors stay on the device: the centres through the public route, equal to rounding)
    model = vectors[:, 0].copy() if vectors is not None else host_vectors(fit, batch_of(x), kwargs)
    return result(out_fisher, a, cov, status, c.value, model, vectors)
