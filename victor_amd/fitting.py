"""Best-fit points on the GPU: ``CCFFit.best_fit`` and ``Realisations.best_fit``.

The reference has no optimiser; its users maximise ``CCFFit.log_likelihood`` (reference: ``ccf_fit.py:356-483``) with a host
optimiser, one call per point and one data vector at a time.  Here every *problem* - one maximisation of lnL over the sampled
parameters inside their uniform prior box, against the fit's data vector or one simulation realisation - runs a bounded
Nelder-Mead search on the device (``vk_fit_run``, ``include/victor_hip.h``): all problems advance together,
one launch per iteration, with no host round trip per iteration.

What is maximised is the fit's own lnL, the value ``log_likelihood`` returns: the likelihood form and, for a beta-dependent
covariance, the log-determinant term are included, so with uniform priors the result is the MAP point.  The chi-square reported
is the chi-square AT that point, not a separate chi-square minimum.
"""

import ctypes as C

import numpy as np

from . import _native as N
from .sampler import parse_cobaya_params
from .utils import InputError


class BestFit:
    """Best-fit points of R problems.

    ``names``: the sampled parameters; ``x``: ``(R, d)`` best vertices; ``params``: name -> ``(R,)`` array of every sampled
    and fixed value; ``lnl``, ``chi2``: lnL and chi-square there; ``status``: ``BestFit.CONVERGED``, ``MAX_ITER`` or
    ``NO_FINITE_START`` (every start vertex failed: ``x`` is the start, lnL -inf); ``n_iter``: iterations (launches) of each
    problem; ``n_evals``: evaluations the search used (what a one-point-at-a-time Nelder-Mead evaluates)."""

    CONVERGED, MAX_ITER, NO_FINITE_START = N.VK_FIT_CONVERGED, N.VK_FIT_MAX_ITER, N.VK_FIT_NO_FINITE_START

    def __init__(self, names, x, fixed, lnl, chi2, status, n_iter, n_evals):
        self.names = list(names)
        self.x = x
        self.params = {name: x[:, j].copy() for j, name in enumerate(self.names)}
        self.params.update(fixed)
        self.lnl, self.chi2, self.status, self.n_iter, self.n_evals = lnl, chi2, status, n_iter, n_evals

    def __len__(self):
        return len(self.x)

    def point(self, i):
        """The sampled and fixed values of problem ``i`` as the dict of scalars ``log_likelihood`` takes."""
        return {name: float(v[i]) for name, v in self.params.items()}


def _per_problem(name, v, R):
    a = np.asarray(v, dtype=float)
    if a.ndim == 0:
        return np.full(R, float(a))
    if a.shape != (R,):
        raise InputError(f"{name}: one value per problem ({R}) or a scalar")
    return a


def best_fit(fit, params, fixed=None, start=None, step=None, xtol=None, ftol=1e-6, max_iter=None, restarts=1, kwargs=None,
             realisations=None):
    """The work of ``CCFFit.best_fit`` (``realisations=None``: against the fit's data vector) and ``Realisations.best_fit``.
    Every argument is checked before the first device call."""
    kwargs = kwargs or {}
    specs, block_fixed = parse_cobaya_params(params)
    fixed_in = dict(fixed or {})
    fixed_all = dict(block_fixed)
    fixed_all.update(fixed_in)
    specs = [s for s in specs if s.name not in fixed_in]
    if not specs:
        raise InputError("best_fit: every parameter is fixed")
    names = [s.name for s in specs]
    for name in names:
        if name not in N.ROW_COLUMNS and name != "epsilon":
            raise InputError(f"best_fit: {name} has no column of its own in a parameter row and cannot be fitted")
    arrays = {k: v for k, v in fixed_all.items() if np.ndim(v) > 0}
    if realisations is not None:
        if arrays:
            raise InputError(f"Realisations.best_fit: fixed values must be scalars ({sorted(arrays)} are not)")
        R = len(realisations)
    else:
        lengths = {len(np.atleast_1d(v)) for v in arrays.values()}
        if len(lengths) > 1:
            raise InputError(f"best_fit: fixed arrays have different lengths: {sorted(lengths)}")
        R = lengths.pop() if lengths else 1
    if "epsilon" in names and np.ndim(fixed_all.get("alpha", 1)) > 0:
        raise InputError("best_fit: alpha must be a scalar when epsilon is fitted")
    fit_options = fit._merged_fit(kwargs)
    if fit_options["beta_interpolation"] == "likelihood" and not fit.fixed_data:
        raise InputError("best_fit: beta_interpolation 'likelihood' on a beta-dependent data vector is not supported "
                         "(its blend of two evaluations runs on the host)")
    d = len(specs)
    lo = np.array([s.lo for s in specs])
    hi = np.array([s.hi for s in specs])
    start = dict(start or {})
    x0 = np.empty((R, d))
    for j, s in enumerate(specs):
        x0[:, j] = _per_problem(f"start of {s.name}", start.pop(s.name, s.ref_loc), R)
    if start:
        raise InputError(f"best_fit: start names parameters that are not fitted: {sorted(start)}")
    if np.any(~(x0 >= lo) | ~(x0 <= hi)):
        p, j = np.argwhere(~(x0 >= lo) | ~(x0 <= hi))[0]
        raise InputError(f"best_fit: the start of {names[j]} ({x0[p, j]}) of problem {p} is outside its prior [{lo[j]}, {hi[j]}]")

    def per_param(what, given, default):
        given = dict(given or {})
        out = np.array([float(given.pop(n, dv)) for n, dv in zip(names, default)])
        if given:
            raise InputError(f"best_fit: {what} names parameters that are not fitted: {sorted(given)}")
        return out

    steps = per_param("step", step, [s.proposal for s in specs])
    if np.any(~(steps > 0)):
        raise InputError(f"best_fit: every step must be > 0 ({dict(zip(names, steps.tolist()))})")
    xtols = per_param("xtol", xtol, 1e-4 * steps)
    if np.any(~(xtols >= 0)) or not float(ftol) >= 0:
        raise InputError("best_fit: xtol and ftol must be >= 0")
    max_iter = 200 * d if max_iter is None else int(max_iter)
    if max_iter < 1 or int(restarts) < 0:
        raise InputError("best_fit: need max_iter >= 1 and restarts >= 0")
    model = fit._merged(kwargs)
    fit._check_supported(model)
    batch = {k: v for k, v in fixed_all.items()}
    batch.update({n: np.ascontiguousarray(x0[:, j]) for j, n in enumerate(names)})
    rows = np.ascontiguousarray(fit._fit_rows(batch, model), dtype=np.float64)
    cols = np.array([N.ROW_COLUMNS.get(n, N.VK_WALK_EPSILON) for n in names], dtype=np.int32)

    # ---- device
    if realisations is None:
        eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
        opts = eng.make_opts(model, fit_options)
        which = None
    else:
        _, _, eng, opts = realisations._plan(kwargs)
        which = np.arange(R, dtype=np.int32)
    lib = eng._lib
    i32 = C.POINTER(C.c_int32)
    err = C.create_string_buffer(512)
    h = lib.vk_fit_create(eng._ctx, C.byref(opts), R, d, cols.ctypes.data_as(i32), N.as_dp(N.f64(lo)), N.as_dp(N.f64(hi)),
                          N.as_dp(rows), float(fixed_all.get("alpha", 1)), None if which is None else which.ctypes.data_as(i32),
                          err, len(err))
    if not h:
        msg = err.value.decode()
        raise (N.NativeError if "device memory" in msg else InputError)(msg)
    x = np.empty((R, d))
    lnl, chi2 = np.empty(R), np.empty(R)
    status, n_iter = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.int32)
    n_evals = np.empty(R, dtype=np.int64)
    try:
        rc = lib.vk_fit_run(h, N.as_dp(N.f64(x0)), N.as_dp(N.f64(steps)), N.as_dp(N.f64(xtols)), float(ftol), max_iter,
                            int(restarts), N.as_dp(x), N.as_dp(lnl), N.as_dp(chi2), status.ctypes.data_as(i32),
                            n_iter.ctypes.data_as(i32), n_evals.ctypes.data_as(C.POINTER(C.c_int64)))
        if rc != 0:
            msg = (lib.vk_fit_last_error(h) or b"").decode() or f"vk_fit_run failed ({rc})"
            raise (InputError if rc == -1 else N.NativeError)(msg)
    finally:
        lib.vk_fit_destroy(h)
    fixed_out = {k: _per_problem(k, v, R) for k, v in fixed_all.items()}
    return BestFit(names, x, fixed_out, lnl, chi2, status, n_iter, n_evals)
