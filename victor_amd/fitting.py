"""Best-fit points on the GPU: ``CCFFit.best_fit`` and ``Realisations.best_fit``; of a joint fit, ``JointFit.best_fit`` and
``JointRealisations.best_fit`` (one parameter row for all blocks, ``vk_fit_create_joint``; with ``"name@q"`` parameters a row per
block, ``vk_fit_create_joint_blocks``: :mod:`victor_amd.joint`).

The reference has no optimiser; its users maximise ``CCFFit.log_likelihood`` (reference: ``ccf_fit.py:356-483``) with a host
optimiser, one call per point and one data vector at a time.  Here every *problem* - one maximisation of lnL over the sampled
parameters inside their uniform prior box, against the fit's data vector or one simulation realisation - runs a bounded
Nelder-Mead search on the device (``vk_fit_run``, ``include/victor_hip.h``): all problems advance together,
one launch per iteration, with no host round trip per iteration.

What is maximised is the fit's own lnL, the value ``log_likelihood`` returns: the likelihood form and, for a beta-dependent
covariance, the log-determinant term are included, so with uniform priors the result is the MAP point.  The chi-square reported
is the chi-square AT that point, not a separate chi-square minimum.  With ``prior=`` (a Gaussian prior multiplied onto the box,
:mod:`victor_amd.priors`) the device adds ln prior to the value of every point the search uses, and the result is the MAP point
of that posterior.
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
    problem; ``n_evals``: evaluations the search used (what a one-point-at-a-time Nelder-Mead evaluates).

    ``lnpost``: what the device maximised, lnL + ln prior at the best vertex, in the device's bits; ``lnprior``: the prior
    evaluated on the host at ``x`` (:mod:`victor_amd.priors`: no normalisation constant).  Without a prior ``lnprior`` is 0 and
    ``lnpost`` is ``lnl``.  With one, ``lnl`` is ``lnpost - lnprior``: the log-likelihood at ``x`` up to that one subtraction's
    rounding.

    With ``best_fit(..., covariance=...)``: ``laplace``, the :class:`victor_amd.laplace.Laplace` of the best vertices (the
    Hessian stencil run on the search's own handle), and ``cov`` (R, d, d), ``sigma`` (R, d), views of it; None otherwise."""

    laplace = cov = sigma = None
    CONVERGED, MAX_ITER, NO_FINITE_START = N.VK_FIT_CONVERGED, N.VK_FIT_MAX_ITER, N.VK_FIT_NO_FINITE_START

    def __init__(self, names, x, fixed, lnl, chi2, status, n_iter, n_evals, lnprior=None):
        self.lnpost = lnl
        self.lnprior = np.zeros(len(x)) if lnprior is None else lnprior
        if lnprior is not None:
            lnl = lnl - lnprior
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


def _per_problem(name, v, R, who=""):
    a = np.asarray(v, dtype=float)
    if a.ndim == 0:
        return np.full(R, float(a))
    if a.shape != (R,):
        raise InputError(f"{who}{name}: one value per problem ({R}) or a scalar")
    return a


def blends(fit, fit_options):
    """Does ``fit`` under these fit options blend the likelihood between two grid betas (``beta_interpolation: likelihood`` on a
    beta-dependent data vector; reference: ``ccf_fit.py:383-440``)?"""
    return fit_options["beta_interpolation"] == "likelihood" and not fit.fixed_data


def blend_opts(fit, fit_options, opts):
    """``opts`` for the create call of a sampled handle of a single ``fit``: a copy with ``VK_OPT_BETA_BLEND`` set when the fit
    options ask for the likelihood-level blend - the handle then evaluates every pending row at its two bracketing nodes of
    ``fit.beta_ccf`` (the context's ``beta_d``) and blends on the device (``include/victor_hip.h``).  The evaluation entry points
    never see the flag: ``Engine.make_opts`` leaves the word 0, and the host blend of ``log_likelihood_batch`` stays what it is."""
    if not blends(fit, fit_options):
        return opts
    out = N.vk_eval_opts.from_buffer_copy(opts)
    out.reserved |= N.VK_OPT_BETA_BLEND
    return out


class _Sampled:
    """What ``best_fit`` and ``sample_chains`` (``who``; their parameters are ``verb``: "fitted" / "sampled") share: the sampled
    parameters of a cobaya ``params`` block with their prior box, the checks on them, and the handle of their device loop.  Each
    caller runs the checks in its own order, so that a call refused for several reasons names the reason it always named."""

    def __init__(self, who, verb, params, fixed):
        self.who, self.verb = who, verb
        specs, block_fixed = parse_cobaya_params(params)
        fixed_in = dict(fixed or {})
        self.fixed_all = dict(block_fixed)
        self.fixed_all.update(fixed_in)
        self.specs = [s for s in specs if s.name not in fixed_in]
        if not self.specs:
            raise InputError(f"{who}: every parameter is fixed")
        self.names = [s.name for s in self.specs]
        self.lo = np.array([s.lo for s in self.specs])
        self.hi = np.array([s.hi for s in self.specs])

    def check_columns(self, fit=None):
        """Every sampled name has a row column of its own (or is epsilon); ``"name@q"`` addresses block q of a joint ``fit``
        and is refused, sampled or fixed, on anything else."""
        from .joint import JointFit, split_name
        joint = fit if isinstance(fit, JointFit) else None
        every = list(self.names) + list(self.fixed_all)
        if joint is not None:
            joint._check_block_names(every, self.who)
            # a plain sampled name means "every block without an entry of its own"; the device writes a sampled value to one
            # block or to all of them, so beside an @ entry of the same name it is refused
            own = {split_name(n)[0] for n in every if split_name(n)[1] is not None}
            mixed = sorted(n for n in self.names if n in own)
            if mixed:
                raise InputError(f"{self.who}: {mixed} cannot be {self.verb} for all blocks beside per-block entries of the same name "
                                 f"({sorted(n for n in every if split_name(n)[1] is not None and split_name(n)[0] in mixed)}): "
                                 "fix the plain name, or give every block an entry of its own (per_block)")
        elif any(split_name(n)[1] is not None for n in every):
            raise InputError(f"{self.who}: per-block parameters ('name@block': {sorted(n for n in every if '@' in n)}) need a "
                             "JointFit")
        for name in self.names:
            base = split_name(name)[0]
            if base not in N.ROW_COLUMNS and base != "epsilon":
                raise InputError(f"{self.who}: {name} has no column of its own in a parameter row and cannot be {self.verb}")

    def check_alpha(self):
        if any(n.partition("@")[0] == "epsilon" for n in self.names) and np.ndim(self.fixed_all.get("alpha", 1)) > 0:
            raise InputError(f"{self.who}: alpha must be a scalar when epsilon is {self.verb}")

    def fit_options(self, fit, kwargs, vectors=None):
        """The merged fit options (of a joint fit: its lead block's; every block is checked).  ``beta_interpolation='likelihood'``
        on a beta-dependent data vector (reference: ``ccf_fit.py:383-440``) is served by a single fit's device loops
        (``VK_OPT_BETA_BLEND``: :func:`blend_opts`) when it is the fit's own option (its data block / ``fit.fit_options``);
        refused here, before any device call: a joint fit, a caller that needs the theory vector of a point (``vectors``: its
        word for what it computes from them) - a blended point has two -, and the option given per call on a fit configured
        otherwise, which these loops have always refused."""
        from .joint import JointFit
        blocks = fit.fits if isinstance(fit, JointFit) else None
        if blocks is not None and fit.covariance is not None:
            kwargs = {k: v for k, v in kwargs.items() if k != "likelihood"}     # (the joint covariance's own form)
        first = None
        for f in blocks if blocks is not None else [fit]:
            fit_options = f._merged_fit(kwargs)
            if blends(f, fit_options):
                if blocks is not None:
                    raise InputError(f"{self.who}: beta_interpolation 'likelihood' on a beta-dependent data vector is not supported "
                                     "for joint fits (a blend per block under one beta is a design of its own)")
                if vectors:
                    raise InputError(f"{self.who}: beta_interpolation 'likelihood' on a beta-dependent data vector is not supported "
                                     f"with {vectors} (a blended point has two theory vectors, one per bracketing grid beta)")
                if f.fit_options.get("beta_interpolation") != "likelihood":
                    # the mode of a loop is the fit's own, as the reference configures it (ccf_fit.py:41-42: read from the data
                    # block); a per-call override into it stays what it always was in these loops - a refusal
                    raise InputError(f"{self.who}: beta_interpolation 'likelihood' on a beta-dependent data vector is not supported "
                                     "as a per-call option here: set it on the fit (`beta_interpolation: likelihood` in its data "
                                     "block, or fit.fit_options), where the reference configures it")
            first = fit_options if first is None else first
        return first

    def per_param(self, what, given, default):
        """One value per sampled parameter: ``given`` (name -> value) over ``default``."""
        given = dict(given or {})
        out = np.array([float(given.pop(n, dv)) for n, dv in zip(self.names, default)])
        if given:
            raise InputError(f"{self.who}: {what} names parameters that are not {self.verb}: {sorted(given)}")
        return out

    def prior(self, prior, fit=None):
        """The :class:`victor_amd.priors.ResolvedPrior` of the ``prior=`` argument against the sampled parameters (None for
        None); every refusal before any device call."""
        from .joint import JointFit
        from .priors import resolve_prior
        return resolve_prior(prior, self.who, self.names, self.lo, self.hi, self.fixed_all, isinstance(fit, JointFit))

    def set_prior(self, entry, lib, h, prior):
        """Hand a resolved prior to the handle ``h`` (``entry``: ``vk_fit_set_prior`` / ``vk_chain_set_prior``)."""
        rc = getattr(lib, entry)(h, N.as_dp(prior.mu), N.as_dp(prior.pp))
        if rc != 0:
            last = lib.vk_fit_last_error if entry.startswith("vk_fit") else lib.vk_chain_last_error
            raise (InputError if rc == -1 else N.NativeError)((last(h) or b"").decode() or f"{entry} failed ({rc})")

    def starts(self, given, R, prefix=""):
        """``(R, d)`` start points inside the prior: ``given`` (name -> scalar or ``(R,)`` array, or a :class:`BestFit`, whose
        fitted values of the sampled names are taken) over the ``ref`` locations."""
        if hasattr(given, "params") and hasattr(given, "names"):
            given = {n: v for n, v in given.params.items() if n in self.names}
        given = dict(given or {})
        x0 = np.empty((R, len(self.specs)))
        for j, s in enumerate(self.specs):
            x0[:, j] = _per_problem(f"start of {s.name}", given.pop(s.name, s.ref_loc), R, prefix)
        if given:
            raise InputError(f"{self.who}: start names parameters that are not {self.verb}: {sorted(given)}")
        bad = ~(x0 >= self.lo) | ~(x0 <= self.hi)
        if np.any(bad):
            p, j = np.argwhere(bad)[0]
            raise InputError(f"{self.who}: the start of {self.names[j]} ({x0[p, j]}) of problem {p} is outside its prior "
                             f"[{self.lo[j]}, {self.hi[j]}]")
        return x0

    def create(self, entry, fit, realisations, kwargs, fit_options, batch, which, shape=()):
        """``(lib, handle, refresh)`` of ``entry`` (``vk_fit_create`` / ``vk_chain_create``; ``vk_nested_create`` with its ``shape``
        arguments, which follow the row count): one problem per row of ``batch``
        (the sampled and fixed values its rows start from), against the fit's data vector or realisation ``which[i]``.
        ``refresh`` (None against the data vector) makes ``realisations`` the ones set on the handle's context(s) again - another
        object's may have been set since.  A :class:`victor_amd.joint.JointFit` builds its own handle, of ``entry + "_joint"``
        (``JointFit._sampled_create``)."""
        from .joint import JointFit
        if isinstance(fit, JointFit):
            return fit._sampled_create(entry + "_joint", self, realisations, kwargs, batch, which, shape)
        model = fit._merged(kwargs)
        fit._check_supported(model)
        rows = np.ascontiguousarray(fit._fit_rows(batch, model), dtype=np.float64)
        cols = np.array([N.ROW_COLUMNS.get(n, N.VK_WALK_EPSILON) for n in self.names], dtype=np.int32)
        refresh = None
        if realisations is None:
            eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
            opts = eng.make_opts(model, fit_options)
        else:
            _, _, eng, opts = realisations._plan(kwargs)

            def refresh():
                realisations._upload(eng)
        i32 = C.POINTER(C.c_int32)
        err = C.create_string_buffer(512)
        opts = blend_opts(fit, fit_options, opts)
        h = getattr(eng._lib, entry)(eng._ctx, C.byref(opts), len(rows), *shape, len(cols), cols.ctypes.data_as(i32), N.as_dp(N.f64(self.lo)),
                                     N.as_dp(N.f64(self.hi)), N.as_dp(rows), float(self.fixed_all.get("alpha", 1)),
                                     None if realisations is None else which.ctypes.data_as(i32), err, len(err))
        if not h:
            msg = err.value.decode()
            raise (N.NativeError if "device memory" in msg else InputError)(msg)
        return eng._lib, h, refresh


def best_fit(fit, params, fixed=None, start=None, step=None, xtol=None, ftol=1e-6, max_iter=None, restarts=1, kwargs=None,
             realisations=None, prior=None, covariance=None):
    """The work of ``CCFFit.best_fit`` (``realisations=None``: against the fit's data vector) and ``Realisations.best_fit``;
    with a ``JointFit`` for ``fit`` (and its ``JointRealisations``), of theirs.  ``prior``: a
    :class:`victor_amd.priors.GaussianPrior` (or a list of them) multiplied onto the box; the search then maximises
    lnL + ln prior (``vk_fit_set_prior``).  ``covariance``: True, or a dict ``{"step", "shrink", "refine", "keep_values"}`` as
    :func:`victor_amd.laplace.laplace` takes them: the Hessian stencil (``vk_fit_hessian``) runs at the best vertices on the
    search's own handle before it is destroyed, and the result carries ``laplace``, ``cov`` and ``sigma``.  Every argument is
    checked before the first device call."""
    kwargs = kwargs or {}
    q = _Sampled("best_fit", "fitted", params, fixed)
    names, fixed_all, d = q.names, q.fixed_all, len(q.names)
    q.check_columns(fit)
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
    q.check_alpha()
    prior = q.prior(prior, fit)
    fit_options = q.fit_options(fit, kwargs)
    x0 = q.starts(start, R)
    steps = q.per_param("step", step, [s.proposal for s in q.specs])
    if np.any(~(steps > 0)):
        raise InputError(f"best_fit: every step must be > 0 ({dict(zip(names, steps.tolist()))})")
    xtols = q.per_param("xtol", xtol, 1e-4 * steps)
    if np.any(~(xtols >= 0)) or not float(ftol) >= 0:
        raise InputError("best_fit: xtol and ftol must be >= 0")
    max_iter = 200 * d if max_iter is None else int(max_iter)
    if max_iter < 1 or int(restarts) < 0:
        raise InputError("best_fit: need max_iter >= 1 and restarts >= 0")
    from .laplace import resolve_covariance
    want_cov = resolve_covariance(covariance, q, R)
    batch = dict(fixed_all)
    batch.update({n: np.ascontiguousarray(x0[:, j]) for j, n in enumerate(names)})

    # ---- device
    lib, h, _ = q.create("vk_fit_create", fit, realisations, kwargs, fit_options, batch, np.arange(R, dtype=np.int32))
    i32 = C.POINTER(C.c_int32)
    x = np.empty((R, d))
    lnl, chi2 = np.empty(R), np.empty(R)
    status, n_iter = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.int32)
    n_evals = np.empty(R, dtype=np.int64)
    try:
        if prior is not None:
            q.set_prior("vk_fit_set_prior", lib, h, prior)
        rc = lib.vk_fit_run(h, N.as_dp(N.f64(x0)), N.as_dp(N.f64(steps)), N.as_dp(N.f64(xtols)), float(ftol), max_iter,
                            int(restarts), N.as_dp(x), N.as_dp(lnl), N.as_dp(chi2), status.ctypes.data_as(i32),
                            n_iter.ctypes.data_as(i32), n_evals.ctypes.data_as(C.POINTER(C.c_int64)))
        if rc != 0:
            msg = (lib.vk_fit_last_error(h) or b"").decode() or f"vk_fit_run failed ({rc})"
            raise (InputError if rc == -1 else N.NativeError)(msg)
        fixed_out = {k: _per_problem(k, v, R) for k, v in fixed_all.items()}
        lap = None
        if want_cov is not None:
            from .laplace import device_pass, run_passes
            requested, shrink, refine, keep_values = want_cov
            lap = run_passes(q, x, requested, shrink, refine, keep_values, prior, fixed_out, device_pass(lib, h, x, R, d))
    finally:
        lib.vk_fit_destroy(h)
    bf = BestFit(names, x, fixed_out, lnl, chi2, status, n_iter, n_evals, None if prior is None else prior.lnprior(x))
    if lap is not None:
        bf.laplace, bf.cov, bf.sigma = lap, lap.cov, lap.sigma
    return bf
