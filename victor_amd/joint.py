"""Joint fit of several data vectors that share one parameter vector (density-split quantiles).

The reference mentions density-split centres only in passing (``ccf_model.py:28-30``) and has no joint-fit
class; BASELINE config "density-split 5-quantile joint fit" is defined as Q independent ``CCFFit`` blocks with a
block-diagonal covariance, so chi-square and log-likelihood add.  Each block keeps its own context (tables in
HBM) on the same GPU; one batch of parameter rows is run through every block.

With ``covariance=`` the blocks are fitted under ONE covariance matrix across the joint vector - the concatenation of the
blocks' data vectors in block order - as the reference's ``CCFFit`` would fit that vector: the quantiles of a density-split
analysis share their galaxies and voids, so their data vectors are correlated.  The blocks' theory vectors come from their
own theory launches; the joint chi-square is one kernel (``vk_joint_cov_eval_device_async``, ``vk_kernel_joint.h``).

Per-block parameters: a name ``"<name>@<q>"`` addresses block ``q`` (0-based, the order of ``fits``), a plain ``"<name>"`` every
block without an ``@`` entry of its own - the quantiles of a density split share fsigma8, beta and epsilon, each has its own
velocity dispersion (and bias / ``Av``).  Block q's rows are ``fits[q]._fit_rows`` of the dictionary resolved for it
(:func:`block_params`); the device entry points are the ``_blocks`` forms of ``include/victor_hip.h``.  Without an ``@`` key every
call is the call it was.  :func:`per_block` writes the ``@`` entries of a cobaya ``params`` block.

``JointFit.realisations()`` validates the joint fit on mocks: joint realisation m is realisation m of every block's own stacked
file (``redshift_space_ccf.simulation_number``, reference ``ccf_fit.py:59-61,93-100``), and every parameter point is evaluated
against all of them in one call (:class:`JointRealisations`).
"""

import os

import numpy as np


import ctypes as C

from . import _native as N
from .realisations import Realisations, check_which
from .utils import InputError


def split_name(name):
    """``("sigma_v", 2)`` of ``"sigma_v@2"``, ``(name, None)`` of a plain name; ``InputError`` for a suffix that is no
    non-negative integer."""
    base, at, suffix = str(name).partition("@")
    if not at:
        return name, None
    if not base or not suffix.isdigit():
        raise InputError(f"{name}: a per-block parameter is named '<name>@<block>' with the block's number (0, 1, ...)")
    return base, int(suffix)


def has_block_names(params):
    """Does the dictionary address a block of its own anywhere (an ``@`` key)?"""
    return isinstance(params, dict) and any("@" in str(k) for k in params)


def check_block_names(names, n_blocks, beta_gridded=False, who="JointFit"):
    """The refusals of per-block names: a block outside ``0 .. n_blocks - 1``, ``alpha@q`` (alpha stays one scalar) and, under
    a joint covariance gridded in beta, ``beta@q`` (the joint chi-square brackets the covariance with ONE beta per point)."""
    for name in names:
        base, q = split_name(name)
        if q is None:
            continue
        if q >= n_blocks:
            raise InputError(f"{who}: {name} names block {q} of {n_blocks} (0..{n_blocks - 1})")
        if base == "alpha":
            raise InputError(f"{who}: {name}: alpha is one scalar for all blocks")
        if base == "beta" and beta_gridded:
            raise InputError(f"{who}: {name}: under a joint covariance gridded in beta every block shares one beta (the joint "
                             "chi-square brackets the covariance with one beta per point)")


def block_params(params, q):
    """The dictionary block ``q`` reads: ``params["name@q"]`` where present, else ``params["name"]``; other blocks' entries
    dropped."""
    out = {k: v for k, v in params.items() if "@" not in str(k)}
    for k, v in params.items():
        base, b = split_name(k)
        if b == q:
            out[base] = v
    return out


def per_block(params, names, n_blocks):
    """A copy of the cobaya ``params`` block in which every entry listed in ``names`` is replaced by its ``n_blocks`` copies
    ``"<name>@0" .. "<name>@<n_blocks - 1>"`` (the same prior, ref and proposal, at the entry's place in the block):
    ``joint.realisations().best_fit(per_block(params, ["sigma_v"], 5))`` fits a velocity dispersion of each quantile's own."""
    import copy
    names = [names] if isinstance(names, str) else list(names)
    missing = [n for n in names if n not in params]
    if missing:
        raise InputError(f"per_block: {missing} are not in the params block")
    if int(n_blocks) < 1:
        raise InputError("per_block: need at least one block")
    check_block_names([f"{n}@0" for n in names], int(n_blocks), who="per_block")
    out = {}
    for key, spec in params.items():
        if key in names:
            for q in range(int(n_blocks)):
                out[f"{key}@{q}"] = copy.deepcopy(spec)
        else:
            out[key] = spec
    return out


class JointFit:
    def __init__(self, fits, covariance=None, likelihood=None):
        """``covariance``: ``None`` - block-diagonal, each block under its own covariance (chi-square and lnL add); a
        ``(NT, NT)`` array - one fixed covariance of the joint vector, NT = the sum of the blocks' N; or a dict in the
        reference's ``covariance_matrix`` schema (``data_file``, ``cov_key``, ``fixed_beta``, ``beta_key``, plus ``dir``), read
        as ``CCFFit`` reads its own.  ``likelihood``: ``{"form", "nmocks", "nparams"}`` of the joint fit (default: the first
        block's); the Hartlap and Percival corrections take p = NT."""
        self.fits = list(fits)
        if not self.fits:
            raise ValueError("need at least one fit")
        self._buffers = None
        self._block_buffers = None
        self.covariance = None
        self._handles = {}
        if covariance is None:
            if likelihood is not None:
                raise InputError("JointFit: likelihood= applies to a joint covariance only (covariance=None keeps each block's own)")
            return
        self.likelihood = dict(likelihood if likelihood is not None else self.fits[0].fit_options["likelihood"])
        self._load_joint_covariance(covariance)

    # ------------------------------------------------------------------ full covariance: set-up (host)
    def _load_joint_covariance(self, covariance):
        from .ccf_fit import load_covariance_matrix
        from .engine import covariance_logdets
        nt = self.n_data
        self.fixed_data = all(f.fixed_data for f in self.fits)
        if isinstance(covariance, dict):
            fn = os.path.join(covariance.get("dir", ""), covariance.get("data_file"))
            if not os.path.isfile(fn):
                raise InputError(f"Data file {fn} not found")
            grids = [f.beta_ccf for f in self.fits if not f.fixed_data]
            self.fixed_covmat, beta_covmat, self.covmat, self.icov = load_covariance_matrix(
                covariance, fn, self.fits[0].extensions, nt, self.fixed_data, grids[0] if grids else None)
            if not self.fixed_covmat:
                # the loader falls back to the data's grid (hands back grids[0] itself) when beta_key is not given or not in
                # the file; with blocks on different data grids there is no such grid
                if beta_covmat is grids[0] and any(not np.array_equal(g, grids[0]) for g in grids[1:]):
                    raise InputError("JointFit: the blocks' data beta grids differ and the covariance file holds no beta grid "
                                     "(beta_key)")
                self.beta_covmat = np.asarray(beta_covmat, dtype=float)
        else:
            covmat = np.asarray(covariance, dtype=float)
            if covmat.shape != (nt, nt):
                raise InputError("Unexpected shape of (fixed) covariance matrix")
            self.fixed_covmat = True
            self.covmat = covmat
            self.icov = np.linalg.inv(covmat)
        if self.fixed_covmat:
            self._logdet = self._eig = None
        else:
            self._logdet, self._eig = covariance_logdets(self.covmat, self.beta_covmat)
        self.covariance = covariance

    def _bracket(self, beta):
        """(low index, weight of the LAST grid entry) of the covariance slices, as ``CCFFit._bracket`` (ccf_fit.py:213-228)."""
        g = self.beta_covmat
        if beta < g.min():
            return 0, 0.0
        if beta > g.max():
            return len(g) - 1, 0.0
        if beta in g:
            return int(np.where(g == beta)[0][0]), 0.0
        lo = int(np.where(g < beta)[0][-1])
        hi = int(np.where(g >= beta)[0][-1])
        return lo, (beta - g[lo]) / (g[hi] - g[lo])

    def _interp_stack(self, stack, beta):
        if self.fixed_covmat:
            return stack
        if beta is None:
            raise InputError("Need to supply a valid value of beta for interpolation")
        lo, t = self._bracket(beta)
        if t == 0.0:
            return stack[lo]
        return (1 - t) * stack[lo] + t * stack[-1]

    def get_interpolated_covariance(self, beta=None):
        """(NT, NT) covariance of the joint vector at ``beta`` (the bracket rule of ccf_fit.py:195-228)."""
        if self.covariance is None:
            import scipy.linalg as sl
            return sl.block_diag(*[f.get_interpolated_covariance(beta) for f in self.fits])
        return self._interp_stack(self.covmat, beta)

    def get_interpolated_precision(self, beta=None):
        """(NT, NT) precision of the joint vector at ``beta`` (ccf_fit.py:230-260): the blend of the precision slices."""
        if self.covariance is None:
            import scipy.linalg as sl
            return sl.block_diag(*[f.get_interpolated_precision(beta) for f in self.fits])
        return self._interp_stack(self.icov, beta)

    def multipole_datavector(self, beta=None):
        """(NT,) joint data vector at ``beta``: the blocks' ``multipole_datavector`` concatenated in the order of ``fits``."""
        return np.concatenate([f.multipole_datavector(beta) for f in self.fits])

    # ------------------------------------------------------------------ full covariance: evaluation (device)
    def _plan_cov(self, kwargs):
        """(engines, opts) of a full-covariance evaluation; InputError where the blocks cannot share one launch: a sum over
        blocks is wrong under a full covariance, so there is no per-block route."""
        kw = dict(kwargs)
        like = kw.pop("likelihood", self.likelihood)
        models, fos, rowsig = [], [], []
        for fit in self.fits:
            model = fit._merged(kw)
            fit._check_supported(model)
            fo = fit._merged_fit(kw)
            fo["likelihood"] = like
            if fo["beta_interpolation"] == "likelihood" and not fit.fixed_data:
                raise InputError("JointFit with a joint covariance: beta_interpolation 'likelihood' with beta-dependent data "
                                 "is not supported")
            models.append(model)
            fos.append(fo)
            rowsig.append((fit._needs_beta(model) or not fit.fixed_data, fit._needs_fsigma8(model), model["bias"]))
        if len({f._device for f in self.fits}) != 1:
            raise InputError("JointFit with a joint covariance: every block must live on the same device")
        if any(m != models[0] for m in models) or any(f != fos[0] for f in fos) or len(set(rowsig)) != 1:
            raise InputError("JointFit with a joint covariance: every block must share its model and fit options and its "
                             "data's beta dependence")
        engines, blobs = [], []
        opts = None
        for fit, model, fo in zip(self.fits, models, fos):
            eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
            opts = eng.make_opts(model, fo)
            engines.append(eng)
            blobs.append(bytes(opts))
        if len(set(blobs)) != 1 or len({e.device for e in engines}) != 1:
            raise InputError("JointFit with a joint covariance: the blocks' option blocks differ")
        return engines, opts

    def _joint_handle(self, lead):
        """The device copy of the joint covariance tables (``vk_joint_cov_create``), made once per lead engine and kept for
        the life of this object: which engine leads depends on a call's options (matter model, Simpson rule), and a handle
        may be held by the best-fit or chain handle of an earlier call (``vk_fit_create_joint`` / ``vk_chain_create_joint``;
        a ``Chains`` keeps this object alive), so a call with other options must never destroy it."""
        h = self._handles.get(id(lead))
        if h is not None:
            return h[1]
        nt = self.n_data
        block_n = np.array([len(f.s) * len(f.poles_s) for f in self.fits], dtype=np.int32)
        t = N.vk_joint_cov_tables()
        t.n_blocks = len(block_n)
        t.block_n = block_n.ctypes.data_as(C.POINTER(C.c_int32))
        prec = N.f64(self.icov)
        t.prec = N.as_dp(prec)
        keep = [block_n, prec]
        if self.fixed_covmat:
            t.n_beta = 0
        else:
            beta, logdet, eig = N.f64(self.beta_covmat), N.f64(self._logdet), N.f64(self._eig)
            keep += [beta, logdet, eig]
            t.n_beta = len(beta)
            t.beta, t.logdet, t.eig = N.as_dp(beta), N.as_dp(logdet), N.as_dp(eig)
        assert prec.size == max(t.n_beta, 1) * nt * nt
        out = C.c_void_p()
        lead._check(lead._lib.vk_joint_cov_create(lead._ctx, C.byref(t), C.byref(out)))
        del keep
        self._handles[id(lead)] = (lead, out.value)              # (the entry keeps the lead engine, and so its id, alive)
        return out.value

    def _release_handle(self):
        """Destroy every device copy of the covariance tables.  Nothing that holds one may be alive: ``__del__``, and tests
        that have finished with this object."""
        handles = getattr(self, "_handles", None) or {}
        while handles:
            lead, h = handles.popitem()[1]
            lead._lib.vk_joint_cov_destroy(h)

    def _release_buffers(self):
        """Free the device buffers of the evaluation calls (the shared calls' and the per-block calls')."""
        for attr in ("_buffers", "_block_buffers"):
            b = getattr(self, attr, None)
            setattr(self, attr, None)
            if b is not None:
                for ptr in b["ptrs"]:
                    b["lead"].free(ptr)

    def __del__(self):
        for release in (self._release_handle, self._release_buffers):
            try:
                release()
            except Exception:
                pass

    def _log_likelihood_cov(self, params, kwargs):
        if has_block_names(params):
            return self._log_likelihood_blocks(params, kwargs)
        engines, opts = self._plan_cov(kwargs)
        fit = self.fits[0]
        rows = fit._fit_rows(params, fit._merged({k: v for k, v in kwargs.items() if k != "likelihood"}))
        n = len(rows)
        if n == 0:
            return np.empty(0), np.empty(0)
        lead = engines[0]
        handle = self._joint_handle(lead)
        ctxs = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
        need = lead._lib.vk_joint_cov_workspace_doubles(handle, n)
        b = self._buffers
        if b is None or b.get("cov", -1) < need or b["n"] < n or b["lead"] is not lead:
            if b is not None:
                for ptr in b["ptrs"]:
                    b["lead"].free(ptr)
            self._buffers = None
            b = self._buffers = {"n": n, "lead": lead, "cov": need,
                                 "ptrs": [lead.alloc(n * N.VK_NPAR), lead.alloc(2 * n), lead.alloc(need)]}
        d_rows, d_out, d_ws = b["ptrs"]
        lead.upload(d_rows, rows)
        d_chi = C.c_void_p(d_out + 8 * n)
        lead._check(lead._lib.vk_joint_cov_eval_device_async(handle, ctxs, len(engines), C.byref(opts), d_rows, n, d_out,
                                                             d_chi, d_ws))
        out = lead.download(d_out, 2 * n)
        return out[:n].copy(), out[n:].copy()

    # ------------------------------------------------------------------ per-block parameters ("name@q")
    def _check_block_names(self, names, who="JointFit"):
        check_block_names(names, len(self.fits), self.covariance is not None and not self.fixed_covmat, who)

    def _block_rows(self, params, kwargs):
        """``(B, n, VK_NPAR)`` rows, block q's formed by ``fits[q]._fit_rows`` from the dictionary resolved for it."""
        self._check_block_names(params)
        kw = {k: v for k, v in kwargs.items() if k != "likelihood"} if self.covariance is not None else kwargs
        rows = [np.asarray(f._fit_rows(block_params(params, q), f._merged(kw))) for q, f in enumerate(self.fits)]
        n = max(len(r) for r in rows)
        if any(len(r) not in (1, n) for r in rows):
            raise InputError(f"parameter arrays have different lengths: {sorted({len(r) for r in rows})}")
        return np.ascontiguousarray([np.broadcast_to(r, (n, N.VK_NPAR)) for r in rows], dtype=np.float64)

    def _log_likelihood_blocks(self, params, kwargs):
        """:meth:`log_likelihood_batch` with ``@`` names: a row set per block through ``vk_joint_cov_eval_blocks_device_async`` /
        ``vk_joint_eval_blocks_device_async``; blocks that cannot share one launch, one call per block and the host's sum."""
        self._check_block_names(params)
        if self.covariance is not None:
            engines, opts = self._plan_cov(kwargs)
        else:
            plan = self._plan(kwargs)
            if plan is None:
                return self._sequential(params, kwargs)
            engines, opts = plan
        rows = self._block_rows(params, kwargs)
        B, n = rows.shape[:2]
        if n == 0:
            return np.empty(0), np.empty(0)
        lead = engines[0]
        ctxs = (C.c_void_p * B)(*[e._ctx for e in engines])
        if self.covariance is not None:
            handle = self._joint_handle(lead)
            need = lead._lib.vk_joint_cov_workspace_doubles(handle, n)
        else:
            need = lead._lib.vk_joint_workspace_doubles(ctxs, B, n)
        b = self._block_buffers                                 # (its own buffers: the shared calls keep theirs as they were)
        if b is None or b["lead"] is not lead or b["n"] < n or b["ws"] < need:
            if b is not None:
                for ptr in b["ptrs"]:
                    b["lead"].free(ptr)
            self._block_buffers = None
            b = self._block_buffers = {"lead": lead, "n": n, "ws": need,
                                       "ptrs": [lead.alloc(B * n * N.VK_NPAR), lead.alloc(2 * n), lead.alloc(need)]}
        d_rows, d_out, d_ws = b["ptrs"]
        lead.upload(d_rows, rows)
        d_chi = C.c_void_p(d_out + 8 * n)
        if self.covariance is not None:
            rc = lead._lib.vk_joint_cov_eval_blocks_device_async(handle, ctxs, B, C.byref(opts), d_rows, n * N.VK_NPAR, n, d_out,
                                                                 d_chi, d_ws)
        else:
            rc = lead._lib.vk_joint_eval_blocks_device_async(ctxs, B, C.byref(opts), d_rows, n * N.VK_NPAR, n, d_out, d_chi, d_ws)
        lead._check(rc)
        out = lead.download(d_out, 2 * n)
        return out[:n].copy(), out[n:].copy()

    # ------------------------------------------------------------------ device-resident joint evaluation
    def _plan(self, kwargs):
        """Engines, option block and row builder when every block can share ONE parameter upload and ONE option block
        (the normal case: same options in every block); None otherwise."""
        engines, blobs, rowsig = [], [], []
        opts = None
        for fit in self.fits:
            model = fit._merged(kwargs)
            fit._check_supported(model)
            fo = fit._merged_fit(kwargs)
            if fo["beta_interpolation"] == "likelihood" and not fit.fixed_data:
                return None
            eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
            o = eng.make_opts(model, fo)
            engines.append(eng)
            blobs.append(bytes(o))
            rowsig.append((fit._needs_beta(model) or not fit.fixed_data, fit._needs_fsigma8(model), model["bias"]))
            opts = o
        if len(set(blobs)) != 1 or len(set(rowsig)) != 1 or len({e.device for e in engines}) != 1:
            return None
        return engines, opts

    def _device_buffers(self, engines, n):
        lead = engines[0]
        ctxs = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
        need = lead._lib.vk_joint_workspace_doubles(ctxs, len(engines), n)
        b = self._buffers
        if b is None or b["n"] < n or b["lead"] is not lead:
            if b is not None:
                for ptr in b["ptrs"]:
                    b["lead"].free(ptr)
            ptrs = [lead.alloc(n * N.VK_NPAR), lead.alloc(2 * n), lead.alloc(need)]
            b = self._buffers = {"n": n, "lead": lead, "ptrs": ptrs}
        return ctxs, b["ptrs"]

    def eval_device_async(self, engines, opts, d_rows, n, d_lnl, d_chi2, d_ws):
        """Enqueue the joint evaluation on buffers already in HBM (``bench.py``); ``engines[0].sync()`` waits for it."""
        lead = engines[0]
        ctxs = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
        lead._check(lead._lib.vk_joint_eval_device_async(ctxs, len(engines), C.byref(opts), d_rows, int(n), d_lnl, d_chi2, d_ws))

    def log_likelihood_batch(self, params, **kwargs):
        """(lnL[n], chi2[n]) summed over the blocks: one parameter upload, every block's kernels enqueued without a host
        synchronisation in between, the sums taken on the device (``vk_joint_eval_device_async``).  Under a joint covariance:
        the chi-square of the joint vector and its likelihood form (``vk_joint_cov_eval_device_async``)."""
        if self.covariance is not None:
            return self._log_likelihood_cov(params, kwargs)
        if has_block_names(params):
            return self._log_likelihood_blocks(params, kwargs)
        plan = self._plan(kwargs)
        if plan is None:
            return self._sequential(params, kwargs)
        engines, opts = plan
        fit = self.fits[0]
        rows = fit._fit_rows(params, fit._merged(kwargs))
        n = len(rows)
        if n == 0:
            return np.empty(0), np.empty(0)
        ctxs, (d_rows, d_out, d_ws) = self._device_buffers(engines, n)
        lead = engines[0]
        lead.upload(d_rows, rows)
        d_chi = C.c_void_p(d_out + 8 * n)
        lead._check(lead._lib.vk_joint_eval_device_async(ctxs, len(engines), C.byref(opts), d_rows, n, d_out, d_chi, d_ws))
        out = lead.download(d_out, 2 * n)
        return out[:n].copy(), out[n:].copy()

    def _sequential(self, params, kwargs):
        """Blocks with different options: one call per block, sums on the host."""
        lnl = chi2 = None
        blocks = has_block_names(params)
        if blocks:
            self._check_block_names(params)
        for q, fit in enumerate(self.fits):
            a, b = fit.log_likelihood_batch(block_params(params, q) if blocks else params, **kwargs)
            lnl = a if lnl is None else lnl + a
            chi2 = b if chi2 is None else chi2 + b
        bad = ~np.isfinite(lnl)
        lnl[bad], chi2[bad] = -np.inf, np.inf
        return lnl, chi2

    def log_likelihood(self, params, **kwargs):
        lnl, chi2 = self.log_likelihood_batch(params, **kwargs)
        return float(lnl[0]), float(chi2[0])

    # ------------------------------------------------------------------ best fits and chains (fitting.py, chains.py)
    def _sampled_create(self, entry, q, realisations, kwargs, batch, which, shape=()):
        """``(lib, handle, refresh)`` of ``vk_fit_create_joint`` / ``vk_chain_create_joint`` (``entry``; with ``@`` names among the
        sampled or fixed parameters their ``_blocks`` forms, a row per block) for the sampled
        parameters ``q`` (the contract of ``fitting._Sampled.create``): one problem per row of ``batch``, against the joint data
        vector or joint realisation ``which[i]`` of ``realisations``.  The rows are the lead fit's, as
        :meth:`log_likelihood_batch` forms them."""
        engines, opts, kwargs = self._sampled_plan(q.who, kwargs)
        rows, cols, param_block, n_rows = self._sampled_rows(q.names, batch, kwargs)
        i32 = C.POINTER(C.c_int32)
        extra = ()
        if param_block is not None:
            extra = (param_block.ctypes.data_as(i32),)
            entry += "_blocks"
        lib, ctxs, handle, refresh = self._sampled_device(engines, realisations)
        err = C.create_string_buffer(512)
        h = getattr(lib, entry)(ctxs, len(engines), handle, C.byref(opts), n_rows, *shape, len(cols), cols.ctypes.data_as(i32),
                                *extra, N.as_dp(N.f64(q.lo)), N.as_dp(N.f64(q.hi)), N.as_dp(rows),
                                float(q.fixed_all.get("alpha", 1)),
                                None if realisations is None else which.ctypes.data_as(i32), err, len(err))
        if not h:
            msg = err.value.decode()
            raise (N.NativeError if "device memory" in msg else InputError)(msg)
        return lib, h, refresh

    # what every handle over the joint lnL shares (the device loops above; ``vk_is_create_joint``: importance.create_handle)
    def _sampled_plan(self, who, kwargs):
        """``(engines, opts, kwargs)`` of a device loop over the joint lnL: the blocks' engines, lead first, their one option
        block, and ``kwargs`` as the blocks' own row builders take them (under a joint covariance without its ``likelihood``).
        Refused: blocks on different devices, and blocks that cannot share one option block."""
        if len({f._device for f in self.fits}) != 1:
            raise InputError(f"{who}: every block of a joint fit must live on the same device")
        if self.covariance is not None:
            engines, opts = self._plan_cov(kwargs)
            return engines, opts, {k: v for k, v in kwargs.items() if k != "likelihood"}
        plan = self._plan(kwargs)
        if plan is None:
            raise InputError(f"{who}: the blocks of a block-diagonal joint fit must share one option block (their model, "
                             "fit options and their data's beta dependence) and one device")
        return plan[0], plan[1], kwargs

    def _sampled_rows(self, names, batch, kwargs):
        """``(rows, cols, param_block, n_rows)`` of the sampled ``names`` and the rows of ``batch``: with ``@`` names anywhere in
        the batch a row set per block, ``rows`` ``(B n_rows, VK_NPAR)`` - block b's base rows from the values resolved for it,
        each sampled value to its own block (``param_block``, -1: every block) -; otherwise the lead fit's rows and None."""
        if has_block_names(batch):
            rows = self._block_rows(batch, kwargs).reshape(-1, N.VK_NPAR)
            split = [split_name(n) for n in names]
            cols = np.array([N.ROW_COLUMNS.get(base, N.VK_WALK_EPSILON) for base, _ in split], dtype=np.int32)
            param_block = np.array([-1 if b is None else b for _, b in split], dtype=np.int32)
            return rows, cols, param_block, len(rows) // len(self.fits)
        fit = self.fits[0]
        rows = np.ascontiguousarray(fit._fit_rows(batch, fit._merged(kwargs)), dtype=np.float64)
        cols = np.array([N.ROW_COLUMNS.get(n, N.VK_WALK_EPSILON) for n in names], dtype=np.int32)
        return rows, cols, None, len(rows)

    def _sampled_device(self, engines, realisations):
        """``(lib, ctxs, covariance handle or None, refresh)`` for a create call: ``refresh`` (None against the data vector)
        makes ``realisations`` the ones set on every block's engine again, and has been called once."""
        refresh = None
        if realisations is not None:
            def refresh(realisations=realisations, engines=list(engines)):
                realisations._upload(engines)
            refresh()
        lead = engines[0]
        handle = self._joint_handle(lead) if self.covariance is not None else None
        ctxs = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
        return lead._lib, ctxs, handle, refresh

    def best_fit(self, params, fixed=None, start=None, step=None, xtol=None, ftol=1e-6, max_iter=None, restarts=1, prior=None,
                 covariance=None, **kwargs):
        """Maximum of the joint lnL (the value :meth:`log_likelihood_batch` returns) over the sampled parameters of a cobaya
        ``params`` block - one parameter vector for all blocks, or with ``"name@q"`` entries (:func:`per_block`) a value of
        that parameter per block, at most 10 sampled values in all - by the bounded Nelder-Mead search of ``CCFFit.best_fit`` on
        the GPU, block-diagonal or under the joint covariance.  Arguments and result as ``CCFFit.best_fit``: arrays in
        ``fixed`` give a profile; a ``prior`` (:class:`victor_amd.priors.GaussianPrior`) may name ``"name@q"`` parameters."""
        from .fitting import best_fit
        return best_fit(self, params, fixed, start, step, xtol, ftol, max_iter, restarts, kwargs, prior=prior, covariance=covariance)

    def laplace(self, params, at, step=None, fixed=None, prior=None, shrink=8, refine=0, keep_values=False, **kwargs):
        """The Laplace approximation of the joint posterior at given points: the Hessian stencil of ``CCFFit.laplace``
        over the joint lnL, block-diagonal or under the joint covariance, ``"name@q"`` parameters included (at most 10 sampled
        values in all).  Arguments and result as ``CCFFit.laplace``."""
        from .laplace import laplace
        return laplace(self, params, at, step, fixed, prior, shrink, refine, keep_values, kwargs)

    def fisher(self, params, at, step=None, fixed=None, prior=None, shrink=8, keep_vectors=False, **kwargs):
        """The Fisher forecast of the joint vector at given points (``CCFFit.fisher``): the blocks' theory vectors
        concatenated, under the joint covariance or block-diagonal, ``"name@q"`` parameters included (at most 10 sampled
        values in all).  Arguments and result as ``CCFFit.fisher``."""
        from .fisher import fisher
        return fisher(self, params, at, step, fixed, prior, shrink, keep_vectors, kwargs)

    def sample_chains(self, params, n_steps, walkers=8, seed=0, fixed=None, start=None, scatter=None, proposal=None, burn=0,
                      thin=1, keep_chain=True, device=True, move="metropolis", stretch_a=2.0, prior=None, marginals=None, autocorr=None, temper=None,
                      predictive=None, **kwargs):
        """``walkers`` Metropolis chains of the joint lnL, stepped on the GPU (``device=True``) or by the NumPy loop over
        :meth:`log_likelihood_batch` that defines them (``device=False``).  Arguments and result as ``CCFFit.sample_chains``
        (:mod:`victor_amd.chains`), ``move="stretch"`` included; the result keeps this joint fit alive."""
        from .chains import sample_chains
        return sample_chains(self, params, n_steps, walkers, seed, fixed, start, scatter, proposal, burn, thin, keep_chain, device,
                             kwargs, move=move, stretch_a=stretch_a, prior=prior, marginals=marginals,
                             autocorr=autocorr, temper=temper, predictive=predictive)

    def nested_sampling(self, params, n_live=256, batch=32, steps=16, scale=None, seed=0, fixed=None, tol=1e-3, max_iter=None, n_iter=None,
                        keep_dead=True, device=True, evaluate=None, prior=None, prior_norm="auto", **kwargs):
        """Nested sampling of the joint lnL - one parameter vector for all blocks, or with ``"name@q"`` entries a value per
        block, at most 10 sampled values in all -, block-diagonal or under the joint covariance.  Arguments and result as
        ``CCFFit.nested_sampling`` (:mod:`victor_amd.nested`); the result keeps this joint fit alive."""
        from .nested import nested_sampling
        return nested_sampling(self, params, n_live, batch, steps, scale, seed, fixed, tol, max_iter, n_iter, keep_dead, device,
                               evaluate, kwargs, prior=prior, prior_norm=prior_norm)

    @property
    def n_data(self):
        return sum(len(f.s) * len(f.poles_s) for f in self.fits)

    def realisations(self, simulation_numbers=None, paired_model=False):
        """Every simulation realisation of the blocks' data files (or the listed ``simulation_numbers``) against this joint fit:
        :class:`JointRealisations`.  Every block's fit must have been built with an integer ``simulation_number``.
        ``paired_model=True`` (``CCFFit.realisations``: every mock with the model of its own real-space CCF) is refused."""
        if paired_model:
            raise InputError("JointFit.realisations: paired_model=True is not supported for joint fits (each block would need the "
                             "table sets of its own real-space CCF stack); use CCFFit.realisations(paired_model=True) per block")
        return JointRealisations(self, simulation_numbers)


class JointRealisations:
    """Realisations ``numbers`` of every block of ``joint`` (``JointFit.realisations``): joint realisation i is realisation
    ``numbers[i]`` of each block, read from that block's own file and keys.  ``blocks[q]`` is block q's
    :class:`victor_amd.realisations.Realisations` (its reader, checks and tables).

    Value contract: entry ``[p, i]`` equals ``JointFit([CCFFit(model_q, data_q with simulation_number=numbers[i]) for q],
    covariance=joint.covariance, likelihood=joint.likelihood).log_likelihood_batch(point p)`` to rounding, ``(-inf, inf)``
    exactly where that call returns it.  Under a joint covariance the theory vectors are computed once per point and every
    (point, realisation) pair is one row of the joint chi-square kernel (``vk_joint_cov_eval_realisations``); block-diagonal,
    the blocks' own ``Realisations`` results are summed on the host in block order."""

    def __init__(self, joint, simulation_numbers=None):
        blocks = [Realisations(f, simulation_numbers) for f in joint.fits]
        for q, r in enumerate(blocks[1:], 1):
            if len(r) != len(blocks[0]):
                raise InputError(f"JointFit.realisations: block 0 holds {len(blocks[0])} realisations and block {q} holds "
                                 f"{len(r)}; pass simulation_numbers to pick the same ones from every block")
        self.joint = joint
        self.blocks = blocks
        self.numbers = blocks[0].numbers

    def __len__(self):
        return len(self.numbers)

    def _upload(self, engines):
        """Make every block's realisations the ones set on its engine (``Realisations._upload``)."""
        for r, eng in zip(self.blocks, engines):
            r._upload(eng)

    def best_fit(self, params, fixed=None, start=None, step=None, xtol=None, ftol=1e-6, max_iter=None, restarts=1, prior=None,
                 covariance=None, **kwargs):
        """Best-fit point of every joint realisation: problem i maximises the joint lnL against realisation ``numbers[i]`` of
        every block, all of them in one run on the GPU.  Arguments as ``JointFit.best_fit``; ``fixed`` values must be scalars."""
        from .fitting import best_fit
        return best_fit(self.joint, params, fixed, start, step, xtol, ftol, max_iter, restarts, kwargs, realisations=self,
                        prior=prior, covariance=covariance)

    def laplace(self, params, at, step=None, fixed=None, prior=None, shrink=8, refine=0, keep_values=False, **kwargs):
        """The Laplace approximation of every joint realisation's posterior at its own point, all of them in one call on
        the GPU.  Arguments and result as ``JointFit.laplace``; ``fixed`` values must be scalars."""
        from .laplace import laplace
        return laplace(self.joint, params, at, step, fixed, prior, shrink, refine, keep_values, kwargs, realisations=self)

    def fisher(self, params, at, step=None, fixed=None, prior=None, shrink=8, keep_vectors=False, **kwargs):
        """The Fisher forecast (``JointFit.fisher``) at every joint realisation's own point, all of them in one call on the
        GPU; the realisations only supply the number of problems.  ``fixed`` values must be scalars."""
        from .fisher import fisher
        return fisher(self.joint, params, at, step, fixed, prior, shrink, keep_vectors, kwargs, realisations=self)

    def sample_chains(self, params, n_steps, walkers=8, seed=0, fixed=None, start=None, scatter=None, proposal=None, burn=0,
                      thin=1, keep_chain=True, device=True, move="metropolis", stretch_a=2.0, prior=None, marginals=None, autocorr=None, temper=None,
                      predictive=None, **kwargs):
        """``walkers`` Metropolis chains of EVERY joint realisation in lock step, on the GPU (``device=True``) or by the NumPy
        loop over :meth:`log_likelihood_pairs` that defines them (``device=False``).  Arguments and result as
        ``Realisations.sample_chains`` (``move="stretch"``: one ensemble per joint realisation); ``start`` may be the ``BestFit``
        of :meth:`best_fit`."""
        from .chains import sample_chains
        return sample_chains(self.joint, params, n_steps, walkers, seed, fixed, start, scatter, proposal, burn, thin, keep_chain,
                             device, kwargs, realisations=self, move=move, stretch_a=stretch_a, prior=prior, marginals=marginals,
                             autocorr=autocorr, temper=temper, predictive=predictive)

    def nested_sampling(self, params, n_live=256, batch=32, steps=16, scale=None, seed=0, fixed=None, tol=1e-3, max_iter=None, n_iter=None,
                        keep_dead=True, device=True, evaluate=None, prior=None, prior_norm="auto", **kwargs):
        """Nested sampling of EVERY joint realisation in lock step: one evidence and one posterior sample per joint mock.
        Arguments and result as ``Realisations.nested_sampling``."""
        from .nested import nested_sampling
        return nested_sampling(self.joint, params, n_live, batch, steps, scale, seed, fixed, tol, max_iter, n_iter, keep_dead, device,
                               evaluate, kwargs, realisations=self, prior=prior, prior_norm=prior_norm)

    def importance_posterior(self, params, proposal=None, n=16384, seed=0, fixed=None, prior=None, bins=64, ranges=None, pairs=None,
                             chunk=None, min_ess=50.0, device=True, evaluate=None, sample=None, ln_proposal=None, **kwargs):
        """The posterior of EVERY joint realisation from ONE shared importance sample (problem i: realisation ``numbers[i]`` of
        every block): a point's theory vectors are computed once per block and compared with all joint realisations, under the
        joint covariance (fixed or gridded in beta) or block-diagonal, and the evidence, the effective sample size, the moments
        and the marginal histograms of each are reduced on the GPU (``device=True``, ``vk_is_create_joint``) or by the NumPy
        loop over :meth:`log_likelihood` that defines them (``device=False``).  ``"name@q"`` parameters (:func:`per_block`) may be
        sampled or fixed - a sampled ``epsilon@q`` is refused - and a ``prior`` may name them.  Arguments and result as
        ``Realisations.importance_posterior`` (:mod:`victor_amd.importance`); ``predictive=True`` gives the band of the JOINT
        vector (``ip.predictive.multipoles_of(q)`` per block) and the DIC, ``tail=True`` every joint mock's Pareto shape and
        smoothed estimates (``ip.tail``).  The joint data vector itself (R = 1) goes through
        ``victor_amd.importance.importance_posterior(joint, params, ...)``."""
        from .importance import importance_posterior
        predictive = kwargs.pop("predictive", None)             # (a keyword of its own, not a model or fit option)
        tail = kwargs.pop("tail", None)                         # (likewise)
        return importance_posterior(self.joint, params, proposal, n, seed, fixed, prior, bins, ranges, pairs, chunk, min_ess, device,
                                    evaluate, sample, ln_proposal, kwargs, realisations=self, predictive=predictive, tail=tail)

    def _eval(self, params, kwargs, which=None):
        joint = self.joint
        blocks = has_block_names(params)
        if blocks:
            joint._check_block_names(params)
        if joint.covariance is None:
            return self._block_diagonal(params, kwargs, which)
        entry = "vk_joint_cov_eval_realisations"
        if blocks:
            # a row set per block, [B][n][VK_NPAR]: each block's theory launch reads its own slice of every chunk
            sets = joint._block_rows(params, kwargs)
            checked = [check_which(r, which, len(self)) for r in sets]
            which = checked[0][1]
            rows = np.ascontiguousarray([r for r, _ in checked], dtype=np.float64)
            n = rows.shape[1]
            entry += "_blocks"
        else:
            fit = joint.fits[0]
            rows = fit._fit_rows(params, fit._merged({k: v for k, v in kwargs.items() if k != "likelihood"}))
            rows, which = check_which(rows, which, len(self))
            rows = N.f64(rows).reshape(-1, N.VK_NPAR)
            n = len(rows)
        engines, opts = joint._plan_cov(kwargs)
        shape = (n,) if which is not None else (n, len(self))
        lnl, chi2 = np.empty(shape), np.empty(shape)
        if n == 0:
            return lnl, chi2
        for r, eng in zip(self.blocks, engines):
            r._upload(eng)
        lead = engines[0]
        handle = joint._joint_handle(lead)
        ctxs = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
        w = None
        if which is not None:
            which = np.ascontiguousarray(which, dtype=np.int32)
            w = which.ctypes.data_as(C.POINTER(C.c_int32))
        lead._check(getattr(lead._lib, entry)(handle, ctxs, len(engines), C.byref(opts), N.as_dp(rows), n, w, N.as_dp(lnl),
                                              N.as_dp(chi2)))
        return lnl, chi2

    def _block_diagonal(self, params, kwargs, which):
        """Each block's realisations under its own covariance, summed in block order; a failed block fails the entry (as
        ``JointFit._sequential``)."""
        lnl = chi2 = None
        blocks = has_block_names(params)
        for q, r in enumerate(self.blocks):
            a, b = r._eval(block_params(params, q) if blocks else params, kwargs, which)
            lnl = a if lnl is None else lnl + a
            chi2 = b if chi2 is None else chi2 + b
        bad = ~np.isfinite(lnl)
        lnl[bad], chi2[bad] = -np.inf, np.inf
        return lnl, chi2

    def log_likelihood(self, params, **kwargs):
        """(lnL, chi2) of the points against every joint realisation: each ``(n_real,)`` for a dict of scalars, ``(n_points,
        n_real)`` for a batch (as ``Realisations.log_likelihood``)."""
        lnl, chi2 = self._eval(params, kwargs)
        if isinstance(params, dict) and all(np.ndim(v) == 0 for v in params.values()):
            return lnl[0], chi2[0]
        return lnl, chi2

    def chi_squared(self, params, **kwargs):
        """The chi-square half of :meth:`log_likelihood` (data vectors interpolated in beta)."""
        return self.log_likelihood(params, **dict(kwargs, beta_interpolation="datavector"))[1]

    def log_likelihood_pairs(self, params, which, **kwargs):
        """(lnL, chi2), each ``(n_points,)``: point p against joint realisation ``numbers[which[p]]`` only.  The same bits as
        the matching entries of :meth:`log_likelihood`."""
        return self._eval(params, kwargs, which)
