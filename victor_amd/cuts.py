"""Scale cuts: every realisation under many s ranges and multipole sets in one call.

The first robustness question asked of a void-galaxy RSD result is how fsigma8 and epsilon move when the innermost bins are
dropped, or when only the monopole is fitted.  The theory vector of a parameter point does not depend on the cut, so the
shared-sample routes (``grid_posterior``, ``importance_posterior``) and every other device loop can serve K cuts of R
realisations from the evaluations they make anyway - provided the likelihood of a cut is formed correctly:

* the precision of a cut is the inverse of the SUB-covariance ``C[idx, idx]``, not a sub-block of the full precision;
* the log-determinant term is the sub-covariance's;
* Hartlap and Percival count the data points the cut keeps.

A problem is the flat index ``v = k * R + m`` (cut-major).  :class:`CutRealisations` is a
:class:`~victor_amd.realisations.Realisations` of ``K * R`` problems: it makes the data blocks AND the cuts' tables resident on
the engine (``vk_set_cuts``, ``include/victor_hip.h``; the kernel: ``csrc/vk_kernel_real_cuts.h``) and hands itself to the
existing drivers as ``realisations=``.  :func:`cut_likelihood` is the NumPy definition the kernel is held to.
"""

import weakref

import numpy as np

from . import _native as N
from .engine import covariance_logdets, data_table
from .realisations import Realisations, check_which
from .utils import InputError


class ScaleCut:
    """A selection of the fit's data vector (layout of ``CCFFit.multipole_datavector``: multipole-major): the s bins with
    ``s_min <= s <= s_max`` (either bound may be None) of the multipoles ``poles`` (None: all of ``fit.poles_s``) - or a boolean
    ``mask`` of length N, given alone."""

    def __init__(self, s_min=None, s_max=None, poles=None, mask=None):
        if mask is not None and (s_min is not None or s_max is not None or poles is not None):
            raise InputError("ScaleCut: a mask is given alone, without s_min / s_max / poles")
        self.s_min = None if s_min is None else float(s_min)
        self.s_max = None if s_max is None else float(s_max)
        self.poles = None if poles is None else tuple(int(p) for p in np.atleast_1d(poles))
        self.mask = None if mask is None else np.asarray(mask)

    def __repr__(self):
        if self.mask is not None:
            return f"ScaleCut(mask: {int(np.count_nonzero(self.mask))} of {self.mask.size})"
        return f"ScaleCut(s_min={self.s_min}, s_max={self.s_max}, poles={self.poles})"

    def resolve(self, fit):
        """The strictly increasing index list of the entries kept, into ``fit``'s data vector."""
        n_s, poles_s = len(fit.s), [int(p) for p in np.atleast_1d(fit.poles_s)]
        n = n_s * len(poles_s)
        if self.mask is not None:
            if self.mask.dtype != np.bool_ or self.mask.shape != (n,):
                raise InputError(f"ScaleCut: mask must be a boolean array of length {n}")
            keep = self.mask
        else:
            poles = poles_s if self.poles is None else list(self.poles)
            if len(set(poles)) != len(poles) or any(p not in poles_s for p in poles):
                raise InputError(f"ScaleCut: poles {poles} must be a subset of the fit's {poles_s}, each named once")
            s = np.asarray(fit.s, dtype=float)
            in_s = np.ones(n_s, dtype=bool)
            if self.s_min is not None:
                in_s &= s >= self.s_min
            if self.s_max is not None:
                in_s &= s <= self.s_max
            if not in_s.any():
                raise InputError(f"{self!r}: the bounds select no s bin (s runs from {s.min():g} to {s.max():g})")
            keep = np.concatenate([in_s if p in poles else np.zeros(n_s, dtype=bool) for p in poles_s])
        idx = np.flatnonzero(keep).astype(np.int32)
        if idx.size == 0:
            raise InputError(f"{self!r} keeps no entry of the data vector")
        return idx


class CutTables:
    """What the likelihood of one cut reads: ``idx`` (n,), the sub-covariance slices ``cov`` and their inverses ``prec``
    (S, n, n; S = 1 for a fixed covariance) and, on a covariance gridded in beta, ``logdet`` (S,) and ``eig`` (S, n) of
    :func:`victor_amd.engine.covariance_logdets`."""

    def __init__(self, idx, cov, prec, logdet, eig):
        self.idx, self.cov, self.prec, self.logdet, self.eig = idx, cov, prec, logdet, eig
        self.n = len(idx)


def cut_tables(fit, cuts):
    """One :class:`CutTables` per cut of ``cuts`` (``ScaleCut`` objects) for ``fit``: the precision slices are
    ``np.linalg.inv(C_j[idx, idx])`` - the call ``load_covariance_matrix`` makes on the full stack -, log det and blend
    eigenvalues those of the sub-covariance stack with the blend rule and failure marks of ``covariance_logdets``.  Refused
    (``InputError``): an empty list, a cut that keeps nothing, two cuts that keep the same entries."""
    cuts = list(cuts)
    if not cuts or not all(isinstance(c, ScaleCut) for c in cuts):
        raise InputError("scale_cuts: give a non-empty list of ScaleCut objects")
    stack = np.asarray(fit.covmat, dtype=float)
    stack = stack[None] if fit.fixed_covmat else stack
    out, seen = [], {}
    for k, cut in enumerate(cuts):
        idx = cut.resolve(fit)
        key = idx.tobytes()
        if key in seen:
            raise InputError(f"scale_cuts: cuts {seen[key]} and {k} keep the same entries ({cuts[seen[key]]!r}, {cut!r})")
        seen[key] = k
        cov = np.ascontiguousarray(stack[:, idx][:, :, idx])
        prec = np.linalg.inv(cov)
        logdet = eig = None
        if not fit.fixed_covmat:
            logdet, eig = covariance_logdets(cov, np.asarray(fit.beta_covmat, dtype=float))
        out.append(CutTables(idx, cov, prec, logdet, eig))
    return out


def pack_cut_tables(tables, n_full, n_beta_c):
    """The arrays of ``vk_set_cuts`` for a data vector of ``n_full`` entries: ``n_keep`` [K], ``index`` [K][N], ``prec``
    [K][S][N N] (slot (k, j) holds the n_k x n_k slice compact, zeros behind), ``logdet`` [K][n_beta_c] and ``eig``
    [K][n_beta_c][N] (None for a fixed covariance): fixed strides of the full N, whatever a cut keeps."""
    K, S = len(tables), max(int(n_beta_c), 1)
    n_keep = np.array([t.n for t in tables], dtype=np.int32)
    index = np.zeros((K, n_full), dtype=np.int32)
    prec = np.zeros((K, S, n_full * n_full))
    logdet = np.zeros((K, n_beta_c)) if n_beta_c else None
    eig = np.ones((K, n_beta_c, n_full)) if n_beta_c else None
    for k, t in enumerate(tables):
        index[k, : t.n] = t.idx
        prec[k, :, : t.n * t.n] = t.prec.reshape(S, t.n * t.n)
        if n_beta_c:
            logdet[k] = t.logdet
            eig[k, :, : t.n] = t.eig
    return n_keep, index, prec, logdet, eig


def cut_likelihood(fit, theory, data_at_beta, beta, tables_k, fit_options):
    """(lnL, chi2) of one theory vector (N,) against one data vector at beta (N,) under the cut ``tables_k`` - the NumPy
    definition.  Bracket and blend of ``CCFFit._bracket`` / ``_interp_stack`` on the cut's slices; the log-determinant rule of
    the reference (``ccf_fit.py:445-453``: ``slogdet`` of the blended sub-covariance, a sign other than +1 fails the point); the
    four likelihood forms of ``ccf_fit.py:455-473`` with the number of data points = n_k; ``(-inf, inf)`` where the reference rule
    gives it (``:448-450``, ``:477-481``)."""
    t_k = tables_k
    r = np.asarray(theory, dtype=float)[t_k.idx] - np.asarray(data_at_beta, dtype=float)[t_k.idx]
    failed = (-np.inf, np.inf)
    if fit.fixed_covmat:
        P, like_factor = t_k.prec[0], 0.0
    else:
        if not np.isfinite(beta):
            return failed                                    # (no bracket: every kernel reports the row as failed)
        lo, w = fit._bracket(beta)
        if w == 0.0:
            P, cov = t_k.prec[lo], t_k.cov[lo]
        else:
            P, cov = (1 - w) * t_k.prec[lo] + w * t_k.prec[-1], (1 - w) * t_k.cov[lo] + w * t_k.cov[-1]
        sign, ld = np.linalg.slogdet(cov)
        if not sign == 1:
            return failed
        like_factor = -0.5 * ld
    chisq = float(np.dot(np.dot(r, P), r))
    like = fit_options["likelihood"]
    form = like["form"].lower()
    nd = t_k.n
    with np.errstate(invalid="ignore", divide="ignore"):
        if form == "sellentin":
            nm = like.get("nmocks", 1)
            lnl = -nm * np.log(1 + chisq / (nm - 1)) / 2 + like_factor
        elif form == "hartlap":
            nm = like.get("nmocks", 1)
            lnl = -0.5 * chisq * ((nm - nd - 2) / (nm - 1)) + like_factor
        elif form == "percival":
            nm = like.get("nmocks", 1)
            npar = like["nparams"]
            B = (nm - nd - 2) / ((nm - nd - 1) * (nm - nd - 4))
            m = npar + 2 + (nm - 1 + B * (nd - npar)) / (1 + B * (nd - npar))
            lnl = -m * np.log(1 + chisq / (nm - 1)) / 2 + like_factor
        elif form == "gaussian":
            lnl = -0.5 * chisq + like_factor
        else:
            raise InputError("Unrecognised likelihood form")
    if np.isnan(lnl):
        return failed
    return float(lnl), chisq


class CutRealisations(Realisations):
    """K cuts x R realisations as ``K * R`` problems (flat index ``k * R + m``), from ``Realisations.scale_cuts`` or
    ``CCFFit.scale_cuts`` (R = 1: the fit's own data vector).  ``len() == K * R``, ``shape == (K, R)``; results of the device
    loops carry the flat problem axis, :meth:`unflatten` reshapes it to ``(K, R, ...)``."""

    def __init__(self, fit, cuts, blocks, numbers):
        from .joint import JointFit
        if isinstance(fit, JointFit):
            raise InputError("scale_cuts: joint fits are not supported (a cut of a joint vector needs the joint covariance's own "
                             "sub-blocks)")
        if getattr(fit, "_broker_spec", False):
            raise InputError("scale_cuts: a fit served by a broker (broker=) is not supported; build the fit with broker=False")
        self.fit = fit
        self.cuts = list(cuts)
        self.tables = cut_tables(fit, self.cuts)
        self.blocks = np.ascontiguousarray(blocks, dtype=np.float64)
        self.numbers = np.asarray(numbers, dtype=int)
        self.shape = (len(self.cuts), len(self.numbers))
        self.paired_model = False
        self._sets, self._sets_of = {}, {}
        n_beta_c = 0 if fit.fixed_covmat else len(fit.beta_covmat)
        self._packed = pack_cut_tables(self.tables, len(fit.s) * len(np.atleast_1d(fit.poles_s)), n_beta_c)

    def __len__(self):
        return self.shape[0] * self.shape[1]

    def unflatten(self, a):
        """``a`` with its leading problem axis (K * R) reshaped to (K, R)."""
        a = np.asarray(a)
        if a.shape[:1] != (len(self),):
            raise InputError(f"unflatten: the leading axis holds {a.shape[:1]} entries, there are {len(self)} problems")
        return a.reshape(self.shape + a.shape[1:])

    def scale_cuts(self, cuts):
        return CutRealisations(self.fit, cuts, self.blocks, self.numbers)

    # ------------------------------------------------------------------ device plumbing -------
    def _plan(self, kwargs):
        fit_options = self.fit._merged_fit(kwargs)
        if fit_options["beta_interpolation"] == "likelihood" and not self.fit.fixed_data:
            raise InputError("scale_cuts: beta_interpolation='likelihood' is not supported on data gridded in beta")
        return super()._plan(kwargs)

    def _upload(self, eng):
        """Make this object's realisations AND cuts the ones resident on ``eng``; a plain ``Realisations`` that uploads afterwards
        clears the cuts (``vk_set_realisations`` drops them)."""
        owner = getattr(eng, "_real_owner", None)
        if owner is None or owner() is not self:
            if getattr(eng, "_model_sets", False):
                eng.set_model_realisations(None, None, None)
                eng._model_sets = False
            eng.set_realisations(self.blocks)
            eng._real_owner = None                          # (until the cuts are there as well)
            eng.set_cuts(*self._packed)
            eng._real_owner = weakref.ref(self)

    # ------------------------------------------------------------------ likelihood ------------
    def data_at(self, m, beta):
        """Data vector (N,) of realisation ``m`` (an index into ``numbers``) at ``beta``, from its uploaded block: the vector
        itself, or Horner on the PCHIP piece the kernels pick (``vk_tables.data``)."""
        fit = self.fit
        if fit.fixed_data:
            return self.blocks[m]
        g = np.asarray(fit.beta_ccf, dtype=float)
        kb = 0
        for i in range(1, len(g) - 1):
            if beta >= g[i]:
                kb = i
        db = beta - g[kb]
        c = self.blocks[m].reshape(len(g) - 1, -1, 4)[kb]
        return c[:, 0] + db * (c[:, 1] + db * (c[:, 2] + db * c[:, 3]))

    def _definition(self, params, kwargs, which):
        """The host definition: the device's theory vectors (``CCFFit.theory_vector_batch``) through :func:`cut_likelihood`."""
        fit = self.fit
        model = fit._merged(kwargs)
        fit._check_supported(model)
        fit_options = fit._merged_fit(kwargs)
        if fit_options["beta_interpolation"] == "likelihood" and not fit.fixed_data:
            raise InputError("scale_cuts: beta_interpolation='likelihood' is not supported on data gridded in beta")
        rows, which = check_which(fit._fit_rows(params, model), which, len(self))
        theory = fit.theory_vector_batch(rows, **kwargs)
        K, R = self.shape
        beta = rows[:, N.P_BETA]
        pairs = [(int(v) // R, int(v) % R) for v in which] if which is not None else None
        out = np.empty((2, len(rows)) + (() if which is not None else (K * R,)))
        for p in range(len(rows)):
            todo = [pairs[p]] if pairs is not None else [(k, m) for k in range(K) for m in range(R)]
            data = {}
            for k, m in todo:
                if m not in data:
                    data[m] = self.data_at(m, beta[p])
                val = cut_likelihood(fit, theory[p], data[m], beta[p], self.tables[k], fit_options)
                if pairs is not None:
                    out[:, p] = val
                else:
                    out[:, p, k * R + m] = val
        return out[0], out[1]

    def _eval(self, params, kwargs, which=None):
        kwargs = dict(kwargs)
        if not kwargs.pop("device", True):
            return self._definition(params, kwargs, which)
        model, fit_options, eng, opts = self._plan(kwargs)
        rows, which = check_which(self.fit._fit_rows(params, model), which, len(self))
        return eng.eval_realisations(opts, rows, len(self), which)

    def log_likelihood(self, params, **kwargs):
        """(lnL, chi2) of the points under every cut against every realisation: each ``(n_points, K, R)``, or ``(K, R)`` for a
        dict of scalars.  ``device=False``: the NumPy definition (:func:`cut_likelihood` on the device's theory vectors)."""
        lnl, chi2 = self._eval(params, kwargs)
        lnl, chi2 = lnl.reshape((-1,) + self.shape), chi2.reshape((-1,) + self.shape)
        if isinstance(params, dict) and all(np.ndim(v) == 0 for v in params.values()):
            return lnl[0], chi2[0]
        return lnl, chi2

    def _cross(self, params, **kwargs):
        """:meth:`log_likelihood` with the problem axis flat, ``(n_points, K * R)``: what the definition routes of the
        shared-sample drivers (``grid_posterior``, ``importance_posterior``) consume in its place."""
        return self._eval(params, kwargs)

    def chi_squared(self, params, **kwargs):
        """The chi-square half of :meth:`log_likelihood` (data vector interpolated in beta, as ``Realisations.chi_squared``)."""
        return self.log_likelihood(params, **dict(kwargs, beta_interpolation="datavector"))[1]

    def log_likelihood_pairs(self, params, which, **kwargs):
        """(lnL, chi2), each ``(n_points,)``: point p against problem ``which[p] = k * R + m`` only.  The same bits as the
        matching entries of :meth:`log_likelihood`; ``device=False``: the NumPy definition."""
        return self._eval(params, kwargs, which)

    # ------------------------------------------------------------------ refusals --------------
    def fisher(self, *args, **kwargs):
        raise InputError("scale_cuts: fisher is not supported (the forecast forms J^T P J from the fit's full precision)")

    def model_sets(self, *args, **kwargs):
        raise InputError("scale_cuts: paired_model realisations are not supported")

    def sample_chains(self, params, n_steps, walkers=8, seed=0, fixed=None, start=None, scatter=None, proposal=None, burn=0,
                      thin=1, keep_chain=True, device=True, move="metropolis", stretch_a=2.0, prior=None, marginals=None, autocorr=None,
                      temper=None, predictive=None, **kwargs):
        if predictive:
            raise InputError("scale_cuts: predictive= is not supported (the band and the DIC are of the full data vector)")
        return super().sample_chains(params, n_steps, walkers, seed, fixed, start, scatter, proposal, burn, thin, keep_chain, device,
                                     move, stretch_a, prior, marginals, autocorr, temper, None, **kwargs)

    def importance_posterior(self, params, *args, **kwargs):
        if kwargs.get("predictive", None):
            raise InputError("scale_cuts: predictive= is not supported (the band and the DIC are of the full data vector)")
        return super().importance_posterior(params, *args, **kwargs)


def from_fit(fit, cuts):
    """``CCFFit.scale_cuts``: the fit's own data vector as the one block (R = 1)."""
    poles = np.atleast_1d(fit.poles_s)
    stack = np.array([fit.redshift_multipoles[f"{ell}"] for ell in poles])
    block = data_table(stack, fit.fixed_data, None if fit.fixed_data else fit.beta_ccf).ravel()
    number = fit._data_source[1].get("simulation_number", None)
    return CutRealisations(fit, cuts, block[None], [0 if number is None else int(number)])


def from_realisations(rs, cuts):
    """``Realisations.scale_cuts``."""
    if getattr(rs, "paired_model", False):
        raise InputError("scale_cuts: realisations(paired_model=True) are not supported (a row's table set is its realisation, "
                         "not the flat problem index)")
    return CutRealisations(rs.fit, cuts, rs.blocks, rs.numbers)
