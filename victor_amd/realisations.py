"""One model against every simulation realisation of a data file: mock validation in one call per parameter batch.

The reference fits one measured CCF at a time; a data file may hold a stack of realisations (mocks), of which
``redshift_space_ccf.simulation_number`` picks one when the fit is built (reference: ``ccf_fit.py:59-61,93-100``;
``utils.convert_hans_quijote_to_hdf5`` writes such stacks, ``utils.py:161-242``).  :class:`Realisations` reads the whole stack
(or a subset) from the same file and keys the fit was built from and evaluates parameter points against all of them: each point's
theory vector is computed once on the GPU and compared with every realisation's data vector there (``vk_eval_realisations``,
``include/victor_hip.h``).  Model, covariance, options and engine are the fit's.

Value contract: entry ``[p, m]`` equals ``CCFFit(model, data with simulation_number=numbers[m]).log_likelihood(point p)`` to
rounding (the chi-square is summed in another order), ``(-inf, inf)`` exactly where that call returns it.

``paired_model=True``: every realisation with the model of ITS OWN real-space CCF.  The reference picks one simulation out of a
stacked model file as it does out of the data file (``realspace_ccf.simulation_number``, reference: ``ccf_model.py:127-162``);
a mock test fits mock m's redshift-space multipoles with the model built from mock m's real-space multipoles.  The object then
compiles the xi^r tables of every listed simulation (:func:`victor_amd.engine.build_tables`), checks that nothing else of the
model's tables depends on the simulation, and keeps the sets on the device next to the data blocks
(``vk_set_model_realisations``): every route evaluates row i from table set ``which[i]``, and the contract reads ``CCFFit(model
with realspace_ccf.simulation_number=numbers[m], data with simulation_number=numbers[m])``.  The streaming model only.
"""

import copy
import weakref

import numpy as np

from . import _native as N
from . import utils
from .engine import data_table
from .utils import InputError


PAIR_CHUNK = 65536        # pairs per device call of a paired object's cross mode (Realisations._eval_rows)


def check_which(rows, which, n_real):
    """(rows, which) of a pairs-mode call: one realisation index in 0 .. n_real - 1 per row (a single row is repeated for
    every index); ``which=None`` passes through."""
    if which is None:
        return rows, None
    which = np.atleast_1d(np.asarray(which))
    if len(rows) == 1 and len(which) > 1:
        rows = np.repeat(rows, len(which), axis=0)
    if which.ndim != 1 or len(which) != len(rows) or not np.issubdtype(which.dtype, np.integer):
        raise InputError(f"which must hold one realisation index per point ({len(rows)})")
    if np.any((which < 0) | (which >= n_real)):
        raise InputError(f"realisation index out of range 0..{n_real - 1}")
    return rows, which


class Realisations:
    """Realisations ``numbers`` of ``fit``'s data file (``CCFFit.realisations``).  ``blocks[i]`` is realisation ``numbers[i]``
    in the layout of ``vk_tables.data``; it is uploaded once per engine the object evaluates on."""

    def __init__(self, fit, simulation_numbers=None, paired_model=False):
        from .joint import JointFit
        if paired_model and isinstance(fit, JointFit):
            raise InputError("paired_model=True is not supported for joint fits")
        data_fn, ccf = fit._data_source
        if not isinstance(ccf.get("simulation_number", None), int):
            raise InputError("realisations() needs a fit constructed with an integer simulation_number "
                             "(redshift_space_ccf.simulation_number)")
        input_data = utils.read_input_file(data_fn, fit.extensions)
        keys = np.atleast_1d(ccf["ccf_keys"])[1:]
        want = fit.s.shape if fit.fixed_data else (len(fit.beta_ccf), len(fit.s))
        stacks = []
        for key in keys:
            a = np.asarray(input_data[key], dtype=float)
            if a.ndim != len(want) + 1:
                raise InputError(f"{key} in {data_fn} has no realisation axis (shape {a.shape})")
            if a.shape[1:] != want:
                raise InputError(f"Shape of a realisation of {key} is {a.shape[1:]}, expected {want}")
            stacks.append(a)
        n_sims = stacks[0].shape[0]
        if any(a.shape[0] != n_sims for a in stacks):
            raise InputError(f"the multipoles in {data_fn} hold different numbers of realisations")
        if simulation_numbers is None:
            numbers = np.arange(n_sims)
        else:
            numbers = np.atleast_1d(np.asarray(simulation_numbers))
            if numbers.size == 0 or numbers.ndim != 1 or not np.issubdtype(numbers.dtype, np.integer):
                raise InputError("simulation_numbers must be a non-empty list of integers")
            bad = numbers[(numbers < 0) | (numbers >= n_sims)]
            if bad.size:
                raise InputError(f"simulation number {int(bad[0])} is out of range: {data_fn} holds {n_sims} realisations")
        self.fit = fit
        self.numbers = numbers.astype(int)
        beta = None if fit.fixed_data else fit.beta_ccf
        self.blocks = np.ascontiguousarray(np.stack(
            [data_table(np.array([a[m] for a in stacks]), fit.fixed_data, beta).ravel() for m in self.numbers]))
        self.paired_model = bool(paired_model)
        self._sets = {}           # (engine key, Simpson rule) -> (xi.coef, uni_xi, uni_xic) of every listed simulation, stacked
        self._sets_of = {}        # id(engine) -> the entry of _sets it evaluates with
        if self.paired_model:
            self._real_input = self._read_real_stack(n_sims, data_fn)

    # ------------------------------------------------------------------ paired model: table sets -------
    def _read_real_stack(self, n_sims, data_fn):
        """The model file's contents, after checking that its real-space CCF keys hold one realisation per realisation of the
        data file (both formats of ``CCFModel._load_realspace_ccf``)."""
        fit = self.fit
        model_fn, rc = fit._real_source
        if not isinstance(rc.get("simulation_number", None), int):
            raise InputError("realisations(paired_model=True) needs a model constructed with an integer simulation_number "
                             "(realspace_ccf.simulation_number)")
        input_data = utils.read_input_file(model_fn, fit.extensions)
        keys = np.atleast_1d(rc["ccf_keys"])
        if rc.get("format", "multipoles") == "multipoles":
            stack_keys = keys[1:]
            want = fit.r.shape if fit.fixed_real_input else (len(fit.beta), len(fit.r))
        else:
            stack_keys = keys[2:]
            n_mu = len(np.asarray(input_data[keys[1]]))
            want = (len(fit.r), n_mu) if fit.fixed_real_input else (len(fit.beta), len(fit.r), n_mu)
        for key in stack_keys:
            a = np.asarray(input_data[key])
            if a.ndim != len(want) + 1:
                raise InputError(f"{key} in {model_fn} has no realisation axis (shape {a.shape})")
            if a.shape[1:] != want:
                raise InputError(f"Shape of a realisation of {key} in {model_fn} is {a.shape[1:]}, expected {want}")
            if a.shape[0] != n_sims:
                raise InputError(f"{key} in {model_fn} holds {a.shape[0]} realisations, the data file {data_fn} holds {n_sims}")
        return input_data

    def _model_of(self, number):
        """The fit with the real-space CCF of simulation ``number`` in place of its own: what ``CCFModel`` reads when it is
        built with that ``realspace_ccf.simulation_number`` (same loader), everything else shared."""
        clone = copy.copy(self.fit)
        clone._engine = None
        _, rc = self.fit._real_source
        clone._load_realspace_ccf(dict(rc, simulation_number=int(number)), self._real_input)
        return clone

    def model_sets(self, matter_model=None, simpson_even=None):
        """``(xi_coef, uni_xi, uni_xic)``: the three xi^r arrays of ``vk_tables`` for every listed simulation, stacked in the
        order of ``numbers`` (``uni_*``: ``None`` for tables without the unified grid).  Every other model-side array must equal
        the fit's own bit for bit - a velocity profile derived from xi^r (``linear_bias``) or another ``r`` grid would need sets
        of their own - else ``InputError`` names the first one that differs."""
        from . import tables as T
        from .engine import build_tables, table_array_lengths
        fit = self.fit
        matter_model = matter_model or fit._engine_key(fit.model)
        rule = T.simpson_even_rule(simpson_even if simpson_even is not None else fit.model["simpson_even"])
        key = (matter_model, rule)
        if key in self._sets:
            return self._sets[key]
        if not self.paired_model:
            raise InputError("model_sets() needs realisations(paired_model=True)")
        mine = ("xi.coef", "uni_xi", "uni_xic")
        data_side = ("beta_d", "data", "beta_c", "prec", "logdet", "eig")

        def arrays(t):
            out = {}
            for name, n in table_array_lengths(t).items():
                obj = t
                for part in name.split("."):
                    obj = getattr(obj, part)
                if name in data_side:
                    continue
                out[name] = np.ctypeslib.as_array(obj, shape=(n,)).copy() if (n and obj) else None
            return out

        def scalars(t):
            return [(n, getattr(t, n)) for n, ct in t._fields_ if isinstance(getattr(t, n), (int, float))] + \
                   [(f"{p}.{n}", getattr(getattr(t, p), n)) for p in ("xi", "vr", "sv") for n in ("n_int", "lead", "inv_h")]

        t0, keep0 = build_tables(fit, None, matter_model, rule)
        ref, ref_s = arrays(t0), scalars(t0)
        del keep0
        stacks = {n: [] for n in mine}
        for number in self.numbers:
            t, keep = build_tables(self._model_of(number), None, matter_model, rule)
            got, got_s = arrays(t), scalars(t)
            del keep
            for (n, a), (_, b) in zip(ref_s, got_s):
                if a != b:
                    raise InputError(f"paired_model: vk_tables.{n} of simulation {int(number)} differs from the fit's own "
                                     f"({b} against {a}); only the real-space CCF may depend on the simulation")
            for n, a in ref.items():
                b = got[n]
                if n in mine:
                    if (a is None) != (b is None) or (a is not None and a.shape != b.shape):
                        raise InputError(f"paired_model: vk_tables.{n} of simulation {int(number)} has another length than the fit's own")
                    stacks[n].append(b)
                elif (a is None) != (b is None) or (a is not None and a.tobytes() != b.tobytes()):
                    raise InputError(f"paired_model: vk_tables.{n} of simulation {int(number)} differs from the fit's own; only the "
                                     "real-space CCF may depend on the simulation (a velocity profile derived from it, as with "
                                     "matter_ccf.model linear_bias, or another r grid would need table sets of their own)")
        sets = tuple(None if stacks[n][0] is None else np.ascontiguousarray(np.stack(stacks[n])) for n in mine)
        self._sets[key] = sets
        return sets

    def __len__(self):
        return len(self.numbers)

    # ------------------------------------------------------------------ device plumbing -------
    def _plan(self, kwargs):
        fit = self.fit
        model = fit._merged(kwargs)
        fit._check_supported(model)
        fit_options = fit._merged_fit(kwargs)
        sets = None
        if self.paired_model:
            if model["rsd_model"] != "streaming":
                raise InputError(f"realisations(paired_model=True) supports rsd_model 'streaming' only, not '{model['rsd_model']}'")
            sets = self.model_sets(fit._engine_key(model), model["simpson_even"])     # (refusals before any device call)
        eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
        if sets is not None:
            self._sets_of[id(eng)] = sets
        self._upload(eng)
        return model, fit_options, eng, eng.make_opts(model, fit_options)

    def _upload(self, eng):
        """Make this object's realisations the ones set on ``eng`` (uploaded only when another object's, or none, are there):
        the data blocks and, paired, the xi^r table sets; an object without them clears the sets another one left."""
        owner = getattr(eng, "_real_owner", None)
        if owner is None or owner() is not self:
            eng.set_realisations(self.blocks)
            if self.paired_model:
                eng.set_model_realisations(*self._sets_of[id(eng)])
                eng._model_sets = True
            elif getattr(eng, "_model_sets", False):
                eng.set_model_realisations(None, None, None)
                eng._model_sets = False
            eng._real_owner = weakref.ref(self)

    def _eval(self, params, kwargs, which=None):
        model, fit_options, eng, opts = self._plan(kwargs)
        rows, which = check_which(self.fit._fit_rows(params, model), which, len(self))
        if fit_options["beta_interpolation"] == "likelihood" and not self.fit.fixed_data:
            return self._likelihood_interp(eng, opts, rows, which)
        return self._eval_rows(eng, opts, rows, which)

    def _eval_rows(self, eng, opts, rows, which):
        """``Engine.eval_realisations``; paired, cross mode (``which=None``) expands to pairs on the host - a point has one
        theory vector per realisation: rows repeated ``n_real`` times, ``which`` tiled, in chunks of whole points, reshaped to
        ``(n_points, n_real)``."""
        if not self.paired_model or which is not None:
            return eng.eval_realisations(opts, rows, len(self), which)
        R = len(self)
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, N.VK_NPAR)
        lnl, chi2 = np.empty((len(rows), R)), np.empty((len(rows), R))
        per = max(1, PAIR_CHUNK // R)
        for lo in range(0, len(rows), per):
            part = rows[lo:lo + per]
            l, c = eng.eval_realisations(opts, np.repeat(part, R, axis=0), R, np.tile(np.arange(R, dtype=np.int32), len(part)))
            lnl[lo:lo + per] = l.reshape(len(part), R)
            chi2[lo:lo + per] = c.reshape(len(part), R)
        return lnl, chi2

    def _likelihood_interp(self, eng, opts, rows, which):
        """beta_interpolation='likelihood' (reference: ccf_fit.py:383-440): both bracketing grid betas against every
        realisation, lnL and chi2 blended as CCFFit blends them."""
        g = self.fit.beta_ccf
        beta = rows[:, N.P_BETA]
        lo = np.array([np.where(g < b)[0][-1] for b in beta])       # IndexError outside the grid, as the reference
        hi = np.array([np.where(g >= b)[0][0] for b in beta])
        t = (beta - g[lo]) / (g[hi] - g[lo])
        both = np.concatenate([rows, rows])
        both[: len(rows), N.P_BETA] = g[lo]
        both[len(rows):, N.P_BETA] = g[hi]
        lnl, chi2 = self._eval_rows(eng, opts, both, None if which is None else np.concatenate([which, which]))
        n = len(rows)
        if which is None:
            t = t[:, None]
        bad = ~np.isfinite(lnl[:n]) | ~np.isfinite(lnl[n:])          # singular at either end fails both (:402-410)
        out_l = (1 - t) * lnl[:n] + t * lnl[n:]
        out_c = (1 - t) * chi2[:n] + t * chi2[n:]
        out_l[bad] = -np.inf
        out_c[bad] = np.inf
        return out_l, out_c

    # ------------------------------------------------------------------ likelihood (device) ---
    def log_likelihood(self, params, **kwargs):
        """(lnL, chi2) of the points against every realisation: each ``(n_real,)`` for a dict of scalars, ``(n_points,
        n_real)`` for a batch (array-valued parameters broadcast as in ``CCFFit.log_likelihood_batch``, or rows)."""
        lnl, chi2 = self._eval(params, kwargs)
        if isinstance(params, dict) and all(np.ndim(v) == 0 for v in params.values()):
            return lnl[0], chi2[0]
        return lnl, chi2

    def scale_cuts(self, cuts):
        """These realisations under every cut of ``cuts`` (:class:`victor_amd.cuts.ScaleCut`) at once: a
        :class:`victor_amd.cuts.CutRealisations` of ``len(cuts) * len(self)`` problems.  Refused with ``paired_model=True``."""
        from .cuts import from_realisations
        return from_realisations(self, cuts)

    def chi_squared(self, params, **kwargs):
        """The chi-square half of :meth:`log_likelihood` (data vector interpolated in beta, as ``CCFFit.chi_squared``)."""
        return self.log_likelihood(params, **dict(kwargs, beta_interpolation="datavector"))[1]

    def best_fit(self, params, fixed=None, start=None, step=None, xtol=None, ftol=1e-6, max_iter=None, restarts=1, prior=None,
                 covariance=None, **kwargs):
        """Best-fit point of every realisation: problem i maximises lnL against realisation ``numbers[i]``, all of them in one
        run on the GPU.  Arguments as ``CCFFit.best_fit`` (``prior``: one Gaussian prior for all realisations); ``fixed``
        values must be scalars here."""
        from .fitting import best_fit
        return best_fit(self.fit, params, fixed, start, step, xtol, ftol, max_iter, restarts, kwargs, realisations=self, prior=prior,
                        covariance=covariance)

    def laplace(self, params, at, step=None, fixed=None, prior=None, shrink=8, refine=0, keep_values=False, **kwargs):
        """The Laplace approximation of EVERY realisation's posterior at its own point (``at``: the ``BestFit`` of
        :meth:`best_fit`, or a dict name -> scalar or one value per realisation): all R stencils in one call on the GPU.
        Arguments and result as ``CCFFit.laplace``; ``fixed`` values must be scalars here."""
        from .laplace import laplace
        return laplace(self.fit, params, at, step, fixed, prior, shrink, refine, keep_values, kwargs, realisations=self)

    def fisher(self, params, at, step=None, fixed=None, prior=None, shrink=8, keep_vectors=False, **kwargs):
        """The Fisher forecast (``CCFFit.fisher``) at EVERY realisation's own point (``at``: typically the ``BestFit`` of
        :meth:`best_fit`), one problem per realisation in one call on the GPU.  The realisations only supply the number of
        problems: the forecast reads no data.  Arguments and result as ``CCFFit.fisher``; ``fixed`` values must be scalars
        here."""
        from .fisher import fisher
        return fisher(self.fit, params, at, step, fixed, prior, shrink, keep_vectors, kwargs, realisations=self)

    def sample_chains(self, params, n_steps, walkers=8, seed=0, fixed=None, start=None, scatter=None, proposal=None, burn=0,
                      thin=1, keep_chain=True, device=True, move="metropolis", stretch_a=2.0, prior=None, marginals=None, autocorr=None, temper=None,
                      predictive=None, **kwargs):
        """``walkers`` Metropolis chains of EVERY realisation, all of them in lock step: problem i samples lnL against realisation
        ``numbers[i]``, on the GPU (``device=True``) or by the NumPy loop over :meth:`log_likelihood_pairs` that defines the
        chains (``device=False``).  Arguments and result as ``CCFFit.sample_chains`` (:mod:`victor_amd.chains`); ``start`` may be
        the :class:`~victor_amd.fitting.BestFit` of :meth:`best_fit`.  ``move="stretch"``: one stretch-move ensemble of
        ``walkers`` walkers per realisation instead."""
        from .chains import sample_chains
        return sample_chains(self.fit, params, n_steps, walkers, seed, fixed, start, scatter, proposal, burn, thin, keep_chain,
                             device, kwargs, realisations=self, move=move, stretch_a=stretch_a, prior=prior, marginals=marginals,
                             autocorr=autocorr, temper=temper, predictive=predictive)

    def grid_posterior(self, params, bins=32, ranges=None, fixed=None, prior=None, pairs=None, chunk=None, device=True, **kwargs):
        """The posterior of EVERY realisation on one shared grid (R = ``len(self)`` problems): a grid point's theory vector is
        computed once and compared with all realisations, and marginals, profiles and the evidence are reduced on the GPU
        (``device=True``) or by the NumPy loop over :meth:`log_likelihood` that defines them (``device=False``).  Arguments and
        result as ``CCFFit.grid_posterior`` (:mod:`victor_amd.grid`).  Refused with ``paired_model=True``: a point then has one
        theory vector per realisation."""
        from .grid import grid_posterior
        return grid_posterior(self.fit, params, bins, ranges, fixed, prior, pairs, chunk, device, kwargs, realisations=self)

    def importance_posterior(self, params, q=None, n=16384, seed=0, fixed=None, prior=None, bins=64, ranges=None, pairs=None, chunk=None,
                             min_ess=50.0, device=True, evaluate=None, sample=None, ln_proposal=None, **kwargs):
        """The posterior of EVERY realisation from ONE shared importance sample (R = ``len(self)`` problems): a point's theory
        vector is computed once and compared with all realisations, and the evidence, the effective sample size, the moments
        and the marginal histograms of each are reduced on the GPU (``device=True``) or by the NumPy loop over
        :meth:`log_likelihood` that defines them (``device=False``).  Arguments and result as ``CCFFit.importance_posterior``
        (:mod:`victor_amd.importance`), ``predictive=True`` included: every mock's band and DIC from the G shared theory
        vectors, and ``tail=True``: every mock's Pareto shape and smoothed estimates (``ip.tail``).  Refused with
        ``paired_model=True``: a point then has one theory vector per realisation.

        ``q`` a :class:`victor_amd.importance.ProposalSet` of ``len(self)`` proposals - every mock's own best fit and Laplace
        covariance, ``ProposalSet.from_fits(bf, lap)`` - runs every mock over ``n`` points of its OWN instead (rule 8 of
        :mod:`victor_amd.importance`): ``n`` x R theory evaluations in pairs mode, for the mocks a shared proposal misses
        (``LOW_ESS``, ``HIGH_K``) and for ``paired_model=True``, which this route serves; ``predictive=True``, ``sample`` and
        ``ln_proposal`` are refused with it."""
        from .importance import importance_posterior
        predictive = kwargs.pop("predictive", None)             # (a keyword of its own, not a model or fit option)
        tail = kwargs.pop("tail", None)                         # (likewise)
        return importance_posterior(self.fit, params, q, n, seed, fixed, prior, bins, ranges, pairs, chunk, min_ess, device, evaluate,
                                    sample, ln_proposal, kwargs, realisations=self, predictive=predictive, tail=tail)

    def nested_sampling(self, params, n_live=256, batch=32, steps=16, scale=None, seed=0, fixed=None, tol=1e-3, max_iter=None, n_iter=None,
                        keep_dead=True, device=True, evaluate=None, prior=None, prior_norm="auto", **kwargs):
        """Nested sampling of EVERY realisation, all of them in lock step (R = ``len(self)`` problems, one evidence and one
        posterior sample per mock): on the GPU (``device=True``) or by the NumPy loop over :meth:`log_likelihood_pairs` that
        defines the runs (``device=False``).  ``paired_model=True`` is honoured: a row is evaluated with the model of its own
        mock.  Arguments and result as ``CCFFit.nested_sampling`` (:mod:`victor_amd.nested`)."""
        from .nested import nested_sampling
        return nested_sampling(self.fit, params, n_live, batch, steps, scale, seed, fixed, tol, max_iter, n_iter, keep_dead, device,
                               evaluate, kwargs, realisations=self, prior=prior, prior_norm=prior_norm)

    def log_likelihood_pairs(self, params, which, **kwargs):
        """(lnL, chi2), each ``(n_points,)``: point p against realisation ``numbers[which[p]]`` only - the form an ensemble of
        independent per-mock chains needs.  The same bits as the matching entries of :meth:`log_likelihood`."""
        return self._eval(params, kwargs, which)
