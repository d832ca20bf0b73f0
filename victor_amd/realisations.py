"""One model against every simulation realisation of a data file: mock validation in one call per parameter batch.

The reference fits one measured CCF at a time; a data file may hold a stack of realisations (mocks), of which
``redshift_space_ccf.simulation_number`` picks one when the fit is built (reference: ``ccf_fit.py:59-61,93-100``;
``utils.convert_hans_quijote_to_hdf5`` writes such stacks, ``utils.py:161-242``).  :class:`Realisations` reads the whole stack
(or a subset) from the same file and keys the fit was built from and evaluates parameter points against all of them: each point's
theory vector is computed once on the GPU and compared with every realisation's data vector there (``vk_eval_realisations``,
``include/victor_hip.h``).  Model, covariance, options and engine are the fit's.

Value contract: entry ``[p, m]`` equals ``CCFFit(model, data with simulation_number=numbers[m]).log_likelihood(point p)`` to
rounding (the chi-square is summed in another order), ``(-inf, inf)`` exactly where that call returns it.
"""

import weakref

import numpy as np

from . import _native as N
from . import utils
from .engine import data_table
from .utils import InputError


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

    def __init__(self, fit, simulation_numbers=None):
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

    def __len__(self):
        return len(self.numbers)

    # ------------------------------------------------------------------ device plumbing -------
    def _plan(self, kwargs):
        fit = self.fit
        model = fit._merged(kwargs)
        fit._check_supported(model)
        fit_options = fit._merged_fit(kwargs)
        eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])
        self._upload(eng)
        return model, fit_options, eng, eng.make_opts(model, fit_options)

    def _upload(self, eng):
        """Make this object's realisations the ones set on ``eng`` (uploaded only when another object's, or none, are there)."""
        owner = getattr(eng, "_real_owner", None)
        if owner is None or owner() is not self:
            eng.set_realisations(self.blocks)
            eng._real_owner = weakref.ref(self)

    def _eval(self, params, kwargs, which=None):
        model, fit_options, eng, opts = self._plan(kwargs)
        rows, which = check_which(self.fit._fit_rows(params, model), which, len(self))
        if fit_options["beta_interpolation"] == "likelihood" and not self.fit.fixed_data:
            return self._likelihood_interp(eng, opts, rows, which)
        return eng.eval_realisations(opts, rows, len(self), which)

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
        lnl, chi2 = eng.eval_realisations(opts, both, len(self), None if which is None else np.concatenate([which, which]))
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

    def log_likelihood_pairs(self, params, which, **kwargs):
        """(lnL, chi2), each ``(n_points,)``: point p against realisation ``numbers[which[p]]`` only - the form an ensemble of
        independent per-mock chains needs.  The same bits as the matching entries of :meth:`log_likelihood`."""
        return self._eval(params, kwargs, which)
