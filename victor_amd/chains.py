"""Metropolis chains and stretch-move ensembles of the data vector and of every realisation, stepped on the GPU: ``CCFFit.sample_chains`` and
``Realisations.sample_chains``; of a joint fit, ``JointFit.sample_chains`` and ``JointRealisations.sample_chains`` (one parameter
row for all blocks: ``fit`` is the ``JointFit`` below, the definition route runs over its ``log_likelihood_batch`` /
``JointRealisations.log_likelihood_pairs``, the device route through ``vk_chain_create_joint``; with ``"name@q"`` parameters, :mod:`victor_amd.joint`, a row per block and
``vk_chain_create_joint_blocks``).

The reference is sampled by cobaya, one likelihood per call and one data vector at a time (reference:
``victor/likelihoods/CCFLikelihood.py:32``).  Mock validation wants the posterior of EVERY mock beside its best fit: here
C = R x W independent random-walk Metropolis chains - R problems (the fit's data vector: R = 1; or the R realisations of a
:class:`victor_amd.realisations.Realisations`), W chains per problem, chain c belonging to problem c // W - advance in lock step.
Prior box, proposal widths and start distribution come from the cobaya ``params`` block (``parse_cobaya_params``), as
:class:`victor_amd.sampler.EnsembleMetropolis` and ``best_fit`` read it.

**A Python loop is the definition and the device loop reproduces it.**  Random numbers are drawn on the host with the generator
and the block protocol of ``EnsembleMetropolis`` (blocks of 64 steps: ``dz = width * rng.standard_normal((64, C, d))``, then
``logu = np.log(rng.random((64, C)))``; the start as ``initialise()`` draws it), so for the same seed and C the numbers are those
an ``EnsembleMetropolis`` of C walkers consumes.  One step of one chain: ``prop = x + dz``; a proposal outside the box is
evaluated at the chain's current position, discarded, and reads -inf (every launch has exactly C rows); accept when
``logu < lnl_prop - lnl`` with IEEE semantics as NumPy applies them (a NaN difference rejects; a NaN lnL is stored as -inf).

``device=False`` runs that loop in NumPy, all C rows per step through ``Realisations.log_likelihood_pairs`` (or
``CCFFit.log_likelihood_batch``, or an ``evaluate`` callable: no GPU needed).  ``device=True`` hands blocks of 64 steps to
``vk_chain_begin`` (``include/victor_hip.h``): per step the same evaluation of the same C rows and a small
step kernel, no host round trip inside a block, the next block's numbers drawn while the block runs.  Both routes launch the same
rows in the same order: with epsilon fixed the rows are the same bytes and so are the log-likelihoods.  **When epsilon is sampled**
the device forms the Alcock-Paczynski factors of a row with its own ``pow``, the host with libm's: the log-likelihoods then agree
to rounding, not bit for bit, and a decision ``logu < lnl_prop - lnl`` taken within that margin could fall the other way (as
documented for ``speculate`` in :mod:`victor_amd.sampler`).

"Kept" steps - step index >= ``burn`` and ``(step - burn) % thin == 0``, counted over the whole life of the object - enter the
history (``keep_chain``) and the per-chain moment sums about the chain's start (the pivot), which are accumulated where the chain
runs; ``mean`` and ``cov`` pool the W chains of a problem from those sums, so they cost O(C d^2) host memory whatever the length.

**``move="stretch"``** replaces the random-walk step by the affine-invariant stretch move of Goodman & Weare (2010) in the
two-half parallel form of :class:`victor_amd.sampler.EnsembleStretch`, which needs no proposal widths: the W chains of a problem
are the W walkers of ONE ensemble (W even, at least 2 (d + 1)), walker c = r W + w; half 0 holds the walkers w < W / 2, half 1
the rest.  One step is one SWEEP: half 0 moves against partners drawn from half 1 of the same problem, then half 1 against the
updated half 0; ``n_steps``, ``burn``, ``thin``, ``n_kept``, the history and ``acceptance`` count sweeps, and a kept sweep takes
all W walkers as they stand after its second half.  Per half-step the generator calls are those of ``EnsembleStretch.step`` at
R W / 2 numbers each - ``z = ((a - 1) rng.random() + 1)**2 / a``, the partners ``rng.integers(0, W / 2)``, ``logu =
log(rng.random())`` - drawn ahead in blocks of 64 sweeps (those three calls 128 times), so with R = 1 the definition route is
the chain of an ``EnsembleStretch`` of the same seed bit for bit.  A half-step of one walker: ``prop = partner + z * (x -
partner)`` (a product and a sum, each rounded: the device forbids the fused multiply-add there); outside the box as above (every
launch has exactly R W / 2 rows, row i of problem i // (W / 2), member i % (W / 2) of the moving half); accept when ``logu <
lz + lnl_prop - lnl``, left to right, with ``lz = (d - 1) * log(z)`` formed on the host.  ``device=True`` hands blocks of 64
sweeps to ``vk_chain_begin_stretch``: per half-step a kernel that forms the proposals and their rows, the evaluation of those
rows, and a kernel that decides - three launches in stream order, because the proposals of a half read what the decisions of
the other half have just written.

**``prior=``** multiplies a Gaussian prior (:class:`victor_amd.priors.GaussianPrior`, or a list of them) onto the box: what is
sampled is the Gaussian truncated by the box (no normalisation constant: it changes no decision).  The Metropolis decision becomes
``logu < (lnl_prop + lp_prop) - (lnl + lp)``, the stretch decision ``logu < (lz + (lnl_prop + lp_prop)) - (lnl + lp)``, with
``lp_prop`` the prior at the proposal and ``lp`` the prior recomputed at the current position, in the arithmetic order of
:meth:`victor_amd.priors.ResolvedPrior.lnprior`; outside the box ``lnl_prop = -inf`` as before (-inf plus a finite prior is
-inf).  The device evaluates the same statement (``vk_chain_set_prior``, ``victor_amd/csrc/vk_prior.h``) bit for bit.  The
state and ``lnl_chain`` keep the log-LIKELIHOOD; ``lnprior_chain`` is the prior of the kept positions, computed on the host.

**``marginals=``** counts every kept position in per-problem histograms (:mod:`victor_amd.marginals`: one of every sampled
parameter, and of chosen pairs), where the moment sums are accumulated and with the same "kept": on the device route by the step
kernels (``vk_chain_set_marginals``; integer atomic increments), on the definition route by the NumPy statement of the same binning
rule - so the two routes give equal counts wherever they give equal positions, with or without a history.  ``Chains.marginals``
reads medians and equal-tailed intervals from them.

**``autocorr=``** keeps, per problem and sampled parameter, the series of the per-step sum over the problem's W chains (one value
per kept step or kept sweep) and its lagged products up to ``max_lag`` (:mod:`victor_amd.autocorr`): on the device route by a
small kernel behind the step kernel of every kept step (``vk_chain_set_autocorr``), on the definition route by the NumPy statement
of the same update - every rounding fixed, so the two routes give the same bytes wherever they give the same positions, with or
without a history.  ``Chains.autocorr`` reads integrated autocorrelation times (Sokal's window) and effective sample sizes from it:
the convergence diagnostic of a run without a history, and of the stretch move, whose ``rhat`` is None by design.

**``temper=``** runs K copies of every problem at inverse temperatures from 1 down to 0 and lets neighbouring temperatures
exchange states (replica exchange; :mod:`victor_amd.tempering` states the step, the energy sums and the swap, the device route
reproduces them bit for bit through ``vk_chain_begin_tempered``): chain ``c = (r K + k) W + w`` is problem r, rung k, walker w, so
everything above that groups W chains sees every (r, k) as a problem, and the public fields of ``Chains`` are the cold rung k = 0.
``Chains.tempering`` carries every rung's state and the evidence by thermodynamic integration.  Metropolis move only.

**``predictive=``** keeps, per chain, the theory vector at its current position - taken from the launch that decided a step
whenever the chain's accept count moved - and sums it per problem at every kept step (kept sweep), with chi2 and lnL beside it
(:mod:`victor_amd.predictive` states the rules): on the device route by two small kernels behind the step kernel
(``vk_chain_set_predictive``), on the definition route by the NumPy statement over ``fit.theory_vector_batch``.  The sums hold
products the device may contract, so the routes agree to rounding.  ``Chains.predictive`` reads the posterior mean and scatter of
the model vector (the band drawn through the data's multipoles), the mean chi-square and the deviance information criterion from
them, with or without a history.  Single fits only, and not with ``temper=``.
"""

import ctypes as C

import numpy as np

from . import _native as N
from .fitting import _Sampled
from .sampler import EnsembleMetropolis, gelman_rubin
from .utils import InputError

BLOCK = EnsembleMetropolis.BLOCK
MAX_CHAINS = 65536


def pooled_moments(n_kept, pivot, sum1, sum2):
    """(mean (R, d), cov (R, d, d)) of each problem's kept steps, pooled over its W chains, from the per-chain sums about the
    chains' pivots: ``n_kept`` (R, W), ``pivot`` and ``sum1`` (R, W, d), ``sum2`` (R, W, d, d).  With delta_w = pivot_w - mean,

        mean = sum_w (n_w pivot_w + S1_w) / n,      (n - 1) cov = sum_w (S2_w + S1_w delta_w^T + delta_w S1_w^T + n_w delta_w delta_w^T)

    formed in extended precision, so that what the result carries is the rounding of the sums it was given (amplified by
    1 + |mean - pivot|^2 / var where a pivot lies far from the mean: tests/test_chains.py).  NaN where a problem kept fewer
    than one (mean) or two (cov) steps."""
    ld = np.longdouble
    nw = np.asarray(n_kept, dtype=ld)
    p, s1, s2 = np.asarray(pivot, dtype=ld), np.asarray(sum1, dtype=ld), np.asarray(sum2, dtype=ld)
    n = nw.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (nw[:, :, None] * p + s1).sum(axis=1) / n[:, None]
        delta = p - mean[:, None, :]
        cross = s1[:, :, :, None] * delta[:, :, None, :]
        m2 = s2 + cross + np.swapaxes(cross, 2, 3) + nw[:, :, None, None] * delta[:, :, :, None] * delta[:, :, None, :]
        cov = m2.sum(axis=1) / (n - 1)[:, None, None]
    mean, cov = mean.astype(float), cov.astype(float)
    mean[np.asarray(n < 1)] = np.nan
    cov[np.asarray(n < 2)] = np.nan
    return mean, cov


class Chains:
    """C = R x W chains and what they have produced so far.

    ``names``; ``x`` (R, W, d), ``lnl``, ``chi2`` (R, W): the final state; ``chain`` (n_kept, R, W, d), ``lnl_chain``,
    ``chi2_chain`` (n_kept, R, W): the kept steps (None with ``keep_chain=False``); ``mean`` (R, d), ``cov`` (R, d, d): pooled
    over a problem's W chains and its kept steps (ddof = 1); ``n_accept`` (R, W), ``acceptance`` (R,); ``rhat`` (R, d):
    :func:`victor_amd.sampler.gelman_rubin` of each problem's history (None without one, for W == 1 or fewer than two kept
    steps); ``pivot`` (R, W, d), ``n_kept``, ``sum1`` (R, W, d), ``sum2`` (R, W, d, d): the per-chain moment sums as the route that
    ran the chains returns them; ``n_steps``: steps taken.  :meth:`extend` continues the same chains.

    ``move``: "metropolis" or "stretch", the move that ran.  Under "stretch" the W chains of a problem are the walkers of one
    ensemble, steps are sweeps, ``stretch_a`` is the move's scale, and ``rhat`` is None: the walkers of an ensemble move along
    lines through each other, they are not independent chains, and a between- over within-chain variance of them means nothing.

    Diagnostics of the definition route only (None on the device route): ``decision_margin``, the smallest
    ``|lnl_prop - lnl - logu|`` (stretch move: ``|lz + lnl_prop - lnl - logu|``) over the decisions taken inside the box with a
    finite difference (how far the closest decision was from falling the other way), and ``n_outside`` (R, W), the proposals that left the box.

    Under a Gaussian prior (``prior=``) ``lnl`` and ``lnl_chain`` stay the log-LIKELIHOOD; ``lnprior_chain`` (n_kept, R, W) is the
    prior of the kept positions, computed on the host (zeros without a prior, None with ``keep_chain=False``), and
    ``decision_margin`` includes the prior terms.  :meth:`extend` keeps the prior.

    ``marginals``: a :class:`victor_amd.marginals.Marginals` of the kept positions' histograms (None without ``marginals=``),
    rebuilt after every :meth:`extend`, which keeps counting.

    ``autocorr``: a :class:`victor_amd.autocorr.Autocorr` of the ensemble series - ``tau``, ``window``, ``ess``, ``reached`` (R, d),
    ``acf`` (R, d, max_lag) - (None without ``autocorr=``), rebuilt after every :meth:`extend`, which keeps accumulating.

    ``tempering``: a :class:`victor_amd.tempering.Tempering` (None without ``temper=``) - the ladder, every rung's state and
    history, the rungs' mean and variance of lnL, swap acceptances and ``ln_evidence`` -, rebuilt after every :meth:`extend`, which
    continues the ladder (the swap-event count and the swap levels' stream run over the chains' whole life).  Every (R, W, ...)
    field above is then the cold rung's.

    ``predictive``: a :class:`victor_amd.predictive.Predictive` (None without ``predictive=``) - the posterior mean and scatter of
    the theory vector and of its multipoles, the mean and variance of chi2 and lnL, ``p_d``, ``p_v`` and ``dic`` -, rebuilt after
    every :meth:`extend`, which keeps accumulating."""

    def __init__(self, names, specs, fixed, R, W, rng, width, burn, thin, keep_chain, evaluator, device_handle, move="metropolis",
                 stretch_a=2.0, prior=None, binning=None, lags=None, temper=None, predictive=None):
        self.names = list(names)
        self._pred = predictive                           # a victor_amd.predictive.PredictiveState, or None
        self._theory = self._at_mean = self._poles = None    # x (m, d) -> theory vectors (m, N); x (m, d), problems (m,) -> (lnL, chi2); (poles, n_s)
        self.predictive = None
        self._series = self._lag_c = self.autocorr = None
        self._temper = temper                             # a victor_amd.tempering.TemperState, or None
        self._K = temper.K if temper is not None else 1
        self._RK = R * self._K                            # the "problems" of the group = W features: every (problem, rung)
        self.tempering = None
        if lags is not None:                              # (max_lag, c) of victor_amd.autocorr.resolve_autocorr
            from .autocorr import SeriesState
            self._series, self._lag_c = SeriesState(self._RK, len(self.names), W, lags[0]), lags[1]
        self._prior = prior                               # a victor_amd.priors.ResolvedPrior, or None
        self._binning = binning                           # a victor_amd.marginals.Binning, or None
        self._h1, self._h2 = binning.zeros(self._RK) if binning is not None else (None, None)
        self.marginals = None
        self.move, self.stretch_a = move, float(stretch_a)
        self._specs, self.fixed = specs, fixed
        self.R, self.W = R, W
        self._rng, self._width = rng, width
        if temper is not None:                            # (C, d): the widths times the rung's scale (a scale of 1 changes no bit)
            self._width = width[None, :] * temper.scale[:, None]
        self._factor = None                               # (C, d, d) proposal factors of a Laplace proposal, or None: the widths
        self.burn, self.thin, self.keep_chain = burn, thin, keep_chain
        self._evaluate = evaluator
        self._dev = device_handle
        self._refresh = self._fit = None
        self._lo = np.array([s.lo for s in specs])
        self._hi = np.array([s.hi for s in specs])
        self._block = None
        self._at = BLOCK
        self.n_steps = 0
        self._hist = ([], [], [])
        self.chain = self.lnl_chain = self.chi2_chain = self.lnprior_chain = None
        self.decision_margin = self.n_outside = None

    # ------------------------------------------------------------------ random numbers: the blocks of EnsembleMetropolis ---
    def _draw_block(self):
        if self.move == "stretch":
            return self._draw_block_stretch()
        C_, d = self._RK * self.W, len(self.names)
        if self._factor is None:
            dz = self._width * self._rng.standard_normal((BLOCK, C_, d))
        else:                                             # correlated proposals: chain c draws dz = F_(c // W) normal(d)
            dz = np.einsum("cjk,tck->tcj", self._factor, self._rng.standard_normal((BLOCK, C_, d)))
        logu = np.log(self._rng.random((BLOCK, C_)))
        if self._temper is not None:                      # the swap levels: a generator of their own, block by block
            return dz, logu, self._temper.draw_logs()
        return dz, logu

    def _draw_block_stretch(self):
        """64 sweeps of two half-steps each, every half-step with the three generator calls of ``EnsembleStretch.step`` at
        R * W / 2 numbers: (z, lz = (d - 1) log z, logu, partner), each [64, 2, R * W / 2]."""
        half, a, d = self.W // 2, self.stretch_a, len(self.names)
        M = self.R * half
        z, logu, partner = np.empty((BLOCK, 2, M)), np.empty((BLOCK, 2, M)), np.empty((BLOCK, 2, M), dtype=np.int32)
        for t in range(BLOCK):
            for h in range(2):
                z[t, h] = ((a - 1.0) * self._rng.random(M) + 1.0) ** 2 / a
                partner[t, h] = self._rng.integers(0, half, size=M)
                logu[t, h] = np.log(self._rng.random(M))
        return z, (d - 1) * np.log(z), logu, partner

    def _piece(self, remaining, ahead=None):
        """The next piece of the current block (drawing a new one when it is used up; ``ahead``: one drawn in advance):
        (dz [k, C, d], logu [k, C]) - under the stretch move (z, lz, logu, partner), each [k, 2, C / 2] -, k <= remaining."""
        if self._at >= BLOCK:
            self._block = ahead if ahead is not None else self._draw_block()
            self._at = 0
        k = min(BLOCK - self._at, remaining)
        t = self._at
        self._at = t + k
        return tuple(a[t:t + k] for a in self._block)

    def _kept(self, step):
        return step >= self.burn and (step - self.burn) % self.thin == 0

    # ------------------------------------------------------------------ the definition -----------------------------------
    def _start_host(self, x0):
        C_, d = x0.shape
        self._x = x0.copy()
        lnl, chi2 = self._evaluate(self._x)
        self._lnl = np.where(np.isnan(lnl), -np.inf, lnl)
        self._chi2 = np.array(chi2, dtype=float)
        self._pivot = x0.copy()
        self._n_accept = np.zeros(C_, dtype=np.int64)
        self._n_kept = np.zeros(C_, dtype=np.int64)
        self._sum1 = np.zeros((C_, d))
        self._sum2 = np.zeros((C_, d, d))
        self._n_outside = np.zeros(C_, dtype=np.int64)
        self.decision_margin = np.inf
        if self._pred is not None:
            self._pred.start(self._theory(self._x), self._n_accept, self._chi2, self._lnl)

    def _hold(self, chains, rows):
        """Behind a decision: the chains (of ``chains``, which the launch's ``rows`` serve) whose accept count moved take the
        theory vector of their row (:mod:`victor_amd.predictive`)."""
        q = self._pred
        take = q.changed(chains, self._n_accept)
        if take.any():
            q.hold(chains[take], self._theory(rows[take]), self._n_accept)

    def _account(self, x, lnl, chi2):
        """The end of a step (a sweep): a kept one enters the moment sums and the history."""
        if self._kept(self.n_steps):
            dx = x - self._pivot
            self._sum1 += dx
            self._sum2 += dx[:, :, None] * dx[:, None, :]
            self._n_kept += 1
            if self._binning is not None:
                self._binning.add(self._h1, self._h2, x, self.W)
            if self._series is not None:
                self._series.add(x)
            if self._pred is not None:
                self._pred.add(chi2, lnl)
            if self.keep_chain:
                for h, a in zip(self._hist, (x, lnl, chi2)):
                    h.append(a.copy())
        self.n_steps += 1

    def _run_host_stretch(self, n_steps):
        """Sweeps of the stretch move: half 0 of every problem against its half 1, then half 1 against the updated half 0; the
        arithmetic of ``EnsembleStretch.step``, R problems side by side, R * W / 2 rows per evaluation."""
        lo, hi = self._lo, self._hi
        x, lnl, chi2 = self._x, self._lnl, self._chi2
        R, W, half = self.R, self.W, self.W // 2
        first = (np.arange(R)[:, None] * W + np.arange(half)[None, :]).ravel()            # half 0, problem by problem
        halves = (first, first + half)
        start = (np.repeat(np.arange(R) * W, half), np.repeat(np.arange(R) * W + half, half))
        which = np.repeat(np.arange(R, dtype=np.int32), half)
        done = 0
        while done < n_steps:
            z, lz, logu, pick = self._piece(n_steps - done)
            for t in range(len(z)):
                for h in range(2):
                    mv = halves[h]
                    partner = x[start[1 - h] + pick[t, h]]
                    xm, lnl_m = x[mv], lnl[mv]
                    prop = partner + z[t, h][:, None] * (xm - partner)
                    inside = ((prop >= lo) & (prop <= hi)).all(axis=1)
                    rows = np.where(inside[:, None], prop, xm)           # outside: the current position, result discarded
                    lnl_p, chi2_p = self._evaluate(rows, which)
                    lnl_p = np.where(inside, lnl_p, -np.inf)
                    with np.errstate(invalid="ignore"):
                        if self._prior is None:
                            gain = lz[t, h] + lnl_p - lnl_m
                        else:                                            # (lz + (lnL' + lp')) - (lnL + lp)
                            gain = (lz[t, h] + (lnl_p + self._prior.lnprior(prop))) - (lnl_m + self._prior.lnprior(xm))
                        accept = logu[t, h] < gain                       # NaN: False
                        margin = np.abs(gain - logu[t, h])
                    margin = margin[np.isfinite(margin)]
                    if margin.size:
                        self.decision_margin = min(self.decision_margin, float(margin.min()))
                    self._n_outside[mv] += ~inside
                    won = mv[accept]
                    x[won] = prop[accept]
                    lnl[won] = lnl_p[accept]
                    chi2[won] = chi2_p[accept]
                    self._n_accept[won] += 1
                    if self._pred is not None:
                        self._hold(mv, rows)
                self._account(x, lnl, chi2)                              # "kept" is decided after the second half, for all W
            done += len(z)

    def _run_host(self, n_steps):
        """Metropolis steps.  Under replica exchange (:mod:`victor_amd.tempering`) the decision is the tempered one at each chain's
        beta, a kept step enters the energy sums, and a swap event may follow the step."""
        if self.move == "stretch":
            return self._run_host_stretch(n_steps)
        from .tempering import gain as tempered_gain
        q, prior = self._temper, self._prior
        lo, hi = self._lo, self._hi
        x, lnl, chi2 = self._x, self._lnl, self._chi2
        done = 0
        while done < n_steps:
            dz, logu, *logs = self._piece(n_steps - done)            # (logs: the swap levels of a tempered block)
            for t in range(len(dz)):
                prop = x + dz[t]
                inside = ((prop >= lo) & (prop <= hi)).all(axis=1)
                rows = np.where(inside[:, None], prop, x)            # outside: the current position, result discarded
                lnl_p, chi2_p = self._evaluate(rows)
                lnl_p = np.where(inside, lnl_p, -np.inf)
                with np.errstate(invalid="ignore"):
                    lp = () if prior is None else (prior.lnprior(prop), prior.lnprior(x))
                    if q is not None:                                # (beta lnL' + lp') - (beta lnL + lp)
                        gain = tempered_gain(q.beta, lnl_p, lnl, *lp)
                    elif prior is None:
                        gain = lnl_p - lnl
                    else:                                            # (lnL' + lp') - (lnL + lp)
                        gain = (lnl_p + lp[0]) - (lnl + lp[1])
                    # NaN (both -inf, 0 * inf, a NaN lnL): False; outside the box the gain is -inf or NaN, `inside` changes nothing
                    accept = inside & (logu[t] < gain)
                    margin = np.abs(gain - logu[t])
                margin = margin[np.isfinite(margin)]
                if margin.size:
                    self.decision_margin = min(self.decision_margin, float(margin.min()))
                self._n_outside += ~inside
                x[accept] = prop[accept]
                lnl[accept] = lnl_p[accept]
                chi2[accept] = chi2_p[accept]
                self._n_accept += accept
                if self._pred is not None:
                    self._hold(np.arange(len(x)), rows)
                step = self.n_steps
                if q is not None and self._kept(step):
                    q.energy_add(lnl)
                self._account(x, lnl, chi2)                          # (before the swap: a kept step is what the decision left)
                if q is not None:
                    q.swap(step, x, lnl, chi2, logs[0][t])
            done += len(dz)

    # ------------------------------------------------------------------ the device route ---------------------------------
    def _check(self, rc, what):
        if rc != 0:
            lib, h = self._dev
            msg = (lib.vk_chain_last_error(h) or b"").decode() or f"{what} failed ({rc})"
            raise (InputError if rc == -1 else N.NativeError)(msg)

    def _run_device(self, n_steps):
        lib, h = self._dev
        C_, d = self._RK * self.W, len(self.names)
        done = 0
        ahead = None
        while done < n_steps:
            piece = [np.ascontiguousarray(a) for a in self._piece(n_steps - done, ahead)]
            ahead = None
            k = len(piece[0])
            n_kept = C.c_int32(0)
            tail = (self.n_steps, self.burn, self.thin, 1 if self.keep_chain else 0, C.byref(n_kept))
            if self.move == "stretch":
                z, lz, logu, partner = piece
                self._check(lib.vk_chain_begin_stretch(h, k, self.W, N.as_dp(z), N.as_dp(lz), N.as_dp(logu),
                                                       partner.ctypes.data_as(C.POINTER(C.c_int32)), *tail), "vk_chain_begin_stretch")
            elif self._temper is not None:
                dz, logu, logs = piece
                self._check(lib.vk_chain_begin_tempered(h, k, N.as_dp(dz), N.as_dp(logu), N.as_dp(logs),
                                                        self._temper.ladder.swap_every, *tail), "vk_chain_begin_tempered")
            else:
                dz, logu = piece
                self._check(lib.vk_chain_begin(h, k, N.as_dp(dz), N.as_dp(logu), *tail), "vk_chain_begin")
            try:
                if self._at >= BLOCK and done + k < n_steps:         # the next block's numbers, drawn while this one runs
                    ahead = self._draw_block()
            finally:
                m = n_kept.value
                hx, hl, hc = np.empty((m, C_, d)), np.empty((m, C_)), np.empty((m, C_))
                self._check(lib.vk_chain_finish(h, N.as_dp(hx), N.as_dp(hl), N.as_dp(hc)), "vk_chain_finish")
            if m:
                for hist, a in zip(self._hist, (hx, hl, hc)):
                    hist.append(a)
            self.n_steps += k
            done += k

    def _read_device(self):
        lib, h = self._dev
        C_, d = self._RK * self.W, len(self.names)
        dp = N.as_dp

        def i64(a):
            return a.ctypes.data_as(C.POINTER(C.c_int64))
        self._x, self._lnl, self._chi2 = np.empty((C_, d)), np.empty(C_), np.empty(C_)
        self._n_accept, self._n_kept = np.empty(C_, dtype=np.int64), np.empty(C_, dtype=np.int64)
        self._pivot, self._sum1, self._sum2 = np.empty((C_, d)), np.empty((C_, d)), np.empty((C_, d, d))
        self._check(lib.vk_chain_state(h, dp(self._x), dp(self._lnl), dp(self._chi2), i64(self._n_accept), None, i64(self._n_kept),
                                       dp(self._pivot), dp(self._sum1), dp(self._sum2)), "vk_chain_state")
        if self._binning is not None:
            self._check(lib.vk_chain_marginals(h, i64(self._h1), i64(self._h2)), "vk_chain_marginals")
        if self._series is not None:
            q, n = self._series, C.c_int64(0)
            self._check(lib.vk_chain_autocorr(h, dp(q.pivot), dp(q.total), dp(q.head), dp(q.ring), dp(q.acc), C.byref(n)), "vk_chain_autocorr")
            q.n = int(n.value)
        if self._pred is not None:
            q = self._pred
            self._check(lib.vk_chain_predictive(h, dp(q.pivot_t), dp(q.sum_t), dp(q.sum_tt), dp(q.deviance), i64(q.n), i64(q.n_skipped),
                                                dp(q.held)), "vk_chain_predictive")
        if self._temper is not None:
            q = self._temper
            self._check(lib.vk_chain_tempering(h, dp(q.pivot_e), dp(q.e1), dp(q.e2), i64(q.n_e), i64(q.n_swap_try), i64(q.n_swap_acc)),
                        "vk_chain_tempering")

    def _attach_device(self, set_prior, x0):
        """Hand the handle what the chains were asked for - the prior (``set_prior``: the call that does it), the binning, the
        series' shape, the ladder, the predictive sums: the W chains of a problem pool - and start the chains at ``x0``.  (The
        handle is this object's from here on: a refusal destroys it with the object.)"""
        lib, h = self._dev
        if self._prior is not None:
            set_prior("vk_chain_set_prior", lib, h, self._prior)
        if self._binning is not None:
            q = self._binning
            pairs = q.pairs.ctypes.data_as(C.POINTER(C.c_int32)) if len(q.pairs) else None
            self._check(lib.vk_chain_set_marginals(h, self.W, q.n_bins, N.as_dp(q.a), N.as_dp(q.b), len(q.pairs), pairs, q.n_bins2),
                        "vk_chain_set_marginals")
        if self._series is not None:
            self._check(lib.vk_chain_set_autocorr(h, self.W, self._series.L), "vk_chain_set_autocorr")
        if self._temper is not None:
            self._check(lib.vk_chain_set_tempering(h, self._K, self.W, N.as_dp(self._temper.ladder.betas)), "vk_chain_set_tempering")
        if self._pred is not None:
            self._check(lib.vk_chain_set_predictive(h, self.W), "vk_chain_set_predictive")
        self._check(lib.vk_chain_start(h, N.as_dp(N.f64(x0))), "vk_chain_start")

    def __del__(self):
        dev = getattr(self, "_dev", None)
        if dev:
            try:
                dev[0].vk_chain_destroy(dev[1])
            except Exception:
                pass
            self._dev = None

    # ------------------------------------------------------------------ public ------------------------------------------
    def extend(self, n_steps):
        """Continue the same chains for ``n_steps`` more steps: the same generator, the same blocks of random numbers, the same
        burn / thin pattern - the chains of one longer call."""
        n_steps = int(n_steps)
        if n_steps < 0:
            raise InputError("sample_chains: n_steps must be >= 0")
        if self._dev and self._refresh is not None:
            self._refresh()                               # another object's realisations may have been set on the engine since
        if n_steps:
            (self._run_device if self._dev else self._run_host)(n_steps)
        if self._dev:
            self._read_device()
        self._publish()
        return self

    def _publish(self):
        R, W, d, K = self.R, self.W, len(self.names), self._K
        P = self._RK                                         # (problem, rung) pairs; the public fields are the cold rung's
        cold = slice(None, None, K)
        self.x = self._x.reshape(P, W, d)[cold].copy()
        self.lnl, self.chi2 = self._lnl.reshape(P, W)[cold].copy(), self._chi2.reshape(P, W)[cold].copy()
        self.n_accept = self._n_accept.reshape(P, W)[cold].copy()
        self.acceptance = self.n_accept.sum(axis=1) / max(1, self.n_steps * W)
        self.pivot, self.sum1 = self._pivot.reshape(P, W, d)[cold].copy(), self._sum1.reshape(P, W, d)[cold].copy()
        self.sum2 = self._sum2.reshape(P, W, d, d)[cold].copy()
        per_chain = self._n_kept.reshape(P, W)[cold]
        self.n_kept = int(per_chain[0, 0])
        self.mean, self.cov = pooled_moments(per_chain, self.pivot, self.sum1, self.sum2)
        if not self._dev:
            self.n_outside = self._n_outside.reshape(P, W)[cold].copy()
        if self._binning is not None:
            from .marginals import Marginals
            self.marginals = Marginals(self._binning, self._h1[cold], self._h2[cold], per_chain.sum(axis=1))
        if self._series is not None:
            from .autocorr import Autocorr
            self.autocorr = Autocorr(self.names, W, self._series.n, self._lag_c, {k: v[cold] for k, v in self._series.arrays().items()})
        if self._pred is not None:
            from .predictive import Predictive
            lnl_at, chi2_at = np.full(R, np.nan), np.full(R, np.nan)
            has = np.flatnonzero(np.all(np.isfinite(self.mean), axis=1))
            if len(has):                                     # one pairs evaluation at the pooled means of the problems that have one
                lnl_at[has], chi2_at[has] = self._at_mean(self.mean[has], has.astype(np.int32))
            self.predictive = Predictive(self._pred.arrays(), *self._poles, chi2_at_mean=chi2_at, lnl_at_mean=lnl_at)
        self.rhat = None
        hist = None
        if self.keep_chain:
            hx, hl, hc = self._hist
            if len(hx) > 1:                                  # one array per block -> one array
                self._hist = ([np.concatenate([a.reshape(-1, P * W, d) for a in hx])],
                              [np.concatenate([a.reshape(-1, P * W) for a in hl])], [np.concatenate([a.reshape(-1, P * W) for a in hc])])
                hx, hl, hc = self._hist
            hist = (hx[0].reshape(-1, P, W, d) if hx else np.empty((0, P, W, d)), hl[0].reshape(-1, P, W) if hl else np.empty((0, P, W)),
                    hc[0].reshape(-1, P, W) if hc else np.empty((0, P, W)))
            self.chain, self.lnl_chain, self.chi2_chain = (a[:, cold] for a in hist) if K > 1 else hist
            self.lnprior_chain = np.zeros(self.chain.shape[:-1]) if self._prior is None else self._prior.lnprior(self.chain)
            if W > 1 and len(self.chain) > 1 and self.move != "stretch":   # (the walkers of an ensemble are not independent chains)
                with np.errstate(invalid="ignore", divide="ignore"):
                    self.rhat = np.stack([gelman_rubin(self.chain[:, r]) for r in range(R)])
        if self._temper is not None:
            from .tempering import Tempering
            self.tempering = Tempering(self._temper, self._n_accept, self.n_steps, self._n_kept, self._x, self._lnl, self._chi2, hist)


def _draw_start(rng, loc, scale, lo, hi, what):
    """One start as ``EnsembleMetropolis.initialise`` draws it: redrawn until inside the box."""
    for _ in range(1000):
        cand = loc + scale * rng.standard_normal(len(loc))
        if np.all((cand >= lo) & (cand <= hi)):
            return cand
    raise InputError(f"sample_chains: {what} lies outside the prior")


def sample_chains(fit, params, n_steps, walkers=8, seed=0, fixed=None, start=None, scatter=None, proposal=None, burn=0, thin=1,
                  keep_chain=True, device=True, kwargs=None, realisations=None, evaluate=None, move="metropolis", stretch_a=2.0,
                  prior=None, marginals=None, autocorr=None, temper=None, predictive=None):
    """The work of ``CCFFit.sample_chains`` (``realisations=None``: the fit's data vector, R = 1) and
    ``Realisations.sample_chains`` (R = the realisations); see the module docstring.  With ``evaluate`` - a callable taking a dict
    of ``(C,)`` arrays (sampled and fixed parameters) and returning ``lnL (C,)`` or ``(lnL, chi2)`` - in place of ``fit`` only the
    definition route (``device=False``) is possible, R = 1 and no GPU is needed (chi2 reads -2 lnL when it is not returned).

    ``params``: the cobaya block; ``fixed``: name -> scalar overrides, which also take a sampled parameter out of the chain;
    ``walkers``: chains per problem; ``start``: None (each chain drawn from the ``ref`` distribution), a
    :class:`victor_amd.fitting.BestFit` or a dict name -> scalar or ``(R,)`` array: every chain of problem i starts at
    ``start_i + scatter * normal`` (``scatter``: name -> scalar, default the proposal widths; 0 starts every chain at the point
    itself), redrawn until inside the box; ``proposal``: name -> width overrides, or a :class:`victor_amd.laplace.Laplace` (or
    a ``BestFit`` carrying one, ``best_fit(..., covariance=True)``) of the same sampled parameters and problems for correlated
    proposals: the increments of the chains of problem r are ``(2.38 / sqrt(d)) chol(cov_r) normal(d)``, problems whose status
    is not OK keep the widths; the increments stay the caller's in the ABI, so both routes take them alike.  ``move``: "metropolis" (the default) or
    "stretch" (module docstring): ``walkers`` must then be even and at least 2 (d + 1), ``stretch_a`` > 1 is the move's scale
    (z lies in [1 / a, a]), ``proposal`` is refused (the move has no widths), ``scatter`` keeps its default but must be > 0 in
    every parameter (an ensemble that starts collapsed onto a point, or into a plane, never leaves it), and the result's
    ``rhat`` is None.  ``prior``: a :class:`victor_amd.priors.GaussianPrior` or a list of them with disjoint names, multiplied
    onto the box (module docstring); both moves and both routes honour it.  ``marginals``: None (off), True (a 128-bin histogram
    of every sampled parameter over its prior box) or a dict ``{"bins": int, "range": {name: (a, b)}, "pairs": [(name, name), ...]
    | "all", "bins2d": int}`` - ranges not given are the box, ``bins`` at most 1024, ``bins2d`` (default 32) at most 128, at
    most 45 pairs - for per-problem histograms of the kept positions, counted where the chains run (:mod:`victor_amd.marginals`;
    ``Chains.marginals``).  ``autocorr``: None (off), True or a dict ``{"max_lag": int, "c": float}`` (defaults 128 and 5.0;
    ``max_lag`` at most 1024) for the integrated autocorrelation time and the effective sample size of every problem and
    parameter, from the series of the per-step sum over the problem's chains, accumulated where the chains run
    (:mod:`victor_amd.autocorr`; ``Chains.autocorr``).  ``temper``: None (off), True or a dict for replica exchange over a ladder
    of inverse temperatures and the evidence by thermodynamic integration (:mod:`victor_amd.tempering`; ``Chains.tempering``):
    ``{"rungs": K, "power": p}`` (defaults 16 and 5) for ``beta_k = ((K - 1 - k) / (K - 1))**p`` or ``{"betas": [...]}`` for an
    explicit ladder (from 1, strictly decreasing, >= 0), ``"swap_every"`` (default 4; 0: never) and ``"scales"``, one factor per
    rung on the proposal widths and on a Laplace proposal's factors (default ``min(1 / sqrt(beta_k), min_j (hi_j - lo_j) / (2
    width_j))``).  R x K x ``walkers`` chains run, at most 65536; every public (R, W, ...) field of the result is the cold rung;
    ``move="stretch"`` is refused with it.  ``predictive``: None (off) or True for the posterior mean and scatter of the theory
    vector, the mean chi-square and the deviance information criterion, summed where the chains run
    (:mod:`victor_amd.predictive`; ``Chains.predictive``); refused (a ``ValueError``) on joint fits, with ``temper`` and with an
    ``evaluate`` callable.  Every argument is checked before the first device call.  Returns a :class:`Chains`."""
    kwargs = kwargs or {}
    n_steps, walkers, burn, thin = int(n_steps), int(walkers), int(burn), int(thin)
    if n_steps < 0:
        raise InputError("sample_chains: n_steps must be >= 0")
    if walkers < 1:
        raise InputError("sample_chains: walkers must be >= 1")
    if burn < 0:
        raise InputError("sample_chains: burn must be >= 0")
    if thin < 1:
        raise InputError("sample_chains: thin must be >= 1")
    if move not in ("metropolis", "stretch"):
        raise InputError(f"sample_chains: move must be 'metropolis' or 'stretch', not {move!r}")
    stretch = move == "stretch"
    if stretch:
        stretch_a = float(stretch_a)
        if not stretch_a > 1.0:
            raise InputError("sample_chains: stretch_a must be > 1")
        if proposal is not None:
            raise InputError("sample_chains: proposal widths mean nothing under move='stretch' (the move has none to tune)")
    if evaluate is not None and device:
        raise InputError("sample_chains: an evaluate callable runs the definition route only (device=False)")
    if evaluate is None and fit is None:
        raise InputError("sample_chains: a fit or an evaluate callable is needed")
    q = _Sampled("sample_chains", "sampled", params, fixed)
    specs, names, fixed_all, lo, hi, d = q.specs, q.names, q.fixed_all, q.lo, q.hi, len(q.names)
    arrays = sorted(k for k, v in fixed_all.items() if np.ndim(v) > 0)
    if evaluate is None:
        q.check_columns(fit)
        if d > 10:
            raise InputError("sample_chains: at most 10 sampled parameters")
        q.check_alpha()
    if arrays:
        raise InputError(f"sample_chains: fixed values must be scalars ({arrays} are not)")
    prior = q.prior(prior, fit)
    from .marginals import resolve_marginals
    binning = resolve_marginals(marginals, "sample_chains", names, lo, hi)
    from .autocorr import resolve_autocorr
    lags = resolve_autocorr(autocorr, "sample_chains")
    from .joint import JointFit
    from .predictive import PredictiveState, resolve_predictive
    predictive = resolve_predictive(predictive, "sample_chains", isinstance(fit, JointFit), temper is not None and temper is not False,
                                    evaluate is None)
    if evaluate is None:
        fit_options = q.fit_options(fit, kwargs, "predictive=" if predictive else None)
    R = len(realisations) if realisations is not None else 1
    W = walkers
    if R * W > MAX_CHAINS:
        raise InputError(f"sample_chains: {R} problems x {W} walkers = {R * W} chains: at most {MAX_CHAINS}")
    if temper is not None and temper is not False and stretch:
        raise InputError("sample_chains: temper runs the Metropolis move only (a tempered stretch move is not provided)")
    if stretch and (W % 2 or W < 2 * (d + 1)):
        raise InputError(f"sample_chains: the stretch move needs an even number of walkers, at least 2 (n_params + 1) = {2 * (d + 1)}")
    lap = getattr(proposal, "laplace", None) if hasattr(proposal, "n_evals") else proposal     # (a BestFit carries its Laplace)
    if proposal is not None and not isinstance(proposal, dict):
        if lap is None or not (hasattr(lap, "proposal_factors") and hasattr(lap, "cov")):
            raise InputError("sample_chains: proposal must be a dict name -> width, a Laplace, or a BestFit of "
                             "best_fit(..., covariance=True)")
        if list(lap.names) != list(names):
            raise InputError(f"sample_chains: the proposal's Laplace holds the parameters {list(lap.names)}, the chains sample "
                             f"{list(names)}")
        if len(lap) != R:
            raise InputError(f"sample_chains: the proposal's Laplace holds {len(lap)} problems, the chains run {R}")
        proposal = None
    else:
        lap = None
    width = q.per_param("proposal", proposal, [s.proposal for s in specs])
    if not stretch and np.any(~(width > 0)):
        raise InputError(f"sample_chains: every proposal width must be > 0 ({dict(zip(names, width.tolist()))})")
    from .tempering import TemperState, resolve_temper
    ladder = resolve_temper(temper, "sample_chains", width, lo, hi)
    K = ladder.K if ladder is not None else 1
    n_chains = R * K * W
    if n_chains > MAX_CHAINS:
        raise InputError(f"sample_chains: {R} problems x {K} rungs x {W} walkers = {n_chains} chains: at most {MAX_CHAINS}")
    centre = None
    if start is not None:
        given = dict(start.params) if hasattr(start, "params") and hasattr(start, "names") else dict(start)
        if hasattr(start, "names"):
            given = {n: v for n, v in given.items() if n in names}      # a BestFit also carries its fixed values
        centre = q.starts(given, R, "sample_chains: ")
        spread = q.per_param("scatter", scatter if not np.isscalar(scatter) else {n: scatter for n in names}, width)
        if np.any(~(spread >= 0)):
            raise InputError("sample_chains: scatter must be >= 0")
        if stretch and np.any(~(spread > 0)):
            raise InputError("sample_chains: under move='stretch' scatter must be > 0 in every parameter (an ensemble that starts "
                             f"collapsed never moves: {dict(zip(names, spread.tolist()))})")
    elif scatter is not None:
        raise InputError("sample_chains: scatter needs a start")

    # ---- the start: the generator's first draws, as EnsembleMetropolis.initialise makes them
    rng = np.random.default_rng(seed)
    x0 = np.empty((n_chains, d))
    if centre is None:
        loc = np.array([s.ref_loc for s in specs])
        scale = np.array([s.ref_scale for s in specs])
        for c in range(n_chains):
            x0[c] = _draw_start(rng, loc, scale, lo, hi, "the reference distribution")
    else:
        for c in range(n_chains):
            x0[c] = _draw_start(rng, centre[c // (K * W)], spread, lo, hi, f"the scattered start of problem {c // (K * W)}")
    which = np.repeat(np.arange(R, dtype=np.int32), K * W)
    fixed_out = {k: float(v) for k, v in fixed_all.items()}

    def batch_of(x):
        batch = dict(fixed_out)
        batch.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names)})
        return batch

    handle = None
    if evaluate is not None:
        def evaluator(x, rows_which=None):
            out = evaluate(batch_of(x))
            if isinstance(out, tuple):
                return np.asarray(out[0], dtype=float), np.asarray(out[1], dtype=float)
            lnl = np.asarray(out, dtype=float)
            return lnl, -2.0 * lnl
    elif not device:
        if predictive and getattr(realisations, "paired_model", False):
            raise InputError("sample_chains: predictive= on the definition route (device=False) takes its theory vectors from the "
                             "fit's own tables; with realisations(paired_model=True) use the device route")
        if realisations is not None:
            def evaluator(x, rows_which=None):
                return realisations.log_likelihood_pairs(batch_of(x), which if rows_which is None else rows_which, **kwargs)
        else:
            def evaluator(x, rows_which=None):
                return fit.log_likelihood_batch(batch_of(x), **kwargs)
    else:
        evaluator = None
        lib, h, refresh = q.create("vk_chain_create", fit, realisations, kwargs, fit_options, batch_of(x0), which)
        handle = (lib, h)
    ch = Chains(names, specs, fixed_out, R, W, rng, width, burn, thin, bool(keep_chain), evaluator, handle, move, stretch_a, prior,
                binning, lags, None if ladder is None else TemperState(ladder, R, W, seed),
                PredictiveState(R, W, len(fit.s) * len(fit.poles_s)) if predictive else None)
    if predictive:
        ch._theory = lambda x: fit.theory_vector_batch(batch_of(x), **kwargs)
        ch._at_mean = ((lambda x, problems: realisations.log_likelihood_pairs(batch_of(x), problems, **kwargs)) if realisations is not None
                       else (lambda x, problems: fit.log_likelihood_batch(batch_of(x), **kwargs)))
        ch._poles = (np.atleast_1d(fit.poles_s), len(fit.s))
    if lap is not None:
        ch._factor = np.repeat(lap.proposal_factors(width), K * W, axis=0)
        if ladder is not None:
            ch._factor = ch._factor * ch._temper.scale[:, None, None]
    if handle:
        ch._refresh = refresh                                # (keeps the realisations and the contexts the handle runs on)
        ch._fit = fit                                        # (a joint fit owns the covariance handles the chains read)
        ch._attach_device(q.set_prior, x0)
    else:
        ch._start_host(x0)
    return ch.extend(n_steps)
