"""Grid posteriors reduced on the GPU (victor_amd/grid.py, vk_grid_run) against the NumPy loop that defines them (device=False:
one log_likelihood_batch / Realisations.log_likelihood call per chunk): rows bit for bit, epsilon axis included; maxima, arg max,
counts, profiles and statuses as bytes, weight sums at the derived bound of tests/test_grid.py; against one independent
evaluation of the whole grid with a plain log-sum-exp; the prior; cuts and repeats of vk_grid_run; a failing node; the refusals
that need a context.  The grids hold 20 - 60 points: a grid kernel goes wrong at chunk cuts, at axes of length 1 and at a problem
count that crosses a wave, not at size."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases, tolerances
from tests.test_chains import same_bytes
from tests.test_grid import assert_exact, assert_sums, sum_bound
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
RANGES = {"fsigma8": (0.35, 0.6), "beta": (0.3, 0.5), "sigma_v": (300.0, 460.0), "epsilon": (0.95, 1.05)}
SYNTH = {"fsigma8": {"prior": {"min": 0.3, "max": 0.6}, "ref": {"loc": 0.45, "scale": 0.02}, "proposal": 0.02},
         "epsilon": {"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0, "scale": 0.02}, "proposal": 0.02},
         "sigma_v": 360.0}
BINS3 = {"fsigma8": 5, "beta": 4, "sigma_v": 3}
BINS2 = {"fsigma8": 5, "epsilon": 4}


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def synth():
    import victor_amd
    return victor_amd.CCFFit(*cases.synth_options(2))


@pytest.fixture(scope="module")
def boss():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


@pytest.fixture(scope="module")
def stack():
    import victor_amd
    return victor_amd.CCFFit(*stack_options())


@pytest.fixture(scope="module")
def rs(stack):
    return stack.realisations()


def ranges_of(names):
    return {n: RANGES[n] for n in names}


def both_routes(obj, params, what, **kw):
    """The device route and the definition route of one call, compared: exact outputs as bytes, sums at the bound."""
    dev = obj.grid_posterior(params, **kw)
    ref = obj.grid_posterior(params, device=False, **kw)
    assert dev.shape == ref.shape and dev.n_problems == ref.n_problems and dev.chunk == ref.chunk
    assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status), what
    assert_sums(dev.raw, ref.raw, dev.n_chunks, what, dev._grid)
    return dev, ref


class Handle:
    """A raw vk_grid handle of a call's arguments (victor_amd.grid.create_handle), for what the public route does not expose."""

    def __init__(self, fit, params, bins, realisations=None, fixed=None, ranges=None, pairs=None, chunk=7, prior=None):
        from victor_amd import grid as G
        from victor_amd.fitting import _Sampled
        q = _Sampled("grid_posterior", "gridded", params, fixed)
        self.grid = G.resolve_grid("test", q.names, q.lo, q.hi, bins, ranges, pairs)
        self.R = 1 if realisations is None else len(realisations)
        self.fixed = {k: float(v) for k, v in q.fixed_all.items()}
        self.prior = q.prior(prior, fit)
        self.lib, self.h, _ = G.create_handle(q, fit, realisations, {}, q.fit_options(fit, {}), self.grid, self.fixed, chunk)
        if self.prior is not None:
            from victor_amd import _native as N
            assert self.lib.vk_grid_set_prior(self.h, N.as_dp(self.prior.mu), N.as_dp(self.prior.pp)) == 0

    def run(self, first, count):
        return self.lib.vk_grid_run(self.h, first, count)

    def error(self):
        return (self.lib.vk_grid_last_error(self.h) or b"").decode()

    def result(self):
        from victor_amd import grid as G
        return G.read_result(self.lib, self.h, self.grid, self.R, self.prior is not None)

    def rows(self, first, count):
        out = np.empty((count, 12))
        rc = self.lib.vk_grid_rows(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0, self.error()
        return out

    def close(self):
        self.lib.vk_grid_destroy(self.h)


def host_rows(fit, handle):
    batch = dict(handle.fixed)
    x = handle.grid.points(np.arange(handle.grid.G))
    batch.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(handle.grid.names)})
    return np.ascontiguousarray(fit._fit_rows(batch, fit._merged({})), dtype=np.float64)


ACCS = ("ln_max", "arg_max", "total", "n_finite", "m1", "p1", "m2", "p2")


# ------------------------------------------------------------------ device route against the definition route ---------------
def test_synthetic_fit_with_an_epsilon_axis(synth):
    assert len(synth.s) * len(np.atleast_1d(synth.poles_s)) == 80
    dev, ref = both_routes(synth, SYNTH, "synthetic (fsigma8, epsilon) 5 x 4, chunk 7", bins=BINS2, chunk=7, pairs=[("epsilon", "fsigma8")])
    assert dev.names == ["fsigma8", "epsilon"] and dev.shape == (5, 4) and dev.n_chunks == 3 and dev.status[0] == dev.OK
    assert np.all(dev.n_finite == 20) and np.isfinite(dev.ln_evidence[0])
    h = Handle(synth, SYNTH, BINS2, pairs=[("fsigma8", "epsilon")], chunk=7)
    try:
        want = host_rows(synth, h)
        got = np.concatenate([h.rows(g0, min(7, 20 - g0)) for g0 in range(0, 20, 7)])
        assert same_bytes(got, want), np.argwhere(got != want)[:4]              # epsilon axis included: the host's own pow
        assert len(set(want[:, 3])) == 4                                        # (four epsilon nodes, four apar)
    finally:
        h.close()


@pytest.mark.parametrize("chunk", [7, 60, 64])
def test_boss_fit_three_axes_and_a_pair(boss, chunk):
    """beta-dependent data and covariance; a cut inside an axis run (7), one exact chunk (60), a chunk larger than G (64)."""
    fixed = {"epsilon": 1.0}
    dev, ref = both_routes(boss, PARAMS, f"BOSS (fsigma8, beta, sigma_v) 5 x 4 x 3, chunk {chunk}", bins=BINS3, fixed=fixed, chunk=chunk,
                           ranges=ranges_of(BINS3), pairs=[("fsigma8", "sigma_v")])
    assert dev.shape == (5, 4, 3) and dev.n_chunks == -(-60 // chunk) and dev.status[0] == dev.OK and dev.n_finite[0] == 60
    h = Handle(boss, PARAMS, BINS3, fixed=fixed, ranges=ranges_of(BINS3), chunk=chunk)
    try:
        want = host_rows(boss, h)
        got = np.concatenate([h.rows(g0, min(chunk, 60 - g0)) for g0 in range(0, 60, chunk)])
        assert same_bytes(got, want)
    finally:
        h.close()


# ------------------------------------------------------------------ realisations -------------------------------------------
@pytest.mark.parametrize("chunk", [7, 20])
def test_sixteen_realisations(rs, chunk):
    fixed = {"beta": 0.37, "sigma_v": 380.0}
    dev, ref = both_routes(rs, PARAMS, f"16 realisations (fsigma8, epsilon) 5 x 4, chunk {chunk}", bins=BINS2, fixed=fixed, chunk=chunk,
                           ranges=ranges_of(BINS2), pairs=[("fsigma8", "epsilon")])
    assert dev.n_problems == 16 and np.all(dev.status == dev.OK) and len(set(dev.ln_max)) == 16


@pytest.mark.parametrize("chunk", [7, 20])
def test_seventy_problems_cross_a_wave(stack, chunk):
    """R = 70: problems r and r + 16 are the same realisation and agree byte for byte in every output."""
    rs70 = stack.realisations(np.arange(70) % 16)
    gp = rs70.grid_posterior(PARAMS, bins=BINS2, fixed={"beta": 0.37, "sigma_v": 380.0}, chunk=chunk, ranges=ranges_of(BINS2),
                             pairs=[("fsigma8", "epsilon")])
    assert gp.n_problems == 70
    for name in ACCS:
        a = getattr(gp.raw, name)
        for r in range(70 - 16):
            assert same_bytes(a[r], a[r + 16]), (name, r)
    assert same_bytes(gp.ln_evidence[:16], gp.ln_evidence[16:32]) and len(set(gp.ln_max[:16])) == 16


# ------------------------------------------------------------------ against an independent evaluation ----------------------
def lnl_bound(fit, batch, lnl):
    """The per-point bound of tests/tolerances.py on lnL of two evaluation orders (64 ulps), as assert_same_lnl forms it."""
    return 0.51 * tolerances.chi2_bound(fit, batch, ulps=64) + 16 * tolerances.U * (np.abs(lnl) + 1000.0)


def independent(gp, lnl, bound, what):
    """``gp`` (one problem) against lnL of the whole grid from ONE call, reduced by a plain NumPy log-sum-exp."""
    grid = gp._grid
    B = float(np.max(bound))
    top = lnl.max()
    w = np.exp(lnl - top)
    ln_sum = top + np.log(w.sum())
    rel = sum_bound(gp.n_chunks, grid.G)
    got = gp.ln_max[0] + np.log(gp.raw.total[0])
    tolerances._record(f"grid ln(sum) {what}", abs(got - ln_sum) / (B + rel))
    assert abs(got - ln_sum) <= B + rel, (what, got - ln_sum, B)
    assert abs(gp.ln_evidence[0] - (ln_sum + np.sum(np.log((grid.b - grid.a) / np.array(grid.shape))) - np.sum(np.log(grid.hi - grid.lo)))) <= B + rel + 64 * tolerances.U
    # a weight over the total moves by e^(+-2 B): the marginals' relative bound, plus the two sums'
    cube = w.reshape(grid.shape) / w.sum()
    worst = 0.0
    for j, name in enumerate(grid.names):
        want = cube.sum(axis=tuple(k for k in range(grid.d) if k != j)) / ((grid.b[j] - grid.a[j]) / grid.shape[j])
        diff = np.abs(gp.marginal(name)[0] - want)
        allowed = (np.expm1(2 * B) + 2 * rel) * want
        worst = max(worst, float(np.max(diff / allowed)))
    tolerances._record(f"grid marginals {what}", worst)
    assert worst <= 1.0, (what, worst)
    assert gp.arg_max[0] == int(np.argmax(lnl)) or lnl[gp.arg_max[0]] >= top - B


def test_data_vector_against_one_batch_call_and_logsumexp(boss):
    fixed = {"epsilon": 1.0}
    gp = boss.grid_posterior(PARAMS, bins=BINS3, fixed=fixed, chunk=7, ranges=ranges_of(BINS3))
    x = gp._grid.points(np.arange(60))
    batch = dict(fixed, **{n: x[:, j] for j, n in enumerate(gp.names)})
    lnl = boss.log_likelihood_batch(batch)[0]
    independent(gp, lnl, lnl_bound(boss, batch, lnl), "BOSS data vector")


def test_realisations_against_one_call_and_logsumexp(rs):
    """Problems 0, 7 and 15: the bound needs the realisation's own data vector, a fit each."""
    import victor_amd
    from victor_amd.grid import GridPosterior
    fixed = {"beta": 0.37, "sigma_v": 380.0}
    gp = rs.grid_posterior(PARAMS, bins=BINS2, fixed=fixed, chunk=7, ranges=ranges_of(BINS2))
    x = gp._grid.points(np.arange(20))
    batch = dict(fixed, **{n: x[:, j] for j, n in enumerate(gp.names)})
    lnl = rs.log_likelihood(batch)[0]
    assert lnl.shape == (20, 16)
    for m in (0, 7, 15):
        one = victor_amd.CCFFit(*stack_options(simulation_number=m))
        acc = type(gp.raw)(gp._grid, 1)
        for name in ACCS:
            setattr(acc, name, getattr(gp.raw, name)[m:m + 1])
        independent(GridPosterior(gp._grid, acc, None, gp.chunk), lnl[:, m], lnl_bound(one, batch, lnl[:, m]), f"realisation {m}")


# ------------------------------------------------------------------ the prior ----------------------------------------------
def test_gaussian_prior(boss, rs):
    from victor_amd.priors import GaussianPrior
    prior = GaussianPrior(["fsigma8", "beta"], [0.45, 0.4], cov=[[0.05 ** 2, 0.5 * 0.05 * 0.04], [0.5 * 0.05 * 0.04, 0.04 ** 2]])
    kw = dict(bins=BINS3, fixed={"epsilon": 1.0}, chunk=7, ranges=ranges_of(BINS3), pairs=[("beta", "sigma_v")])
    dev, ref = both_routes(boss, PARAMS, "BOSS with a Gaussian prior", prior=prior, **kw)
    plain = boss.grid_posterior(PARAMS, **kw)
    assert not same_bytes(dev.ln_max, plain.ln_max)
    # lnpost follows vkprior::lnprior's bits: the maximum IS lnL + ln prior of its node, as the host states it
    assert same_bytes(dev.prior_ln_max, ref.prior_ln_max)
    assert abs(dev.prior_total - ref.prior_total) <= sum_bound(dev.n_chunks, 60) * ref.prior_total
    want = (dev.ln_max[0] + np.log(dev.raw.total[0])) - (dev.prior_ln_max + np.log(dev.prior_total))
    assert same_bytes(dev.ln_evidence[0], want) and abs(dev.ln_evidence[0] - ref.ln_evidence[0]) <= 4 * sum_bound(dev.n_chunks, 60)
    # against every realisation: one prior for all, its own problem once
    kw2 = dict(bins=BINS2, fixed={"beta": 0.37, "sigma_v": 380.0}, chunk=7, ranges=ranges_of(BINS2))
    both_routes(rs, PARAMS, "16 realisations with a Gaussian prior", prior=GaussianPrior(["fsigma8"], [0.45], sigma=[0.05]), **kw2)


# ------------------------------------------------------------------ cuts and repeats ---------------------------------------
def test_cuts_and_repeats_give_the_same_bytes(rs, stack):
    h = Handle(stack, PARAMS, BINS2, realisations=rs, fixed={"beta": 0.37, "sigma_v": 380.0}, ranges=ranges_of(BINS2),
               pairs=[("fsigma8", "epsilon")], chunk=7)
    try:
        assert h.lib.vk_grid_result(h.h, *([None] * 10)) == -1 and "reached 0 of 20" in h.error()
        assert h.run(0, 20) == 0, h.error()
        whole, _ = h.result()
        assert h.run(0, 1 << 40) == 0, h.error()                                # the same call twice (count past the end: to G)
        again, _ = h.result()
        assert h.run(0, 14) == 0, h.error()
        assert h.lib.vk_grid_result(h.h, *([None] * 10)) == -1 and "reached 14 of 20" in h.error()
        assert h.run(7, 7) == -1 and "first must be 0" in h.error()             # not where the run stands
        assert h.run(15, 5) == -1 and "multiple of the chunk" in h.error()
        assert h.run(14, 3) == -1 and "whole chunks" in h.error()
        assert h.run(14, 6) == 0, h.error()                                     # two calls cut at a chunk multiple
        cut, _ = h.result()
        for name in ACCS:
            assert same_bytes(getattr(whole, name), getattr(again, name)), ("twice", name)
            assert same_bytes(getattr(whole, name), getattr(cut, name)), ("14 + 6", name)
        assert np.all(whole.n_finite == 20)
    finally:
        h.close()


# ------------------------------------------------------------------ a failing node -----------------------------------------
def test_a_failing_node(synth):
    """An epsilon box that reaches below zero: a negative epsilon makes the Alcock-Paczynski factors of the row NaN and the
    library reports (-inf, inf) for it."""
    block = dict(SYNTH, epsilon={"prior": {"min": -0.2, "max": 1.2}, "ref": {"loc": 1.0, "scale": 0.02}, "proposal": 0.02})
    kw = dict(bins=BINS2, chunk=7, pairs=[("fsigma8", "epsilon")])
    with np.errstate(invalid="ignore"):
        dev, ref = both_routes(synth, block, "a failing epsilon node", **kw)
        x = dev._grid.points(np.arange(20))
        lnl, chi2 = synth.log_likelihood_batch({"fsigma8": x[:, 0], "epsilon": x[:, 1], "sigma_v": 360.0})
    fails = ~np.isfinite(lnl)
    assert dev.axes["epsilon"][0] < 0 and np.all(fails[x[:, 1] < 0]) and np.all(chi2[fails] == np.inf) and 0 < fails.sum() < 20
    assert dev.n_finite[0] == 20 - fails.sum() and dev.status[0] == dev.OK
    dead = [k for k in range(4) if np.all(fails[x[:, 1] == dev.axes["epsilon"][k]])]
    assert 0 in dead
    for k in dead:                                               # untouched: the sums 0, the maxima -inf
        assert dev.marginal("epsilon")[0, k] == 0 and dev.profile("epsilon")[0, k] == -np.inf
        assert np.all(dev.marginal2d("fsigma8", "epsilon")[0, :, k] == 0)
    for name in ACCS:
        assert not np.any(np.isnan(getattr(dev.raw, name))), name
    for arr in (dev.ln_evidence, dev.mean, dev.sigma, dev.edge_mass, dev.marginal("fsigma8"), dev.profile("fsigma8")):
        assert not np.any(np.isnan(arr))


# ------------------------------------------------------------------ refusals that need a context ---------------------------
def test_refusals_with_a_context(rs, tmp_path):
    import victor_amd
    from tests.test_paired_realisations import NUMBERS, paired_boss_options, write_boss_model_stack
    from victor_amd.utils import InputError
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        rs.grid_posterior(PARAMS, bins=2, beta_interpolation="likelihood")
    paired = victor_amd.CCFFit(*paired_boss_options(tmp_path, number=NUMBERS[0], model_file=write_boss_model_stack(tmp_path)))
    with pytest.raises(InputError, match="paired_model"):
        paired.realisations(NUMBERS, paired_model=True).grid_posterior(PARAMS, bins=2)
