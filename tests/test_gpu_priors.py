"""Gaussian priors on the GPU (``prior=`` of ``best_fit`` / ``sample_chains``; vk_fit_set_prior / vk_chain_set_prior; DESIGN.md
sections 7a and 7b): the device's Metropolis chains and stretch-move ensembles under a prior against the NumPy loop that defines
them (``device=False``) - with epsilon fixed both routes launch the same rows in launches of the same shape and evaluate the same
prior statement, so everything is compared byte for byte; with epsilon sampled, positions and decisions under the decision-margin
precondition of tests/test_gpu_chains.py (the margin includes the prior terms) -, best fits of lnL + ln prior, joint fits with a
prior on ``"sigma_v@q"`` parameters, and the handles: no prior means no change, cuts, and the refusal while a block is in flight.

Fixtures: the BOSS golden configuration with its 16-realisation stack; the five density-split blocks with stacks of 5
realisations, block-diagonal and under ``correlated(...)``, as tests/test_gpu_joint_blocks.py sets its three up.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_joint_blocks import blocks_bound
from tests.test_gpu_joint_sampled import fits_of
from tests.test_gpu_stretch import Raw, stretch_numbers
from tests.test_joint_cov import correlated
from tests.test_joint_realisations import dsplit_stacks, with_number
from tests.test_realisations import stack_options
from tests.tolerances import U, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
EPS_FIXED = {"epsilon": 1.0}
MARGIN = 1e-6            # as tests/test_gpu_chains.py
HISTORY = ("pivot", "chain", "lnl_chain", "chi2_chain", "lnprior_chain", "x", "lnl", "chi2", "n_accept", "acceptance")
WALK = ("pivot", "chain", "lnprior_chain", "x", "n_accept", "acceptance")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def boss_prior():
    """Correlated on (fsigma8, sigma_v) - not adjacent in sampled order: beta lies between them - and diagonal on beta."""
    from victor_amd import GaussianPrior
    return [GaussianPrior(["sigma_v", "fsigma8"], [360.0, 0.45], cov=[[625.0, 0.625], [0.625, 0.0025]]),
            GaussianPrior(["beta"], [0.42], sigma=[0.05])]


def resolved(prior, names, params=PARAMS):
    from victor_amd.priors import resolve_prior
    base = [n.partition("@")[0] for n in names]
    lo = np.array([params[b]["prior"]["min"] for b in base], dtype=float)
    hi = np.array([params[b]["prior"]["max"] for b in base], dtype=float)
    return resolve_prior(prior, "test", names, lo, hi)


def same_run(dev, ref, what, attrs=HISTORY):
    assert dev.move == ref.move and dev.n_steps == ref.n_steps and dev.n_kept == ref.n_kept, what
    for a in attrs:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)


def lnl_allowance(lnl, chi2_bounds):
    """The launch-shape rounding allowance for lnL of tests/tolerances.py: the bound ``assert_same_lnl`` applies (0.51 of the
    chi-square bound plus 16 u (|lnL| + the log-determinant scale 1000)), restated for a one-sided comparison."""
    return 0.51 * np.asarray(chi2_bounds, dtype=float) + 16 * U * (np.abs(lnl) + 1000.0)


@pytest.fixture(scope="module")
def fit():
    import victor_amd
    return victor_amd.CCFFit(*stack_options())


@pytest.fixture(scope="module")
def rs9(fit):
    """Nine realisations: with W = 8, 72 chains - a partial wave, two workgroups."""
    return fit.realisations(list(range(9)))


# ------------------------------------------------------------------ 1. Metropolis, epsilon fixed ----------------------------
METRO = dict(walkers=8, seed=2, burn=5, thin=2, fixed=EPS_FIXED)


@pytest.fixture(scope="module")
def metro_ref(rs9):
    """The definition route's 70 steps of the 72 chains under the prior, computed once."""
    return rs9.sample_chains(PARAMS, 70, device=False, prior=boss_prior(), **METRO)


def test_metropolis_is_the_definition_route_byte_for_byte(rs9, metro_ref):
    ref = metro_ref
    dev = rs9.sample_chains(PARAMS, 70, prior=boss_prior(), **METRO)
    assert dev.names == ["fsigma8", "beta", "sigma_v"] and dev.chain.shape == (33, 9, 8, 3)       # steps 5, 7, .. 69: across the block of 64
    print("acceptance of the definition route:", ref.acceptance, "smallest margin:", ref.decision_margin)
    assert np.all((0.02 < ref.acceptance) & (ref.acceptance < 0.98)), ref.acceptance
    same_run(dev, ref, "metropolis under a prior")
    assert same_bytes(dev.lnprior_chain, resolved(boss_prior(), dev.names).lnprior(dev.chain))
    assert np.all(dev.lnprior_chain < 0.0) and dev.lnprior_chain.shape == (33, 9, 8)
    free = rs9.sample_chains(PARAMS, 70, **METRO)
    assert not same_bytes(free.chain, dev.chain), "the prior changed no decision: the test does not reach it"
    assert np.all(free.lnprior_chain == 0.0)


# ------------------------------------------------------------------ 2. stretch, epsilon fixed -------------------------------
STRETCH = dict(walkers=8, seed=2, burn=5, thin=3, move="stretch", fixed=EPS_FIXED)
NARROW = dict(PARAMS, sigma_v=dict(PARAMS["sigma_v"], prior={"dist": "uniform", "min": 350.0, "max": 400.0}, ref={"loc": 375.0, "scale": 5.0}))


@pytest.mark.parametrize("box", ["whole", "narrow"])
def test_stretch_is_the_definition_route_byte_for_byte(rs9, box):
    block = PARAMS if box == "whole" else NARROW
    ref = rs9.sample_chains(block, 40, device=False, prior=boss_prior(), **STRETCH)
    dev = rs9.sample_chains(block, 40, prior=boss_prior(), **STRETCH)
    assert dev.chain.shape == (12, 9, 8, 3) and dev.rhat is None
    print(box, "acceptance of the definition route:", ref.acceptance, "outside:", ref.n_outside.sum(), "of", 40 * 72)
    assert np.all((0.02 < ref.acceptance) & (ref.acceptance < 0.98)), ref.acceptance
    if box == "narrow":
        assert ref.n_outside.sum() > 0, "no proposal left the box: the test does not reach that rule"
        j = dev.names.index("sigma_v")
        assert np.all(dev.chain[..., j] >= 350.0) and np.all(dev.chain[..., j] <= 400.0)
    same_run(dev, ref, f"stretch under a prior, {box} box")
    assert same_bytes(dev.lnprior_chain, resolved(boss_prior(), dev.names, block).lnprior(dev.chain))
    free = rs9.sample_chains(block, 40, **STRETCH)
    assert not same_bytes(free.chain, dev.chain), "the prior changed no decision: the test does not reach it"


# ------------------------------------------------------------------ 3. epsilon sampled ---------------------------------------
@pytest.mark.parametrize("move,walkers", [("metropolis", 4), ("stretch", 10)])
def test_epsilon_sampled(fit, move, walkers):
    """The seed is the first of 0, 1, 2, ... whose smallest decision margin on the definition route - prior terms included -
    exceeds MARGIN: chosen here, with the definition route alone, before the device route runs."""
    from victor_amd import GaussianPrior
    rs = fit.realisations([0, 1, 2])
    prior = boss_prior() + [GaussianPrior(["epsilon"], [1.01], sigma=[0.03])]
    ref = None
    for seed in range(8):
        kw = dict(walkers=walkers, seed=seed, move=move, prior=prior)
        ref = rs.sample_chains(PARAMS, 70, device=False, **kw)
        print(move, "seed", seed, "smallest decision margin (definition route):", ref.decision_margin)
        if ref.decision_margin > MARGIN:
            break
    assert ref.decision_margin > MARGIN, ref.decision_margin            # a condition on the inputs, not on the code under test
    dev = rs.sample_chains(PARAMS, 70, **kw)
    assert dev.names == ["fsigma8", "beta", "sigma_v", "epsilon"] and dev.chain.shape == (70, 3, walkers, 4)
    same_run(dev, ref, f"epsilon sampled, {move}", WALK)
    assert np.allclose(dev.lnl_chain, ref.lnl_chain, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 4. best fits ---------------------------------------------
def test_best_fit_under_a_prior(fit):
    import victor_amd
    from victor_amd import GaussianPrior
    rs = fit.realisations()
    R = len(rs)
    assert R == 16
    bf0 = rs.best_fit(PARAMS)
    assert np.all(bf0.lnprior == 0.0) and same_bytes(bf0.lnpost, bf0.lnl)
    # one prior for all realisations, 3 sigma away from the nearest of their best-fit dispersions (on the side with room in the box)
    sv, sigma = bf0.params["sigma_v"], 20.0
    lo, hi = PARAMS["sigma_v"]["prior"]["min"], PARAMS["sigma_v"]["prior"]["max"]
    centre = sv.min() - 3 * sigma if sv.min() - 3 * sigma >= lo else sv.max() + 3 * sigma
    assert lo <= centre <= hi and np.all(np.abs(sv - centre) >= 3 * sigma * (1 - 1e-12))
    p = GaussianPrior(["sigma_v"], [centre], sigma=[sigma])
    r = resolved(p, bf0.names)
    bf1 = rs.best_fit(PARAMS, prior=p, start=bf0)
    again = rs.best_fit(PARAMS, prior=p, start=bf0)
    for a in ("x", "lnl", "chi2", "lnpost", "lnprior", "status", "n_iter", "n_evals"):
        assert getattr(bf1, a).tobytes() == getattr(again, a).tobytes(), a
    # Nelder-Mead never ends below its start vertex
    pts = {n: bf0.params[n] for n in bf0.names}
    lnl0, _ = rs.log_likelihood_pairs(pts, np.arange(R))
    single = [victor_amd.CCFFit(*stack_options(simulation_number=k)) for k in range(R)]
    bound = np.array([chi2_bound(single[k], bf0.point(k))[0] for k in range(R)])
    m = lnl_allowance(lnl0, bound)
    start_value = lnl0 + r.lnprior(bf0.x)
    print("lnpost - (lnL + lp at the start):", bf1.lnpost - start_value, "allowance:", m)
    assert np.all(bf1.lnpost >= start_value - m), (bf1.lnpost - start_value, m)
    assert np.all(np.any(bf1.x != bf0.x, axis=1)), "the prior moved no best fit"
    assert same_bytes(bf1.lnprior, r.lnprior(bf1.x)) and np.all(bf1.lnprior < 0.0)
    assert same_bytes(bf1.lnl, bf1.lnpost - bf1.lnprior)
    # lnl is the log-likelihood at x, up to that subtraction's rounding and the launch-shape allowance
    lnl1, chi1 = rs.log_likelihood_pairs({n: bf1.params[n] for n in bf1.names}, np.arange(R))
    bound1 = np.array([chi2_bound(single[k], bf1.point(k))[0] for k in range(R)])
    rounding = 2 * U * (np.abs(bf1.lnpost) + np.abs(bf1.lnprior))        # the device's addition and the host's subtraction
    assert np.all(np.abs(bf1.lnl - lnl1) <= lnl_allowance(lnl1, bound1) + rounding), bf1.lnl - lnl1
    # the best fits start chains under the same prior
    ch = rs.sample_chains(PARAMS, 3, walkers=2, start=bf1, prior=p)
    assert ch.chain.shape == (3, R, 2, 4) and np.all(np.isfinite(ch.lnl)) and np.all(ch.lnprior_chain < 0.0)


# ------------------------------------------------------------------ 5. joint fits, a prior on "sigma_v@q" ------------------------
BETA = 0.4                # the density-split blocks ignore beta: fixed at the cobaya block's reference value


class Five:
    """The five density-split blocks with stacks of 5 realisations, block-diagonal or under ``correlated(...)``."""

    def __init__(self, tmp, cov):
        from victor_amd.joint import JointFit
        self.opts = dsplit_stacks(tmp, 5)
        self.fits = fits_of(self.opts)
        self.covariance = correlated([f.covmat for f in self.fits]) if cov else None
        self.joint = JointFit(self.fits, covariance=self.covariance)
        self._single = {}

    def of(self, m):
        from victor_amd.joint import JointFit
        if m not in self._single:
            self._single[m] = JointFit(fits_of(with_number(self.opts, m)), covariance=self.covariance)
        return self._single[m]


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    made = {}

    def get(cov):
        if cov not in made:
            made[cov] = Five(tmp_path_factory.mktemp("five_cov" if cov else "five_diag"), cov)
        return made[cov]
    return get


def blocked():
    from victor_amd.joint import per_block
    return per_block(PARAMS, ["sigma_v"], 5)


def joint_prior():
    from victor_amd import GaussianPrior
    return GaussianPrior(["sigma_v@3", "sigma_v@1"], [395.0, 350.0], cov=[[400.0, 180.0], [180.0, 625.0]])


JOINT_NAMES = ["fsigma8"] + [f"sigma_v@{q}" for q in range(5)]


@pytest.mark.parametrize("cov", [True, False], ids=["joint_cov", "block_diagonal"])
@pytest.mark.parametrize("data", [True, False], ids=["data", "mocks"])
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_joint_chains_are_the_definition_route_byte_for_byte(five, cov, data, move):
    c = five(cov)
    target = c.joint if data else c.joint.realisations([0, 1, 2])
    W = 14 if move == "stretch" else 8 if data else 2          # stretch: W >= 2 (d + 1), d = 6
    n = 20 if move == "stretch" else 70                          # (70 steps cross the block of 64)
    kw = dict(walkers=W, seed=2, fixed={"beta": BETA, "epsilon": 1.0}, move=move, prior=joint_prior())
    ref = target.sample_chains(blocked(), n, device=False, **kw)
    dev = target.sample_chains(blocked(), n, **kw)
    assert dev.names == JOINT_NAMES and dev.chain.shape == (n, 1 if data else 3, W, 6)
    print("joint", "cov" if cov else "diag", "data" if data else "mocks", move, "acceptance of the definition route:", ref.acceptance)
    assert 0.02 < ref.acceptance.mean() < 0.98                   # a condition on the inputs
    same_run(dev, ref, "joint chains under a prior")
    assert same_bytes(dev.lnprior_chain, resolved(joint_prior(), JOINT_NAMES).lnprior(dev.chain))
    free = target.sample_chains(blocked(), n, **dict(kw, prior=None))
    assert not same_bytes(free.chain, dev.chain), "the prior changed no decision: the test does not reach it"


def test_joint_best_fit_under_a_prior(five):
    c = five(True)
    jr = c.joint.realisations([0, 1, 2])
    fixed = {"beta": BETA, "epsilon": 1.0}
    bf0 = jr.best_fit(blocked(), fixed=fixed)
    assert bf0.names == JOINT_NAMES
    p, r = joint_prior(), resolved(joint_prior(), JOINT_NAMES)
    bf1 = jr.best_fit(blocked(), fixed=fixed, prior=p, start=bf0)
    pts = {n: bf0.params[n] for n in list(bf0.names) + list(fixed)}
    lnl0, _ = jr.log_likelihood_pairs(pts, np.arange(3))
    bound = np.array([blocks_bound(c.of(k), {key: v[k:k + 1] for key, v in pts.items()})[0] for k in range(3)])
    m = lnl_allowance(lnl0, bound)
    start_value = lnl0 + r.lnprior(bf0.x)
    print("joint lnpost - (lnL + lp at the start):", bf1.lnpost - start_value, "allowance:", m)
    assert np.all(bf1.lnpost >= start_value - m), (bf1.lnpost - start_value, m)
    assert np.all(np.any(bf1.x != bf0.x, axis=1))
    assert same_bytes(bf1.lnprior, r.lnprior(bf1.x)) and same_bytes(bf1.lnl, bf1.lnpost - bf1.lnprior)
    # the parameters the prior names moved; the prior is read per block (another block's dispersion carries none)
    assert np.all(bf1.params["sigma_v@1"] != bf0.params["sigma_v@1"]) and np.all(bf1.params["sigma_v@3"] != bf0.params["sigma_v@3"])


# ------------------------------------------------------------------ 6. no prior means no change ------------------------------
def test_no_prior_means_no_change(rs9, metro_ref):
    a = rs9.sample_chains(PARAMS, 70, **METRO)
    b = rs9.sample_chains(PARAMS, 70, prior=None, **METRO)
    for name in HISTORY + ("mean", "cov", "rhat"):
        assert same_bytes(getattr(a, name), getattr(b, name)), name
    # a prior set and then cleared: the bytes of a handle that never had one
    r = resolved(boss_prior(), ["fsigma8", "beta", "sigma_v"])
    x0 = np.ascontiguousarray(metro_ref.pivot.reshape(72, 3))
    rng = np.random.default_rng(4)
    width = np.array([PARAMS[n]["proposal"] for n in ("fsigma8", "beta", "sigma_v")], dtype=float)
    dz, lu = width * rng.standard_normal((6, 72, 3)), np.log(rng.random((6, 72)))
    z, lz, logu, k = stretch_numbers(rng, 3, 36, 4, 3)
    dp = C.POINTER(C.c_double)
    out = []
    for cleared in (False, True, None):                             # never set; set and cleared; set (must differ)
        raw = Raw(rs9, x0, 8)
        try:
            if cleared is not False:
                assert raw.lib.vk_chain_set_prior(raw.h, r.mu.ctypes.data_as(dp), r.pp.ctypes.data_as(dp)) == 0, raw.error()
            if cleared:
                assert raw.lib.vk_chain_set_prior(raw.h, None, None) == 0, raw.error()
            assert raw.start(x0) == 0, raw.error()
            rc, m = raw.metropolis(dz, lu, 0)
            assert rc == 0 and m == 6, raw.error()
            got = list(raw.finish(6)[1:])
            rc, m = raw.stretch(z, lz, logu, k, first=6)
            assert rc == 0 and m == 3, raw.error()
            got += list(raw.finish(3)[1:]) + list(raw.state())
            out.append(got)
        finally:
            raw.close()
    for u, v in zip(out[0], out[1]):
        assert same_bytes(u, v)
    assert not same_bytes(out[0][0], out[2][0]), "the prior set on the handle changed nothing"


# ------------------------------------------------------------------ 7. handles -----------------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_a_run_cut_with_extend_is_the_uncut_run(rs9, move):
    kw = METRO if move == "metropolis" else STRETCH
    whole = rs9.sample_chains(PARAMS, 70, prior=boss_prior(), **kw)
    cut = rs9.sample_chains(PARAMS, 30, prior=boss_prior(), **kw).extend(34).extend(6)     # a cut inside a block and one at its end
    same_run(cut, whole, f"30 + 34 + 6, {move}", HISTORY + ("sum1", "sum2", "mean", "cov"))


def test_metropolis_stretch_metropolis_on_one_handle_with_a_prior(rs9, metro_ref):
    """Blocks of both moves on one handle with a prior set, against the definitions restated on the same numbers; setting a prior
    while a block is in flight is refused with VK_E_ARG and changes nothing."""
    r = resolved(boss_prior(), ["fsigma8", "beta", "sigma_v"])
    x0 = np.ascontiguousarray(metro_ref.pivot.reshape(72, 3))
    rng = np.random.default_rng(9)
    width = np.array([PARAMS[n]["proposal"] for n in ("fsigma8", "beta", "sigma_v")], dtype=float)
    dz1, lu1 = width * rng.standard_normal((5, 72, 3)), np.log(rng.random((5, 72)))
    z, lz, logu, k = stretch_numbers(rng, 4, 36, 4, 3)
    dz2, lu2 = width * rng.standard_normal((6, 72, 3)), np.log(rng.random((6, 72)))
    dp = C.POINTER(C.c_double)
    raw = Raw(rs9, x0, 8)
    try:
        mu, pp = r.mu.ctypes.data_as(dp), r.pp.ctypes.data_as(dp)
        bad = r.pp.copy()
        bad[1] = np.nan
        assert raw.lib.vk_chain_set_prior(raw.h, mu, bad.ctypes.data_as(dp)) == -1 and "not finite" in raw.error()
        assert raw.lib.vk_chain_set_prior(raw.h, mu, None) == -1 and "both" in raw.error()
        assert raw.lib.vk_chain_set_prior(raw.h, mu, pp) == 0, raw.error()
        assert raw.start(x0) == 0, raw.error()
        x, lnl, chi2 = raw.state()[:3]
        assert same_bytes(x, x0)

        def metropolis(dz, lu, first):
            rc, m = raw.metropolis(dz, lu, first)
            assert rc == 0 and m == len(dz), raw.error()
            assert raw.lib.vk_chain_set_prior(raw.h, None, None) == -1 and "awaiting vk_chain_finish" in raw.error()   # in flight
            assert raw.lib.vk_chain_set_prior(raw.h, mu, pp) == -1
            rc, hx, hl, hc = raw.finish(len(dz))
            assert rc == 0, raw.error()
            for t in range(len(dz)):                                 # the definition (victor_amd/chains.py), restated
                prop = x + dz[t]
                inside = ((prop >= raw.lo) & (prop <= raw.hi)).all(axis=1)
                l, c2 = rs9.log_likelihood_pairs(raw.batch(np.where(inside[:, None], prop, x)), raw.which)
                l = np.where(inside, l, -np.inf)
                with np.errstate(invalid="ignore"):
                    acc = lu[t] < (l + r.lnprior(prop)) - (lnl + r.lnprior(x))
                x[acc], lnl[acc], chi2[acc] = prop[acc], l[acc], c2[acc]
                assert same_bytes(hx[t], x) and same_bytes(hl[t], lnl) and same_bytes(hc[t], chi2), t
        metropolis(dz1, lu1, 0)
        rc, m = raw.stretch(z, lz, logu, k, first=5)
        assert rc == 0 and m == 4, raw.error()
        assert raw.lib.vk_chain_set_prior(raw.h, None, None) == -1                       # in flight
        rc, hx, hl, hc = raw.finish(4)
        assert rc == 0, raw.error()
        which = np.repeat(np.arange(9, dtype=np.int32), 4)
        for t in range(4):                                           # the stretch definition, restated
            for h in range(2):
                mv = (np.arange(9)[:, None] * 8 + 4 * h + np.arange(4)).ravel()
                p = x[np.repeat(np.arange(9) * 8 + 4 * (1 - h), 4) + k[t, h]]
                prop = p + z[t, h][:, None] * (x[mv] - p)
                inside = ((prop >= raw.lo) & (prop <= raw.hi)).all(axis=1)
                l, c2 = rs9.log_likelihood_pairs(raw.batch(np.where(inside[:, None], prop, x[mv])), which)
                l = np.where(inside, l, -np.inf)
                with np.errstate(invalid="ignore"):
                    acc = logu[t, h] < (lz[t, h] + (l + r.lnprior(prop))) - (lnl[mv] + r.lnprior(x[mv]))
                x[mv[acc]], lnl[mv[acc]], chi2[mv[acc]] = prop[acc], l[acc], c2[acc]
            assert same_bytes(hx[t], x) and same_bytes(hl[t], lnl) and same_bytes(hc[t], chi2), t
        metropolis(dz2, lu2, 9)
        end = raw.state()
        assert same_bytes(end[0], x) and same_bytes(end[1], lnl) and np.all(end[4] == 15) and end[3].sum() > 0
    finally:
        raw.close()


def test_fit_handle_refusals(rs9):
    """vk_fit_set_prior on a live handle: a value that is not finite and a single NULL are refused, NULL NULL clears."""
    from victor_amd.fitting import _Sampled
    q = _Sampled("best_fit", "fitted", PARAMS, EPS_FIXED)
    x0 = np.tile([0.47, 0.4, 380.0], (9, 1))
    batch = dict({k: float(v) for k, v in q.fixed_all.items()}, **{n: np.ascontiguousarray(x0[:, j]) for j, n in enumerate(q.names)})
    lib, h, _ = q.create("vk_fit_create", rs9.fit, rs9, {}, q.fit_options(rs9.fit, {}), batch, np.arange(9, dtype=np.int32))
    try:
        r = resolved(boss_prior(), q.names)
        dp = C.POINTER(C.c_double)
        bad = r.mu.copy()
        bad[2] = np.inf
        assert lib.vk_fit_set_prior(h, bad.ctypes.data_as(dp), r.pp.ctypes.data_as(dp)) == -1
        assert b"not finite" in lib.vk_fit_last_error(h)
        assert lib.vk_fit_set_prior(h, None, r.pp.ctypes.data_as(dp)) == -1 and b"both" in lib.vk_fit_last_error(h)
        assert lib.vk_fit_set_prior(h, r.mu.ctypes.data_as(dp), r.pp.ctypes.data_as(dp)) == 0
        assert lib.vk_fit_set_prior(h, None, None) == 0
    finally:
        lib.vk_fit_destroy(h)
