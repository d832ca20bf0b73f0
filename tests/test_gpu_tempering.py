"""Replica exchange stepped on the GPU (``temper=`` of ``sample_chains``; vk_chain_set_tempering / vk_chain_begin_tempered /
vk_chain_tempering; vk_kernel_temper.h) against the NumPy loop that defines it (``device=False``,
victor_amd/tempering.py): with epsilon fixed both routes launch the same rows, so positions, log-likelihoods, the history of every
rung, every counter and the energy sums are compared byte for byte - with and without a Gaussian prior, on realisations and on the
data vector, K even and odd, a joint fit; the cold rung's histograms and series; a ladder of one rung against the plain chains;
epsilon sampled at the bounds of tests/test_gpu_chains.py; every kept sample of every rung against ``log_likelihood_pairs``; and
the refusals of the C entry points.  The shapes are the smallest that reach every path: 3 problems x 4 (3) rungs x 4 walkers = 48
(36) chains - a partial wave -, 130 steps = two blocks of 64 and two steps, burn 10, thin 2; swap_every = 3 puts events of both
parities inside the blocks (after steps 2, 5, ..., 128), swap_every = 4 (the three-rung ladder) puts one behind the last step of a
block (step 63), where the rows that follow the swap are the next block's first.  No assertion is on elapsed time."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_chains import MARGIN
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
FIXED = {"epsilon": 1.0, "sigma_v": 380.0}            # d = 2: fsigma8 and beta, the kinked direction
LADDER4 = {"betas": [1.0, 0.5, 0.1, 0.0], "swap_every": 3}
LADDER3 = {"betas": [1.0, 0.3, 0.0], "swap_every": 4}
RUN = dict(walkers=4, seed=2, burn=10, thin=2, fixed=FIXED)
PUBLIC = ("pivot", "chain", "x", "lnl", "chi2", "n_accept", "acceptance", "lnl_chain", "chi2_chain", "rhat")
RUNGS = ("x", "lnl", "chi2", "chain", "lnl_chain", "chi2_chain", "pivot_e", "e1", "e2", "n_e", "n_swap_try", "n_swap_acc", "acceptance",
         "swap_acceptance", "n_not_finite", "mean_lnl", "var_lnl", "ln_evidence", "ln_evidence_trapezoid", "ln_evidence_error")
# Seed of the epsilon-sampled comparison: the first of 0, 1, 2, ... whose smallest decision margin on the definition route exceeds
# MARGIN, picked with the definition route alone before the device route was looked at.
SEED_EPSILON = 0         # observed smallest margin 2.2e-3 (seeds 1 .. 3: 9.5e-3, 1.4e-2, 1.2e-2)


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fit():
    import victor_amd
    return victor_amd.CCFFit(*stack_options())


@pytest.fixture(scope="module")
def rs3(fit):
    return fit.realisations([0, 1, 2])


@pytest.fixture(scope="module")
def single_fits():
    import victor_amd
    made = {}

    def get(m):
        if m not in made:
            made[m] = victor_amd.CCFFit(*stack_options(simulation_number=m))
        return made[m]
    return get


def prior2():
    from victor_amd import GaussianPrior
    return GaussianPrior(["beta", "fsigma8"], [0.42, 0.45], cov=[[0.0025, 0.0005], [0.0005, 0.0025]])


def same_tempered(dev, ref, what):
    """Two routes' tempered runs: the cold rung's public fields and every rung's state, history, counters and energy sums."""
    assert dev.n_steps == ref.n_steps and dev.n_kept == ref.n_kept and dev.chain.shape == ref.chain.shape, what
    for a in PUBLIC:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)
    for a in RUNGS:
        assert same_bytes(getattr(dev.tempering, a), getattr(ref.tempering, a)), (what, "tempering." + a)
    for a in ("_n_accept", "_n_kept"):
        assert np.array_equal(getattr(dev, a), getattr(ref, a)), (what, a)


def exercised(ref, K, n_steps, swap_every, what):
    """The definition route's run reached what the test is about (a condition on the inputs, not on the code under test)."""
    q = ref.tempering
    events = n_steps // swap_every
    assert np.all(q.n_swap_try[:, 0] == (events + 1) // 2) and np.all(q.n_swap_try[:, K - 1] == 0), what
    if K > 2:
        assert np.all(q.n_swap_try[:, 1] == events // 2), what
    acc = q.n_swap_acc.sum(axis=(0, 2))[:K - 1] / q.n_swap_try.sum(axis=(0, 2))[:K - 1]
    print(what, "acceptance per rung", q.acceptance.mean(axis=0), "swap acceptance", acc, "margin", ref.decision_margin)
    assert np.all(acc > 0.0) and np.all(acc < 1.0), (what, acc)        # both outcomes of a swap, between every pair of rungs
    assert np.all((0.0 < q.acceptance) & (q.acceptance < 1.0)), (what, q.acceptance)
    assert ref._n_outside.sum() > 0, "no proposal left the box: the test does not reach that rule"
    assert np.all(q.n_e == ref.n_kept), what                            # every kept lnL was finite and entered the sums


# ------------------------------------------------------------------ 1. the device route is the definition route --------------
@pytest.fixture(scope="module")
def dev4(rs3):
    """The device route's 130 steps of the 48 chains, computed once."""
    return rs3.sample_chains(PARAMS, 130, temper=LADDER4, **RUN)


@pytest.fixture(scope="module")
def ref4(rs3):
    return rs3.sample_chains(PARAMS, 130, device=False, temper=LADDER4, **RUN)


def test_device_route_is_the_definition_route_bit_for_bit(dev4, ref4):
    dev, ref = dev4, ref4
    assert dev.names == ["fsigma8", "beta"] and dev.chain.shape == (60, 3, 4, 2) and dev.tempering.chain.shape == (60, 3, 4, 4, 2)
    exercised(ref, 4, 130, 3, "K = 4")
    same_tempered(dev, ref, "K = 4")
    assert same_bytes(dev.tempering.chain[:, :, 0], dev.chain) and same_bytes(dev.tempering.x[:, 0], dev.x)
    assert dev.decision_margin is None and ref.decision_margin is not None


def test_with_a_gaussian_prior(rs3, ref4):
    ref = rs3.sample_chains(PARAMS, 130, device=False, temper=LADDER4, prior=prior2(), **RUN)
    dev = rs3.sample_chains(PARAMS, 130, temper=LADDER4, prior=prior2(), **RUN)
    exercised(ref, 4, 130, 3, "K = 4 under a prior")
    same_tempered(dev, ref, "K = 4 under a prior")
    assert same_bytes(dev.lnprior_chain, ref.lnprior_chain) and np.all(dev.lnprior_chain < 0.0)
    assert not same_bytes(ref.tempering.chain, ref4.tempering.chain), "the prior changed no decision: the test does not reach it"


def test_an_odd_number_of_rungs(rs3):
    ref = rs3.sample_chains(PARAMS, 130, device=False, temper=LADDER3, **RUN)
    dev = rs3.sample_chains(PARAMS, 130, temper=LADDER3, **RUN)
    assert dev.tempering.chain.shape == (60, 3, 3, 4, 2)
    exercised(ref, 3, 130, 4, "K = 3")
    same_tempered(dev, ref, "K = 3")


def test_data_vector():
    import victor_amd
    data_fit = victor_amd.CCFFit(*cases.boss_options("config"))
    ref = data_fit.sample_chains(PARAMS, 130, device=False, temper=LADDER4, **RUN)
    dev = data_fit.sample_chains(PARAMS, 130, temper=LADDER4, **RUN)
    assert dev.chain.shape == (60, 1, 4, 2) and dev.tempering.x.shape == (1, 4, 4, 2)
    exercised(ref, 4, 130, 3, "data vector")
    same_tempered(dev, ref, "data vector")


# ------------------------------------------------------------------ 2. a ladder of one rung is the plain chains --------------
def test_a_ladder_of_one_rung_is_the_plain_device_chains(rs3):
    plain = rs3.sample_chains(PARAMS, 130, **RUN)
    one = rs3.sample_chains(PARAMS, 130, temper={"betas": [1.0]}, **RUN)
    for a in PUBLIC + ("sum1", "sum2", "mean", "cov"):
        assert same_bytes(getattr(one, a), getattr(plain, a)), a
    assert plain.tempering is None and one.tempering.n_swap_try.sum() == 0 and np.all(one.tempering.n_e == one.n_kept)


# ------------------------------------------------------------------ 3. epsilon sampled ----------------------------------------
def test_device_route_with_epsilon_sampled(rs3, single_fits):
    kw = dict(walkers=2, seed=SEED_EPSILON, burn=4, thin=3, temper=LADDER3)
    ref = rs3.sample_chains(PARAMS, 70, device=False, **kw)
    print("smallest decision margin (definition route, tempered):", ref.decision_margin)
    assert ref.decision_margin > MARGIN, ref.decision_margin            # a condition on the inputs, not on the code under test
    dev = rs3.sample_chains(PARAMS, 70, **kw)
    assert dev.names == ["fsigma8", "beta", "sigma_v", "epsilon"] and dev.tempering.chain.shape == (22, 3, 3, 2, 4)
    for a in ("pivot", "chain", "x", "n_accept", "acceptance"):
        assert same_bytes(getattr(dev, a), getattr(ref, a)), a
    for a in ("x", "chain", "n_e", "n_swap_try", "n_swap_acc", "acceptance"):
        assert same_bytes(getattr(dev.tempering, a), getattr(ref.tempering, a)), a
    hist = ref.tempering.chain                                           # (n, R, K, W, d)
    n = len(hist)
    bound = np.empty(hist.shape[:-1])
    for m in range(3):
        x = hist[:, m].reshape(-1, 4)
        bound[:, m] = chi2_bound(single_fits(m), {name: x[:, j] for j, name in enumerate(dev.names)}).reshape(n, 3, 2)
    assert_same_chi2(dev.tempering.chi2_chain, ref.tempering.chi2_chain, bound, what="tempered chains: device vs definition route")
    assert_same_lnl(dev.tempering.lnl_chain, ref.tempering.lnl_chain, bound, what="tempered chains: device vs definition route")


# ------------------------------------------------------------------ 4. the cold rung's histograms and series ------------------
def test_cold_rung_marginals_and_autocorr(rs3):
    kw = dict(RUN, temper=LADDER3, marginals={"bins": 16, "pairs": "all", "bins2d": 8}, autocorr={"max_lag": 16})
    ref = rs3.sample_chains(PARAMS, 70, device=False, **kw)
    dev = rs3.sample_chains(PARAMS, 70, **kw)
    same_tempered(dev, ref, "with marginals and autocorr")
    m, w = dev.marginals, ref.marginals
    assert np.array_equal(m.n, w.n) and np.all(m.n == dev.n_kept * 4)
    for name in dev.names:
        assert np.array_equal(m.counts[name], w.counts[name]) and m.counts[name].shape == (3, 16)
        assert np.array_equal(m.below[name], w.below[name]) and np.array_equal(m.above[name], w.above[name])
        # the cold rung's own histogram: every kept position of its W chains once, nothing of the hotter rungs
        assert np.array_equal(m.counts[name].sum(axis=1) + m.below[name] + m.above[name], np.full(3, dev.n_kept * 4))
    for key in m.counts2d:
        assert np.array_equal(m.counts2d[key], w.counts2d[key])
    a, b = dev.autocorr, ref.autocorr
    assert a.n == b.n == dev.n_kept and a.tau.shape == (3, 2)
    for k in a.state:
        assert same_bytes(a.state[k], b.state[k]), k
    for k in ("tau", "window", "ess", "acf"):
        assert same_bytes(getattr(a, k), getattr(b, k)), k


# ------------------------------------------------------------------ 5. a joint fit -------------------------------------------
def test_joint_realisations(tmp_path_factory):
    from tests.test_gpu_joint_sampled import Case
    c = Case("dsplit_cov", tmp_path_factory.mktemp("temper_dsplit_cov"))
    kw = dict(walkers=2, seed=2, burn=3, thin=2, fixed=dict(c.fixed, epsilon=1.0), temper={"betas": [1.0, 0.2], "swap_every": 3})
    ref = c.jr.sample_chains(PARAMS, 70, device=False, **kw)
    dev = c.jr.sample_chains(PARAMS, 70, **kw)
    R = len(c.jr)
    assert dev.names == c.without("epsilon") and dev.tempering.chain.shape == (34, R, 2, 2, 2)
    q = ref.tempering
    assert np.all(q.n_swap_try[:, 0] == 12) and np.all(q.n_swap_try[:, 1] == 0) and 0 < q.n_swap_acc.sum() < q.n_swap_try.sum()
    same_tempered(dev, ref, "joint realisations")
    assert np.all(np.isnan(dev.tempering.ln_evidence))                   # the ladder does not reach beta = 0


# ------------------------------------------------------------------ 6. every kept sample is what the likelihood says ---------
def test_every_kept_sample_of_every_rung_is_what_the_likelihood_says(rs3, single_fits, dev4):
    q = dev4.tempering
    n, R, K, W, d = q.chain.shape
    t, m, k, w = (a.ravel() for a in np.indices((n, R, K, W)))
    x = q.chain[t, m, k, w]
    pts = {name: np.ascontiguousarray(x[:, j]) for j, name in enumerate(dev4.names)}
    pts.update({name: np.full(len(x), v) for name, v in FIXED.items()})
    lnl, chi2 = rs3.log_likelihood_pairs(pts, m.astype(np.int32))
    bound = np.empty(len(t))
    for r in range(R):
        bound[m == r] = chi2_bound(single_fits(r), {name: v[m == r] for name, v in pts.items()})
    assert_same_chi2(q.chi2_chain[t, m, k, w], chi2, bound, what="tempered kept samples vs log_likelihood_pairs")
    assert_same_lnl(q.lnl_chain[t, m, k, w], lnl, bound, what="tempered kept samples vs log_likelihood_pairs")
    # the final state as well: what the last swap left belongs together
    xs = q.x.reshape(-1, d)
    pts = {name: np.ascontiguousarray(xs[:, j]) for j, name in enumerate(dev4.names)}
    pts.update({name: np.full(len(xs), v) for name, v in FIXED.items()})
    which = np.repeat(np.arange(R, dtype=np.int32), K * W)
    lnl, chi2 = rs3.log_likelihood_pairs(pts, which)
    bound = np.concatenate([chi2_bound(single_fits(r), {name: v[which == r] for name, v in pts.items()}) for r in range(R)])
    assert_same_lnl(q.lnl.ravel(), lnl, bound, what="tempered final state vs log_likelihood_pairs")
    assert_same_chi2(q.chi2.ravel(), chi2, bound, what="tempered final state vs log_likelihood_pairs")


# ------------------------------------------------------------------ 7. the C entry points ------------------------------------
def begin_tempered(raw, dz, logu, logs, swap_every, first):
    dp = C.POINTER(C.c_double)
    kept = C.c_int32(-1)
    ptr = [None if a is None else a.ctypes.data_as(dp) for a in (dz, logu, logs)]
    return raw.lib.vk_chain_begin_tempered(raw.h, len(logu), *ptr, swap_every, first, 0, 1, 1, C.byref(kept)), kept.value


def set_tempering(raw, rungs, walkers, betas):
    b = None if betas is None else np.ascontiguousarray(betas, dtype=np.float64)
    return raw.lib.vk_chain_set_tempering(raw.h, rungs, walkers, None if b is None else b.ctypes.data_as(C.POINTER(C.c_double)))


def read_tempering(raw):
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    f = [np.empty(raw.C) for _ in range(3)]
    n = [np.empty(raw.C, dtype=np.int64) for _ in range(3)]
    rc = raw.lib.vk_chain_tempering(raw.h, *[a.ctypes.data_as(dp) for a in f], *[a.ctypes.data_as(lp) for a in n])
    return rc, f, n


def test_c_abi_refusals_leave_the_handle_usable_and_clearing_restores_the_plain_bytes(rs3):
    from tests.test_gpu_stretch import Raw
    width = np.array([PARAMS[n]["proposal"] for n in ("fsigma8", "beta", "sigma_v")], dtype=float)
    rng = np.random.default_rng(4)
    x0 = np.array([PARAMS[n]["ref"]["loc"] for n in ("fsigma8", "beta", "sigma_v")], dtype=float) + 0.5 * width * rng.standard_normal((48, 3))
    dz, lu, ls = width * rng.standard_normal((6, 48, 3)), np.log(rng.random((6, 48))), np.log(rng.random((6, 48)))
    betas = [1.0, 0.5, 0.1, 0.0]
    plain = Raw(rs3, x0, 16)
    raw = Raw(rs3, x0, 16)                                   # 16 chains per realisation: K W = 16 is one problem per realisation
    try:
        def refused(text, rc):
            assert rc == -1 and text in raw.error(), (text, rc, raw.error())
        refused("has no tempering", begin_tempered(raw, dz, lu, ls, 3, 0)[0])
        refused("has no tempering", read_tempering(raw)[0])
        refused("not a whole number of problems", set_tempering(raw, 3, 5, [1.0, 0.5, 0.0]))        # 48 % 15 != 0
        refused("not a whole number of problems", set_tempering(raw, 7, 7, np.linspace(1, 0, 7)))  # 49 > 48
        refused("need rungs >= 1 and walkers >= 1", set_tempering(raw, 4, 0, betas))
        refused("need rungs >= 1 and walkers >= 1", set_tempering(raw, -1, 4, betas))
        refused("NULL argument", set_tempering(raw, 4, 4, None))
        refused("betas[0] must be 1", set_tempering(raw, 4, 4, [0.9, 0.5, 0.1, 0.0]))
        refused("decrease strictly", set_tempering(raw, 4, 4, [1.0, 0.5, 0.5, 0.0]))
        refused("decrease strictly", set_tempering(raw, 4, 4, [1.0, 0.1, 0.5, 0.0]))
        refused("not finite and >= 0", set_tempering(raw, 4, 4, [1.0, 0.5, 0.1, -0.1]))
        refused("not finite and >= 0", set_tempering(raw, 4, 4, [1.0, np.nan, 0.1, 0.0]))
        refused("not of the realisation", set_tempering(raw, 2, 12, [1.0, 0.0]))                   # a problem of 24 chains spans two
        assert set_tempering(raw, 4, 4, betas) == 0, raw.error()
        refused("no start", begin_tempered(raw, dz, lu, ls, 3, 0)[0])
        assert raw.start(x0) == 0 and plain.start(x0) == 0, raw.error()
        refused("NULL argument", begin_tempered(raw, dz, lu, None, 3, 0)[0])
        refused("swap_every >= 0", begin_tempered(raw, dz, lu, ls, -1, 0)[0])
        rc, m = begin_tempered(raw, dz, lu, ls, 2, 0)
        assert rc == 0 and m == 6, raw.error()
        refused("awaiting vk_chain_finish", set_tempering(raw, 4, 4, betas))                       # a block in flight
        refused("awaiting vk_chain_finish", read_tempering(raw)[0])
        refused("has not been finished", begin_tempered(raw, dz, lu, ls, 2, 6)[0])
        rc, hx, hl, hc = raw.finish(6)
        assert rc == 0, raw.error()
        rc, (pivot_e, e1, e2), (n_e, n_try, n_acc) = read_tempering(raw)
        assert rc == 0 and np.all(n_e == 6) and same_bytes(pivot_e, hl[0]), raw.error()
        s1, s2 = np.zeros(48), np.zeros(48)
        for t in range(6):                                   # the sums in step order, each product rounded before its sum
            a = hl[t] - hl[0]
            s1, s2 = s1 + a, s2 + a * a
        assert same_bytes(e1, s1) and same_bytes(e2, s2)
        rung = (np.arange(48) // 4) % 4
        assert np.all(n_try[rung == 0] == 2) and np.all(n_try[rung == 1] == 1) and np.all(n_try[rung == 2] == 2) and np.all(n_try[rung == 3] == 0)
        assert np.all(n_acc <= n_try) and n_acc.sum() > 0
        # vk_chain_start zeroes the sums and the counters again; NULL swap levels are allowed without swaps
        assert raw.start(x0) == 0, raw.error()
        rc, _, (n_e, n_try, n_acc) = read_tempering(raw)
        assert rc == 0 and not n_e.any() and not n_try.any() and not n_acc.any()
        rc, m = begin_tempered(raw, dz, lu, None, 0, 0)
        assert rc == 0 and raw.finish(m)[0] == 0, raw.error()
        assert read_tempering(raw)[2][1].sum() == 0
        # cleared: the launches and the bytes of a handle that never had it
        assert set_tempering(raw, 0, 0, None) == 0, raw.error()
        refused("has no tempering", begin_tempered(raw, dz, lu, ls, 3, 0)[0])
        assert raw.start(x0) == 0, raw.error()
        for h in (raw, plain):
            rc, m = h.metropolis(dz, lu, 0)
            assert rc == 0 and m == 6, h.error()
        a, b = raw.finish(6), plain.finish(6)
        assert a[0] == 0 and b[0] == 0
        for u, v in zip(a[1:], b[1:]):
            assert same_bytes(u, v)
        for u, v in zip(raw.state(), plain.state()):
            assert same_bytes(u, v)
        assert b[1].std(axis=0).min() > 0                                # the chains moved
    finally:
        raw.close()
        plain.close()
