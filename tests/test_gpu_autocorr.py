"""The ensemble series and its lagged products on the GPU (``autocorr=`` of ``sample_chains``; vk_chain_set_autocorr /
vk_chain_autocorr; vk_chain_series_kernel): the state the series kernel accumulates against the definition
route's (``device=False``) and against the NumPy statement of the update applied to the run's own history - doubles, compared
byte for byte: every rounding of the statistic is fixed -, for both moves, single and joint handles, with and without a prior,
histograms or a history, across cuts; the rest of a run is byte for byte the run without ``autocorr=``; and the handle: what
vk_chain_start resets, set-and-clear, the refusals.

Fixtures and shapes are those of tests/test_gpu_marginals.py: the BOSS golden configuration with nine realisations x 8 chains (72
chains: a partial wave, two workgroups of the step kernel), 70 steps across the block of 64; one fit x 72 chains (two rows of the
lane sum, the second partial); the five density-split blocks with ``"sigma_v@q"``.  L = 16 with 33 kept steps: the ring wraps.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests.test_autocorr import FIELDS, rebuilt, same_state
from tests.test_chains import same_bytes
from tests.test_gpu_marginals import OPTION as HISTOGRAMS
from tests.test_gpu_marginals import OPTION_NARROW as HISTOGRAMS_NARROW
from tests.test_gpu_marginals import SUMS
from tests.test_gpu_priors import BETA, JOINT_NAMES, METRO, NARROW, PARAMS, STRETCH, Five, blocked, boss_prior, same_run
from tests.test_gpu_stretch import Raw, stretch_numbers
from tests.test_marginals import same_marginals
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
NAMES = ["fsigma8", "beta", "sigma_v"]
OPTION = {"max_lag": 16, "c": 5.0}


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
def rs9(fit):
    """Nine realisations: with W = 8, 72 chains - a partial wave, two workgroups."""
    return fit.realisations(list(range(9)))


def check_run(dev, ref, what):
    """Device state == the definition route's == the update applied to the device run's own history."""
    same_run(dev, ref, what)
    same_state(dev.autocorr, ref.autocorr, what)
    own = rebuilt(dev.chain, dev.autocorr.max_lag)
    same_state(dev.autocorr, own, what + ", own history")
    ac = dev.autocorr
    R, d, L = dev.R, len(dev.names), ac.max_lag
    assert ac.n == dev.n_kept and ac.tau.shape == (R, d) and ac.acf.shape == (R, d, L) and ac.names == dev.names
    assert np.all(ac.acf[:, :, 0] == 1.0) and np.all(ac.state["acc"][:, :, 0] > 0.0), "a series never moved"
    for k in ("tau", "window", "ess", "reached", "acf"):                                    # the read-out of equal states
        assert same_bytes(getattr(ac, k), getattr(ref.autocorr, k)), (what, k)


# ------------------------------------------------------------------ 1. Metropolis, single fit --------------------------------
@pytest.fixture(scope="module")
def metro_dev(rs9):
    """The device route's 70 Metropolis steps of the 72 chains with the series on, computed once."""
    return rs9.sample_chains(PARAMS, 70, autocorr=OPTION, **METRO)


def test_metropolis_state_is_the_definition_routes(rs9, metro_dev):
    dev = metro_dev
    ref = rs9.sample_chains(PARAMS, 70, device=False, autocorr=OPTION, **METRO)
    assert dev.names == NAMES and dev.chain.shape == (33, 9, 8, 3)                # steps 5, 7, .. 69: across the block of 64
    assert dev.autocorr.n == 33 and dev.autocorr.state["ring"].shape == (9, 3, 16)    # 33 > 2 L: the ring has wrapped twice
    check_run(dev, ref, "metropolis")
    print("tau:", dev.autocorr.tau.tolist(), "reached:", dev.autocorr.reached.tolist())
    plain = rs9.sample_chains(PARAMS, 70, **METRO)
    assert plain.autocorr is None
    same_run(dev, plain, "autocorr changes nothing else", SUMS)


# ------------------------------------------------------------------ 2. one fit x 72 chains: two rows of the lane sum ---------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_one_problem_of_72_chains(fit, move):
    kw = dict(walkers=72, seed=2, burn=5, thin=2, fixed={"epsilon": 1.0}, move=move, autocorr=OPTION)
    dev = fit.sample_chains(PARAMS, 70, **kw)
    ref = fit.sample_chains(PARAMS, 70, device=False, **kw)
    assert dev.chain.shape == (33, 1, 72, 3) and dev.autocorr.state["acc"].shape == (1, 3, 16)
    check_run(dev, ref, f"W = 72, {move}")


# ------------------------------------------------------------------ 3. stretch, the 72 walkers in the narrowed box -----------
@pytest.fixture(scope="module")
def stretch_dev(rs9):
    return rs9.sample_chains(NARROW, 70, autocorr=OPTION, **STRETCH)


def test_stretch_state_is_the_definition_routes(rs9, stretch_dev):
    dev = stretch_dev
    ref = rs9.sample_chains(NARROW, 70, device=False, autocorr=OPTION, **STRETCH)
    assert dev.chain.shape == (22, 9, 8, 3) and dev.move == "stretch" and dev.rhat is None      # sweeps 5, 8, .. 68
    assert ref.n_outside.sum() > 0, "no proposal left the box: the test does not reach that rule"
    check_run(dev, ref, "stretch")
    plain = rs9.sample_chains(NARROW, 70, **STRETCH)
    same_run(dev, plain, "autocorr changes nothing else", SUMS)


# ------------------------------------------------------------------ 4. epsilon sampled ---------------------------------------
@pytest.mark.parametrize("move,walkers", [("metropolis", 4), ("stretch", 10)])
def test_epsilon_sampled_state_is_that_of_the_runs_own_history(fit, move, walkers):
    """With epsilon sampled the two routes agree to rounding only, so the device's state is held against the update applied to
    the positions the device itself kept."""
    rs = fit.realisations([0, 1, 2])
    dev = rs.sample_chains(PARAMS, 70, walkers=walkers, seed=1, move=move, burn=5, thin=2, autocorr=OPTION)
    assert dev.names == NAMES + ["epsilon"] and dev.chain.shape == (33, 3, walkers, 4)
    same_state(dev.autocorr, rebuilt(dev.chain, 16), f"epsilon sampled, {move}")
    assert dev.autocorr.state["head"].shape == (3, 4, 16) and np.all(dev.autocorr.state["acc"][:, :, 0] > 0.0)


# ------------------------------------------------------------------ 5. without a history -------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_keep_chain_false_gives_the_same_state(rs9, metro_dev, stretch_dev, move):
    kept, block, kw = (metro_dev, PARAMS, METRO) if move == "metropolis" else (stretch_dev, NARROW, STRETCH)
    bare = rs9.sample_chains(block, 70, keep_chain=False, autocorr=OPTION, **kw)
    assert bare.chain is None and bare.rhat is None
    same_state(bare.autocorr, kept.autocorr, f"keep_chain=False, {move}")
    for a in ("x", "lnl", "n_accept", "sum1", "sum2", "mean", "cov"):
        assert same_bytes(getattr(bare, a), getattr(kept, a)), a
    assert same_bytes(bare.autocorr.tau, kept.autocorr.tau) and same_bytes(bare.autocorr.ess, kept.autocorr.ess)


# ------------------------------------------------------------------ 6. cut runs -----------------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_a_cut_run_keeps_what_the_uncut_run_keeps(rs9, metro_dev, stretch_dev, move):
    whole, block, kw = (metro_dev, PARAMS, METRO) if move == "metropolis" else (stretch_dev, NARROW, STRETCH)
    cut = rs9.sample_chains(block, 0, autocorr=OPTION, **kw)
    assert cut.autocorr.n == 0 and not any(cut.autocorr.state[k].any() for k in FIELDS) and np.all(np.isnan(cut.autocorr.tau))
    cut.extend(40)
    part = cut.autocorr
    cut.extend(30)                                                                 # across the block of 64
    same_run(cut, whole, f"40 + 30, {move}", SUMS)
    same_state(cut.autocorr, whole.autocorr, f"40 + 30, {move}")
    assert 0 < part.n < whole.autocorr.n and cut.autocorr is not part              # (rebuilt after every extend)
    same_state(part, rebuilt(cut.chain[:part.n], 16), "the first piece")


# ------------------------------------------------------------------ 7. and 10. the handle ------------------------------------
def read_autocorr(raw, R, L):
    dp = C.POINTER(C.c_double)
    out = {"pivot": np.full((R, raw.d), -1.0), "total": np.full((R, raw.d), -1.0), "head": np.full((R, raw.d, L), -1.0),
           "ring": np.full((R, raw.d, L), -1.0), "acc": np.full((R, raw.d, L), -1.0)}
    n = C.c_int64(-1)
    assert raw.lib.vk_chain_autocorr(raw.h, *(out[k].ctypes.data_as(dp) for k in FIELDS), C.byref(n)) == 0, raw.error()
    return out, n.value


def state_of(hx, R, W, L):
    """The state of positions hx (m, R W, d), step by step."""
    return rebuilt(hx.reshape(len(hx), R, W, hx.shape[-1]), L)


def assert_state(got, n, want):
    assert n == want.n
    for k in FIELDS:
        assert same_bytes(got[k], getattr(want, k)), k


def test_start_zeroes_and_clear_restores(rs9, metro_dev):
    x0 = np.ascontiguousarray(metro_dev.pivot.reshape(72, 3))
    rng = np.random.default_rng(4)
    width = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
    dz, lu = width * rng.standard_normal((6, 72, 3)), np.log(rng.random((6, 72)))
    z, lz, logu, k = stretch_numbers(rng, 3, 36, 4, 3)
    out = []
    for mode in ("never", "cleared", "set"):
        raw = Raw(rs9, x0, 8)
        try:
            if mode != "never":
                assert raw.lib.vk_chain_set_autocorr(raw.h, 8, 4) == 0, raw.error()
            if mode == "cleared":
                assert raw.lib.vk_chain_set_autocorr(raw.h, 0, 0) == 0, raw.error()
            assert raw.start(x0) == 0, raw.error()
            rc, m = raw.metropolis(dz, lu, 0)
            assert rc == 0 and m == 6, raw.error()
            got = list(raw.finish(6)[1:])
            if mode == "set":
                first = read_autocorr(raw, 9, 4)
                assert_state(*first, state_of(got[0], 9, 8, 4))                   # six steps, four lags: the ring has wrapped
            rc, m = raw.stretch(z, lz, logu, k, first=6)
            assert rc == 0 and m == 3, raw.error()
            hx = raw.finish(3)
            assert hx[0] == 0, raw.error()
            got += list(hx[1:]) + list(raw.state())
            out.append(got)
            if mode == "set":
                # Metropolis and stretch blocks add to the same series
                assert_state(*read_autocorr(raw, 9, 4), state_of(np.concatenate([got[0], hx[1]]), 9, 8, 4))
                # any pointer may be NULL
                dp = C.POINTER(C.c_double)
                acc, n = np.empty((9, 3, 4)), C.c_int64(-1)
                assert raw.lib.vk_chain_autocorr(raw.h, None, None, None, None, acc.ctypes.data_as(dp), None) == 0, raw.error()
                assert raw.lib.vk_chain_autocorr(raw.h, None, None, None, None, None, C.byref(n)) == 0 and n.value == 9
                # a second start: fresh chains, fresh series - and the same numbers give the same state again
                assert raw.start(x0) == 0, raw.error()
                zero, n0 = read_autocorr(raw, 9, 4)
                assert n0 == 0 and not any(zero[f].any() for f in FIELDS)
                rc, m = raw.metropolis(dz, lu, 0)
                assert rc == 0 and m == 6, raw.error()
                assert raw.finish(6)[0] == 0
                again = read_autocorr(raw, 9, 4)
                assert again[1] == first[1] and all(same_bytes(again[0][f], first[0][f]) for f in FIELDS)
            else:
                assert raw.lib.vk_chain_autocorr(raw.h, None, None, None, None, None, None) == -1 and "has no autocorrelation" in raw.error()
        finally:
            raw.close()
    for u, v, w in zip(*out):                                        # never set == set and cleared == set: the series decide nothing
        assert same_bytes(u, v) and same_bytes(u, w)


def test_live_refusals_leave_the_handle_usable(rs9, metro_dev):
    x0 = np.ascontiguousarray(metro_dev.pivot.reshape(72, 3))
    rng = np.random.default_rng(6)
    width = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
    dz, lu = width * rng.standard_normal((4, 72, 3)), np.log(rng.random((4, 72)))
    raw = Raw(rs9, x0, 8)
    try:
        def refused(text, group, L):
            assert raw.lib.vk_chain_set_autocorr(raw.h, group, L) == -1 and text in raw.error(), (text, raw.error())
        refused("not a whole number of groups", 7, 16)                         # 72 % 7 != 0
        refused("not a whole number of groups", 0, 16)
        refused("not a whole number of groups", -8, 16)
        refused("max_lag", 8, 1025)
        refused("max_lag", 8, -1)
        assert raw.lib.vk_chain_autocorr(raw.h, None, None, None, None, None, None) == -1 and "has no autocorrelation" in raw.error()
        assert raw.start(x0) == 0, raw.error()
        assert raw.lib.vk_chain_set_autocorr(raw.h, 8, 1024) == 0, raw.error()   # the largest lag count
        assert raw.lib.vk_chain_set_autocorr(raw.h, 8, 3) == 0, raw.error()      # a second call replaces the state
        rc, m = raw.metropolis(dz, lu, 0)
        assert rc == 0 and m == 4, raw.error()
        refused("awaiting vk_chain_finish", 8, 3)                              # a block in flight
        refused("awaiting vk_chain_finish", 0, 0)
        assert raw.lib.vk_chain_autocorr(raw.h, None, None, None, None, None, None) == -1 and "awaiting vk_chain_finish" in raw.error()
        rc, hx, hl, hc = raw.finish(4)
        assert rc == 0, raw.error()
        refused("not a whole number of groups", 7, 3)                          # a refusal keeps the state the handle had
        refused("max_lag", 8, 2000)
        assert_state(*read_autocorr(raw, 9, 3), state_of(hx, 9, 8, 3))
        # one group of all chains, one lag: set between blocks, the series start there
        assert raw.lib.vk_chain_set_autocorr(raw.h, 72, 1) == 0, raw.error()
        zero, n0 = read_autocorr(raw, 1, 1)
        assert n0 == 0 and zero["acc"].shape == (1, 3, 1) and not zero["acc"].any()
        rc, m = raw.metropolis(dz, lu, 4)
        assert rc == 0, raw.error()
        rc, hx2, _, _ = raw.finish(4)
        assert rc == 0, raw.error()
        assert_state(*read_autocorr(raw, 1, 1), state_of(hx2, 1, 72, 1))
    finally:
        raw.close()


# ------------------------------------------------------------------ 8. with a prior and histograms ---------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_with_a_prior_and_marginals_the_rest_is_the_run_without_autocorr(rs9, metro_dev, stretch_dev, move):
    free, block, hist, kw = (metro_dev, PARAMS, HISTOGRAMS, METRO) if move == "metropolis" else (stretch_dev, NARROW, HISTOGRAMS_NARROW, STRETCH)
    both = dict(prior=boss_prior(), marginals=hist, **kw)
    dev = rs9.sample_chains(block, 70, autocorr=OPTION, **both)
    plain = rs9.sample_chains(block, 70, **both)
    assert plain.autocorr is None
    same_run(dev, plain, f"{move}: positions, lnL, chi2, counts", SUMS)
    same_marginals(dev.marginals, plain.marginals, move)
    same_state(dev.autocorr, rebuilt(dev.chain, 16), f"{move} under a prior, with histograms")
    assert not same_bytes(dev.chain, free.chain), "the prior changed no decision: the test does not reach it"
    bare = rs9.sample_chains(block, 70, keep_chain=False, autocorr=OPTION, **both)            # everything together, no history
    same_state(bare.autocorr, dev.autocorr, f"{move}: keep_chain=False, prior, marginals")
    same_marginals(bare.marginals, dev.marginals, move)


# ------------------------------------------------------------------ 9. joint handles -----------------------------------------
@pytest.fixture(scope="module")
def five(tmp_path_factory):
    made = {}

    def get(cov):
        if cov not in made:
            made[cov] = Five(tmp_path_factory.mktemp("five_cov" if cov else "five_diag"), cov)
        return made[cov]
    return get


@pytest.mark.parametrize("cov", [True, False], ids=["joint_cov", "block_diagonal"])
@pytest.mark.parametrize("data", [True, False], ids=["data", "mocks"])
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_joint_state_is_the_definition_routes(five, cov, data, move):
    c = five(cov)
    target = c.joint if data else c.joint.realisations([0, 1, 2])
    W = 14 if move == "stretch" else 8 if data else 2          # stretch: W >= 2 (d + 1), d = 6
    n = 20 if move == "stretch" else 70                          # (70 steps cross the block of 64)
    kw = dict(walkers=W, seed=2, fixed={"beta": BETA, "epsilon": 1.0}, move=move, burn=3, thin=2, autocorr={"max_lag": 5})
    ref = target.sample_chains(blocked(), n, device=False, **kw)
    dev = target.sample_chains(blocked(), n, **kw)
    R = 1 if data else 3
    assert dev.names == JOINT_NAMES and dev.chain.shape == ((n - 3 + 1) // 2, R, W, 6)
    assert 0.02 < ref.acceptance.mean() < 0.98                   # a condition on the inputs
    check_run(dev, ref, "joint chains")
    assert dev.autocorr.state["acc"].shape == (R, 6, 5) and dev.autocorr.c == 5.0
