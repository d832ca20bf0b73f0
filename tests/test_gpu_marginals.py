"""Marginal histograms on the GPU (``marginals=`` of ``sample_chains``; vk_chain_set_marginals / vk_chain_marginals; DESIGN.md
section 7b): the counts the step kernels accumulate against the definition route's (``device=False``) and against the binning
rule restated in NumPy on the run's own history - integers, compared by equality -, for both moves, single and joint handles,
with and without a prior or a history, across cuts; the rest of a run is byte for byte the run without histograms; and the
handle: what vk_chain_start resets, set-and-clear, the refusals.

Fixtures and shapes are those of tests/test_gpu_priors.py: the BOSS golden configuration with nine realisations x 8 chains (72
chains: a partial wave, two workgroups), 70 steps across the block of 64; the five density-split blocks with ``"sigma_v@q"``.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests.test_chains import same_bytes
from tests.test_gpu_priors import BETA, HISTORY, JOINT_NAMES, METRO, NARROW, PARAMS, STRETCH, Five, blocked, boss_prior, same_run
from tests.test_gpu_stretch import Raw, stretch_numbers
from tests.test_marginals import assert_marginals, restated, same_marginals
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
SUMS = HISTORY + ("sum1", "sum2", "mean", "cov")
NAMES = ["fsigma8", "beta", "sigma_v"]
# all three parameters, two pairs; sigma_v over a range narrower than the chains' excursion (starts are drawn from N(380, 20);
# in the narrowed box of the stretch tests from N(375, 5)), so that the outside slots and the inside-both rule are reached
OPTION = {"bins": 32, "bins2d": 8, "pairs": [("fsigma8", "sigma_v"), ("fsigma8", "beta")], "range": {"sigma_v": (370.0, 390.0)}}
OPTION_NARROW = dict(OPTION, range={"sigma_v": (372.0, 378.0)})


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


def box_of(names, block):
    base = [n.partition("@")[0] for n in names]
    return (np.array([block[b]["prior"]["min"] for b in base], dtype=float), np.array([block[b]["prior"]["max"] for b in base], dtype=float))


def own_history(ch, option, block=PARAMS):
    """The binning rule restated on the run's own history."""
    return restated(ch.chain, option, ch.names, *box_of(ch.names, block))


def reaches_outside(m, name):
    print(name, "below:", m.below[name].tolist(), "above:", m.above[name].tolist(), "inside:", m.counts[name].sum(axis=1).tolist())
    assert m.below[name].sum() > 0 and m.above[name].sum() > 0, "no sample left the range: the test does not reach the outside slots"
    mine = [v for pair, v in m.counts2d.items() if name in pair]          # inside both ranges, or not counted
    assert mine and all(0 < v.sum() < m.n.sum() for v in mine)


def check_run(dev, ref, option, what, block=PARAMS):
    """Device histograms == the definition route's == the rule on the history; every kept sample is counted once.  (The moment
    sums hold products the device may contract: tests/test_gpu_chains.py bounds them, they are not compared between routes.)"""
    same_run(dev, ref, what)
    same_marginals(dev.marginals, ref.marginals, what)
    assert_marginals(dev.marginals, own_history(dev, option, block), what)
    m = dev.marginals
    assert np.all(m.n == dev.n_kept * dev.W) and m.n.shape == (dev.R,)
    for k in m.names:
        assert np.array_equal(m.counts[k].sum(axis=1) + m.below[k] + m.above[k], m.n), (what, k)


# ------------------------------------------------------------------ 5. Metropolis, single fit --------------------------------
@pytest.fixture(scope="module")
def metro_dev(rs9):
    """The device route's 70 Metropolis steps of the 72 chains with histograms, computed once."""
    return rs9.sample_chains(PARAMS, 70, marginals=OPTION, **METRO)


def test_metropolis_counts_are_the_definition_routes(rs9, metro_dev):
    dev = metro_dev
    ref = rs9.sample_chains(PARAMS, 70, device=False, marginals=OPTION, **METRO)
    assert dev.names == NAMES and dev.chain.shape == (33, 9, 8, 3)                # steps 5, 7, .. 69: across the block of 64
    m = dev.marginals
    assert m.counts["beta"].shape == (9, 32) and m.counts2d[("fsigma8", "sigma_v")].shape == (9, 8, 8) and m.n.tolist() == [264] * 9
    check_run(dev, ref, OPTION, "metropolis")
    reaches_outside(m, "sigma_v")
    # the rest of the run is the run without histograms, byte for byte
    plain = rs9.sample_chains(PARAMS, 70, **METRO)
    assert plain.marginals is None
    same_run(dev, plain, "marginals change nothing else", SUMS)


# ------------------------------------------------------------------ 6. stretch, single fit ----------------------------------
@pytest.fixture(scope="module")
def stretch_dev(rs9):
    return rs9.sample_chains(NARROW, 70, marginals=OPTION_NARROW, **STRETCH)


def test_stretch_counts_are_the_definition_routes(rs9, stretch_dev):
    dev = stretch_dev
    ref = rs9.sample_chains(NARROW, 70, device=False, marginals=OPTION_NARROW, **STRETCH)
    assert dev.chain.shape == (22, 9, 8, 3) and dev.move == "stretch"          # sweeps 5, 8, .. 68
    print("outside the box (definition route):", ref.n_outside.sum(), "of", 70 * 72)
    assert ref.n_outside.sum() > 0, "no proposal left the box: the test does not reach that rule"
    check_run(dev, ref, OPTION_NARROW, "stretch", NARROW)
    assert dev.marginals.edges["sigma_v"][0] == 372.0 and dev.marginals.edges["beta"][-1] == 0.6
    reaches_outside(dev.marginals, "sigma_v")
    plain = rs9.sample_chains(NARROW, 70, **STRETCH)
    same_run(dev, plain, "marginals change nothing else", SUMS)


# ------------------------------------------------------------------ 7. epsilon sampled ---------------------------------------
@pytest.mark.parametrize("move,walkers", [("metropolis", 4), ("stretch", 10)])
def test_epsilon_sampled_counts_are_those_of_the_runs_own_history(fit, move, walkers):
    """With epsilon sampled the two routes agree to rounding only, so the device's counts are held against the rule applied to
    the positions the device itself kept: every histogram, every pair."""
    rs = fit.realisations([0, 1, 2])
    option = {"bins": 24, "bins2d": 5, "pairs": "all", "range": {"epsilon": (0.97, 1.03), "sigma_v": (370.0, 390.0)}}
    dev = rs.sample_chains(PARAMS, 70, walkers=walkers, seed=1, move=move, burn=5, thin=2, marginals=option)
    assert dev.names == NAMES + ["epsilon"] and dev.chain.shape == (33, 3, walkers, 4)
    m = dev.marginals
    assert len(m.counts2d) == 6 and m.counts2d[("sigma_v", "epsilon")].shape == (3, 5, 5) and m.n.tolist() == [33 * walkers] * 3
    assert_marginals(m, own_history(dev, option), f"epsilon sampled, {move}")
    reaches_outside(m, "epsilon")


# ------------------------------------------------------------------ 8. without a history -------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_keep_chain_false_gives_the_same_histograms(rs9, metro_dev, stretch_dev, move):
    kept, block, option, kw = (metro_dev, PARAMS, OPTION, METRO) if move == "metropolis" else (stretch_dev, NARROW, OPTION_NARROW, STRETCH)
    bare = rs9.sample_chains(block, 70, keep_chain=False, marginals=option, **kw)
    assert bare.chain is None and bare.rhat is None
    same_marginals(bare.marginals, kept.marginals, f"keep_chain=False, {move}")
    for a in ("x", "lnl", "n_accept", "sum1", "sum2", "mean", "cov"):
        assert same_bytes(getattr(bare, a), getattr(kept, a)), a


# ------------------------------------------------------------------ 9. cut runs -----------------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_a_cut_run_counts_what_the_uncut_run_counts(rs9, metro_dev, stretch_dev, move):
    whole, block, option, kw = (metro_dev, PARAMS, OPTION, METRO) if move == "metropolis" else (stretch_dev, NARROW, OPTION_NARROW, STRETCH)
    cut = rs9.sample_chains(block, 0, marginals=option, **kw)
    assert cut.marginals.n.tolist() == [0] * 9 and all(v.sum() == 0 for v in cut.marginals.counts.values())
    cut.extend(40)
    part = cut.marginals
    cut.extend(30)
    same_run(cut, whole, f"40 + 30, {move}", SUMS)
    same_marginals(cut.marginals, whole.marginals, f"40 + 30, {move}")
    assert 0 < part.n[0] < whole.marginals.n[0] and part.counts["beta"].sum() == part.n.sum()      # (rebuilt after every extend)


# ------------------------------------------------------------------ 10. and 13. the handle ------------------------------------
def set_marginals(raw, group, n_bins, lo, hi, pairs, n_bins2):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
    hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    return raw.lib.vk_chain_set_marginals(raw.h, group, n_bins, None if lo is None else lo.ctypes.data_as(dp),
                                          None if hi is None else hi.ctypes.data_as(dp), len(pr), pr.ctypes.data_as(ip) if len(pr) else None,
                                          n_bins2)


def read_marginals(raw, R, n_bins, n_pairs, n_bins2):
    lp = C.POINTER(C.c_int64)
    h1, h2 = np.full((R, raw.d, n_bins + 2), -1, dtype=np.int64), np.full((R, n_pairs, n_bins2, n_bins2), -1, dtype=np.int64)
    assert raw.lib.vk_chain_marginals(raw.h, h1.ctypes.data_as(lp), h2.ctypes.data_as(lp)) == 0, raw.error()
    return h1, h2


LO_R, HI_R = [0.05, 0.2, 370.0], [1.5, 0.6, 390.0]
PAIRS_R = [[0, 2], [1, 2]]


def raw_counts(x, n_bins, n_bins2):
    """h1, h2 of positions x (m, 72, 3), 8 chains per problem: the rule through ``Binning.add``."""
    from victor_amd.marginals import Binning
    q = Binning(NAMES, n_bins, LO_R, HI_R, PAIRS_R, [("fsigma8", "sigma_v"), ("beta", "sigma_v")], n_bins2)
    h1, h2 = q.zeros(9)
    for t in range(len(x)):
        q.add(h1, h2, x[t], 8)
    return h1, h2


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
                assert set_marginals(raw, 8, 16, LO_R, HI_R, PAIRS_R, 4) == 0, raw.error()
            if mode == "cleared":
                assert set_marginals(raw, 0, 0, None, None, [], 0) == 0, raw.error()
            assert raw.start(x0) == 0, raw.error()
            rc, m = raw.metropolis(dz, lu, 0)
            assert rc == 0 and m == 6, raw.error()
            got = list(raw.finish(6)[1:])
            if mode == "set":
                first = read_marginals(raw, 9, 16, 2, 4)
                want = raw_counts(got[0], 16, 4)
                assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1])
                assert np.all(first[0].sum(axis=2) == 6 * 8) and first[0][:, 2, 0].sum() > 0 and first[0][:, 2, -1].sum() > 0
            rc, m = raw.stretch(z, lz, logu, k, first=6)
            assert rc == 0 and m == 3, raw.error()
            hx = raw.finish(3)
            assert hx[0] == 0, raw.error()
            got += list(hx[1:]) + list(raw.state())
            out.append(got)
            if mode == "set":
                both = read_marginals(raw, 9, 16, 2, 4)                        # Metropolis and stretch blocks add to the same counts
                more = raw_counts(hx[1], 16, 4)
                assert np.array_equal(both[0], want[0] + more[0]) and np.array_equal(both[1], want[1] + more[1])
                # a second start: fresh chains, fresh histograms - and the same numbers count the same again
                assert raw.start(x0) == 0, raw.error()
                zero = read_marginals(raw, 9, 16, 2, 4)
                assert not zero[0].any() and not zero[1].any()
                rc, m = raw.metropolis(dz, lu, 0)
                assert rc == 0 and m == 6, raw.error()
                assert raw.finish(6)[0] == 0
                again = read_marginals(raw, 9, 16, 2, 4)
                assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
                # h1 alone, h2 alone
                lp = C.POINTER(C.c_int64)
                h1 = np.empty_like(again[0])
                assert raw.lib.vk_chain_marginals(raw.h, h1.ctypes.data_as(lp), None) == 0 and np.array_equal(h1, again[0])
                h2 = np.empty_like(again[1])
                assert raw.lib.vk_chain_marginals(raw.h, None, h2.ctypes.data_as(lp)) == 0 and np.array_equal(h2, again[1])
            else:
                assert raw.lib.vk_chain_marginals(raw.h, None, None) == -1 and "has no marginals" in raw.error()
        finally:
            raw.close()
    for u, v, w in zip(*out):                                        # never set == set and cleared == set: histograms decide nothing
        assert same_bytes(u, v) and same_bytes(u, w)


def test_live_refusals_leave_the_handle_usable(rs9, metro_dev):
    x0 = np.ascontiguousarray(metro_dev.pivot.reshape(72, 3))
    rng = np.random.default_rng(6)
    width = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
    dz, lu = width * rng.standard_normal((4, 72, 3)), np.log(rng.random((4, 72)))
    raw = Raw(rs9, x0, 8)
    try:
        def refused(text, *a):
            assert set_marginals(raw, *a) == -1 and text in raw.error(), (text, raw.error())
        good = (8, 16, LO_R, HI_R, PAIRS_R, 4)
        refused("not a whole number of groups", 7, *good[1:])                  # 72 % 7 != 0
        refused("not a whole number of groups", 0, *good[1:])
        refused("n_bins", 8, 1025, *good[2:])
        refused("n_bins", 8, -1, *good[2:])
        refused("n_bins", 8, 0, LO_R, HI_R, [], 0)                            # 0 clears only with NULL ranges
        refused("n_bins2", *good[:5], 129)
        refused("n_bins2", *good[:5], 0)
        refused("n_pairs", *good[:4], [[0, 1]] * 46, 4)
        refused("needs 0 <= j < k < 3", *good[:4], [[2, 0]], 4)
        refused("needs 0 <= j < k < 3", *good[:4], [[1, 1]], 4)
        refused("needs 0 <= j < k < 3", *good[:4], [[1, 3]], 4)
        refused("needs 0 <= j < k < 3", *good[:4], [[-1, 2]], 4)
        refused("repeats pair", *good[:4], [[0, 2], [1, 2], [0, 2]], 4)
        refused("not finite with lo < hi", 8, 16, LO_R, [1.5, np.inf, 390.0], PAIRS_R, 4)
        refused("not finite with lo < hi", 8, 16, [0.05, np.nan, 370.0], HI_R, PAIRS_R, 4)
        refused("not finite with lo < hi", 8, 16, LO_R, [1.5, 0.2, 390.0], PAIRS_R, 4)
        refused("NULL", 8, 16, LO_R, None, PAIRS_R, 4)
        assert raw.lib.vk_chain_marginals(raw.h, None, None) == -1 and "has no marginals" in raw.error()
        assert raw.start(x0) == 0, raw.error()
        assert set_marginals(raw, *good) == 0, raw.error()
        rc, m = raw.metropolis(dz, lu, 0)
        assert rc == 0 and m == 4, raw.error()
        refused("awaiting vk_chain_finish", *good)                             # a block in flight
        refused("awaiting vk_chain_finish", 0, 0, None, None, [], 0)
        assert raw.lib.vk_chain_marginals(raw.h, None, None) == -1 and "awaiting vk_chain_finish" in raw.error()
        rc, hx, hl, hc = raw.finish(4)
        assert rc == 0, raw.error()
        refused("not a whole number of groups", 7, *good[1:])                  # a refusal keeps the marginals the handle had
        h1, h2 = read_marginals(raw, 9, 16, 2, 4)
        want = raw_counts(hx, 16, 4)
        assert np.array_equal(h1, want[0]) and np.array_equal(h2, want[1])
        # one group of all chains, no pairs: a second call replaces the buffers (and zeroes them)
        assert set_marginals(raw, 72, 8, LO_R, HI_R, [], 0) == 0, raw.error()
        h1, h2 = read_marginals(raw, 1, 8, 0, 1)
        assert h1.shape == (1, 3, 10) and not h1.any()
        rc, m = raw.metropolis(dz, lu, 4)
        assert rc == 0 and raw.finish(4)[0] == 0, raw.error()
        h1, _ = read_marginals(raw, 1, 8, 0, 1)
        assert np.all(h1.sum(axis=2) == 4 * 72)
    finally:
        raw.close()


# ------------------------------------------------------------------ 11. under a prior ----------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_under_a_prior_the_counts_are_the_definition_routes(rs9, metro_dev, stretch_dev, move):
    free, block, option, kw = (metro_dev, PARAMS, OPTION, METRO) if move == "metropolis" else (stretch_dev, NARROW, OPTION_NARROW, STRETCH)
    ref = rs9.sample_chains(block, 70, device=False, prior=boss_prior(), marginals=option, **kw)
    dev = rs9.sample_chains(block, 70, prior=boss_prior(), marginals=option, **kw)
    check_run(dev, ref, option, f"{move} under a prior", block)
    assert not same_bytes(dev.chain, free.chain), "the prior changed no decision: the test does not reach it"
    assert any(not np.array_equal(dev.marginals.counts[k], free.marginals.counts[k]) for k in NAMES)


# ------------------------------------------------------------------ 12. joint handles ----------------------------------------
@pytest.fixture(scope="module")
def five(tmp_path_factory):
    made = {}

    def get(cov):
        if cov not in made:
            made[cov] = Five(tmp_path_factory.mktemp("five_cov" if cov else "five_diag"), cov)
        return made[cov]
    return get


JOINT_OPTION = {"bins": 20, "bins2d": 6, "pairs": [("sigma_v@1", "sigma_v@3"), ("sigma_v@4", "fsigma8")],
                "range": {"sigma_v@1": (360.0, 400.0), "sigma_v@3": (370.0, 390.0)}}


@pytest.mark.parametrize("cov", [True, False], ids=["joint_cov", "block_diagonal"])
@pytest.mark.parametrize("data", [True, False], ids=["data", "mocks"])
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_joint_counts_are_the_definition_routes(five, cov, data, move):
    c = five(cov)
    target = c.joint if data else c.joint.realisations([0, 1, 2])
    W = 14 if move == "stretch" else 8 if data else 2          # stretch: W >= 2 (d + 1), d = 6
    n = 20 if move == "stretch" else 70                          # (70 steps cross the block of 64)
    kw = dict(walkers=W, seed=2, fixed={"beta": BETA, "epsilon": 1.0}, move=move, burn=3, thin=2, marginals=JOINT_OPTION)
    ref = target.sample_chains(blocked(), n, device=False, **kw)
    dev = target.sample_chains(blocked(), n, **kw)
    R = 1 if data else 3
    assert dev.names == JOINT_NAMES and dev.chain.shape == ((n - 3 + 1) // 2, R, W, 6)
    print("joint", "cov" if cov else "diag", "data" if data else "mocks", move, "acceptance of the definition route:", ref.acceptance)
    assert 0.02 < ref.acceptance.mean() < 0.98                   # a condition on the inputs
    check_run(dev, ref, JOINT_OPTION, "joint chains")            # (every block's sigma_v has the box of sigma_v)
    m = dev.marginals
    assert m.counts2d[("sigma_v@1", "sigma_v@3")].shape == (R, 6, 6) and m.counts2d[("sigma_v@4", "fsigma8")].shape == (R, 6, 6)
    assert m.counts["sigma_v@2"].shape == (R, 20) and m.edges["sigma_v@3"][0] == 370.0 and m.edges["sigma_v@2"][0] == 100.0
    reaches_outside(m, "sigma_v@3")
