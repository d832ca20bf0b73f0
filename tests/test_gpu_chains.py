"""Metropolis chains stepped on the GPU (victor_amd/chains.py, vk_chain_begin) against the NumPy loop that defines them
(device=False: one log_likelihood_pairs / log_likelihood_batch call per step): positions, decisions and log-likelihoods, every
kept sample against the likelihood and the oracle, determinism and cuts, the moment sums, the prior box, the
best_fit -> sample_chains workflow, and several optional states (histograms, series, predictive sums, tempering) on one handle.  No test asserts a posterior mean or width against a number."""

import faulthandler
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_chains import assert_pooled, assert_sums, same_bytes
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "beta", "sigma_v", "epsilon"]
LO = np.array([PARAMS[n]["prior"]["min"] for n in NAMES], dtype=float)
HI = np.array([PARAMS[n]["prior"]["max"] for n in NAMES], dtype=float)
MARGIN = 1e-6            # smallest decision margin the epsilon-sampled comparisons need on the definition route (three orders above
                         # the 1e-9 to-rounding allowance of the walker tests)
# Seeds of the epsilon-sampled comparisons: picked with the definition route alone (the first of 0, 1, 2, ... whose smallest
# decision margin exceeds MARGIN), before the device route was looked at.
SEED_REALISATIONS = 0    # observed smallest margin 2.2e-5 (seeds 1 .. 4: 1.2e-5, 5.8e-4, 1.1e-4, 2.2e-4)
SEED_DATA_VECTOR = 0     # observed smallest margin 6.9e-5 (seeds 1 .. 4: 5.0e-5, 1.2e-4, 2.4e-5, 3.0e-4)
SEED_BOX = 0             # observed smallest margin 1.2e-4, 31.7 % of the proposals outside the box


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle as vo
    return vo


@pytest.fixture(scope="module")
def rs():
    import victor_amd
    return victor_amd.CCFFit(*stack_options()).realisations()


@pytest.fixture(scope="module")
def single_fits():
    """One fit per realisation of the stack (for chi2_bound, which needs the realisation's own data vector)."""
    import victor_amd
    made = {}

    def get(m):
        if m not in made:
            made[m] = victor_amd.CCFFit(*stack_options(simulation_number=m))
        return made[m]
    return get


def history_bounds(single_fits, ch, fixed=None):
    """chi2_bound of every kept sample: (n_kept, R, W)."""
    n, R, W, d = ch.chain.shape
    out = np.empty((n, R, W))
    for m in range(R):
        x = ch.chain[:, m].reshape(n * W, d)
        pts = {name: x[:, j] for j, name in enumerate(ch.names)}
        pts.update(fixed or {})
        out[:, m] = chi2_bound(single_fits(m), pts).reshape(n, W)
    return out


def same_walk(dev, ref, what):
    """Positions, decisions and accept counts of two routes, bit for bit."""
    assert dev.chain.shape == ref.chain.shape, what
    assert same_bytes(dev.pivot, ref.pivot), what
    assert same_bytes(dev.chain, ref.chain), (what, "positions", int(np.argmax(np.any(dev.chain != ref.chain, axis=(1, 2, 3)))))
    assert same_bytes(dev.x, ref.x) and np.array_equal(dev.n_accept, ref.n_accept), what
    assert same_bytes(dev.acceptance, ref.acceptance), what
    assert dev.n_steps == ref.n_steps and dev.n_kept == ref.n_kept


def test_device_route_is_the_definition_route_bit_for_bit_with_epsilon_fixed(rs):
    kw = dict(walkers=4, seed=2, fixed={"epsilon": 1.0})
    ref = rs.sample_chains(PARAMS, 300, device=False, **kw)
    dev = rs.sample_chains(PARAMS, 300, **kw)
    assert dev.names == ["fsigma8", "beta", "sigma_v"] and dev.chain.shape == (300, 16, 4, 3)
    assert 0.02 < ref.acceptance.mean() < 0.98
    same_walk(dev, ref, "epsilon fixed")
    # the same rows in launches of the same shape: the same bits
    assert same_bytes(dev.lnl_chain, ref.lnl_chain), float(np.nanmax(np.abs(dev.lnl_chain - ref.lnl_chain)))
    assert same_bytes(dev.chi2_chain, ref.chi2_chain), float(np.nanmax(np.abs(dev.chi2_chain - ref.chi2_chain)))
    assert same_bytes(dev.lnl, ref.lnl) and same_bytes(dev.chi2, ref.chi2)


def test_device_route_with_epsilon_sampled(rs, single_fits):
    kw = dict(walkers=4, seed=SEED_REALISATIONS)
    ref = rs.sample_chains(PARAMS, 300, device=False, **kw)
    print("smallest decision margin (definition route, realisations):", ref.decision_margin)
    assert ref.decision_margin > MARGIN, ref.decision_margin            # a condition on the inputs, not on the code under test
    dev = rs.sample_chains(PARAMS, 300, **kw)
    assert dev.names == NAMES
    same_walk(dev, ref, "epsilon sampled")
    bound = history_bounds(single_fits, ref)
    assert_same_chi2(dev.chi2_chain, ref.chi2_chain, bound, what="chains: device vs definition route")
    assert_same_lnl(dev.lnl_chain, ref.lnl_chain, bound, what="chains: device vs definition route")


def test_data_vector_chains():
    import victor_amd
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    kw = dict(walkers=64, seed=SEED_DATA_VECTOR)
    ref = fit.sample_chains(PARAMS, 300, device=False, **kw)
    print("smallest decision margin (definition route, data vector):", ref.decision_margin)
    assert ref.decision_margin > MARGIN, ref.decision_margin
    dev = fit.sample_chains(PARAMS, 300, **kw)
    assert dev.chain.shape == (300, 1, 64, 4) and dev.rhat.shape == (1, 4)
    same_walk(dev, ref, "data vector")
    x = ref.chain.reshape(-1, 4)
    bound = chi2_bound(fit, {n: x[:, j] for j, n in enumerate(NAMES)}).reshape(300, 1, 64)
    assert_same_chi2(dev.chi2_chain, ref.chi2_chain, bound, what="data-vector chains: device vs definition route")
    assert_same_lnl(dev.lnl_chain, ref.lnl_chain, bound, what="data-vector chains: device vs definition route")


def test_every_kept_sample_is_what_the_likelihood_says(rs, single_fits, oracle):
    ch = rs.sample_chains(PARAMS, 120, walkers=4, seed=5, burn=20, thin=4)
    n, R, W, d = ch.chain.shape
    assert n == 25
    rng = np.random.default_rng(0)
    pick = rng.choice(n * R * W, size=400, replace=False)
    t, m, w = np.unravel_index(pick, (n, R, W))
    x = ch.chain[t, m, w]
    pts = {name: x[:, j] for j, name in enumerate(NAMES)}
    lnl, chi2 = rs.log_likelihood_pairs(pts, m.astype(np.int32))
    bound = np.empty(len(pick))
    for k in range(R):
        sel = m == k
        if sel.any():
            bound[sel] = chi2_bound(single_fits(k), {name: v[sel] for name, v in pts.items()})
    assert_same_chi2(ch.chi2_chain[t, m, w], chi2, bound, what="kept samples vs log_likelihood_pairs")
    assert_same_lnl(ch.lnl_chain[t, m, w], lnl, bound, what="kept samples vs log_likelihood_pairs")
    for i in (0, 150, 399):                     # the oracle: a wrongly formed row (AP factors, beta, a fixed parameter) would show here
        ofit = oracle.OracleFit(*stack_options(simulation_number=int(m[i])))
        ol, oc = ofit.log_likelihood({name: float(v[i]) for name, v in pts.items()})
        got_l, got_c = ch.lnl_chain[t[i], m[i], w[i]], ch.chi2_chain[t[i], m[i], w[i]]
        assert abs(ol - got_l) <= 1e-9 * abs(ol) and abs(oc - got_c) <= 1e-9 * abs(oc), (i, ol, got_l, oc, got_c)


def test_determinism_cuts_and_thinning(rs):
    kw = dict(walkers=4, seed=7)
    a = rs.sample_chains(PARAMS, 200, **kw)
    b = rs.sample_chains(PARAMS, 200, **kw)
    attrs = ("x", "lnl", "chi2", "chain", "lnl_chain", "chi2_chain", "mean", "cov", "n_accept", "sum1", "sum2", "pivot", "rhat")
    for name in attrs:
        assert same_bytes(getattr(a, name), getattr(b, name)), name
    cut = rs.sample_chains(PARAMS, 120, **kw).extend(80)
    for name in attrs:
        assert same_bytes(getattr(a, name), getattr(cut, name)), ("120 + 80", name)
    odd = rs.sample_chains(PARAMS, 1, **kw).extend(63).extend(1).extend(135)           # across a block boundary, one step at a time
    for name in attrs:
        assert same_bytes(getattr(a, name), getattr(odd, name)), ("1 + 63 + 1 + 135", name)
    lean = rs.sample_chains(PARAMS, 200, keep_chain=False, **kw)
    assert lean.chain is None and lean.rhat is None
    for name in ("x", "lnl", "chi2", "mean", "cov", "n_accept", "sum1", "sum2", "pivot"):
        assert same_bytes(getattr(a, name), getattr(lean, name)), ("keep_chain=False", name)
    for burn, thin in ((0, 3), (50, 1), (37, 7), (199, 5), (300, 1)):
        want = list(range(burn, 200, thin))
        th = rs.sample_chains(PARAMS, 200, burn=burn, thin=thin, **kw)
        assert th.n_kept == len(want) and th.chain.shape[0] == len(want)
        assert same_bytes(th.chain, a.chain[want]) and same_bytes(th.lnl_chain, a.lnl_chain[want]), (burn, thin)
        assert same_bytes(th.chi2_chain, a.chi2_chain[want]) and same_bytes(th.x, a.x), (burn, thin)
        piecewise = rs.sample_chains(PARAMS, 70, burn=burn, thin=thin, **kw).extend(130)
        assert same_bytes(piecewise.chain, th.chain) and same_bytes(piecewise.sum2, th.sum2), (burn, thin)


def test_moment_sums_and_pooled_moments(rs):
    ch = rs.sample_chains(PARAMS, 200, walkers=4, seed=7, burn=40, thin=2)
    n = ch.n_kept
    assert n == 80
    for m in range(16):
        assert_sums(ch.sum1[m], ch.sum2[m], ch.chain[:, m], ch.pivot[m], f"device sums, realisation {m}")
        assert_pooled(ch.mean[m], ch.cov[m], ch.chain[:, m], ch.pivot[m], n * 2.0 ** -52, f"realisation {m}")
    assert same_bytes(ch.sum2, np.swapaxes(ch.sum2, 2, 3))


def test_the_prior_box(rs):
    lo, hi = 360.0, 400.0
    narrow = dict(PARAMS, sigma_v=dict(PARAMS["sigma_v"], prior={"dist": "uniform", "min": lo, "max": hi}, ref={"loc": 380.0, "scale": 5.0}))
    kw = dict(walkers=4, seed=SEED_BOX, proposal={"sigma_v": 16.0})
    ref = rs.sample_chains(narrow, 300, device=False, **kw)
    out = ref.n_outside.sum() / (300 * 64)
    print("proposals outside the box:", out, " smallest decision margin:", ref.decision_margin)
    assert 0.25 < out < 0.45, out                   # a Gaussian step of 16 in a box of 40: 0.32 for a flat density, plus the other faces
    assert ref.decision_margin > MARGIN, ref.decision_margin       # (epsilon is sampled here: identical decisions need the margin)
    dev = rs.sample_chains(narrow, 300, **kw)
    j = dev.names.index("sigma_v")
    assert np.all(dev.chain[..., j] >= lo) and np.all(dev.chain[..., j] <= hi)
    assert np.all(dev.chain >= LO) and np.all(dev.chain <= HI)
    same_walk(dev, ref, "narrow box")


def test_best_fit_then_chains(rs, single_fits):
    bf = rs.best_fit(PARAMS)
    at = rs.sample_chains(PARAMS, 0, walkers=2, start=bf, scatter=0)
    assert same_bytes(at.x, np.repeat(bf.x[:, None, :], 2, axis=1))
    bound = np.array([chi2_bound(single_fits(m), bf.point(m))[0] for m in range(16)])
    for w in range(2):
        assert_same_chi2(at.chi2[:, w], bf.chi2, bound, what="chain started at the best fit vs best_fit")
        assert_same_lnl(at.lnl[:, w], bf.lnl, bound, what="chain started at the best fit vs best_fit")
    ch = rs.sample_chains(PARAMS, 64, walkers=8, start=bf, seed=1)
    assert np.all(ch.pivot >= LO) and np.all(ch.pivot <= HI) and np.all(ch.pivot != np.repeat(bf.x[:, None, :], 8, axis=1))
    first = rs.sample_chains(PARAMS, 0, walkers=8, start=bf, seed=1)
    assert same_bytes(first.x, ch.pivot) and np.all(np.isfinite(first.lnl))
    assert np.all(np.isfinite(ch.lnl)) and ch.mean.shape == (16, 4) and np.all(np.isfinite(ch.cov))


# ------------------------------------------------------------------ several optional states on one handle ---------------------
# Each optional state of a handle (histograms, the autocorrelation series, predictive sums, tempering) has a test module of its
# own; here they share a handle, across a block boundary (64 + 5 steps), kept and unkept steps (burn 3, thin 2) and an extend.
# Shapes, options and bounds are those of the modules named in the imports: nothing here is a new tolerance.
@pytest.fixture(scope="module")
def rs2(rs):
    """Two realisations: with W = 8, 16 chains."""
    return rs.fit.realisations([0, 1])


def same_series(a, b, what):
    assert a.autocorr.n == b.autocorr.n, what
    for k, v in a.autocorr.state.items():
        assert same_bytes(v, b.autocorr.state[k]), (what, k)


@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_marginals_autocorr_and_predictive_share_a_handle(rs2, move):
    from tests.test_gpu_predictive import LAGS, RUNS, check_history, check_routes
    from tests.test_gpu_priors import same_run
    from tests.test_marginals import same_marginals
    block, kw, option = RUNS[move]
    kw = dict(kw, burn=3, thin=2, marginals=option, autocorr=LAGS, predictive=True)
    ref = rs2.sample_chains(block, 69, device=False, **kw).extend(5)
    dev = rs2.sample_chains(block, 69, **kw).extend(5)
    assert dev.chain.shape == (36, 2, 8, 3) and dev.n_steps == 74                # steps 3, 5, .. 73: both sides of the block of 64
    assert np.all((0 < dev.n_accept) & (dev.n_accept < 74))
    same_run(dev, ref, move)
    same_marginals(dev.marginals, ref.marginals, move)
    assert dev.marginals.n.tolist() == [36 * 8] * 2
    same_series(dev, ref, move)
    assert dev.autocorr.n == 36
    bounds = check_history(rs2.fit, dev, f"three states on a handle, {move}, device")
    check_routes(dev, ref, bounds, f"three states on a handle, {move}")


def test_tempering_marginals_and_autocorr_share_a_handle(rs2):
    from tests.test_gpu_marginals import OPTION
    from tests.test_gpu_predictive import LAGS
    from tests.test_gpu_tempering import same_tempered
    from tests.test_marginals import same_marginals
    kw = dict(walkers=4, seed=2, burn=3, thin=2, fixed={"epsilon": 1.0}, temper={"betas": [1.0, 0.3], "swap_every": 2},
              marginals=OPTION, autocorr=LAGS)
    ref = rs2.sample_chains(PARAMS, 69, device=False, **kw).extend(5)
    dev = rs2.sample_chains(PARAMS, 69, **kw).extend(5)
    assert dev.chain.shape == (36, 2, 4, 3)
    assert ref.tempering.n_swap_try[:, 0].tolist() == [[19] * 4] * 2        # 37 events; two rungs have a pair at even parity only
    assert 0 < ref.tempering.n_swap_acc.sum() < ref.tempering.n_swap_try.sum()
    same_tempered(dev, ref, "tempering with histograms and series")
    same_marginals(dev.marginals, ref.marginals, "tempering with histograms and series")
    same_series(dev, ref, "tempering with histograms and series")


def test_clearing_one_state_leaves_the_others_on_the_handle(rs2):
    """Through the C ABI: three states set, the autocorrelation cleared again, a second start, one block - the histograms and
    the predictive sums are those of the block's own history, and the walk is that of a handle that never had any of them."""
    from types import SimpleNamespace
    from tests.test_gpu_marginals import HI_R, LO_R, PAIRS_R, read_marginals, set_marginals
    from tests.test_gpu_predictive import read_predictive, restate, within
    from tests.test_gpu_stretch import Raw
    from victor_amd.marginals import Binning
    rng = np.random.default_rng(4)
    x0 = np.ascontiguousarray(rs2.sample_chains(PARAMS, 0, walkers=8, seed=2, fixed={"epsilon": 1.0}).pivot.reshape(16, 3))
    names = ["fsigma8", "beta", "sigma_v"]
    width = np.array([PARAMS[n]["proposal"] for n in names], dtype=float)
    dz, lu = width * rng.standard_normal((6, 16, 3)), np.log(rng.random((6, 16)))
    plain, raw = Raw(rs2, x0, 8), Raw(rs2, x0, 8)
    try:
        assert plain.start(x0) == 0, plain.error()
        assert plain.metropolis(dz, lu, 0) == (0, 6), plain.error()
        want = plain.finish(6)
        assert raw.start(x0) == 0, raw.error()
        assert set_marginals(raw, 8, 16, LO_R, HI_R, PAIRS_R, 4) == 0, raw.error()
        assert raw.lib.vk_chain_set_autocorr(raw.h, 8, 16) == 0, raw.error()
        assert raw.lib.vk_chain_set_predictive(raw.h, 8) == 0, raw.error()
        assert raw.lib.vk_chain_set_autocorr(raw.h, 0, 0) == 0, raw.error()
        assert raw.start(x0) == 0, raw.error()
        assert raw.metropolis(dz, lu, 0) == (0, 6), raw.error()
        got = raw.finish(6)
        assert got[0] == 0 and all(same_bytes(u, v) for u, v in zip(got[1:], want[1:])), raw.error()
        assert all(same_bytes(u, v) for u, v in zip(raw.state(), plain.state()))
        assert raw.lib.vk_chain_autocorr(raw.h, *[None] * 6) == -1 and "has no autocorrelation" in raw.error()
        q = Binning(names, 16, LO_R, HI_R, PAIRS_R, [("fsigma8", "sigma_v"), ("beta", "sigma_v")], 4)
        h1, h2 = q.zeros(2)
        for t in range(6):
            q.add(h1, h2, got[1][t], 8)
        d1, d2 = read_marginals(raw, 2, 16, 2, 4)
        assert np.array_equal(d1, h1) and np.array_equal(d2, h2) and np.all(d1.sum(axis=2) == 6 * 8)
        state = read_predictive(raw, 2)
        ch = SimpleNamespace(predictive=SimpleNamespace(state=state), names=names, fixed=raw.fixed, chain=got[1].reshape(6, 2, 8, 3),
                             lnl_chain=got[2].reshape(6, 2, 8), chi2_chain=got[3].reshape(6, 2, 8))
        rules = restate(rs2.fit, ch)
        assert state["n"].tolist() == [48] * 2 and np.array_equal(state["n"], rules["n"]) and not state["n_skipped"].any()
        within(state["sum_t"], rules["sum_t"], rules["b_t"], "one state cleared: sum_t against the history")
        within(state["sum_tt"], rules["sum_tt"], rules["b_tt"], "one state cleared: sum_tt against the history")
        within(state["deviance"][:, 2:], rules["dev"], rules["b_dev"], "one state cleared: deviance sums against the history")
    finally:
        plain.close()
        raw.close()
