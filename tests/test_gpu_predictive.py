"""Posterior-predictive sums on the GPU (``predictive=`` of ``sample_chains``; vk_chain_set_predictive / vk_chain_predictive;
vk_chain_hold_kernel, vk_chain_predict_kernel): the sums the device keeps against the definition route's
(``device=False``) and against the rules of victor_amd/csrc/vk_predictive.h restated on the run's own history, for both moves, on
the realisation route and on the fit's own data vector (on both sides of the threshold between the point-major and the cells
theory kernel, fused chi-square tail and NO_FUSE); the held vectors at the chains' final
positions; the rest of a run is byte for byte the run without ``predictive=``; without a history and across cuts; combined with a
prior, histograms and the autocorrelation; the handle; and the deviance information criterion.

Fixtures and shapes are those of tests/test_gpu_priors.py and tests/test_gpu_marginals.py: the BOSS golden configuration with
nine realisations x 8 chains (72 chains: a partial wave, two workgroups of the step kernels; N = 60 entries is a partial wave of the
predict kernel), 70 steps across the block of 64, with burn and thin.

Tolerances.  Two correct evaluations of a theory vector differ per entry by at most delta, the bound of
``tests/tolerances.assert_same_theory`` (512 unit roundoffs of the summed magnitude).  With n samples and v = t - pivot, u = 2^-53:

    |d sum_t|  <= n delta + (n - 1) u sum |v|
    |d sum_tt| <= 2 delta sum |v| + n delta^2 + (n + 1) u sum v^2

(each term moves by delta; a sum of n terms carries n - 1 roundings; v^2 one more for the product, fewer when it is contracted).
The deviance sums follow the same pattern with delta = 0: the history holds the device's own chi2 and lnL bits, so only the
summation remains.  ``sum_bounds`` forms them; nothing here is fitted.  Between the two routes the pivots differ by up to delta
as well, so the definition route's sums are first moved onto the device's pivot, exactly, in extended precision.  Every
comparison records its worst margin through ``tolerances._record``.
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests.test_chains import same_bytes
from tests.test_gpu_kernel_matrix import knobs
from tests.test_gpu_marginals import OPTION, OPTION_NARROW
from tests.test_gpu_priors import BETA, HISTORY, METRO, NARROW, PARAMS, STRETCH, boss_prior, same_run
from tests.test_gpu_stretch import Raw, stretch_numbers
from tests.test_marginals import same_marginals
from tests.test_realisations import stack_options
from tests.tolerances import U, _record, assert_same_theory

pytestmark = pytest.mark.gpu
LD = np.longdouble
SUMS = HISTORY + ("sum1", "sum2", "mean", "cov")
NAMES = ["fsigma8", "beta", "sigma_v"]
STATE = ("pivot_t", "sum_t", "sum_tt", "deviance", "n", "n_skipped", "held")
LAGS = {"max_lag": 16}
RUNS = {"metropolis": (PARAMS, METRO, OPTION), "stretch": (NARROW, STRETCH, OPTION_NARROW)}


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


@pytest.fixture(scope="module")
def metro_dev(rs9):
    """The device route's 70 Metropolis steps of the 72 chains with predictive sums, computed once."""
    return rs9.sample_chains(PARAMS, 70, predictive=True, **METRO)


@pytest.fixture(scope="module")
def stretch_dev(rs9):
    return rs9.sample_chains(NARROW, 70, predictive=True, **STRETCH)


# ------------------------------------------------------------------ the rules on a run's own history, and the bounds ---------
def theory_at(fit, ch, x):
    """Theory vectors (..., N) at positions x (..., d) of the chains ``ch``."""
    flat = np.ascontiguousarray(x.reshape(-1, x.shape[-1]))
    p = dict(ch.fixed)
    p.update({n: np.ascontiguousarray(flat[:, j]) for j, n in enumerate(ch.names)})
    return fit.theory_vector_batch(p).reshape(x.shape[:-1] + (-1,))


def delta_of(t):
    """The per-entry bound of ``assert_same_theory`` (ulps = 512, tau = 2) for theory vectors of this magnitude."""
    return 512 * U * 2.0 * 4.0 * max(1.0, float(np.max(np.abs(t))))


def sum_bounds(n, abs_v, v2, delta):
    """(bound on sum_t, bound on sum_tt) of the module docstring; ``n`` broadcasts against the sums of |v| and v^2."""
    n = np.asarray(n, dtype=float)
    return n * delta + (n - 1) * U * abs_v, 2 * delta * abs_v + n * delta ** 2 + (n + 1) * U * v2


def restate(fit, ch):
    """The accumulate rule on the run's own history, about the run's own pivots, every sum in longdouble: a dict with ``sum_t``,
    ``sum_tt`` (R, N), ``dev`` (R, 4), ``n``, ``n_skipped`` (R,) and the bounds ``b_t``, ``b_tt`` (R, N), ``b_dev`` (R, 4)."""
    q = ch.predictive.state
    t = theory_at(fit, ch, ch.chain)                                     # (m, R, W, N)
    ok = np.isfinite(ch.chi2_chain) & np.isfinite(ch.lnl_chain)          # (m, R, W)
    v = np.where(ok[..., None], t - q["pivot_t"][None, :, None, :], 0.0).astype(LD)
    n = ok.sum(axis=(0, 2))
    delta = delta_of(t)
    abs_v, v2 = np.abs(v).sum(axis=(0, 2)).astype(float), (v * v).sum(axis=(0, 2)).astype(float)
    b_t, b_tt = sum_bounds(n[:, None], abs_v, v2, delta)
    a = np.where(ok, ch.chi2_chain - q["deviance"][None, :, None, 0], 0.0).astype(LD)
    b = np.where(ok, ch.lnl_chain - q["deviance"][None, :, None, 1], 0.0).astype(LD)
    dev = np.stack([a.sum(axis=(0, 2)), (a * a).sum(axis=(0, 2)), b.sum(axis=(0, 2)), (b * b).sum(axis=(0, 2))], axis=1)
    mag = np.stack([np.abs(a).sum(axis=(0, 2)), (a * a).sum(axis=(0, 2)), np.abs(b).sum(axis=(0, 2)), (b * b).sum(axis=(0, 2))], axis=1).astype(float)
    ba, baa = sum_bounds(n, mag[:, 0], mag[:, 1], 0.0)
    bb, bbb = sum_bounds(n, mag[:, 2], mag[:, 3], 0.0)
    return dict(sum_t=v.sum(axis=(0, 2)), sum_tt=(v * v).sum(axis=(0, 2)), dev=dev, n=n, n_skipped=(~ok).sum(axis=(0, 2)), b_t=b_t, b_tt=b_tt,
                b_dev=np.stack([ba, baa, bb, bbb], axis=1), delta=delta)


def within(got, want, bound, what):
    diff = np.abs(np.asarray(got, dtype=LD) - np.asarray(want, dtype=LD)).astype(float)
    ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
    margin = float(np.max(ratio)) if ratio.size else 0.0
    print(f"{what}: worst margin {margin:.3e}")
    _record(f"predictive {what}", margin)
    assert margin <= 1.0, (what, margin, float(np.max(diff)))


def check_history(fit, ch, what):
    """The run's sums are the rules applied to its own history; counters as integers; the pivots are the start's."""
    q, p = ch.predictive.state, ch.predictive
    want = restate(fit, ch)
    assert np.array_equal(p.n, want["n"]) and np.array_equal(p.n_skipped, want["n_skipped"]), what
    assert p.n.dtype == np.int64 and np.all(p.n == ch.n_kept * ch.W) and not p.n_skipped.any(), (what, p.n, p.n_skipped)
    within(q["sum_t"], want["sum_t"], want["b_t"], f"{what}: sum_t against the history")
    within(q["sum_tt"], want["sum_tt"], want["b_tt"], f"{what}: sum_tt against the history")
    within(q["deviance"][:, 2:], want["dev"], want["b_dev"], f"{what}: deviance sums against the history")
    assert_same_theory(q["pivot_t"], theory_at(fit, ch, ch.pivot[:, 0]), f"predictive {what}: pivots")
    assert np.all(np.isfinite(q["deviance"][:, :2])) and np.all(q["deviance"][:, 0] > 0)
    return want


def check_routes(dev, ref, bounds, what):
    """The device's sums against the definition route's, moved onto the device's pivot in extended precision."""
    d, r = dev.predictive.state, ref.predictive.state
    assert np.array_equal(d["n"], r["n"]) and np.array_equal(d["n_skipped"], r["n_skipped"]), what
    assert same_bytes(d["deviance"][:, :2], r["deviance"][:, :2]), what          # (epsilon fixed: the start's chi2 and lnL are the same bytes)
    n = d["n"].astype(LD)[:, None]
    shift = r["pivot_t"].astype(LD) - d["pivot_t"].astype(LD)
    assert float(np.max(np.abs(shift))) <= bounds["delta"], what
    s1, s2 = r["sum_t"].astype(LD), r["sum_tt"].astype(LD)
    within(d["sum_t"], s1 + n * shift, bounds["b_t"], f"{what}: sum_t against the definition route")
    within(d["sum_tt"], s2 + 2 * shift * s1 + n * shift * shift, bounds["b_tt"], f"{what}: sum_tt against the definition route")
    within(d["deviance"][:, 2:], r["deviance"][:, 2:], bounds["b_dev"], f"{what}: deviance sums against the definition route")


def same_sums(a, b, what, keys=STATE):
    for k in keys:
        assert same_bytes(a.predictive.state[k], b.predictive.state[k]), (what, k)


# ------------------------------------------------------------------ 1. Metropolis, realisations ------------------------------
def test_metropolis_sums_are_the_definition_routes_and_the_historys(fit, rs9, metro_dev):
    dev = metro_dev
    ref = rs9.sample_chains(PARAMS, 70, device=False, predictive=True, **METRO)
    assert dev.names == NAMES and dev.chain.shape == (33, 9, 8, 3)                # steps 5, 7, .. 69: across the block of 64
    p = dev.predictive
    assert p.mean.shape == (9, 60) and p.std.shape == (9, 60) and p.n.tolist() == [264] * 9 and p.n_skipped.tolist() == [0] * 9
    assert sorted(p.multipoles) == [0, 2] and p.multipoles[2][0].shape == (9, 30) and np.array_equal(p.multipoles[2][1], p.std[:, 30:])
    print("accepted per chain:", dev.n_accept.min(), "..", dev.n_accept.max(), "of 70")
    assert np.all((0 < dev.n_accept) & (dev.n_accept < 70)), "a chain does not reach both branches of the hold"
    same_run(dev, ref, "metropolis")
    bounds = check_history(fit, dev, "metropolis, device")
    check_history(fit, ref, "metropolis, definition route")
    check_routes(dev, ref, bounds, "metropolis")
    assert np.all(p.std > 0) and np.all(np.isfinite(p.mean))


# ------------------------------------------------------------------ 2. stretch, realisations --------------------------------
def test_stretch_sums_are_the_definition_routes_and_the_historys(fit, rs9, stretch_dev):
    dev = stretch_dev
    ref = rs9.sample_chains(NARROW, 70, device=False, predictive=True, **STRETCH)
    assert dev.chain.shape == (22, 9, 8, 3) and dev.move == "stretch"          # sweeps 5, 8, .. 68
    print("outside the box (definition route):", ref.n_outside.sum(), "of", 70 * 72, "; accepted per walker:", dev.n_accept.min(), "..",
          dev.n_accept.max())
    assert ref.n_outside.sum() > 0, "no proposal left the box: the test does not reach that rule"
    assert np.all((0 < dev.n_accept) & (dev.n_accept < 70)), "a walker does not reach both branches of the hold"
    assert dev.predictive.n.tolist() == [176] * 9
    same_run(dev, ref, "stretch")
    bounds = check_history(fit, dev, "stretch, device")
    check_history(fit, ref, "stretch, definition route")
    check_routes(dev, ref, bounds, "stretch")


# ------------------------------------------------------------------ 3. the held vectors --------------------------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_held_vectors_are_the_theory_at_the_final_positions(fit, metro_dev, stretch_dev, move):
    """A wrong row <-> walker map or a missed accept shows here directly, for all 72 chains."""
    dev = metro_dev if move == "metropolis" else stretch_dev
    held = dev.predictive.state["held"]
    assert held.shape == (72, 60)
    want = theory_at(fit, dev, dev.x.reshape(72, 3))
    assert_same_theory(held, want, f"predictive held, {move}")
    # the test can tell chains apart: the final vectors of two chains differ by far more than the bound
    assert np.min(np.max(np.abs(want[1:] - want[:-1]), axis=1)) > 100 * delta_of(want)


# ------------------------------------------------------------------ 4. the fit's own data vector ------------------------------
# Launches of fewer than 20 rows go to the point-major theory kernel, whose fused tail stores the theory vector anyway; from 20
# rows on the cells kernel runs, and its fused tail stores it ONLY when asked (TheoryArgs::want_theory).  So the data-vector
# route is run on both sides of that threshold: 8 walkers, and 32 (Metropolis: 32 rows a launch) or 40 (stretch: 20 rows a
# half-step).  Without the request the larger runs would sum whatever the workspace held.
DATA_WALKERS = {"metropolis": (8, 32), "stretch": (8, 40)}


def engine_of(fit):
    return fit._get_engine(fit._engine_key(fit._merged({})))


def launch_of(fit, block, kw):
    """(instance, fused) of the evaluation launches a predictive run makes: two steps before the burn, so nothing is kept, no
    mean exists and no evaluation at a mean follows the last step's launch."""
    ch = fit.sample_chains(block, 2, predictive=True, **dict(kw, burn=10))
    assert ch.n_kept == 0 and np.all(np.isnan(ch.predictive.chi2_at_mean))
    eng = engine_of(fit)
    return eng.last_instance(), eng.last_fused()


@pytest.mark.parametrize("move,walkers", [(m, w) for m, ws in DATA_WALKERS.items() for w in ws])
def test_data_vector_route_keeps_its_theory_vectors(fit, move, walkers):
    """R = 1.  At 32 / 40 walkers the launches are the cells kernel with the fused chi-square tail, which stores the theory vectors
    only because the handle asks (want_theory) - asserted on the launch itself; at 8 the point-major kernel.  The same again with
    the tail unfused.  The run is byte for byte the run without ``predictive=``."""
    block, kw, _ = RUNS[move]
    kw = dict(kw, walkers=walkers)
    instance, fused = launch_of(fit, block, kw)
    print(move, walkers, "walkers:", instance)
    assert fused and instance.endswith("+fused"), instance
    assert instance.startswith("cells") == (walkers > 8), instance
    plain = fit.sample_chains(block, 70, **kw)
    for knob in ({}, {"NO_FUSE": "1"}):
        with knobs(**knob):
            if knob:
                instance, fused = launch_of(fit, block, kw)
                assert not fused and instance.startswith("cells") == (walkers > 8), instance
            dev = fit.sample_chains(block, 70, predictive=True, **kw)
            what = f"data vector, {move}, {walkers} walkers, {'unfused' if knob else 'fused'}"
            assert dev.R == 1 and dev.predictive.mean.shape == (1, 60) and 0 < dev.n_accept.sum() < 70 * walkers
            check_history(fit, dev, what)
            assert_same_theory(dev.predictive.state["held"], theory_at(fit, dev, dev.x.reshape(walkers, 3)), f"predictive held, {what}")
        if not knob:
            same_run(dev, plain, "predictive changes nothing else on the data-vector route", SUMS)
            # the evaluation at the mean on this route: the fit's own likelihood there
            at = dict(dev.fixed)
            at.update({n: np.ascontiguousarray(dev.mean[:, j]) for j, n in enumerate(dev.names)})
            lnl_at, chi2_at = fit.log_likelihood_batch(at)
            p = dev.predictive
            assert np.array_equal(p.lnl_at_mean, lnl_at) and np.array_equal(p.chi2_at_mean, chi2_at) and p.chi2_at_mean.shape == (1,)
            assert same_bytes(p.p_d, -2.0 * p.mean_lnl - (-2.0 * lnl_at)) and np.all(np.isfinite(p.dic))


# ------------------------------------------------------------------ 5. nothing else moves ------------------------------------
@pytest.mark.parametrize("route", ["realisations", "data"])
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_the_rest_of_a_run_is_the_run_without_predictive(fit, rs9, move, route):
    block, kw, option = RUNS[move]
    target = rs9 if route == "realisations" else fit
    if route == "data":                                      # (the cells kernel and its fused tail: see DATA_WALKERS)
        kw = dict(kw, walkers=DATA_WALKERS[move][1])
    both = dict(marginals=option, autocorr=LAGS, **kw)
    with_, without = target.sample_chains(block, 70, predictive=True, **both), target.sample_chains(block, 70, **both)
    assert without.predictive is None and with_.predictive is not None
    same_run(with_, without, f"{move}, {route}", SUMS)
    same_marginals(with_.marginals, without.marginals, f"{move}, {route}")
    for k, v in with_.autocorr.state.items():
        assert same_bytes(v, without.autocorr.state[k]), k
    assert with_.autocorr.n == without.autocorr.n


# ------------------------------------------------------------------ 6. without a history and across cuts ---------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_keep_chain_false_and_a_cut_run_give_the_same_bytes(rs9, metro_dev, stretch_dev, move):
    whole = metro_dev if move == "metropolis" else stretch_dev
    block, kw, _ = RUNS[move]
    bare = rs9.sample_chains(block, 70, keep_chain=False, predictive=True, **kw)
    assert bare.chain is None
    same_sums(bare, whole, f"keep_chain=False, {move}")
    cut = rs9.sample_chains(block, 0, predictive=True, **kw)
    p0 = cut.predictive
    assert p0.n.tolist() == [0] * 9 and not p0.state["sum_t"].any() and np.all(np.isnan(p0.mean)) and np.all(np.isnan(p0.dic))
    assert same_bytes(p0.state["pivot_t"], whole.predictive.state["pivot_t"]) and p0.state["held"].any()
    cut.extend(40)
    part = cut.predictive
    cut.extend(30)                                                                 # across the block of 64
    same_run(cut, whole, f"40 + 30, {move}", SUMS)
    same_sums(cut, whole, f"40 + 30, {move}")
    assert 0 < part.n[0] < whole.predictive.n[0] and cut.predictive is not part     # (rebuilt after every extend)
    for a in ("mean", "std", "mean_chi2", "var_lnl", "chi2_at_mean", "p_d", "p_v", "dic"):
        assert same_bytes(getattr(cut.predictive, a), getattr(whole.predictive, a)), a


# ------------------------------------------------------------------ 7. combined -----------------------------------------------
def test_combined_with_prior_marginals_and_autocorr_each_is_what_it_is_alone(fit, rs9, metro_dev):
    kw = dict(prior=boss_prior(), **METRO)
    every = rs9.sample_chains(PARAMS, 70, marginals=OPTION, autocorr=LAGS, predictive=True, **kw)
    alone = rs9.sample_chains(PARAMS, 70, predictive=True, **kw)
    others = rs9.sample_chains(PARAMS, 70, marginals=OPTION, autocorr=LAGS, **kw)
    same_run(every, alone, "combined against predictive alone", SUMS)
    same_sums(every, alone, "combined against predictive alone")
    same_run(every, others, "combined against the others alone", SUMS)
    same_marginals(every.marginals, others.marginals, "combined")
    for k, v in every.autocorr.state.items():
        assert same_bytes(v, others.autocorr.state[k]), k
    check_history(fit, every, "combined, under a prior")
    assert not same_bytes(every.chain, metro_dev.chain), "the prior changed no decision: the test does not reach it"


@pytest.mark.parametrize("move,walkers", [("metropolis", 4), ("stretch", 10)])
def test_epsilon_sampled_sums_are_those_of_the_runs_own_history(fit, move, walkers):
    """With epsilon sampled the two routes agree to rounding only: the device's sums are held against its own history."""
    rs = fit.realisations([0, 1, 2])
    dev = rs.sample_chains(PARAMS, 70, walkers=walkers, seed=1, move=move, burn=5, thin=2, predictive=True)
    assert dev.names == NAMES + ["epsilon"] and dev.chain.shape == (33, 3, walkers, 4)
    check_history(fit, dev, f"epsilon sampled, {move}")
    assert_same_theory(dev.predictive.state["held"], theory_at(fit, dev, dev.x.reshape(3 * walkers, 4)), f"predictive held, epsilon sampled, {move}")


# ------------------------------------------------------------------ 8. the handle ---------------------------------------------
def read_predictive(raw, R, N=60):
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    out = {"pivot_t": np.full((R, N), -1.0), "sum_t": np.full((R, N), -1.0), "sum_tt": np.full((R, N), -1.0), "deviance": np.full((R, 6), -1.0),
           "n": np.full(R, -1, dtype=np.int64), "n_skipped": np.full(R, -1, dtype=np.int64), "held": np.full((raw.C, N), -1.0)}
    assert raw.lib.vk_chain_predictive(raw.h, *(out[k].ctypes.data_as(lp if out[k].dtype == np.int64 else dp) for k in STATE)) == 0, raw.error()
    return out


def test_start_resets_set_clear_set_and_clear_restores(rs9, metro_dev):
    x0 = np.ascontiguousarray(metro_dev.pivot.reshape(72, 3))
    rng = np.random.default_rng(4)
    width = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
    dz, lu = width * rng.standard_normal((6, 72, 3)), np.log(rng.random((6, 72)))
    z, lz, logu, k = stretch_numbers(rng, 3, 36, 4, 3)
    none = "has no predictive sums"
    out = []
    for mode in ("never", "cleared", "set"):
        raw = Raw(rs9, x0, 8)
        try:
            if mode != "never":
                assert raw.lib.vk_chain_set_predictive(raw.h, 8) == 0, raw.error()
            if mode == "cleared":
                assert raw.lib.vk_chain_set_predictive(raw.h, 0) == 0, raw.error()
            if mode == "set":                                                  # set, clear, set again
                assert raw.lib.vk_chain_set_predictive(raw.h, 0) == 0, raw.error()
                assert raw.lib.vk_chain_predictive(raw.h, *[None] * 7) == -1 and none in raw.error()
                assert raw.lib.vk_chain_set_predictive(raw.h, 8) == 0, raw.error()
            assert raw.start(x0) == 0, raw.error()
            if mode == "set":
                at_start = read_predictive(raw, 9)
                assert not at_start["n"].any() and not at_start["sum_t"].any() and not at_start["deviance"][:, 2:].any()
                assert same_bytes(at_start["pivot_t"], at_start["held"][::8]) and at_start["pivot_t"].all()
            rc, m = raw.metropolis(dz, lu, 0)
            assert rc == 0 and m == 6, raw.error()
            got = list(raw.finish(6)[1:])
            if mode == "set":
                first = read_predictive(raw, 9)
                assert first["n"].tolist() == [48] * 9 and first["sum_tt"].all() and same_bytes(first["pivot_t"], at_start["pivot_t"])
            rc, m = raw.stretch(z, lz, logu, k, first=6)
            assert rc == 0 and m == 3, raw.error()
            hx = raw.finish(3)
            assert hx[0] == 0, raw.error()
            got += list(hx[1:]) + list(raw.state())
            out.append(got)
            if mode == "set":
                both = read_predictive(raw, 9)                                 # Metropolis and stretch blocks add to the same sums
                assert both["n"].tolist() == [72] * 9 and not same_bytes(both["sum_t"], first["sum_t"])
                # any pointer may be NULL
                n = np.full(9, -1, dtype=np.int64)
                assert raw.lib.vk_chain_predictive(raw.h, None, None, None, None, n.ctypes.data_as(C.POINTER(C.c_int64)), None, None) == 0
                assert n.tolist() == [72] * 9
                # a second start: fresh sums, the pivots taken again - and the same numbers give the same bytes again
                assert raw.start(x0) == 0, raw.error()
                zero = read_predictive(raw, 9)
                assert all(same_bytes(zero[f], at_start[f]) for f in STATE)
                rc, m = raw.metropolis(dz, lu, 0)
                assert rc == 0 and m == 6, raw.error()
                assert raw.finish(6)[0] == 0
                again = read_predictive(raw, 9)
                assert all(same_bytes(again[f], first[f]) for f in STATE)
            else:
                assert raw.lib.vk_chain_predictive(raw.h, *[None] * 7) == -1 and none in raw.error()
        finally:
            raw.close()
    for u, v, w in zip(*out):                                        # never set == set and cleared == set: the sums decide nothing
        assert same_bytes(u, v) and same_bytes(u, w)


def set_tempering(raw, rungs, walkers, betas):
    b = None if betas is None else np.ascontiguousarray(betas, dtype=np.float64)
    return raw.lib.vk_chain_set_tempering(raw.h, rungs, walkers, None if b is None else b.ctypes.data_as(C.POINTER(C.c_double)))


def test_live_refusals_leave_the_handle_usable(rs9, metro_dev):
    x0 = np.ascontiguousarray(metro_dev.pivot.reshape(72, 3))
    rng = np.random.default_rng(6)
    width = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
    dz, lu = width * rng.standard_normal((4, 72, 3)), np.log(rng.random((4, 72)))
    raw = Raw(rs9, x0, 8)
    try:
        def refused(text, group):
            assert raw.lib.vk_chain_set_predictive(raw.h, group) == -1 and text in raw.error(), (text, raw.error())
        refused("not a whole number of groups", 7)                             # 72 % 7 != 0
        refused("not a whole number of groups", -8)
        assert raw.lib.vk_chain_predictive(raw.h, *[None] * 7) == -1 and "has no predictive sums" in raw.error()
        # tempering and predictive sums refuse each other, whichever comes second
        assert set_tempering(raw, 2, 4, [1.0, 0.5]) == 0, raw.error()
        refused("tempered", 8)
        assert set_tempering(raw, 0, 0, None) == 0, raw.error()
        assert raw.lib.vk_chain_set_predictive(raw.h, 8) == 0, raw.error()
        assert set_tempering(raw, 2, 4, [1.0, 0.5]) == -1 and "predictive sums" in raw.error(), raw.error()
        # the held vectors are taken at the start: chains need one after the sums were asked for
        rc, _ = raw.metropolis(dz, lu, 0)
        assert rc == -1 and "no start" in raw.error()
        assert raw.start(x0) == 0, raw.error()
        rc, m = raw.metropolis(dz, lu, 0)
        assert rc == 0 and m == 4, raw.error()
        refused("awaiting vk_chain_finish", 8)                                 # a block in flight
        refused("awaiting vk_chain_finish", 0)
        assert raw.lib.vk_chain_predictive(raw.h, *[None] * 7) == -1 and "awaiting vk_chain_finish" in raw.error()
        assert raw.finish(4)[0] == 0, raw.error()
        before = read_predictive(raw, 9)
        assert before["n"].tolist() == [32] * 9
        refused("not a whole number of groups", 7)                             # a refusal keeps the state the handle had
        refused("not a whole number of groups", 5)
        assert set_tempering(raw, 2, 4, [1.0, 0.5]) == -1
        after = read_predictive(raw, 9)
        assert all(same_bytes(after[f], before[f]) for f in STATE)
        rc, m = raw.metropolis(dz, lu, 4)                                      # ... and goes on
        assert rc == 0 and raw.finish(4)[0] == 0, raw.error()
        assert read_predictive(raw, 9)["n"].tolist() == [64] * 9
        # one group of all chains: a second call replaces the state, and asks for a new start
        assert raw.lib.vk_chain_set_predictive(raw.h, 72) == 0, raw.error()
        rc, _ = raw.metropolis(dz, lu, 8)
        assert rc == -1 and "no start" in raw.error()
        assert raw.start(x0) == 0, raw.error()
        rc, m = raw.metropolis(dz, lu, 0)
        assert rc == 0 and raw.finish(4)[0] == 0, raw.error()
        one = read_predictive(raw, 1)
        assert one["n"].tolist() == [4 * 72] and one["sum_t"].shape == (1, 60) and one["sum_tt"].all()
    finally:
        raw.close()


def test_joint_handles_are_refused(tmp_path):
    from tests.test_gpu_joint_sampled import fits_of
    from tests.test_joint_realisations import dsplit_stacks
    from victor_amd.joint import JointFit
    joint = JointFit(fits_of(dsplit_stacks(tmp_path, 5))[:2])
    ch = joint.sample_chains(PARAMS, 2, walkers=2, seed=2, fixed={"beta": BETA, "epsilon": 1.0})
    lib, h = ch._dev
    assert lib.vk_chain_set_predictive(h, 2) == -1 and "joint handle" in lib.vk_chain_last_error(h).decode()
    assert lib.vk_chain_predictive(h, *[None] * 7) == -1 and "has no predictive sums" in lib.vk_chain_last_error(h).decode()
    before = ch.x.copy()
    ch.extend(3)                                                               # the handle is as usable as it was
    assert ch.n_steps == 5 and ch.predictive is None and ch.x.shape == before.shape
    with pytest.raises(ValueError, match="joint fits"):
        joint.sample_chains(PARAMS, 2, walkers=2, predictive=True)


# ------------------------------------------------------------------ 9. the deviance information criterion ---------------------
@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_dic_is_numpy_on_the_history(fit, rs9, metro_dev, stretch_dev, move):
    """p_d = mean D - D(mean position), p_v = var D / 2, dic = mean D + p_d with D = -2 lnL, against NumPy on the history at the
    bounds of the sums: with b1, b2 the bounds on s_lnl and s_lnlsq, the mean of lnL moves by at most b1 / n and the variance by
    at most (b2 + 2 |s_lnl| b1 / n + b1^2 / n) / (n - 1); a handful of roundings of the read-out itself are added (16 u of the
    magnitudes involved)."""
    dev = metro_dev if move == "metropolis" else stretch_dev
    p = dev.predictive
    p_of = dict(dev.fixed)
    p_of.update({n: np.ascontiguousarray(dev.mean[:, j]) for j, n in enumerate(dev.names)})
    lnl_at, chi2_at = rs9.log_likelihood_pairs(p_of, np.arange(9, dtype=np.int32))
    assert np.array_equal(p.chi2_at_mean, chi2_at) and np.array_equal(p.lnl_at_mean, lnl_at)
    want = restate(fit, dev)
    n = p.n.astype(float)
    lnl = dev.lnl_chain.astype(LD)
    mean_l = lnl.mean(axis=(0, 2))
    var_l = (((lnl - mean_l[None, :, None]) ** 2).sum(axis=(0, 2)) / (p.n - 1)).astype(float)
    mean_l = mean_l.astype(float)
    b1, b2 = want["b_dev"][:, 2], want["b_dev"][:, 3]
    s1 = np.abs(p.state["deviance"][:, 4])
    b_mean = b1 / n + 16 * U * np.abs(mean_l)
    b_var = (b2 + 2 * s1 * b1 / n + b1 * b1 / n) / (n - 1) + 16 * U * (var_l + p.state["deviance"][:, 5] / (n - 1))
    within(p.mean_lnl, mean_l, b_mean, f"dic, {move}: mean lnL")
    within(p.var_lnl, var_l, b_var, f"dic, {move}: var lnL")
    mean_d, d_at = -2.0 * mean_l, -2.0 * lnl_at
    scale = 16 * U * (np.abs(mean_d) + np.abs(d_at))
    within(p.p_d, mean_d - d_at, 2 * b_mean + scale, f"dic, {move}: p_d")
    within(p.p_v, 2.0 * var_l, 2 * b_var, f"dic, {move}: p_v")
    within(p.dic, 2 * mean_d - d_at, 4 * b_mean + 2 * scale, f"dic, {move}: dic")
    chi2 = dev.chi2_chain.astype(LD)
    within(p.mean_chi2, chi2.mean(axis=(0, 2)).astype(float), want["b_dev"][:, 0] / n + 16 * U * np.abs(p.mean_chi2), f"dic, {move}: mean chi2")
    print(move, "p_d:", p.p_d, "p_v:", p.p_v, "mean chi2:", p.mean_chi2)
    assert np.all(np.isfinite(p.dic)) and np.all(p.p_v > 0)
