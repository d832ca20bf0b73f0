"""Realisations with each mock's own real-space CCF on the GPU (``realisations(paired_model=True)``, vk_set_model_realisations;
the per-point xi^r tables of vk_kernel_fast.h / vk_kernel_cells.h / vk_kernel_generic.h).

Value contract: entry [p, m] equals CCFFit(model with realspace_ccf.simulation_number = numbers[m], data with
redshift_space_ccf.simulation_number = numbers[m]).log_likelihood(point p).  The kernel test holds the paired route to the
shared route of a fit built on mock m's own tables, evaluated on the same rows in one call - the same kernel at the same launch
shape on the same coefficients - bit for bit, in every launch regime of the evaluator; the oracle test holds it to the parity
bound of tests/test_gpu_realisations.py.  Fixtures: tests/test_paired_realisations.py."""

import ctypes as C
import faulthandler
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

from tests import cases
from tests import launch_shapes as LS
from tests.test_chains import same_bytes
from tests.test_gpu_realisations import FORMS, RTOL, with_form
from tests.test_paired_realisations import (NUMBERS, paired_boss_options, paired_fixed_options, which_of, write_boss_model_stack,
                                            write_fixed_stacks)
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
BLOCK2 = {n: PARAMS[n] for n in ("fsigma8", "sigma_v")}          # d = 2; the rest fixed
FIXED2 = {"beta": 0.37, "epsilon": 1.0}
FAST, CELLS, GENERIC = "vk_theory_fast_kernel", "vk_theory_cells_kernel", "vk_theory_kernel"
P_FSIGMA8, P_BETA = 0, 5


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle as vo
    return vo


@contextmanager
def knobs(**kv):
    from victor_amd import _native
    for k, v in kv.items():
        _native.set_knob("VICTOR_HIP_" + k, v)
    try:
        yield
    finally:
        for k in kv:
            _native.set_knob("VICTOR_HIP_" + k, None)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("paired")
    return {"tmp": tmp, "boss": write_boss_model_stack(tmp), "fixed": write_fixed_stacks(tmp)}


def options(files, fixture, number=0):
    if fixture == "boss":
        return paired_boss_options(files["tmp"], number=number, model_file=files["boss"])
    return paired_fixed_options(files["tmp"], number=number, files=files["fixed"])


def engine_of(fit):
    model = fit._merged({})
    return fit._get_engine(fit._engine_key(model), model["simpson_even"])


@pytest.fixture(scope="module")
def pair(files):
    """fixture name -> (the paired object over NUMBERS, [the shared object of the fit built on mock m's own tables and data])."""
    import victor_amd
    made = {}

    def get(fixture):
        if fixture not in made:
            paired = victor_amd.CCFFit(*options(files, fixture, NUMBERS[0])).realisations(NUMBERS, paired_model=True)
            own = [victor_amd.CCFFit(*options(files, fixture, m)).realisations([m]) for m in NUMBERS]
            made[fixture] = (paired, own)
        return made[fixture]
    return get


def rows_of(rs, fixture, n, guard=True):
    """n parameter rows of the cobaya prior box (Halton points); the last one fails its guards."""
    fit = rs.fit
    rows = fit._fit_rows(cases.halton_params(n, with_beta=fixture == "boss"), fit._merged({}))
    rows = np.array(rows, dtype=np.float64)
    if guard:
        rows[-1, P_BETA if fixture == "boss" else P_FSIGMA8] = np.nan
    return rows


def regimes():
    """(name, rows, kernel, knobs) of every launch regime of the evaluator, the row counts checked against the sources."""
    t = LS.thresholds()
    assert 3 < t["cells_min"] <= 24 < t["band1"] <= 130 < t["band2"] <= 260 <= t["kFuseMaxDefault"] < 600 <= t["kPartialPoints"] < 2049
    assert LS.cells_range(3, t) == 0 and LS.cells_range(24, t) == t["cpi0"] == 256
    assert LS.cells_range(130, t) == t["cpi1"] == 512 and LS.cells_range(260, t) == LS.cells_range(600, t) == t["cpi2"] == 1024
    assert LS.cells_range(2049, t) == -1
    return [("point-major", 3, FAST, {}), ("cells-256", 24, CELLS, {}), ("cells-512", 130, CELLS, {}), ("cells-1024", 260, CELLS, {}),
            ("unfused", 600, CELLS, {}), ("point-per-workgroup", 2049, CELLS, {}), ("generic", 3, GENERIC, {"FORCE_GENERIC": "1"})]


# ------------------------------------------------------------------ 1. parity with the per-mock fit, by launch regime ----------
@pytest.mark.parametrize("regime", regimes(), ids=lambda r: r[0])
@pytest.mark.parametrize("fixture", ["boss", "fixed"])
def test_pairs_equal_the_fit_on_each_mocks_own_tables_bit_for_bit(pair, fixture, regime):
    _, n, kernel, kn = regime
    paired, own = pair(fixture)
    rows, which = rows_of(paired, fixture, n), which_of(n)
    with knobs(**kn):
        lnl, chi2 = paired.log_likelihood_pairs(rows, which)
        assert engine_of(paired.fit).last_kernel() == kernel
        want_l, want_c = np.empty(n), np.empty(n)
        for m, shared in enumerate(own):
            l, c = shared.log_likelihood_pairs(rows, np.zeros(n, dtype=np.int32))     # every row: the launch has the same shape
            assert engine_of(shared.fit).last_kernel() == kernel
            want_l[which == m], want_c[which == m] = l[which == m], c[which == m]
        # the shared route of the paired object's own fit, in a launch of the same shape (below)
        l0, c0 = paired.fit.realisations(NUMBERS).log_likelihood_pairs(rows, which)
    assert np.isneginf(lnl[-1]) and np.isposinf(chi2[-1]) and np.all(np.isfinite(chi2[:-1]))
    diff = np.abs(chi2[:-1] - want_c[:-1])
    print(f"{fixture} {regime[0]}: max |chi2 - chi2 of the mock's own fit| = {diff.max():.3g}")
    assert same_bytes(chi2, want_c), (fixture, regime[0], int(np.argmax(chi2 != want_c)))
    assert same_bytes(lnl, want_l), (fixture, regime[0])
    # ... and the sets matter in this launch: rows of another set than the fit's own differ from the shared route of that fit
    other = (which != 0)[:-1]
    assert np.all(chi2[:-1][other] != c0[:-1][other]) and same_bytes(chi2[:-1][~other], c0[:-1][~other])


# ------------------------------------------------------------------ 2. against the oracle ---------------------------------------
def test_against_the_oracle_per_mock(files, oracle):
    import victor_amd
    hp = cases.halton_params(4, with_beta=True)
    pts = [cases.point(hp, i) for i in range(4)]
    theory = {}
    for form in FORMS:
        rs = victor_amd.CCFFit(*with_form(options(files, "boss", NUMBERS[0]), form)).realisations(NUMBERS, paired_model=True)
        lnl, chi2 = rs.log_likelihood(hp)
        assert lnl.shape == chi2.shape == (4, len(NUMBERS))
        for m, number in enumerate(NUMBERS):
            ofit = oracle.OracleFit(*with_form(options(files, "boss", number), form))
            for p, q in enumerate(pts):
                if (m, p) not in theory:                    # the theory vector does not depend on the likelihood form
                    theory[m, p] = type(ofit).theory_multipole_vector(ofit, ofit.s, dict(q), ofit.poles_s)
                ofit.theory_multipole_vector = lambda *a, _t=theory[m, p], **k: _t
                ol, oc = ofit.log_likelihood(dict(q))
                assert abs(chi2[p, m] - oc) <= RTOL * abs(oc), (form, p, m, chi2[p, m], oc)
                assert abs(lnl[p, m] - ol) <= RTOL * abs(oc), (form, p, m, lnl[p, m], ol)
        rs.fit._engine = None


# ------------------------------------------------------------------ 3. the pairing is real --------------------------------------
def test_the_pairing_is_real(files):
    import victor_amd
    numbers = [0, 1, 2]
    fit = victor_amd.CCFFit(*options(files, "boss", 0))            # realisation 0 of the model stack is the base model
    hp = cases.halton_params(4, with_beta=True)
    rows = np.repeat(fit._fit_rows(hp, fit._merged({})), 3, axis=0)
    which = np.tile(np.arange(3, dtype=np.int32), 4)
    shared = fit.realisations(numbers).log_likelihood_pairs(rows, which)[1].reshape(4, 3)
    paired_l, paired_c = fit.realisations(numbers, paired_model=True).log_likelihood(hp)
    again = fit.realisations(numbers, paired_model=True).log_likelihood_pairs(rows, which)[1].reshape(4, 3)
    assert same_bytes(paired_c, again)                             # cross mode is its expansion into pairs
    bound = chi2_bound(victor_amd.CCFFit(*options(files, "boss", 1)), hp)
    print("the pairing: |chi2 paired - chi2 shared| of mock 1:", np.abs(paired_c[:, 1] - shared[:, 1]), "100 x chi2_bound:", 100 * bound)
    assert np.all(np.abs(paired_c[:, 1] - shared[:, 1]) > 100 * bound)
    assert same_bytes(paired_c[:, 0], shared[:, 0])


# ------------------------------------------------------------------ 4. theory vectors -------------------------------------------
def test_fisher_vectors_are_those_of_the_per_mock_fits(files):
    import victor_amd
    at = {"fsigma8": np.array([0.45, 0.5, 0.4]), "sigma_v": np.array([370.0, 390.0, 350.0])}
    paired = victor_amd.CCFFit(*options(files, "boss", NUMBERS[0])).realisations(NUMBERS, paired_model=True)
    res = paired.fisher(BLOCK2, at, fixed=FIXED2, keep_vectors=True)
    assert res.vectors.shape[:2] == (3, 5) and np.all(res.ok)
    plain = paired.fisher(BLOCK2, at, fixed=FIXED2)                # the centres come from the stencil, not the fit's own tables
    assert plain.vectors is None and same_bytes(plain.model, res.model) and same_bytes(plain.fisher, res.fisher)
    from victor_amd import fisher as F
    with pytest.raises(victor_amd.InputError, match="device route"):
        F.fisher(paired.fit, BLOCK2, at, fixed=FIXED2, realisations=paired, device=False)
    for m, number in enumerate(NUMBERS):
        # the same three problems at the same points, all on mock m: a launch of the same shape on its own tables
        own = victor_amd.CCFFit(*options(files, "boss", number)).realisations([number] * 3).fisher(BLOCK2, at, fixed=FIXED2, keep_vectors=True)
        assert same_bytes(res.model[m], own.model[m]) and same_bytes(res.vectors[m], own.vectors[m]), m
        assert same_bytes(res.jacobian[m], own.jacobian[m]) and same_bytes(res.fisher[m], own.fisher[m]), m
    assert not same_bytes(res.model[0], res.model[2])


# ------------------------------------------------------------------ 5. sampled routes, smallest shapes --------------------------
def test_best_fit_is_its_definition_route(pair):
    from tests.test_gpu_fit_definition import both, same_fit
    paired, own = pair("boss")
    ref, dev = both(paired, BLOCK2, fixed=FIXED2, max_iter=40, restarts=0)
    same_fit(dev, ref, "paired best fit, d = 2")
    # the values at the best-fit points are the pairs-mode values there, and those of the mock's own fit (launches of other
    # shapes than the search's: to the bound of two evaluation orders)
    pts = dict({n: dev.x[:, j] for j, n in enumerate(dev.names)}, **{k: np.full(3, v) for k, v in FIXED2.items()})
    lnl, chi2 = paired.log_likelihood_pairs(pts, np.arange(3))
    mine = [shared.log_likelihood_pairs(pts, np.zeros(3, dtype=np.int32)) for shared in own]
    bound = np.array([chi2_bound(shared.fit, pts)[m] for m, shared in enumerate(own)])
    for what, c, l in (("pairs at the best fits", chi2, lnl),
                       ("the mocks' own fits at the best fits", np.array([mine[m][1][m] for m in range(3)]), np.array([mine[m][0][m] for m in range(3)]))):
        assert_same_chi2(c, dev.chi2, bound, what="paired best fit: " + what)
        assert_same_lnl(l, dev.lnl, bound, what="paired best fit: " + what)


# 3 mocks x 4 walkers x 10 steps, epsilon fixed.  Metropolis samples (fsigma8, beta, sigma_v); a stretch ensemble of 4 walkers holds
# at most one parameter (it needs 2 (d + 1) walkers), so there fsigma8 alone is sampled.
CHAIN_CASES = {"metropolis": (PARAMS, {"epsilon": 1.0}), "stretch": ({"fsigma8": PARAMS["fsigma8"]}, {"beta": 0.37, "sigma_v": 380.0, "epsilon": 1.0})}


@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_chains_device_route_is_the_definition_route(pair, move):
    from tests.test_gpu_chains import same_walk
    paired, _ = pair("boss")
    block, fixed = CHAIN_CASES[move]
    kw = dict(walkers=4, seed=3, fixed=fixed, move=move)
    ref = paired.sample_chains(block, 10, device=False, **kw)
    dev = paired.sample_chains(block, 10, **kw)
    assert dev.chain.shape == (10, 3, 4, len(block) - (1 if move == "metropolis" else 0))
    same_walk(dev, ref, f"paired {move}")
    assert same_bytes(dev.lnl_chain, ref.lnl_chain) and same_bytes(dev.chi2_chain, ref.chi2_chain)
    # every kept sample re-evaluated through pairs returns the stored lnL
    n, R, W, d = dev.chain.shape
    x = dev.chain.reshape(n * R * W, d)
    pts = dict({name: x[:, j] for j, name in enumerate(dev.names)}, **{k: np.full(len(x), v) for k, v in fixed.items()})
    which = np.tile(np.repeat(np.arange(R, dtype=np.int32), W), n)
    lnl, chi2 = paired.log_likelihood_pairs(pts, which)
    bound = np.empty(len(x))
    for m in range(R):
        sel = which == m
        bound[sel] = chi2_bound(_own_fit(pair, m), {k: v[sel] for k, v in pts.items()})
    assert_same_chi2(chi2, dev.chi2_chain.reshape(-1), bound, what=f"paired {move}: kept samples re-evaluated")
    assert_same_lnl(lnl, dev.lnl_chain.reshape(-1), bound, what=f"paired {move}: kept samples re-evaluated")


def _own_fit(pair, m):
    return pair("boss")[1][m].fit


def test_laplace_and_tempered_chains_are_paired(pair, files):
    """The Hessian stencil and the tempered step go through the same launches: paired like the rest, with no argument of their own."""
    import victor_amd
    from tests.test_gpu_chains import same_walk
    from tests.test_gpu_hessian import same_laplace
    paired, _ = pair("boss")
    at = {"fsigma8": np.array([0.45, 0.5, 0.4]), "sigma_v": np.array([370.0, 390.0, 350.0])}
    dev = paired.laplace(BLOCK2, at, fixed=FIXED2, keep_values=True)
    for m, number in enumerate(NUMBERS):
        # the same three problems at the same points, all on mock m: launches of the same shape on its own tables
        mine = victor_amd.CCFFit(*options(files, "boss", number)).realisations([number] * 3).laplace(BLOCK2, at, fixed=FIXED2, keep_values=True)
        same_laplace(dev, mine, f"paired laplace, problem {m}", rows=slice(m, m + 1))
    assert not same_bytes(dev.values[0], dev.values[2])
    kw = dict(walkers=4, seed=5, fixed={"epsilon": 1.0}, temper={"betas": [1.0, 0.3, 0.0], "swap_every": 4})
    ref = paired.sample_chains(PARAMS, 10, device=False, **kw)
    tem = paired.sample_chains(PARAMS, 10, **kw)
    same_walk(tem, ref, "paired tempered chains")
    assert same_bytes(tem.lnl_chain, ref.lnl_chain)


# ------------------------------------------------------------------ 6. engine ownership -----------------------------------------
def test_engine_ownership(files):
    import victor_amd
    rows = None
    fresh = victor_amd.CCFFit(*options(files, "boss", NUMBERS[0]))
    rows = fresh._fit_rows(cases.halton_params(24, with_beta=True), fresh._merged({}))
    which = which_of(24)
    want_shared = fresh.realisations(NUMBERS).log_likelihood_pairs(rows, which)
    want_batch = fresh.log_likelihood_batch(rows)
    fit = victor_amd.CCFFit(*options(files, "boss", NUMBERS[0]))
    paired, shared = fit.realisations(NUMBERS, paired_model=True), fit.realisations(NUMBERS)
    first = paired.log_likelihood_pairs(rows, which)
    got_shared = shared.log_likelihood_pairs(rows, which)
    second = paired.log_likelihood_pairs(rows, which)
    got_batch = fit.log_likelihood_batch(rows)
    for a, b in zip(got_shared, want_shared):
        assert same_bytes(a, b)
    for a, b in zip(got_batch, want_batch):
        assert same_bytes(a, b)
    for a, b in zip(first, second):
        assert same_bytes(a, b)
    assert not same_bytes(first[1], got_shared[1])
    lc, sc = shared.log_likelihood(rows[:2])                       # cross mode of a shared object on the engine a paired one used
    assert lc.shape == (2, 3)


# ------------------------------------------------------------------ 7. ABI refusals ---------------------------------------------
def test_abi_refusals(files):
    import victor_amd
    from victor_amd import _native as N
    fit = victor_amd.CCFFit(*options(files, "boss", NUMBERS[0]))
    rs = fit.realisations(NUMBERS, paired_model=True)
    rows = fit._fit_rows(cases.halton_params(6, with_beta=True), fit._merged({}))
    which = which_of(6)
    fresh = victor_amd.CCFFit(*options(files, "boss", NUMBERS[0])).realisations(NUMBERS).log_likelihood_pairs(rows, which)
    rs.log_likelihood_pairs(rows, which)
    eng = engine_of(fit)
    lib, ctx = eng._lib, eng._ctx
    opts = eng.make_opts(fit._merged({}), fit._merged_fit({}))
    out_l, out_c = np.empty((6, 3)), np.empty((6, 3))
    w = np.ascontiguousarray(which, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))

    def refused(rc, *texts):
        msg = (lib.vk_last_error(ctx) or b"").decode()
        assert rc == -1 and msg and all(t in msg for t in texts), (rc, msg)

    # cross mode with sets resident
    refused(lib.vk_eval_realisations(ctx, C.byref(opts), N.as_dp(rows), 6, None, N.as_dp(out_l), N.as_dp(out_c)), "vk_set_model_realisations")
    # n_sets != n_real
    sets = rs.model_sets()
    assert lib.vk_set_model_realisations(ctx, *[N.as_dp(np.ascontiguousarray(s[:2])) for s in sets], 2) == 0
    refused(lib.vk_eval_realisations(ctx, C.byref(opts), N.as_dp(rows), 6, w, N.as_dp(out_l), N.as_dp(out_c)), "2 model realisations", "3")
    # bad arguments
    refused(lib.vk_set_model_realisations(ctx, None, None, None, -1), "negative")
    refused(lib.vk_set_model_realisations(ctx, None, N.as_dp(sets[1]), N.as_dp(sets[2]), 3), "xi_coef")
    refused(lib.vk_set_model_realisations(ctx, N.as_dp(sets[0]), None, N.as_dp(sets[2]), 3), "uni_xi")
    # a joint evaluation over a context with sets
    assert lib.vk_set_model_realisations(ctx, *[N.as_dp(s) for s in sets], 3) == 0
    other = victor_amd.CCFFit(*options(files, "boss", NUMBERS[0]))
    ctxs = (C.c_void_p * 2)(engine_of(other)._ctx, ctx)
    lead = engine_of(other)._ctx
    rc = lib.vk_joint_eval_device_async(ctxs, 2, C.byref(opts), None, 0, None, None, None)
    msg = (lib.vk_last_error(lead) or b"").decode()
    assert rc == -1 and "model realisations" in msg, (rc, msg)
    # sets on a context whose velocity tables depend on the real-space CCF
    model, data = options(files, "boss", NUMBERS[0])
    model["matter_ccf"]["model"] = "linear_bias"
    lb = victor_amd.CCFFit(model, data)
    eng_lb = engine_of(lb)
    rc = lib.vk_set_model_realisations(eng_lb._ctx, *[N.as_dp(s) for s in sets], 3)
    msg = (lib.vk_last_error(eng_lb._ctx) or b"").decode()
    assert rc == -1 and "velocity tables" in msg, (rc, msg)
    # n_sets = 0 leaves a context whose pairs-mode results are a fresh one's
    assert lib.vk_set_model_realisations(ctx, None, None, None, 0) == 0
    l, c = np.empty(6), np.empty(6)
    assert lib.vk_eval_realisations(ctx, C.byref(opts), N.as_dp(rows), 6, w, N.as_dp(l), N.as_dp(c)) == 0
    assert same_bytes(l, fresh[0]) and same_bytes(c, fresh[1])
    assert lib.vk_eval_realisations(ctx, C.byref(opts), N.as_dp(rows), 6, None, N.as_dp(out_l), N.as_dp(out_c)) == 0      # cross mode again
    eng._real_owner = None                          # (the sets were changed behind the objects' backs)
    eng._model_sets = False
