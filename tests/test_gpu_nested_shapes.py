"""Nested sampling at the live-point counts and row bands the product runs ("Launch shapes under test"):
vk_nested_start and vk_nested_begin at the shapes of ``NESTED`` (tests/launch_shapes.py) - 256 to 4096 live points, so that the
five strided loops of the select kernel make two to sixteen trips and its LDS arrays fill up, problems whose walkers lie on
both sides of a workgroup edge of the load, adopt, step and commit kernels, 64 start passes, more problems than the select
kernel has threads, and the evaluation between the nested kernels in every regime of ``launch_theory`` a run can meet (the
point-major kernel, the three range bands, fused and unfused on the data-vector route, at and past the partial-sum limit, 8192
rows, the paired and the block-diagonal joint routes).

The method is that of tests/test_gpu_nested.py, whose helpers are imported, the shapes are new; no bound is.  With epsilon fixed
both routes launch the same R K rows in the same order, so everything in ``BYTES`` is compared as bytes (``both``), after the
definition route alone has shown that the run reached both outcomes of a step (``exercised``).  Beside it every row is held to
the statement of the algorithm without the definition route (``holds_the_statement``), and the three largest rows to ONE
independent likelihood call over their dead and final live points at the per-point bound of tests/tolerances.py - which closes
the case of both routes being fed the same wrong rows.  Then the cuts at product size, a run with stuck walkers (duplicate live
points, equal lnL among the dead) and a start with two planted pairs of identical live points whose second members lie in the
second trip of the select kernel's loops.  No assertion is on elapsed time."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import launch_shapes as LS
from tests.test_chains import same_bytes
from tests.test_gpu_nested import BYTES, EPS1, PARAMS, Raw, boss, both, exercised, rs3, same_run, stack  # noqa: F401  (fixtures among them)
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
T = LS.thresholds()
IDS = {}                                                     # test function -> its case ids (tests/test_launch_shapes.py reads it)
INDEPENDENT = ("N4", "N5", "N6")                             # the rows held to one likelihood call of their own


def order(case):
    return int(case[1:])


CASES = [(case, f"{v['L']}x{v['K']}") for case in sorted(LS.NESTED, key=order) for v in LS.nested_variants(LS.NESTED[case])]
IDS["test_a_row"] = [f"{case}-{variant}" for case, variant in CASES]


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def mock_fit():
    """mock number -> the fit on that mock's own data vector (the bound on chi2 reads it)."""
    import victor_amd
    made = {}

    def get(m):
        if m not in made:
            made[m] = victor_amd.CCFFit(*stack_options(simulation_number=m))
        return made[m]
    return get


@pytest.fixture(scope="module")
def setting(stack, boss, tmp_path_factory):  # noqa: F811
    """row -> (the object whose ``nested_sampling`` is called, its params block, its fixed values, the mock number of every
    problem or None)."""
    def get(v):
        route, R = v["route"], v["R"]
        if route == "data":
            assert R == 1
            return boss, PARAMS, EPS1, None
        if route.startswith("mocks"):
            numbers = np.arange(R) % 16
            return stack.realisations(list(numbers)), PARAMS, EPS1, numbers
        if route == "paired models":
            import victor_amd
            from tests.test_paired_realisations import NUMBERS, paired_boss_options
            assert R == len(NUMBERS)
            fit = victor_amd.CCFFit(*paired_boss_options(tmp_path_factory.mktemp("nested_shapes_paired"), number=NUMBERS[0]))
            return fit.realisations(NUMBERS, paired_model=True), PARAMS, EPS1, None
        assert route.startswith("dsplit_diag")
        from tests.test_gpu_joint_sampled import BETA, Case
        from victor_amd.joint import per_block
        c = Case("dsplit_diag", tmp_path_factory.mktemp("nested_shapes_dsplit_diag"))
        assert len(c.jr) == R, (len(c.jr), "the joint mocks of tests/test_gpu_joint_sampled.py are no longer the R of row N10")
        return c.jr, per_block(PARAMS, ["sigma_v"], 3), {"beta": BETA, "epsilon": 1.0}, None
    return get


def call_of(v, **more):
    return dict(dict(n_live=v["L"], batch=v["K"], steps=v["S"], n_iter=v["n_iter"], seed=v["seed"]), **more)


def holds_the_statement(ns, v, what):
    """The device result against the statement of DESIGN.md section 7d, without the definition route."""
    T_, R, K, S, L = v["n_iter"], v["R"], v["K"], v["S"], v["L"]
    assert ns.dead_lnl.shape == (T_, R, K) and ns.dead_x.shape[:3] == (T_, R, K) and ns.x.shape[:2] == (R, L) and ns.lnl.shape == (R, L), what
    assert np.all(np.isfinite(ns.dead_lnl)) and np.all(np.diff(ns.dead_lnl, axis=2) >= 0), (what, "dead_lnl falls inside an iteration")
    assert np.all(np.diff(ns.dead_lnl.transpose(1, 0, 2).reshape(R, -1), axis=1) >= 0), (what, "dead_lnl falls between iterations")
    assert np.all(ns.lnl >= ns.dead_lnl[-1, :, -1][:, None]), (what, "a final live point lies below the last L*")
    assert ns.n_steps.tolist() == [T_ * K * S] * R and np.all(ns.n_stuck <= T_ * K) and np.all(ns.n_accept <= ns.n_steps), what
    for x in (ns.dead_x, ns.x):
        assert np.all(x >= ns._lo) and np.all(x <= ns._hi), (what, "a point outside the box")


def one_likelihood_call(obj, ns, numbers, mock_fit, what):
    """The dead and final live points against ONE likelihood call of all of them (T R K + R L rows: another launch shape than
    any of the run), at the per-point bound of two evaluation orders."""
    T_, R, K, d = ns.dead_x.shape
    x = np.concatenate([ns.dead_x.reshape(T_ * R * K, d), ns.x.reshape(-1, d)])
    which = np.concatenate([np.tile(np.repeat(np.arange(R, dtype=np.int32), K), T_), np.repeat(np.arange(R, dtype=np.int32), ns.n_live)])
    pts = dict({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(ns.names)}, epsilon=np.ones(len(x)))
    if numbers is None:
        lnl, chi2 = obj.log_likelihood_batch(pts)
        bound = chi2_bound(obj, pts)
    else:
        lnl, chi2 = obj.log_likelihood_pairs(pts, which)
        bound = np.empty(len(x))
        for m in sorted(set(int(n) for n in numbers)):
            sel = np.isin(which, np.nonzero(numbers == m)[0])
            bound[sel] = chi2_bound(mock_fit(m), {n: a[sel] for n, a in pts.items()})
    got_chi2, got_lnl = np.concatenate([ns.dead_chi2.ravel(), ns.chi2.ravel()]), np.concatenate([ns.dead_lnl.ravel(), ns.lnl.ravel()])
    print(what, "-", len(x), "points against one call: worst |chi2 - one call| / bound", float(np.max(np.abs(got_chi2 - chi2) / np.maximum(bound, 1e-300))))
    assert_same_chi2(got_chi2, chi2, bound, what=f"{what}: dead and live points vs one likelihood call")
    assert_same_lnl(got_lnl, lnl, bound, what=f"{what}: dead and live points vs one likelihood call")


# ------------------------------------------------------------------ 1. every row of the table ------------------------------
@pytest.mark.parametrize("case,variant", CASES, ids=IDS["test_a_row"])
def test_a_row(setting, mock_fit, case, variant):
    (v,) = [v for v in LS.nested_variants(LS.NESTED[case]) if f"{v['L']}x{v['K']}" == variant]
    what = f"{case} ({v['route']}, R = {v['R']}, L = {v['L']}, K = {v['K']}: {LS.nested_rows(v)} rows, {LS.passes(v)} passes)"
    obj, params, fixed, numbers = setting(v)
    dev, ref = both(obj, params, what, fixed=fixed, **call_of(v))
    exercised(ref, what)
    assert dev.R == v["R"] and dev.n_iter == v["n_iter"] and dev.n_live == v["L"] and dev.batch == v["K"], what
    holds_the_statement(dev, v, what)
    if v["route"] == "data":                                 # the evaluation regime the row names is the one that ran
        from tests.test_gpu_launch_shapes import fuse_of
        fuse_of(obj, LS.nested_rows(v), what)
    if case == "N7":
        # problems r and r + 16 run on the same mock from the same start: the first dead points are the same bytes, then they part
        n = v["R"] - 16
        assert same_bytes(dev.dead_lnl[0, :n], dev.dead_lnl[0, 16:]) and same_bytes(dev.dead_x[0, :n], dev.dead_x[0, 16:]), what
        assert not same_bytes(dev.x[:n], dev.x[16:]) and not same_bytes(dev.dead_lnl[0, 0], dev.dead_lnl[0, 1]), what
    if case == "N6":
        assert not same_bytes(dev.dead_lnl[:, 0], dev.dead_lnl[:, 1]), what
    if case in INDEPENDENT:
        one_likelihood_call(obj, dev, numbers, mock_fit, what)


# ------------------------------------------------------------------ 2. cuts at product size --------------------------------
def test_nine_iterations_equal_seven_plus_two_at_the_default_shape(setting):
    v = LS.NESTED["N1"]
    assert v["n_iter"] == 9
    obj, params, fixed, _ = setting(v)
    whole = obj.nested_sampling(params, fixed=fixed, **call_of(v))
    cut = obj.nested_sampling(params, fixed=fixed, **call_of(v, n_iter=7)).extend(2)
    same_run(cut, whole, "N1: 7 + 2")


# ------------------------------------------------------------------ 3. duplicates and ties on the device -------------------
STUCK = dict(n_live=8, batch=2, steps=1, n_iter=16)
SCALES, SEEDS = (1.0, 2.0, 4.0, 8.0), range(8)


def equal_dead_pairs(ns):
    """Per problem, the neighbours of equal lnL in its dead record (which is in increasing order)."""
    flat = ns.dead_lnl.transpose(1, 0, 2).reshape(ns.R, -1)
    return (np.diff(flat, axis=1) == 0).sum(axis=1)


def test_a_stuck_run(rs3):  # noqa: F811
    """The first (scale, seed) for which the definition route alone has a stuck walker, both outcomes of a step in every problem
    and two dead points of equal lnL in one problem: the duplicate a stuck walker leaves died with its original, so the order of
    equal lnL by index was decided in the select kernel's rank loop.  (On an MI355X the choice is scale 1.0, seed 1 - stuck
    walkers 28, 27, 29 of 32 per problem, 20 to 22 equal neighbours among the 32 dead points of each; seed 0 has a problem
    without an accepted step.)"""
    chosen = None
    for scale in SCALES:
        for seed in SEEDS:
            ref = rs3.nested_sampling(PARAMS, device=False, fixed=EPS1, scale=scale, seed=seed, **STUCK)
            ok = ref.n_stuck.sum() > 0 and np.all((0 < ref.n_accept) & (ref.n_accept < ref.n_steps)) and equal_dead_pairs(ref).sum() > 0
            print("scale", scale, "seed", seed, "stuck", ref.n_stuck, "accepted", ref.n_accept, "of", ref.n_steps, "equal dead pairs", equal_dead_pairs(ref), "->", bool(ok))
            if ok:
                chosen = (scale, seed)
                break
        if chosen:
            break
    assert chosen is not None, "no candidate has a stuck walker, both outcomes and an equal pair among the dead: extend SCALES or SEEDS"
    print("a stuck run: chosen scale", chosen[0], "seed", chosen[1])
    what = f"stuck walkers (scale {chosen[0]}, seed {chosen[1]})"
    dev = rs3.nested_sampling(PARAMS, fixed=EPS1, scale=chosen[0], seed=chosen[1], **STUCK)
    same_run(dev, ref, what)
    exercised(ref, what, stuck=True)
    assert same_bytes(dev.n_stuck, ref.n_stuck) and dev.n_stuck.sum() > 0, what
    assert np.array_equal(equal_dead_pairs(dev), equal_dead_pairs(ref)), what


PLANTED = ((3, 300), (7, 260))


def test_a_planted_tie(rs3):  # noqa: F811
    """Two pairs of identical live points, the lowest of their problem, the second member of each behind index kNestedSelect:
    equal lnL goes by index in the ranks, the dead record and the slots the walkers are committed to.  S = 1, so what a slot
    holds afterwards is its walker's survivor or that survivor's one proposal: both are formed here from the numbers handed in."""
    L, K = 512, 2
    assert all(a < T["kNestedSelect"] <= b < L for a, b in PLANTED)
    raw = Raw(rs3, L=L, K=K, S=1)
    try:
        lib, h, R, d, dp = raw.lib, raw.h, raw.R, raw.d, raw.N.as_dp
        x0 = raw.x0(seed=3)
        names = ["fsigma8", "beta", "sigma_v"]
        pts = dict({n: np.ascontiguousarray(x0.reshape(R * L, d)[:, j]) for j, n in enumerate(names)}, epsilon=np.ones(R * L))
        lnl_host = np.asarray(rs3.log_likelihood_pairs(pts, np.repeat(np.arange(R, dtype=np.int32), L))[0]).reshape(R, L)
        assert np.all(np.isfinite(lnl_host))
        for r in range(R):
            lowest = np.argsort(lnl_host[r], kind="stable")[:2]
            assert lnl_host[r, lowest[0]] < lnl_host[r, lowest[1]]
            points = x0[r, lowest].copy()
            x0[r, lowest] = x0[r, [PLANTED[0][0], PLANTED[1][0]]]          # (what stood there lives on where the lowest two were)
            for pair, point in zip(PLANTED, points):
                x0[r, list(pair)] = point
        x0 = np.ascontiguousarray(x0)
        assert lib.vk_nested_start(h, dp(x0)) == 0, raw.error()
        lnl0, xs = np.empty((R, L)), np.empty((R, L, d))
        assert lib.vk_nested_state(h, dp(xs), dp(lnl0), None, None, None, None) == 0, raw.error()
        assert same_bytes(xs, x0)
        planted = [i for pair in PLANTED for i in pair]
        for r in range(R):                                   # conditions on the inputs: the planted points are the four lowest
            assert np.argsort(lnl0[r], kind="stable")[:4].tolist() == planted, (r, np.argsort(lnl0[r], kind="stable")[:4])
        pick, dz = raw.numbers(1)
        state, live = (lnl0, xs), None
        for t, pair in enumerate(PLANTED):
            lnl_before, x_before = state
            assert raw.begin(1, t) == 0, raw.error()
            dl, dc, dx, live = np.empty((1, R, K)), np.empty((1, R, K)), np.empty((1, R, K, d)), np.empty((R, L))
            assert lib.vk_nested_finish(h, dp(dl), dp(dc), dp(dx), dp(live)) == 0, raw.error()
            lnl_after, x_after = np.empty((R, L)), np.empty((R, L, d))
            assert lib.vk_nested_state(h, dp(x_after), dp(lnl_after), None, None, None, None) == 0, raw.error()
            assert same_bytes(live, lnl_after)
            for r in range(R):
                dead = np.argsort(lnl_before[r], kind="stable")[:K]
                # the smaller index dies first.  (Iteration 1: a statement about the live points iteration 0 left - its walkers
                # ended above the second pair, which nothing guarantees but these numbers give.)
                assert dead.tolist() == list(pair), (t, r, dead)
                assert same_bytes(dl[0, r], lnl_before[r, dead]) and same_bytes(dx[0, r], x_before[r, dead]), (t, r)
                assert same_bytes(dl[0, r, :1], dl[0, r, 1:]), (t, r, "the planted pair's lnL are not the same bytes")
                if t == 0:                                   # the pair still alive: equal bytes in the live lnL that came home
                    a, b = PLANTED[1]
                    assert same_bytes(live[r, a:a + 1], live[r, b:b + 1]), (r, "the second pair's lnL are not the same bytes")
                changed = np.nonzero(np.any(x_after[r] != x_before[r], axis=1) | (lnl_after[r] != lnl_before[r]))[0]
                assert changed.tolist() == list(pair), (t, r, changed)                 # the replaced slots are exactly those two
                # walker k went into the slot of dead point k: it holds the walker's survivor or that survivor's proposal
                survivors = np.setdiff1d(np.arange(L), dead)
                span = x_before[r].max(axis=0) - x_before[r].min(axis=0)
                src = survivors[np.minimum(np.floor(pick[0, r] * float(L - K)).astype(np.int64), L - K - 1)]
                assert src[0] != src[1], (t, r, "both walkers start at one survivor: choose other numbers")
                for k in range(K):
                    stay = x_before[r, src[k]]
                    move = stay + (0.3 * span) * dz[0, 0, r, k]
                    held = x_after[r, pair[k]]
                    assert same_bytes(held, stay) or same_bytes(held, move), (t, r, k, "slot", pair[k], "does not hold walker", k)
                    if same_bytes(held, stay):
                        assert same_bytes(lnl_after[r, pair[k]:pair[k] + 1], lnl_before[r, src[k]:src[k] + 1]), (t, r, k)
            state = (lnl_after, x_after)
        n = np.empty(R, dtype=np.int64)
        assert lib.vk_nested_state(h, None, None, None, None, n.ctypes.data_as(C.POINTER(C.c_int64)), None) == 0 and n.tolist() == [2 * K] * R
    finally:
        raw.close()
