"""The device best-fit search (``vk_fit_run``: ``vk_fit_init_kernel`` / ``vk_fit_step_kernel`` / ``vk_fit_emit_kernel`` and
``fit_loop``) against its definition route, ``tests/fit_definition.py``: the same search restated in NumPy
slot for slot, driven through ``log_likelihood_batch`` / ``log_likelihood_pairs`` with the launches ``fit_loop`` makes - the
active problems' S rows each, in active-list order, finished problems dropped every ``FIT_CHECK`` iterations.

With epsilon fixed both routes put the same rows into launches of the same size through the same entry points (the argument
DESIGN.md section 7b makes for chains): ``x``, ``lnl`` (``lnpost`` under a prior), ``chi2``, ``status``, ``n_iter`` and
``n_evals`` are compared as BYTES.  A wrong slot, a stale row after compaction, a miscounted evaluation, a restart not taken or
the prior on a slot it does not belong to changes one of them.  With epsilon sampled the rows agree to rounding only, so the
comparison is conditioned on the mirror's smallest comparison margin, as tests/test_gpu_chains.py conditions its chains.

Every input below (tolerances, starts, ``max_iter``) was chosen with the mirror alone; the mirror's own coverage figures - the
compactions, the end statuses, the dead candidate slots - are asserted before the device result is looked at, and printed.
"""

import faulthandler

import numpy as np
import pytest

from tests import cases
from tests import fit_definition as FD
from tests.test_chains import same_bytes
from tests.test_gpu_chains import MARGIN
from tests.test_gpu_joint_blocks import blocks_bound
from tests.test_gpu_joint_sampled import Case
from tests.test_gpu_priors import BETA, NARROW, Five, boss_prior, resolved
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
EPS_FIXED = {"epsilon": 1.0}
NAMES3 = ["fsigma8", "beta", "sigma_v"]
LO3 = np.array([PARAMS[n]["prior"]["min"] for n in NAMES3], dtype=float)
HI3 = np.array([PARAMS[n]["prior"]["max"] for n in NAMES3], dtype=float)
RESULT = ("x", "lnpost", "chi2", "status", "n_iter", "n_evals")
DECISION = ("vertices", "expand", "reflect", "outside", "inside", "shrunk", "restart", "converged", "max_iter", "no_finite_start")


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
def rs(fit):
    return fit.realisations()


@pytest.fixture(scope="module")
def data_fit():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


def both(target, params, **kw):
    """(mirror, device) of one ``best_fit`` call - the mirror first."""
    ref = FD.best_fit(target, params, **kw)
    dev = target.best_fit(params, **kw)
    assert dev.names == ref.names
    return ref, dev


def first_difference(dev, ref, attrs=RESULT):
    for a in attrs:
        u, v = np.asarray(getattr(dev, a)), np.asarray(getattr(ref, a))
        if u.shape != v.shape or not same_bytes(u, v):
            rows = u.reshape(len(u), -1).view(np.uint64 if u.dtype.itemsize == 8 else np.uint32) != \
                v.reshape(len(v), -1).view(np.uint64 if v.dtype.itemsize == 8 else np.uint32)
            return a, int(np.argmax(rows.any(axis=1)))
    return None


def same_fit(dev, ref, what, attrs=RESULT):
    """Equal bytes; on failure the first differing problem and the mirror's decisions for it."""
    diff = first_difference(dev, ref, attrs)
    if diff is not None:
        a, p = diff
        print(f"{what}: {a} differs first at problem {p}: device {getattr(dev, a)[p]!r}, mirror {getattr(ref, a)[p]!r}")
        print("  device status / n_iter / n_evals:", dev.status[p], dev.n_iter[p], dev.n_evals[p],
              " mirror:", ref.status[p], ref.n_iter[p], ref.n_evals[p])
        print("  the mirror's decisions for it:", [DECISION[k] for k in ref.decisions[p]])
        print("  the mirror's launches (rows):", ref.launches[:40], "active list at each look:", ref.n_active)
    assert diff is None, (what, diff)


def figures(ref, what):
    print(f"{what}: status {np.bincount(ref.status, minlength=3).tolist()} (converged, max_iter, no finite start), n_iter "
          f"{ref.n_iter.min()} .. {ref.n_iter.max()}, active list {ref.n_active}, {ref.compactions} compactions, "
          f"{len(ref.launches)} launches of {min(ref.launches)} .. {max(ref.launches)} rows, dead candidate slots "
          f"{int(ref.n_dead_candidates.sum())}, shrinks {sum(d.count(FD.SHRUNK) for d in ref.decisions)}, restarts "
          f"{sum(d.count(FD.RESTART) for d in ref.decisions)}, smallest margin {ref.margin.min():.3g}")


# ------------------------------------------------------------------ epsilon fixed: equal bytes --------------------------------
def test_a_stack_d3_across_compaction_windows(rs):
    """(a) The 16 realisations, d = 3, S = 4, one restart; 1e-6 of each width and 1e-9 in lnL, at which the problems need from
    a hundred to several hundred launches each and so leave the active list in different windows of FIT_CHECK."""
    kw = dict(fixed=EPS_FIXED, xtol={n: 1e-6 * w for n, w in zip(NAMES3, HI3 - LO3)}, ftol=1e-9, max_iter=3000, restarts=1)
    ref, dev = both(rs, PARAMS, **kw)
    figures(ref, "(a)")
    assert ref.names == NAMES3 and ref.x.shape == (16, 3)
    assert ref.compactions >= 2, ref.n_active
    assert all(d.count(FD.RESTART) == 1 for d in ref.decisions) and np.all(ref.status == FD.ST_CONVERGED)
    same_fit(dev, ref, "(a) 16 realisations")
    assert np.all(dev.lnprior == 0.0) and same_bytes(dev.lnl, dev.lnpost)


def test_b_seventy_problems_with_their_own_starts(fit):
    """(b) 70 problems - two workgroups of kFitBlock = 64, the second partial - each from a start of its own; after the first
    compaction launch positions and problem numbers differ.  ``max_iter`` is the median of the iteration counts the mirror's
    searches take when nothing limits them (chosen here, by the mirror alone, before the device runs): about half the searches
    converge and the others are cut."""
    rs70 = fit.realisations(np.arange(70) % 16)
    rng = np.random.default_rng(3)
    x0 = LO3 + (HI3 - LO3) * (0.3 + 0.4 * rng.random((70, 3)))
    kw = dict(fixed=EPS_FIXED, start={n: x0[:, j] for j, n in enumerate(NAMES3)}, restarts=0)
    free = FD.best_fit(rs70, PARAMS, **kw)
    figures(free, "(b) without a limit")
    assert np.all(free.status == FD.ST_CONVERGED)
    kw["max_iter"] = int(np.median(free.n_iter))
    print("(b) max_iter:", kw["max_iter"], "of iteration counts", np.sort(free.n_iter).tolist())
    ref, dev = both(rs70, PARAMS, **kw)
    figures(ref, "(b)")
    n_conv, n_cut = int(np.sum(ref.status == FD.ST_CONVERGED)), int(np.sum(ref.status == FD.ST_MAX_ITER))
    assert n_conv > 0 and n_cut > 0 and n_conv + n_cut == 70, (n_conv, n_cut)
    assert ref.compactions >= 1 and ref.launches[0] == 280
    same_fit(dev, ref, "(b) 70 problems")


def test_b_520_problems_shrink_through_every_regime_of_the_evaluator(fit):
    """(b') 520 problems (``np.arange(520) % 16``), d = 3, S = 4, each from a start of its own: the first launches hold 2080
    rows, just past ``kPartialPoints`` - one workgroup per point -, and as problems finish the compacted launches pass through
    the ranges of 1024, 512 and 256 cells down to the point-major kernel below 20 rows (tests/launch_shapes.py reads the
    thresholds from the sources).  No other case starts from that height, and here the regime changes from one compaction to the
    next.  Tolerances of 1e-3 of the proposal widths and 1e-4 in lnL without a restart keep the mirror's Python loop to a few
    seconds at d = 3; chosen, like the starts, with the mirror alone, whose launches are held to every regime before the device
    runs."""
    from tests import launch_shapes as LS
    t = LS.thresholds()
    R = 520
    rs = fit.realisations(np.arange(R) % 16)
    rng = np.random.default_rng(5)
    x0 = LO3 + (HI3 - LO3) * (0.3 + 0.4 * rng.random((R, 3)))
    kw = dict(fixed=EPS_FIXED, start={n: x0[:, j] for j, n in enumerate(NAMES3)}, restarts=0, ftol=1e-4,
              xtol={n: 1e-3 * PARAMS[n]["proposal"] for n in NAMES3})
    ref = FD.best_fit(rs, PARAMS, **kw)
    figures(ref, "(b') 520 problems")
    regimes = sorted({LS.cells_range(m, t) for m in ref.launches})
    print("(b') launches by regime (-1: a workgroup per point, 0: point-major, else cells per range):",
          {g: sum(LS.cells_range(m, t) == g for m in ref.launches) for g in regimes})
    assert ref.launches[0] == 4 * R and t["kPartialPoints"] < 4 * R <= t["kPartialPoints"] + 32
    assert regimes == sorted([-1, 0, t["cpi0"], t["cpi1"], t["cpi2"]]), regimes
    assert ref.compactions >= 4, ref.n_active
    dev = rs.best_fit(PARAMS, **kw)
    assert dev.names == ref.names == NAMES3 and dev.x.shape == (R, 3)
    same_fit(dev, ref, "(b') 520 problems")


def test_c_data_vector_profile_and_one_problem(data_fit):
    """(c) The fit's own data vector: a profile over eight fixed values of fsigma8 (per-problem base rows, no realisation
    index; d = 2, launches of 32 rows and fewer) and one problem on its own (d = 3: launches of four rows, below the
    point-major threshold of 20; the five-row launch of d = 4 needs epsilon sampled and is the margin-conditioned test below)."""
    fs8 = np.linspace(0.3, 0.6, 8)
    ref, dev = both(data_fit, PARAMS, fixed=dict(EPS_FIXED, fsigma8=fs8), restarts=1)
    figures(ref, "(c) profile")
    assert ref.names == ["beta", "sigma_v"] and ref.launches[0] == 32 and np.array_equal(dev.params["fsigma8"], fs8)
    same_fit(dev, ref, "(c) profile of the data vector")
    ref, dev = both(data_fit, PARAMS, fixed=EPS_FIXED, restarts=1)
    figures(ref, "(c) one problem")
    assert ref.names == NAMES3 and set(ref.launches) == {4}
    same_fit(dev, ref, "(c) one problem, four-row launches")


def test_d_a_narrow_box_kills_candidates(rs):
    """(d) sigma_v confined to [350, 400] around its start: candidates fall outside the box (dead slots carrying v_0) and the
    simplex shrinks against the faces."""
    kw = dict(fixed=EPS_FIXED, step={"sigma_v": 30.0}, xtol={n: 1e-6 * w for n, w in zip(NAMES3, HI3 - LO3)}, ftol=1e-9,
              max_iter=2000, restarts=2)
    ref, dev = both(rs, NARROW, **kw)
    figures(ref, "(d)")
    assert int(ref.n_dead_candidates.sum()) > 0
    assert any(FD.SHRUNK in d for d in ref.decisions)
    j = ref.names.index("sigma_v")
    assert np.all(dev.x[:, j] >= 350.0) and np.all(dev.x[:, j] <= 400.0)
    same_fit(dev, ref, "(d) narrow box")


def test_e_under_a_correlated_prior(fit):
    """(e) lnL + ln prior on the live slots alone: ``lnpost`` in the device's bits, ``lnprior`` the host's."""
    rs5 = fit.realisations([0, 3, 5, 11, 12])
    kw = dict(fixed=EPS_FIXED, prior=boss_prior(), restarts=1)
    ref, dev = both(rs5, PARAMS, **kw)
    figures(ref, "(e)")
    same_fit(dev, ref, "(e) under a prior")
    r = resolved(boss_prior(), NAMES3)
    assert same_bytes(dev.lnprior, r.lnprior(dev.x)) and same_bytes(dev.lnprior, ref.lnprior) and np.all(dev.lnprior < 0.0)
    assert same_bytes(dev.lnl, dev.lnpost - dev.lnprior)
    free = rs5.best_fit(PARAMS, fixed=EPS_FIXED, restarts=1)
    assert not same_bytes(free.x, dev.x), "the prior moved no best fit: the test does not reach it"
    # the same under the narrow box of (d): launches that carry dead slots beside the live ones the prior is added to
    ref, dev = both(rs5, NARROW, step={"sigma_v": 30.0}, **kw)
    figures(ref, "(e) narrow box")
    assert int(ref.n_dead_candidates.sum()) > 0
    same_fit(dev, ref, "(e) under a prior, narrow box")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory.mktemp(name))
        return made[name]
    return get


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    return Five(tmp_path_factory.mktemp("five_cov"), True)


@pytest.mark.parametrize("name,data", [("dsplit_cov", True), ("dsplit_cov", False), ("dsplit_diag", True), ("dsplit_diag", False),
                                       ("boss_grid", True), ("boss_grid", False)])
def test_f_joint_fits(case, name, data):
    """(f) Three density-split blocks (beta fixed: d = 2), one parameter row for all: the data vectors and the 5 mocks, under
    the joint covariance and block-diagonal - the four routes of ``sampled_evaluate`` for joint fits - and the BOSS pair under its
    covariance gridded in beta (d = 3, 4 mocks: the slice sort and the log-determinant factor)."""
    c = case(name)
    target = c.joint if data else c.jr
    ref, dev = both(target, PARAMS, fixed=dict(c.fixed, epsilon=1.0), restarts=1)
    figures(ref, f"(f) {name} {'data' if data else 'mocks'}")
    assert ref.names == c.without("epsilon") and len(ref.x) == (1 if data else len(c.jr))
    same_fit(dev, ref, f"(f) {name} {'data' if data else 'mocks'}")


def test_f_joint_fit_with_a_dispersion_per_block(five):
    """(f) ``"sigma_v@q"``: a row set per block, d = 6, S = 7, three mocks of the five blocks under the joint covariance."""
    from victor_amd.joint import per_block
    jr = five.joint.realisations([0, 1, 2])
    ref, dev = both(jr, per_block(PARAMS, ["sigma_v"], 5), fixed={"beta": BETA, "epsilon": 1.0}, restarts=1)
    figures(ref, "(f) sigma_v@q")
    assert ref.names == ["fsigma8"] + [f"sigma_v@{q}" for q in range(5)] and ref.launches[0] == 21
    same_fit(dev, ref, "(f) five blocks, sigma_v per block")
    assert not same_bytes(dev.params["sigma_v@0"], dev.params["sigma_v@4"])


def test_g_ten_parameters(five):
    """(g) d = kMaxP = 10, S = kMaxS = 11: fsigma8 and sigma_v of each of the five blocks, 3 mocks, 100 launches - whatever
    the status."""
    from victor_amd.joint import per_block
    jr = five.joint.realisations([0, 1, 2])
    block = per_block(PARAMS, ["fsigma8", "sigma_v"], 5)
    ref, dev = both(jr, block, fixed={"beta": BETA, "epsilon": 1.0}, max_iter=100, restarts=0)
    figures(ref, "(g)")
    assert ref.names == [f"fsigma8@{q}" for q in range(5)] + [f"sigma_v@{q}" for q in range(5)]
    assert ref.x.shape == (3, 10) and ref.launches[0] == 33
    assert sum(len(set(d) & {FD.EXPAND, FD.REFLECT, FD.OUTSIDE, FD.INSIDE}) for d in ref.decisions) >= 3      # the search moved
    same_fit(dev, ref, "(g) d = 10")
    assert len({dev.x[0, j] for j in range(5, 10)}) == 5                  # (every block's dispersion went its own way)


# ------------------------------------------------------------------ epsilon sampled: conditioned on the margin -----------------
# With epsilon sampled the device forms a row's Alcock-Paczynski factors with its own pow and the host with libm's: lnL agrees
# to rounding, and a comparison of the search taken within that rounding could fall the other way.  The start is the first of
# the seeds 0, 1, 2, ... whose run on the mirror keeps every comparison it takes (decide, the ftol test, the sort) further
# apart than MARGIN; MAX_ITER_EPS ends the searches before the simplex - and with it the differences compared - has contracted.
# Chosen with the mirror alone, before the device result was looked at.
MAX_ITER_EPS = 40        # observed smallest margins at seed 0: data vector 1.5e-2, realisations 0, 5, 11 1.2e-4 (MARGIN is 1e-6)
NAMES4 = NAMES3 + ["epsilon"]


def margin_conditioned(target, R, what):
    lo = np.array([PARAMS[n]["prior"]["min"] for n in NAMES4], dtype=float)
    hi = np.array([PARAMS[n]["prior"]["max"] for n in NAMES4], dtype=float)
    ref = kw = None
    for seed in range(8):
        x0 = lo + (hi - lo) * (0.3 + 0.4 * np.random.default_rng(seed).random((R, 4)))
        kw = dict(start={n: x0[:, j] for j, n in enumerate(NAMES4)}, max_iter=MAX_ITER_EPS, restarts=0)
        ref = FD.best_fit(target, PARAMS, **kw)
        print(f"{what}: seed {seed}, smallest margin of the mirror's comparisons {ref.margin.min():.3g} (MARGIN {MARGIN:g})")
        if ref.margin.min() > MARGIN:
            break
    assert ref.margin.min() > MARGIN, ref.margin                      # a condition on the inputs, not on the code under test
    figures(ref, what)
    return ref, target.best_fit(PARAMS, **kw)


def test_epsilon_sampled_data_vector(data_fit):
    """d = 4, R = 1: the five-row launches.  Status, iteration and evaluation counts and the bytes of x identical - the device
    returns no decision list, and these agree only if every decision did; lnL and chi2 to the rounding bound of
    tests/tolerances.py."""
    ref, dev = margin_conditioned(data_fit, 1, "epsilon sampled, data vector")
    assert dev.names == NAMES4 and set(ref.launches) == {5}
    same_fit(dev, ref, "epsilon sampled, data vector", ("status", "n_iter", "n_evals", "x"))
    bound = chi2_bound(data_fit, dev.point(0))
    assert_same_chi2(dev.chi2, ref.chi2, bound, what="epsilon sampled, data vector: device vs mirror")
    assert_same_lnl(dev.lnl, ref.lnl, bound, what="epsilon sampled, data vector: device vs mirror")


def test_epsilon_sampled_realisations(fit):
    import victor_amd
    numbers = [0, 5, 11]
    ref, dev = margin_conditioned(fit.realisations(numbers), 3, "epsilon sampled, realisations")
    assert dev.names == NAMES4 and ref.launches[0] == 15
    same_fit(dev, ref, "epsilon sampled, realisations", ("status", "n_iter", "n_evals", "x"))
    bound = np.array([chi2_bound(victor_amd.CCFFit(*stack_options(simulation_number=m)), dev.point(i))[0] for i, m in enumerate(numbers)])
    assert_same_chi2(dev.chi2, ref.chi2, bound, what="epsilon sampled, realisations: device vs mirror")
    assert_same_lnl(dev.lnl, ref.lnl, bound, what="epsilon sampled, realisations: device vs mirror")
