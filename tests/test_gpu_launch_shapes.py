"""The device step loops past one workgroup and across the evaluator's batch-size regimes ("Launch shapes
under test"): Metropolis chains, stretch ensembles, replica exchange and the optional per-handle state at the shapes of
tests/launch_shapes.py - three and more workgroups of one wave, ensembles and swap pairs across a workgroup edge, and every
regime of ``launch_theory`` a step can meet (ranges of 256 / 512 / 1024 cells, one workgroup per point, chi-square fused and in a
launch of its own, the joint routes) inside blocks of up to 64 steps enqueued without a host synchronisation.

The method is that of the neighbouring files, the shapes are new.  With epsilon fixed both routes launch the same bytes of rows,
so the device route is compared with the definition route (``device=False``) by ``same_bytes``, through the helpers of the test
of each move: ``same_run`` of tests/test_gpu_priors.py, ``same_tempered`` of tests/test_gpu_tempering.py, ``assert_sums``,
``same_marginals``, ``same_series``; the predictive sums of O1 at the DERIVED BOUNDS of tests/test_gpu_predictive.py
(``check_history`` / ``check_routes``: not bytes - the two routes' pivots differ to rounding).  Beside it every case has a check
that does not go through the definition loop: the final position of every chain is evaluated again in one call of as many rows
as a launch of the loop has - hence by the same launches - and must return the handle's final lnL and chi2 in bytes (for
tempered runs every rung, lnL untempered; for the stretch move a call per half, whose walkers' values come from half-launches,
conditioned on every walker having moved at least once).

Each case first asserts, on the definition route's run alone, that the run reached what the case is about (``reached``,
``exercised`` of tests/test_gpu_tempering.py): conditions on the inputs, checked before the device route runs.  Sampled
dispersions live in the narrow box of tests/test_gpu_priors.py (350 .. 400 km/s, proposal width 10) so that proposals leave the
box in every run.  Step counts: 130 = two blocks of 64 and two, burn 10, thin 2, up to 600 chains; 66 above.  No assertion is on
elapsed time.
"""

import faulthandler

import numpy as np
import pytest

from tests import cases
from tests import launch_shapes as LS
from tests.test_chains import assert_sums, same_bytes
from tests.test_gpu_chains import same_series
from tests.test_gpu_joint_sampled import Case
from tests.test_gpu_priors import BETA, NARROW, Five, boss_prior, same_run
from tests.test_gpu_tempering import FIXED as TEMPER_FIXED, exercised, prior2, same_tempered
from tests.test_marginals import same_marginals
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
EPS_FIXED = {"epsilon": 1.0}
T = LS.thresholds()
CUTS = dict(seed=2, burn=10, thin=2)
STATES = dict(marginals={"bins": 16, "pairs": "all", "bins2d": 8}, autocorr={"max_lag": 16})
IDS = {}                                                     # test function -> its case ids (tests/test_launch_shapes.py reads it)


def table(name, *cases_):
    """Parametrise over (row of the table, variant): ids "<row>-<variant>"."""
    IDS[name] = [f"{row}-{variant}" for row, variant in cases_]
    return pytest.mark.parametrize("row,variant", cases_, ids=IDS[name])


def shape(row, **pick):
    """The variant of a table row with the given move / W."""
    (v,) = [v for v in LS.variants(LS.TABLE[row]) if all(v[k] == w for k, w in pick.items())]
    return v


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
def mocks(fit):
    """R problems on the 16-mock stack: mock r % 16 for problem r (the precedent of tests/test_gpu_fit_definition.py)."""
    made = {}

    def get(R):
        if R not in made:
            made[R] = fit.realisations(np.arange(R) % 16)
        return made[R]
    return get


@pytest.fixture(scope="module")
def data_fit():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


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


# ------------------------------------------------------------------ what every case does ------------------------------------------
def reached(ref, what, stretch=False):
    """Conditions on the inputs, on the definition route's run: every problem's pooled acceptance strictly between 0 and 1, and
    at least one proposal outside the box.  Stretch move: every walker moved, so that its lnL comes from a half-launch."""
    print(what, "- definition route: acceptance", float(ref.acceptance.min()), "..", float(ref.acceptance.max()), "; outside the box",
          int(ref.n_outside.sum()), "of", ref.n_steps * ref.R * ref.W, "; smallest margin", ref.decision_margin)
    assert np.all((0.0 < ref.acceptance) & (ref.acceptance < 1.0)), (what, ref.acceptance)
    assert ref.n_outside.sum() > 0, (what, "no proposal left the box: the test does not reach that rule")
    if stretch:
        assert np.all(ref.n_accept > 0), (what, "a walker never moved: its lnL is the start's, from a launch of another size")


def points(ch, x):
    p = dict(ch.fixed)
    p.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(ch.names)})
    return p


def evaluate(target, ch, x, which):
    """One call of len(x) rows: pairs mode against the problems ``which``, or the data vector(s)."""
    if hasattr(target, "log_likelihood_pairs"):
        return target.log_likelihood_pairs(points(ch, x), which.astype(np.int32))
    return target.log_likelihood_batch(points(ch, x))


def final_state_is_the_likelihoods(target, ch, what):
    """Not through the definition loop: the chains' final positions in one call of the loop's row count against the final state."""
    if ch.tempering is not None:
        q = ch.tempering
        x, lnl, chi2 = q.x, q.lnl, q.chi2                               # (R, K, W, d): chain c = (r K + k) W + w
    else:
        x, lnl, chi2 = ch.x, ch.lnl, ch.chi2
    d = x.shape[-1]
    x, lnl, chi2 = x.reshape(-1, d), lnl.ravel(), chi2.ravel()
    which = np.repeat(np.arange(ch.R), len(x) // ch.R)
    if ch.move == "stretch":
        half = ch.W // 2
        sets = [((2 * np.arange(ch.R)[:, None] + side) * half + np.arange(half)).ravel() for side in (0, 1)]      # stretch_walker
    else:
        sets = [np.arange(len(x))]
    for rows in sets:
        got_l, got_c = evaluate(target, ch, x[rows], which[rows])
        assert same_bytes(got_l, lnl[rows]), (what, "lnl", int(np.sum(got_l != lnl[rows])), float(np.nanmax(np.abs(got_l - lnl[rows]))))
        assert same_bytes(got_c, chi2[rows]), (what, "chi2", int(np.sum(got_c != chi2[rows])), float(np.nanmax(np.abs(got_c - chi2[rows]))))
    assert np.all(np.isfinite(lnl)) and np.all(chi2 > 0.0), what


def moment_sums(ch, what):
    """``assert_sums`` forms exact sums in rationals, chain by chain: every chain of a problem up to 600 of them; above, its
    first two and last two workgroups of chains and every 61st in between (each thread sums its own chain: what a wrong index
    would do to the others shows in the byte comparisons)."""
    W = ch.W
    pick = np.arange(W) if W <= LS.MANY_CHAINS else np.unique(np.concatenate([np.arange(128), np.arange(W - 128, W), np.arange(0, W, 61)]))
    for m in range(ch.R):
        assert_sums(ch.sum1[m][pick], ch.sum2[m][pick], ch.chain[:, m][:, pick], ch.pivot[m][pick], f"{what}: device sums, problem {m}")


def both_routes(target, block, v, what, conditions=reached, **kw):
    """(definition route, device route) of the variant ``v``: the definition route first, its conditions before the device runs."""
    n = LS.steps(v)
    kw = dict(CUTS, walkers=v["W"], **kw)
    if v["move"] == "stretch":
        kw["move"] = "stretch"
    ref = target.sample_chains(block, n, device=False, **kw)
    assert ref.R == v["R"] and ref.W == v["W"] and ref.n_steps == n and ref.n_kept == (n - 10 + 1) // 2
    if conditions is reached:
        reached(ref, what, stretch=v["move"] == "stretch")
    else:
        conditions(ref)
    dev = target.sample_chains(block, n, **kw)
    assert dev.decision_margin is None and dev.n_outside is None        # the device route ran
    return ref, dev


def plain_comparison(target, dev, ref, what):
    same_run(dev, ref, what)
    assert np.array_equal(dev._n_accept, ref._n_accept) and np.array_equal(dev._n_kept, ref._n_kept), what
    moment_sums(dev, what)
    final_state_is_the_likelihoods(target, dev, what)


def fuse_of(data_fit, m, what):
    """The last evaluation of the engine, against what the row count predicts."""
    from tests.test_gpu_predictive import engine_of
    eng = engine_of(data_fit)
    instance, is_fused = eng.last_instance(), eng.last_fused()
    print(what, m, "rows:", instance)
    assert instance.startswith("cells"), (what, instance)
    assert is_fused == LS.fused(m, T) and instance.endswith("+fused") == LS.fused(m, T), (what, m, instance)


# ------------------------------------------------------------------ M: Metropolis ------------------------------------------------
@table("test_metropolis_on_mocks", ("M1", "plain"), ("M1", "prior"), ("M2", "plain"), ("M3", "plain"))
def test_metropolis_on_mocks(mocks, row, variant):
    v = shape(row)
    rs = mocks(v["R"])
    prior = boss_prior() if variant == "prior" else None
    ref, dev = both_routes(rs, NARROW, v, f"{row} {variant}", fixed=EPS_FIXED, prior=prior)
    assert dev.chain.shape == (ref.n_kept, v["R"], v["W"], 3)
    plain_comparison(rs, dev, ref, f"{row} {variant}")
    if prior is not None:
        assert np.all(dev.lnprior_chain < 0.0)


@table("test_metropolis_on_the_data_vector", *[("M4", str(w)) for w in LS.TABLE["M4"]["W"]])
def test_metropolis_on_the_data_vector(data_fit, row, variant):
    v = shape(row, W=int(variant))
    what = f"{row} W = {variant}"
    n = LS.steps(v)
    kw = dict(CUTS, walkers=v["W"], fixed=EPS_FIXED)
    ref = data_fit.sample_chains(NARROW, n, device=False, **kw)
    fuse_of(data_fit, v["W"], what + ", definition route")
    reached(ref, what)
    dev = data_fit.sample_chains(NARROW, n, **kw)
    fuse_of(data_fit, v["W"], what + ", device route")
    assert dev.chain.shape == ((n - 10 + 1) // 2, 1, v["W"], 3) and dev.n_outside is None
    plain_comparison(data_fit, dev, ref, what)
    fuse_of(data_fit, v["W"], what + ", one call")


# ------------------------------------------------------------------ S: the stretch move ------------------------------------------
@table("test_stretch_on_mocks", ("S1", "plain"), ("S1", "prior"), ("S2", "plain"))
def test_stretch_on_mocks(mocks, row, variant):
    v = shape(row)
    rs = mocks(v["R"])
    prior = boss_prior() if variant == "prior" else None
    ref, dev = both_routes(rs, NARROW, v, f"{row} {variant}", fixed=EPS_FIXED, prior=prior)
    assert dev.move == "stretch" and dev.chain.shape == (60, v["R"], v["W"], 3)
    plain_comparison(rs, dev, ref, f"{row} {variant}")


@table("test_stretch_on_the_data_vector", ("S3", "plain"))
def test_stretch_on_the_data_vector(data_fit, row, variant):
    v = shape(row)
    ref, dev = both_routes(data_fit, NARROW, v, row, fixed=EPS_FIXED)
    fuse_of(data_fit, LS.rows(v), row + ", device route")
    assert dev.move == "stretch" and dev.chain.shape == (28, 1, v["W"], 3)
    plain_comparison(data_fit, dev, ref, row)
    fuse_of(data_fit, LS.rows(v), row + ", one call per half")


# ------------------------------------------------------------------ T: replica exchange ------------------------------------------
def tempered(target, v, what, **kw):
    ladder = v["temper"]
    ref, dev = both_routes(target, PARAMS, v, what, temper=ladder, fixed=TEMPER_FIXED,
                           conditions=lambda ref: exercised(ref, v["K"], LS.steps(v), ladder["swap_every"], what), **kw)
    assert dev.tempering.chain.shape == (60, v["R"], v["K"], v["W"], 2) and LS.chains(v) == dev.tempering.x[..., 0].size
    same_tempered(dev, ref, what)
    final_state_is_the_likelihoods(target, dev, what)
    return ref, dev


@table("test_tempered_on_mocks", ("T1", "plain"), ("T1", "prior"), ("T1", "states"), ("T2", "plain"))
def test_tempered_on_mocks(mocks, row, variant):
    v = shape(row)
    what = f"{row} {variant}"
    more = dict(prior=prior2()) if variant == "prior" else STATES if variant == "states" else {}
    ref, dev = tempered(mocks(v["R"]), v, what, **more)
    if variant == "prior":
        assert same_bytes(dev.lnprior_chain, ref.lnprior_chain) and np.all(dev.lnprior_chain < 0.0)
    if variant == "states":                                  # the cold rung's histograms (as integers) and series (bytes)
        same_marginals(dev.marginals, ref.marginals, what)
        assert np.all(dev.marginals.n == dev.n_kept * v["W"])
        same_series(dev, ref, what)
        for k in ("tau", "window", "ess", "acf"):
            assert same_bytes(getattr(dev.autocorr, k), getattr(ref.autocorr, k)), (what, k)


@table("test_tempered_on_the_data_vector", ("T3", "plain"))
def test_tempered_on_the_data_vector(data_fit, row, variant):
    v = shape(row)
    tempered(data_fit, v, row)
    fuse_of(data_fit, LS.rows(v), row)


# ------------------------------------------------------------------ O: the optional states on one handle --------------------------
@table("test_marginals_autocorr_and_predictive", ("O1", "metropolis"), ("O1", "stretch"))
def test_marginals_autocorr_and_predictive(fit, mocks, row, variant):
    from tests.test_gpu_predictive import check_history, check_routes, theory_at
    from tests.tolerances import assert_same_theory
    v = shape(row, move=variant)
    what = f"{row} {variant}"
    rs = mocks(v["R"])
    ref, dev = both_routes(rs, NARROW, v, what, fixed=EPS_FIXED, predictive=True, **STATES)
    plain_comparison(rs, dev, ref, what)
    same_marginals(dev.marginals, ref.marginals, what)                  # integers
    assert dev.marginals.n.tolist() == [60 * v["W"]] * v["R"] and len(dev.marginals.counts2d) == 3
    same_series(dev, ref, what)                                         # bytes: state and read-out
    assert dev.autocorr.n == 60
    for k in ("tau", "window", "ess", "acf"):
        assert same_bytes(getattr(dev.autocorr, k), getattr(ref.autocorr, k)), (what, k)
    # the predictive sums: the derived bounds of tests/test_gpu_predictive.py, not bytes
    bounds = check_history(fit, dev, f"launch shapes {what}, device")
    check_routes(dev, ref, bounds, f"launch shapes {what}")
    C_ = LS.chains(v)
    assert_same_theory(dev.predictive.state["held"], theory_at(fit, dev, dev.x.reshape(C_, 3)), f"predictive held, launch shapes {what}")


# ------------------------------------------------------------------ J: joint fits ----------------------------------------------
@table("test_joint_fits", ("J1", "metropolis"), ("J1", "stretch"), ("J2", "plain"), ("J3", "plain"), ("J4", "plain"))
def test_joint_fits(case, row, variant):
    v = shape(row, **({"move": variant} if row == "J1" else {}))
    what = f"{row} {variant}"
    c = case(v["route"].split()[0])
    if v["route"].endswith("data"):
        target = c.joint
    else:
        target = c.jr if v["R"] == len(c.jr) else c.joint.realisations(list(range(v["R"])))
    ref, dev = both_routes(target, NARROW, v, what, fixed=dict(c.fixed, epsilon=1.0))
    assert dev.names == c.without("epsilon") and dev.chain.shape[1:] == (v["R"], v["W"], len(c.names) - 1)
    plain_comparison(target, dev, ref, what)


@table("test_joint_fit_of_ten_parameters", ("J5", "plain"))
def test_joint_fit_of_ten_parameters(five, row, variant):
    from tests.test_gpu_priors import resolved
    from tests.test_gpu_ten_parameters import TEN, full_prior
    from victor_amd.joint import per_block
    v = shape(row)
    jr = five.joint.realisations(list(range(v["R"])))
    ref, dev = both_routes(jr, per_block(NARROW, ["fsigma8", "sigma_v"], 5), v, row, fixed={"beta": BETA, "epsilon": 1.0}, prior=full_prior())
    assert dev.names == TEN and dev.chain.shape == (60, v["R"], v["W"], 10)
    plain_comparison(jr, dev, ref, row)
    assert same_bytes(dev.lnprior_chain, resolved(full_prior(), TEN, NARROW).lnprior(dev.chain)) and np.all(dev.lnprior_chain < 0.0)
