"""The chunked pipeline of the grid and importance posteriors at the chunk sizes the product runs (DESIGN.md sections 7c and 7e,
"Launch shapes under test"): vk_is_run and vk_grid_run at the shapes of ``CHUNKS`` (tests/launch_shapes.py) - chunks of 130 to
8192 rows, so that the rows, max, weight and accumulate kernels run past one workgroup and past one batch of loads in flight, the
tail's filter kernel over several blocks of rows (``blockIdx.y > 0``, uneven cuts, the clamp at 256 slices), its merge kernel
over two to eight batches (the side flips, the list just written is read back, ``h > kBatch``, ``K > kBlock``), the predict
kernel over slices of many rows, and the evaluation behind them in every regime of ``launch_theory`` (the upper cells band,
unfused on partial sums, one workgroup per point, fused again under the gridded covariance, the joint chi-square kernels past
two sort chunks).

The method is that of the neighbouring files, the shapes are new; no bound is.  The device route against the definition route
(``device=False``): maxima, arg max, counts, statuses, best points and everything the tail holds as BYTES; the sums at the
two-route bound of tests/test_importance.py (``assert_sums`` with the row's own chunk count and term counts), the predictive
sums at the bounds of tests/test_gpu_importance_predictive.py, the grid's at those of tests/test_gpu_grid.py - through the
``both_routes`` of those files.  Beside it every row has a reference that no chunked route stands behind: ONE public likelihood
call over the whole sample (all nodes), reduced by a log-sum-exp in ``np.longdouble``, against ``ln_evidence`` within the
per-point bound on lnL of two evaluation orders (``lnl_bound``) plus the sum's own bound.

The samples are those of ``tests.test_gpu_importance.sample_of`` with ``kept=G``: G is exact whatever the generator draws.  The
fits are the neighbouring files' (the synthetic fit with a stack of 3 mocks, N = 80; the BOSS fit; three density-split blocks
under one covariance), made once per module.  No assertion is on elapsed time."""

import faulthandler
import functools
import types

import numpy as np
import pytest

from tests import cases, tolerances
from tests import launch_shapes as LS
from tests import test_gpu_grid as GG
from tests import test_gpu_importance as GI
from tests import test_gpu_importance_predictive as GP
from tests import test_gpu_importance_tail as GT
from tests import test_gpu_joint_importance as GJ
from tests.test_chains import same_bytes
from tests.test_gpu_importance import Handle, boss, lnl_bound, sample_of  # noqa: F401  (boss: a fixture)
from tests.test_gpu_importance_predictive import SYNTH, case, synth_rs  # noqa: F401  (fixtures)
from tests.test_gpu_joint_sampled import BETA
from tests.test_grid import sum_bound as grid_sum_bound
from tests.test_importance import EXACT, SUMS, Recorder, abs_sums, assert_exact, assert_sums, sum_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "sigma_v", "epsilon"]
NAMES4 = ["fsigma8", "beta", "sigma_v", "epsilon"]
T = LS.thresholds()
IDS = {}                                                     # test function -> its case ids (tests/test_launch_shapes.py reads it)
ROWS = {kind: sorted(k for k, r in LS.CHUNKS.items() if r["kind"] == kind) for kind in ("importance", "grid")}


def table(name, cases_):
    """Parametrise over (row of the table, variant): ids "<row>-<variant>"."""
    IDS[name] = [f"{row}-{variant}" for row, variant in cases_]
    return pytest.mark.parametrize("row,variant", cases_, ids=IDS[name])


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def setting(synth_rs, boss, case):  # noqa: F811
    """row name -> what its calls need: ``obj`` (whose method is called), ``params``, ``names``, ``fixed``, and ``zero`` - the
    fit whose data vector is problem 0's (the bound on lnL reads it).  R problems of the synthetic stack: mock r % 3."""
    fit, lost = synth_rs
    made = {}

    def get(name):
        if name not in made:
            row = LS.CHUNKS[name]
            if row["route"].startswith("synthetic"):
                obj = fit.realisations(np.arange(row["R"]) % 3)
                made[name] = types.SimpleNamespace(obj=obj, params=SYNTH, names=NAMES, fixed={"beta": BETA}, zero=fit, lost=lost, joint=None)
            elif row["route"] == "BOSS data vector":
                made[name] = types.SimpleNamespace(obj=boss, params=PARAMS, names=NAMES4, fixed=None, zero=boss, joint=None)
            else:
                c = case("dsplit_cov")
                made[name] = types.SimpleNamespace(obj=c.joint.realisations([0, 1, 2]), params=PARAMS, names=c.names, fixed=c.fixed, zero=c.joint, joint=c)
            assert (len(made[name].obj) if row["R"] > 1 else 1) == row["R"]
        return made[name]
    return get


@functools.lru_cache(maxsize=None)
def _sample(block, names, kept):
    return sample_of(SYNTH if block == "synth" else PARAMS, list(names), kept=kept)


def call_of(row, s, **more):
    """The keywords of a row's importance call: its sample of exactly G kept points, its chunk, 6 bins and one pair."""
    sample = _sample("synth" if s.params is SYNTH else "cobaya", tuple(s.names), row["G"])
    return dict(chunk=row["chunk"], bins=6, pairs=[(s.names[0], s.names[-1])], min_ess=2.0, fixed=s.fixed, **dict(sample, **more))


def one_call(obj):
    """The object's own likelihood call: (lnL, chi2) of a batch."""
    return obj.log_likelihood if hasattr(obj, "log_likelihood_pairs") else obj.log_likelihood_batch


def whole_batch(ip, fixed):
    batch = {k: np.full(ip.n_inside, float(v)) for k, v in (fixed or {}).items()}
    batch.update({n: np.ascontiguousarray(ip._sample.x[:, j]) for j, n in enumerate(ip.names)})
    return batch


def ran_the_row(ip, row, what):
    assert ip.n_inside == row["G"] and ip.chunk == row["chunk"] and ip.n_chunks == len(LS.chunk_lengths(row)), what
    assert ip.n_problems == row["R"] and ip.n_drawn >= row["G"], what


def longdouble_logsumexp(v):
    v = np.asarray(v, dtype=np.longdouble)
    top = v.max()
    return top + np.log(np.sum(np.exp(v - top)))


def independent(ip, m, lnl, bound, what):
    """Problem ``m`` of ``ip`` against lnL of the whole sample from ONE call, reduced by a log-sum-exp in ``np.longdouble``: the
    allowance of ``tests.test_gpu_importance.independent`` - the per-point bound on lnL, the sum's bound, the roundings of the
    float64 read-out."""
    B = float(np.max(bound))
    lnpost = np.where(np.isfinite(lnl), lnl, -np.inf) + ip._sample.lno
    ln_z = float(longdouble_logsumexp(lnpost) - np.log(np.longdouble(ip.n_drawn)))
    allowed = B + sum_bound("total", ip.n_chunks, ip.n_inside) + 64 * tolerances.U * (1.0 + abs(ln_z))
    margin = abs(ip.ln_evidence[m] - ln_z) / allowed
    print(f"{what}: |ln_evidence - longdouble log-sum-exp of one call| / allowed = {margin:.3e} (per-point bound on lnL {B:.3e})")
    tolerances._record(f"chunk shapes ln_evidence {what}", margin)
    assert margin <= 1.0, (what, ip.ln_evidence[m] - ln_z, allowed)
    assert ip.arg_max[m] == int(np.argmax(lnpost)) or lnpost[ip.arg_max[m]] >= lnpost.max() - B, what


def bound_of(s, batch, lnl):
    if s.joint is not None:
        return GJ.lnl_bound(s.joint, s.zero, batch, lnl)
    return lnl_bound(s.zero, batch, lnl)


def repeated_problems_agree(raw, R, names, what):
    """Problems r and r + 3 are the same mock."""
    for name in names:
        a = getattr(raw, name)
        assert same_bytes(a[:R - 3], a[3:]), (what, name)


# ------------------------------------------------------------------ 1. the plain sums --------------------------------------
@table("test_importance", [(row, "plain") for row in ROWS["importance"]])
def test_importance(setting, row, variant):
    r, s = LS.CHUNKS[row], setting(row)
    what = f"{row} ({r['route']}, R = {r['R']}, chunks {LS.chunk_lengths(r)})"
    kw = call_of(r, s)
    dev = s.obj.importance_posterior(s.params, **kw)
    rec = Recorder(lambda batch: one_call(s.obj)(batch)[0])
    ref = s.obj.importance_posterior(s.params, device=False, evaluate=rec, **kw)
    for ip in (dev, ref):
        ran_the_row(ip, r, what)
    assert dev.names == s.names and np.all(dev.n_finite == r["G"]), what       # (every row is a candidate of the first chunk's tail)
    assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status), what
    for name in dev.names:
        assert same_bytes(dev.best[name], ref.best[name]), (what, name)
    assert_sums(dev.raw, ref.raw, abs_sums(ref, rec.chunks), dev.n_chunks, what, dev._layout, dev._sample.x)
    if r["R"] > 3:
        repeated_problems_agree(dev.raw, r["R"], EXACT + SUMS, what)
    # ... and against one call over the whole sample
    batch = whole_batch(dev, s.fixed)
    lnl = np.asarray(one_call(s.obj)(batch)[0]).reshape(r["G"], -1)[:, 0]
    bound = bound_of(s, batch, lnl)
    independent(dev, 0, lnl, bound, what)
    GI.independent(dev, 0, np.where(np.isfinite(lnl), lnl, -np.inf), bound, what)       # (the neighbouring file's, in float64)


# ------------------------------------------------------------------ 2. the tail ---------------------------------------------
TAILS = [(row, size) for row in ROWS["importance"] for size in LS.CHUNKS[row]["tail"]] + [("I3", "duplicated"), ("I3", "lost")]


def expected_batches(r, K):
    """The batches of the merge of every chunk of a row for a problem whose points are all finite: every row is a candidate
    while fewer than K entries are held; afterwards the number depends on the values."""
    held, out = 0, []
    for n in LS.chunk_lengths(r):
        out.append(len(LS.batches(n, T)) if held < K else None)
        held = min(K, held + n)
    return out


@table("test_tail", TAILS)
def test_tail(setting, row, variant):
    r, s = LS.CHUNKS[row], setting(row)
    what = f"{row} tail {variant} ({r['route']}, R = {r['R']}, chunks {LS.chunk_lengths(r)})"
    if variant == "duplicated":
        # every point twice, side by side: equal values in neighbouring slices of a block of rows and on both sides of a batch edge
        half = _sample("synth", tuple(NAMES), r["G"] // 2)
        kw = dict(call_of(r, s), sample=np.repeat(half["sample"], 2, axis=0), ln_proposal=np.repeat(half["ln_proposal"], 2))
        dev, ref = GT.both_routes(s.obj, s.params, what, 300, **kw)
        t = dev.tail
        ran_the_row(dev, r, what)
        for p in range(r["R"]):
            same = t.lnpost[p, 1:] == t.lnpost[p, :-1]
            assert same.sum() >= 100 and np.all(t.index[p, 1:][same] == t.index[p, :-1][same] + 1), what
        return
    if variant == "lost":
        dev, ref = GT.both_routes(s.lost.realisations(), s.params, what, 300, **call_of(r, s))
        t = dev.tail
        ran_the_row(dev, r, what)
        assert list(t.status == t.NO_FINITE) == [False, True, False] and list(t.count) == [301, 0, 301], what
        assert np.all(t.index[1] == -1) and np.all(t.lnpost[1] == -np.inf) and np.isnan(t.k[1])
        for name in ("total", "sq", "s1", "s2"):
            assert not np.any(np.isnan(t.sums[name])) and np.all(t.sums[name][1] == 0), name
        return
    K = LS.tail_entries(r, variant)
    dev, ref = GT.both_routes(s.obj, s.params, what, variant, **call_of(r, s))
    t = dev.tail
    ran_the_row(dev, r, what)
    print(what, "- batches of the merge per chunk (None: depends on the values):", expected_batches(r, K))
    assert t.size + 1 == K and np.all(t.count == K) and np.all(dev.n_finite == r["G"]), what
    assert np.all(np.diff(t.lnpost, axis=1) <= 0), what
    if variant == "all":
        for p in range(r["R"]):
            assert same_bytes(np.sort(t.index[p]), np.arange(r["G"])), what
    if r["R"] > 3:
        repeated_problems_agree(t, r["R"], ("lnpost", "index", "count", "k"), what)
        assert not same_bytes(t.lnpost[0], t.lnpost[1])


# ------------------------------------------------------------------ 3. the predictive sums ----------------------------------
@table("test_predictive", [(row, "predictive") for row in ROWS["importance"] if LS.CHUNKS[row]["predictive"]])
def test_predictive(setting, row, variant):
    """``both_routes`` of tests/test_gpu_importance_predictive.py; it also asserts that ``EXACT + SUMS`` are the same bytes with
    ``predictive`` on and off - the weights go to a buffer of their own so that the chi-squares survive, whatever regime of the
    evaluator left them."""
    r, s = LS.CHUNKS[row], setting(row)
    what = f"{row} predictive ({r['route']}, R = {r['R']}, chunks {LS.chunk_lengths(r)})"
    kw = call_of(r, s)
    fixed = kw.pop("fixed")
    dev, ref = GP.both_routes(s.obj, s.params, what, fixed=fixed, **kw)
    ran_the_row(dev, r, what)
    off = GP.run(s.obj, s.params, fixed=fixed, **kw)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(dev.raw, name), getattr(off.raw, name)), (what, name)
    if r["R"] > 3:
        repeated_problems_agree(dev.raw, r["R"], ("pt", "ptt"), what)


# ------------------------------------------------------------------ 4. cuts and repeats of one handle -----------------------
@table("test_cuts", [("I3", "cuts")])
def test_cuts(setting, row, variant):
    """One ``vk_is_run(0, G)`` against a run in two cuts at a chunk edge and against a second run of the same handle: the tail
    and all sums as bytes."""
    from victor_amd import importance as I
    r, s = LS.CHUNKS[row], setting(row)
    G, chunk, K = r["G"], r["chunk"], LS.tail_entries(r, 300)
    h = Handle(s.zero, s.params, s.names, realisations=s.obj, fixed=s.fixed, bins=6, pairs=[(s.names[0], s.names[-1])], chunk=chunk, kept=G)
    try:
        assert h.sample.G == G and h.R == r["R"]
        assert h.lib.vk_is_set_tail(h.h, K) == 0, h.error()

        def read():
            return I.read_result(h.lib, h.h, h.layout, h.R, False, None, K)[0]
        assert h.run(0, G) == 0, h.error()
        whole = read()
        assert h.run(0, chunk) == 0, h.error()
        assert h.run(chunk, G - chunk) == 0, h.error()
        cut = read()
        assert h.run(0, G) == 0, h.error()
        again = read()
        assert np.all(whole.n_finite == G) and np.all(whole.tail.count == K)
        for other, text in ((cut, "two cuts"), (again, "a second run")):
            for name in EXACT + SUMS:
                assert same_bytes(getattr(other, name), getattr(whole, name)), (text, name)
            for name in ("lnpost", "index", "count"):
                assert same_bytes(getattr(other.tail, name), getattr(whole.tail, name)), (text, name)
    finally:
        h.close()


# ------------------------------------------------------------------ 5. the grid ---------------------------------------------
GRID_AXES = {"G1": ["fsigma8", "epsilon"], "G2": ["fsigma8", "epsilon"], "G3": ["fsigma8", "beta", "sigma_v"]}


def grid_independent(gp, lnl, lnprior, bound, what):
    """Problem 0 of ``gp`` against lnL of all nodes from ONE call: the midpoint sum in ``np.longdouble``.  ``ln(sum)`` within the
    per-point bound on lnL plus the sum's own bound; ``ln_evidence`` - with a prior over the prior's own midpoint sum, which
    carries that sum's bound once more - plus the roundings of the float64 read-out."""
    grid = gp._grid
    B, rel = float(np.max(bound)), grid_sum_bound(gp.n_chunks, grid.G)
    lnpost = np.where(np.isfinite(lnl), lnl, -np.inf) + (0.0 if lnprior is None else lnprior)
    ln_sum = float(longdouble_logsumexp(lnpost))
    got = gp.ln_max[0] + np.log(gp.raw.total[0])
    if lnprior is None:
        want = ln_sum + np.sum(np.log((grid.b - grid.a) / np.array(grid.shape))) - np.sum(np.log(grid.hi - grid.lo))
        allowed = B + rel + 64 * tolerances.U * (1.0 + abs(want))
    else:
        want = ln_sum - float(longdouble_logsumexp(lnprior))
        allowed = B + 2 * rel + 64 * tolerances.U * (1.0 + abs(want))
    margins = (abs(got - ln_sum) / (B + rel + 64 * tolerances.U * (1.0 + abs(ln_sum))), abs(gp.ln_evidence[0] - want) / allowed)
    print(f"{what}: |ln(sum) - longdouble| / allowed = {margins[0]:.3e}, |ln_evidence - longdouble| / allowed = {margins[1]:.3e}")
    tolerances._record(f"chunk shapes grid ln(sum), ln_evidence {what}", max(margins))
    assert max(margins) <= 1.0, (what, margins)
    assert gp.arg_max[0] == int(np.argmax(lnpost)) or lnpost[gp.arg_max[0]] >= lnpost.max() - B, what


@table("test_grid", [(row, "grid") for row in ROWS["grid"]])
def test_grid(synth_rs, boss, row, variant):  # noqa: F811
    from victor_amd.fitting import _Sampled
    from victor_amd.grid import GridPosterior
    from victor_amd.priors import GaussianPrior
    r = LS.CHUNKS[row]
    names = GRID_AXES[row]
    what = f"{row} ({r['route']}, R = {r['R']}, bins {r['bins']}, chunks {LS.chunk_lengths(r)})"
    bins = dict(zip(names, r["bins"]))
    pairs = [(names[a], names[b]) for a, b in r["pairs"]]
    prior = None
    if r["route"] == "BOSS data vector":
        obj = zero = boss
        params, fixed = PARAMS, {"epsilon": 1.0}
        kw = dict(ranges=GG.ranges_of(names))
        if r.get("prior"):
            prior = GaussianPrior(["fsigma8", "beta"], [0.45, 0.4], cov=[[0.05 ** 2, 0.5 * 0.05 * 0.04], [0.5 * 0.05 * 0.04, 0.04 ** 2]])
            kw["prior"] = prior
    else:
        zero = synth_rs[0]
        obj = zero.realisations(np.arange(r["R"]) % 3)
        params, fixed, kw = GG.SYNTH, {"beta": BETA}, {}
    dev, ref = GG.both_routes(obj, params, what, bins=bins, pairs=pairs, chunk=r["chunk"], fixed=fixed, **kw)
    assert dev.names == names and dev.shape == tuple(r["bins"]) and dev.n_chunks == len(LS.chunk_lengths(r)) and dev.chunk == r["chunk"], what
    assert dev.n_problems == r["R"] and np.all(dev.n_finite == r["G"]), what
    if prior is not None:
        assert same_bytes(dev.prior_ln_max, ref.prior_ln_max), what
        assert abs(dev.prior_total - ref.prior_total) <= grid_sum_bound(dev.n_chunks, r["G"]) * ref.prior_total, what
    if r["R"] > 3:
        repeated_problems_agree(dev.raw, r["R"], GG.ACCS, what)
    # ... and against one call over all nodes
    x = dev._grid.points(np.arange(r["G"]))
    batch = {k: np.full(r["G"], float(v)) for k, v in dict({k: v for k, v in params.items() if isinstance(v, (int, float))}, **fixed).items()}
    batch.update({n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names)})
    lnl = np.asarray(one_call(obj)(batch)[0]).reshape(r["G"], -1)[:, 0]
    bound = lnl_bound(zero, batch, lnl)
    lnprior = None if prior is None else _Sampled("grid_posterior", "gridded", params, fixed).prior(prior, obj).lnprior(x)
    grid_independent(dev, lnl, lnprior, bound, what)
    if prior is None:                                            # the marginals too: problem 0 as a posterior of its own
        acc = type(dev.raw)(dev._grid, 1)
        for name in GG.ACCS:
            setattr(acc, name, getattr(dev.raw, name)[:1])
        GG.independent(GridPosterior(dev._grid, acc, None, dev.chunk), lnl, bound, what)
