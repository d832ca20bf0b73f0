"""The tail of an importance sample selected on the GPU (``tail=``: vk_is_set_tail, vk_is_tail_filter_kernel and
vk_is_tail_merge_kernel) against the NumPy route that defines it (``device=False``: rule 7 of victor_amd/importance.py over the
object's own likelihood call, a stable sort per chunk).  The held values, their points, the counts, the fitted shapes and the
statuses are compared as BYTES: the selection is exact and its order total, so neither the chunk nor the slot a candidate took
may show.  With the keyword every array ``vk_is_result`` returned before is the same bytes as without it.

The smoothed ``total``, ``sq``, ``s1`` and ``s2``: the correction is one ``np.longdouble`` number computed on the host from bytes
both routes share, added to sums that differ between the routes as tests/test_importance.py derives - so the corrected sums are
held to that file's two-route bound (:func:`tests.test_importance.assert_sums`, the scale A from the definition route's own
absolute terms), with nothing added.

Shapes: the synthetic fit (N = 80) with 3 mocks, 200 draws in chunks of 64 (four chunks, the last partial).  ``size`` 7: below
the chunk, a threshold after the first chunk (the steady-state path); 100: above the chunk, no threshold for two chunks; G - 1:
the whole sample, never a threshold; the data vector (R = 1); R = 70 from repeated mocks (past one wave of problems, identical
columns); a mock without a finite point; duplicated points; a Gaussian prior; ``predictive=True`` beside it; a raw handle run
twice and in cuts, with the refusals of the two entry points; joint realisations under one covariance."""

import ctypes as C
import faulthandler
import types

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_importance import Handle, synth  # noqa: F401  (synth: a fixture)
from tests.test_gpu_importance_predictive import JOINT_KW, SYNTH, SYNTH_KW, case, proposal, synth_rs  # noqa: F401  (fixtures)
from tests.test_gpu_joint_sampled import BETA
from tests.test_importance import EXACT, SUMS, Recorder, abs_sums, assert_sums

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "sigma_v", "epsilon"]
HELD = ("lnpost", "index", "count", "n_tail", "k", "scale", "status", "weight", "smoothed_weight")
FIGURES = ("ln_evidence", "ln_evidence_error", "ess", "max_weight_share", "mean", "cov", "sigma", "status")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def sort_of(lnpost, K):
    """The K first entries of every column of ``lnpost`` (G, R) in the total order, from one ``np.lexsort`` each."""
    lnpost = np.where(np.isfinite(lnpost), lnpost, -np.inf)
    G, R = lnpost.shape
    values, points = np.full((R, K), -np.inf), np.full((R, K), -1, dtype=np.int64)
    for r in range(R):
        order = np.lexsort((np.arange(G), -lnpost[:, r]))[:K]
        keep = order[lnpost[order, r] > -np.inf]
        values[r, :len(keep)], points[r, :len(keep)] = lnpost[keep, r], keep
    return values, points


def both_routes(obj, params, what, size, q=None, **kw):
    """The device route and the definition route of one call with ``tail``, compared; the device route once more without it.
    ``size``: M, None for the default, or ``"all"`` for G - 1; ``q``: the proposal (None: ``sample=`` and ``ln_proposal=``).
    Returns ``(dev, ref)``."""
    off = obj.importance_posterior(params, q, **kw)
    assert off.tail is None and not hasattr(off.raw, "tail")
    G = off.n_inside
    tail = True if size is None else {"size": G - 1 if size == "all" else size}
    dev = obj.importance_posterior(params, q, tail=tail, **kw)
    one = obj.log_likelihood if hasattr(obj, "log_likelihood_pairs") else obj.log_likelihood_batch
    rec = Recorder(lambda batch: one(batch)[0])
    ref = obj.importance_posterior(params, q, tail=tail, device=False, evaluate=rec, **kw)
    for name in EXACT + SUMS:                                    # the keyword on or off: what vk_is_result returned before
        assert same_bytes(getattr(dev.raw, name), getattr(off.raw, name)), (what, name)
    for name in FIGURES:
        assert same_bytes(getattr(dev, name), getattr(off, name)), (what, name)
    assert dev.n_problems == ref.n_problems and dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks and dev.n_inside == ref.n_inside == G
    for name in EXACT:
        assert same_bytes(getattr(dev.raw, name), getattr(ref.raw, name)), (what, name)
    t, q = dev.tail, ref.tail
    assert t.size == q.size and t.lnpost.shape == (dev.n_problems, t.size + 1) and t.index.dtype == np.int64
    for name in HELD:
        assert same_bytes(getattr(t, name), getattr(q, name)), (what, name)
    # ... and both are the sort of the whole sample
    lnpost = np.concatenate([c.reshape(len(c), -1) for c in rec.chunks], axis=0) + ref._sample.lno[:, None]
    values, points = sort_of(lnpost, t.size + 1)
    assert same_bytes(t.lnpost, values) and same_bytes(t.index, points), what
    assert same_bytes(t.count, np.minimum(t.size + 1, dev.n_finite)), what
    live = dev.n_finite > 0
    assert same_bytes(t.lnpost[live, 0], dev.ln_max[live]) and same_bytes(t.index[live, 0], dev.arg_max[live]), what
    # the smoothed sums at the two-route bound of the raw ones
    sums = [types.SimpleNamespace(h1=ip.raw.h1, h2=ip.raw.h2, **ip.tail.sums) for ip in (dev, ref)]
    assert_sums(sums[0], sums[1], abs_sums(ref, rec.chunks), dev.n_chunks, f"smoothed sums, {what}", dev._layout, dev._sample.x)
    for name in ("ln_evidence", "ess", "mean", "sigma"):
        a, b = getattr(t, name), getattr(q, name)
        assert np.allclose(a[live], b[live], rtol=1e-9, atol=1e-12), (what, name)
    print(f"{what}: M = {t.size}, count {t.count[:4]}, k {np.round(t.k[:4], 3)}, status {t.status[:4]}, raw - smoothed ln_evidence "
          f"{(dev.ln_evidence[live] - t.ln_evidence[live])[:4]}")
    return dev, ref


KW = dict(fixed={"beta": BETA}, **SYNTH_KW)
Q = proposal(NAMES)


# ------------------------------------------------------------------ 1. the synthetic fit -----------------------------------
@pytest.mark.parametrize("size", [7, 100, "all"])
def test_three_mocks(synth_rs, size):
    fit, _ = synth_rs
    dev, ref = both_routes(fit.realisations(), SYNTH, f"synthetic, 3 mocks, size {size}", size, q=Q, **KW)
    t = dev.tail
    assert dev.n_problems == 3 and dev.n_chunks == 4 and dev.n_inside % 64 != 0 and dev.chunk == 64
    assert np.all(t.count == t.size + 1) and np.all(np.isfinite(t.k)) and np.all(t.n_tail == t.size)
    assert np.all((t.status == t.OK) | (t.status == t.HIGH_K))
    assert not same_bytes(t.lnpost[0], t.lnpost[1]) and not same_bytes(t.ln_evidence, dev.ln_evidence)
    if size == "all":
        for r in range(3):
            assert sorted(t.index[r]) == list(range(dev.n_inside))


def test_data_vector(synth_rs):
    fit, _ = synth_rs
    dev, ref = both_routes(fit, SYNTH, "synthetic data vector, default size", None, q=Q, **KW)
    G = dev.n_inside
    assert dev.n_problems == 1 and dev.tail.size == min(int(0.2 * G), int(np.ceil(3 * np.sqrt(G)))) and dev.tail.count[0] == dev.tail.size + 1


def test_seventy_problems_from_repeated_mocks(synth_rs):
    fit, _ = synth_rs
    rs70 = fit.realisations(np.arange(70) % 3)
    dev, ref = both_routes(rs70, SYNTH, "synthetic, R = 70", 20, q=Q, **KW)
    t = dev.tail
    assert dev.n_problems == 70
    for name in ("lnpost", "index", "count", "k", "ln_evidence", "ess"):
        a = getattr(t, name)
        assert same_bytes(a[:67], a[3:]), name
    assert not same_bytes(t.lnpost[0], t.lnpost[1])


def test_a_mock_without_a_finite_point(synth_rs):
    _, lost = synth_rs
    dev, ref = both_routes(lost.realisations(), SYNTH, "synthetic, mock 1 without a finite point", 30, q=Q, **KW)
    t = dev.tail
    assert list(t.status == t.NO_FINITE) == [False, True, False] and list(t.count) == [31, 0, 31]
    assert np.all(t.index[1] == -1) and np.all(t.lnpost[1] == -np.inf) and np.isnan(t.k[1])
    for name in ("total", "sq", "s1", "s2"):
        assert not np.any(np.isnan(t.sums[name])) and np.all(t.sums[name][1] == 0), name
    assert t.ln_evidence[1] == -np.inf and t.ess[1] == 0


def test_duplicated_points(synth_rs):
    from victor_amd import GaussianProposal
    fit, _ = synth_rs
    pts = np.repeat(GaussianProposal.draw(Q.mean, Q.chol, None, 90, 8), 2, axis=0)          # every point twice, side by side
    lnq = GaussianProposal.ln_density(pts, Q.mean, Q.chol, None)
    dev, ref = both_routes(fit.realisations(), SYNTH, "duplicated points", 40, sample=pts, ln_proposal=lnq, fixed={"beta": BETA},
                           chunk=64, bins=6, min_ess=2.0)
    t = dev.tail
    assert dev.n_chunks >= 2
    for r in range(3):
        same = t.lnpost[r, 1:] == t.lnpost[r, :-1]
        assert same.sum() >= 15 and np.all(t.index[r, 1:][same] == t.index[r, :-1][same] + 1)


def test_gaussian_prior(synth_rs):
    from victor_amd.priors import GaussianPrior
    fit, _ = synth_rs
    prior = GaussianPrior(["fsigma8"], [0.45], sigma=[0.03])
    rs = fit.realisations()
    dev, ref = both_routes(rs, SYNTH, "synthetic with a Gaussian prior", 25, prior=prior, q=Q, **KW)
    plain = rs.importance_posterior(SYNTH, Q, tail={"size": 25}, **KW)
    assert dev.tail.lnpost.shape == (3, 26) and not same_bytes(dev.tail.lnpost, plain.tail.lnpost)      # the prior's own problem keeps no tail
    norm = dev.prior_ln_max + np.log(dev.prior_total)
    assert same_bytes(dev.tail.ln_evidence, dev.ln_max + np.log(dev.tail.sums["total"]) - norm)


def test_beside_the_predictive_sums(synth_rs):
    fit, _ = synth_rs
    rs = fit.realisations()
    dev, ref = both_routes(rs, SYNTH, "synthetic, for predictive", 12, q=Q, **KW)
    both = rs.importance_posterior(SYNTH, Q, tail={"size": 12}, predictive=True, **KW)
    pred = rs.importance_posterior(SYNTH, Q, predictive=True, **KW)
    host = rs.importance_posterior(SYNTH, Q, tail={"size": 12}, predictive=True, device=False, **KW)
    for name in HELD:
        assert same_bytes(getattr(both.tail, name), getattr(dev.tail, name)), name
        assert same_bytes(getattr(both.tail, name), getattr(host.tail, name)), name
    for name in EXACT + SUMS + ("pt", "ptt", "dev", "pivot_t", "pivots"):
        assert same_bytes(getattr(both.raw, name), getattr(pred.raw, name)), name
    assert same_bytes(both.predictive.dic, pred.predictive.dic) and pred.tail is None
    for name in ("total", "sq", "s1", "s2"):
        assert same_bytes(both.tail.sums[name], dev.tail.sums[name]), name


# ------------------------------------------------------------------ 2. a raw handle ----------------------------------------
def test_two_runs_cuts_and_refusals_of_one_handle(synth):
    from victor_amd import importance as I
    h = Handle(synth, SYNTH, NAMES, chunk=7)
    lib, G = h.lib, h.sample.G
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    try:
        assert G == 23
        for bad in (1, -3, 4097, G + 1):
            assert lib.vk_is_set_tail(h.h, bad) != 0 and "vk_is_set_tail" in h.error()
        assert lib.vk_is_tail(h.h, None, None, None) != 0 and "keeps no tail" in h.error()
        plain = (h.run(0, G), h.result()[0])[1]
        assert lib.vk_is_set_tail(h.h, 9) == 0
        assert lib.vk_is_tail(h.h, None, None, None) != 0 and "has reached 0 of 23" in h.error()      # the setter starts the run over
        assert h.run(0, G) == 0, h.error()

        def read(K):
            return I.read_result(lib, h.h, h.layout, h.R, h.sample.lnop is not None, None, K)[0]
        first = read(9)
        for name in EXACT + SUMS:
            assert same_bytes(getattr(first, name), getattr(plain, name)), name
        assert np.all(first.tail.count == 9) and first.tail.index[0, 0] == first.arg_max[0] and first.tail.lnpost[0, 0] == first.ln_max[0]
        assert np.all(np.diff(first.tail.lnpost[0]) <= 0) and len(set(first.tail.index[0])) == 9
        assert h.run(0, G) == 0, h.error()                       # a second run of the same handle
        again = read(9)
        assert h.run(0, 14) == 0, h.error()                      # ... and one in two cuts
        assert lib.vk_is_tail(h.h, None, None, None) != 0 and "has reached 14 of 23" in h.error()
        assert lib.vk_is_set_tail(h.h, 5) != 0 and "a run is under way" in h.error()
        assert h.run(14, G) == 0, h.error()
        cut = read(9)
        for other in (again, cut):
            for name in ("lnpost", "index", "count"):
                assert same_bytes(getattr(other.tail, name), getattr(first.tail, name)), name
        # any output may be NULL
        count = np.zeros(1, dtype=np.int64)
        assert lib.vk_is_tail(h.h, None, None, count.ctypes.data_as(lp)) == 0 and count[0] == 9
        # K = G: the whole sample; then off: the state is gone and the run is the parent's
        assert lib.vk_is_set_tail(h.h, G) == 0 and h.run(0, G) == 0, h.error()
        whole = read(G)
        assert sorted(whole.tail.index[0]) == list(range(G)) and same_bytes(whole.tail.lnpost[0, :9], first.tail.lnpost[0])
        assert lib.vk_is_set_tail(h.h, 0) == 0 and h.run(0, G) == 0, h.error()
        out = np.zeros(G)
        assert lib.vk_is_tail(h.h, out.ctypes.data_as(dp), None, None) != 0 and "keeps no tail" in h.error()
        for name in EXACT + SUMS:
            assert same_bytes(getattr(h.result()[0], name), getattr(plain, name)), name
    finally:
        h.close()


# ------------------------------------------------------------------ 3. joint realisations ----------------------------------
def test_joint_realisations_under_one_covariance(case):
    c = case("dsplit_cov")
    jr = c.joint.realisations([0, 1, 2])
    dev, ref = both_routes(jr, PARAMS, "dsplit under one covariance, 3 joint mocks", 10, q=proposal(c.names), fixed=c.fixed, **JOINT_KW)
    assert dev.n_problems == 3 and dev.n_chunks == 3 and np.all(dev.tail.count == 11)
