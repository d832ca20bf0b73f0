"""Importance-sampled posteriors with a proposal per problem reduced on the GPU (victor_amd/importance.py rule 8,
vk_is_create_own) against the NumPy loop that defines them (device=False: one Realisations.log_likelihood_pairs call per chunk,
every problem stepped on its own column): rows bit for bit with epsilon sampled; maxima, arg max, counts, statuses and the held
tail entries as bytes, sums at the derived bounds of tests/test_importance.py, per problem over the points it holds inside the
box; against one independent pairs call over the whole sample and a ``np.longdouble`` log-sum-exp; seventy problems; the prior;
paired-model mocks; identical proposals against the shared route; cuts of vk_is_run; the refusals of the C ABI.  Every problem
draws 23 points about ``CENTRE`` shifted by its own multiple of ``WIDTH``.

The independent check's bounds (:func:`independent`), with B the bound of tests/tolerances.py on lnL of two evaluation orders and
the sum bounds of tests/test_importance.py: a weight ``exp(lnpost - M)`` moves by at most 2 B relative (its own lnpost and M's),
so ``ln_evidence`` by B (a log-sum-exp moves by no more than its largest argument) plus the bound of ``total``; ``ess = total^2 /
sq`` by ``8 B`` plus twice the bound of ``total`` plus that of ``sq``; ``mean - centre = s1 / total`` by ``(4 B + bound(s1) +
bound(total)) sum w |y| / total``."""

import copy
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases, tolerances
from tests.test_chains import same_bytes
from tests.test_gpu_importance import CENTRE, PARAMS, RANGES, WIDTH, lnl_bound
from tests.test_importance import EXACT, SUMS, assert_exact, assert_sums, sum_bound
from tests.test_importance_own import one_problem
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
N23 = 23
NAMES4 = ["fsigma8", "beta", "sigma_v", "epsilon"]
NAMES2 = ["fsigma8", "epsilon"]
FIXED2 = {"beta": 0.37, "sigma_v": 380.0}
# how far, in WIDTHs, the proposals' means spread over the problems: beta reaches 0.24 .. 0.52 in its box [0.2, 0.6], so the
# problems at either end draw points outside it
SPREAD = {"fsigma8": 1.0, "beta": 3.5, "sigma_v": -1.0, "epsilon": 0.5}


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def stack():
    import victor_amd
    return victor_amd.CCFFit(*stack_options())


@pytest.fixture(scope="module")
def rs(stack):
    return stack.realisations()


def proposals(names, R, scale=1.0, spread=1.0):
    """Problem r: ``CENTRE + spread m_r SPREAD WIDTH``, m_r from -1 to 1 over the problems, under the correlated covariance of
    tests/test_gpu_importance.py's sample (times ``scale``^2)."""
    from victor_amd import ProposalSet
    d = len(names)
    cov = np.diag([WIDTH[n] ** 2 for n in names])
    for j in range(1, d):
        cov[0, j] = cov[j, 0] = 0.4 * WIDTH[names[0]] * WIDTH[names[j]]
    m = np.linspace(-1.0, 1.0, R) if R > 1 else np.zeros(1)
    mean = np.array([[CENTRE[n] + spread * m[r] * SPREAD[n] * WIDTH[n] for n in names] for r in range(R)])
    return ProposalSet(names, mean, np.repeat((scale ** 2 * cov)[None], R, axis=0))


class PairsRecorder:
    """An ``evaluate`` callable of the own route over ``Realisations.log_likelihood_pairs`` that keeps lnL chunk by chunk."""

    def __init__(self, rs):
        self.rs, self.chunks = rs, []

    def __call__(self, batch, which):
        v = np.asarray(self.rs.log_likelihood_pairs(batch, which)[0], dtype=np.float64)
        self.chunks.append(v)
        return v


def abs_sums_own(ip, chunks):
    """The sums of the absolute terms of a definition-route result: the definition once more over the same lnL with ``|y|``."""
    from victor_amd.importance import run_definition_own
    s = copy.copy(ip._sample)
    s.y = np.abs(s.y)
    it = iter(chunks)
    return run_definition_own(ip._layout, s, ip._lists, lambda x, which: next(it))[0]


def compare(dev, ref, absolute, what, chunks=None):
    """Two results of the own route: exact outputs as bytes, sums per problem at the bound."""
    assert dev.n_problems == ref.n_problems and dev.n_drawn == ref.n_drawn == N23
    assert np.all(np.asarray(dev.n_inside) == np.asarray(ref.n_inside))
    assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status), what
    smp = ref._sample
    for r in range(dev.n_problems):
        if smp.own:
            inside = smp.x[smp.inside[:, r], r]
        else:
            inside = smp.x
        if not len(inside):
            for name in SUMS:
                assert not np.any(getattr(dev.raw, name)[r]) and not np.any(getattr(ref.raw, name)[r]), (what, r, name)
            continue
        assert_sums(one_problem(dev.raw, r), one_problem(ref.raw, r), one_problem(absolute, r), dev.n_chunks if chunks is None else chunks,
                    f"{what}, problem {r}", dev._layout, inside)
    for name in dev.names:
        assert same_bytes(dev.best[name], ref.best[name]), (what, name)


def both_routes(rs, params, qs, what, **kw):
    dev = rs.importance_posterior(params, qs, n=N23, **kw)
    rec = PairsRecorder(rs)
    ref = rs.importance_posterior(params, qs, n=N23, device=False, evaluate=rec, **kw)
    assert dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks == len(rec.chunks) and dev.proposals is qs
    compare(dev, ref, abs_sums_own(ref, rec.chunks), what)
    if dev.tail is not None:
        for name in ("lnpost", "index", "count", "status", "n_tail"):
            assert same_bytes(getattr(dev.tail, name), getattr(ref.tail, name)), (what, "tail", name)
    return dev, ref, rec


class Handle:
    """A raw vk_is handle of the own route (victor_amd.importance.create_own_handle), for what the public route does not expose."""

    def __init__(self, fit, rs, params, names, qs, fixed=None, bins=4, ranges=None, pairs=None, chunk=7, spoil=None, which=None):
        from victor_amd import importance as I
        from victor_amd.fitting import _Sampled
        q = _Sampled("importance_posterior", "sampled", params, fixed)
        assert q.names == names
        self.layout = I.resolve_layout("test", q.names, q.lo, q.hi, bins, ranges, pairs)
        self.sample = I.OwnSample(*I.draw_own(*qs.ordered("test", names), None, N23, 5), q.lo, q.hi, None)
        self.lists = I.OwnLists(self.layout, self.sample, chunk)
        if spoil is not None:
            spoil(self.lists)
        self.R = len(qs)
        self.fixed = {k: float(v) for k, v in q.fixed_all.items()}
        self.lib, self.h = I.create_own_handle(fit, rs, {}, self.layout, self.sample, self.lists, self.fixed, which=which)

    def run(self, first, count):
        return self.lib.vk_is_run(self.h, first, count)

    def error(self):
        return (self.lib.vk_is_last_error(self.h) or b"").decode()

    def result(self):
        from victor_amd import importance as I
        return I.read_result(self.lib, self.h, self.layout, self.R, False, own=True)[0]

    def rows(self, first, count):
        out = np.empty((count * self.R, 12))
        rc = self.lib.vk_is_rows(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0, self.error()
        return out

    def close(self):
        self.lib.vk_is_destroy(self.h)


# ------------------------------------------------------------------ device route against the definition route ---------------
@pytest.mark.parametrize("chunk", [7, 23, 64])
def test_sixteen_mocks_four_parameters_with_epsilon(stack, rs, chunk):
    """d = 4 with epsilon sampled; a cut inside the sample (7), one exact chunk (23), a chunk larger than n (64); a pair and, at 6
    bins over 23 points, empty cells; problems at either end of the spread hold points outside the box."""
    qs = proposals(NAMES4, 16)
    kw = dict(bins=6, ranges=RANGES, pairs=[("epsilon", "fsigma8")], chunk=chunk, min_ess=2.0)
    dev, ref, rec = both_routes(rs, PARAMS, qs, f"16 mocks, d = 4, chunk {chunk}", **kw)
    assert dev.names == NAMES4 and dev.n_chunks == -(-N23 // chunk) and dev.n_inside.shape == (16,)
    assert np.any(dev.n_inside < N23) and np.all(dev.n_inside > 0) and same_bytes(dev.n_finite, dev.n_inside)
    smp = dev._sample
    assert np.all(smp.x[~smp.inside] == np.broadcast_to(smp.centre[None], smp.x.shape)[~smp.inside])     # the device saw centres there
    assert np.any(np.diff(dev._lists.offsets[:, :, :8], axis=2) == 0) and len(set(dev.ln_max)) == 16
    assert np.all(np.isfinite(dev.ln_evidence)) and dev.mean.shape == (16, 4) and dev.cov.shape == (16, 4, 4)
    if chunk == 7:
        h = Handle(stack, rs, PARAMS, NAMES4, qs, bins=6, ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=7)
        try:
            batch = {n: np.ascontiguousarray(h.sample.x[:, :, j].ravel()) for j, n in enumerate(NAMES4)}
            want = np.ascontiguousarray(stack._fit_rows(batch, stack._merged({})), dtype=np.float64)       # row g R + r
            got = np.concatenate([h.rows(g0, min(7, N23 - g0)) for g0 in range(0, N23, 7)])
            assert got.shape == want.shape == (N23 * 16, 12)
            assert same_bytes(got, want), np.argwhere(got != want)[:4]                  # epsilon sampled: the host's own pow
            assert len(set(want[:, 3])) > 16 * (N23 - 8)                                # (an apar per point and problem)
        finally:
            h.close()


def independent(ip, r, lnl, bound, what):
    """Problem ``r`` of ``ip`` against lnL of its whole sample from ONE pairs call, reduced in ``np.longdouble`` (module docstring)."""
    ld = np.longdouble
    smp = ip._sample
    B = float(np.max(bound))
    lnpost = (lnl + smp.lno[:, r]).astype(ld)
    top = lnpost.max()
    w = np.exp(lnpost - top)
    total, sq = w.sum(), (w * w).sum()
    ln_z = float(top + np.log(total) - np.log(ld(ip.n_drawn)))
    sb = {name: float(sum_bound(name, ip.n_chunks, N23)) for name in ("total", "sq", "s1")}
    allowed = B + sb["total"] + 64 * tolerances.U * (1.0 + abs(ln_z))
    tolerances._record(f"own importance ln_evidence {what}", abs(ip.ln_evidence[r] - ln_z) / allowed)
    assert abs(ip.ln_evidence[r] - ln_z) <= allowed, (what, ip.ln_evidence[r] - ln_z, allowed)
    ess = float(total * total / sq)
    allowed = (8 * B + 2 * sb["total"] + sb["sq"] + 64 * tolerances.U) * ess
    assert abs(ip.ess[r] - ess) <= allowed, (what, ip.ess[r] - ess, allowed)
    mean = (w[:, None] * smp.y[:, r].astype(ld)).sum(axis=0) / total
    spread = (w[:, None] * np.abs(smp.y[:, r]).astype(ld)).sum(axis=0) / total
    allowed = (4 * B + sb["s1"] + sb["total"] + 64 * tolerances.U) * spread.astype(np.float64) + 4 * tolerances.U * np.abs(smp.centre[r])
    got = ip.mean[r] - smp.centre[r]
    assert np.all(np.abs(got - mean.astype(np.float64)) <= allowed), (what, got - mean, allowed)
    assert ip.arg_max[r] == int(np.argmax(lnpost)) or lnpost[ip.arg_max[r]] >= top - B


def test_against_one_pairs_call_and_a_longdouble_logsumexp(rs):
    """Problems 0, 7 and 15: evidence, ess and mean independent of the chunked definition (the bound needs the realisation's own
    data vector, a fit each)."""
    import victor_amd
    qs = proposals(NAMES2, 16)
    ip = rs.importance_posterior(PARAMS, qs, n=N23, fixed=FIXED2, bins=5, chunk=7)
    smp = ip._sample
    batch = dict(FIXED2, **{n: np.ascontiguousarray(smp.x[:, :, j].ravel()) for j, n in enumerate(ip.names)})
    lnl = rs.log_likelihood_pairs(batch, np.tile(np.arange(16, dtype=np.int32), N23))[0].reshape(N23, 16)
    for r in (0, 7, 15):
        one = victor_amd.CCFFit(*stack_options(simulation_number=r))
        mine = {k: (v if np.ndim(v) == 0 else v.reshape(N23, 16)[:, r].copy()) for k, v in batch.items()}
        independent(ip, r, lnl[:, r], lnl_bound(one, mine, lnl[:, r]), f"mock {r}")


def test_seventy_problems_cross_a_wave(stack):
    """R = 70 from repeated mocks, chunk 5: 350 rows per launch; problems r and r + 16 share their data and differ in their
    proposals, points and lists."""
    rs70 = stack.realisations(np.arange(70) % 16)
    qs = proposals(NAMES2, 70)
    dev, ref, _ = both_routes(rs70, PARAMS, qs, "70 problems, chunk 5", fixed=FIXED2, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")],
                              chunk=5, min_ess=2.0)
    assert dev.n_problems == 70 and dev.n_chunks == 5 and len(set(dev.ln_max)) == 70
    assert not same_bytes(dev._lists.entries[0], dev._lists.entries[16]) and not same_bytes(dev.raw.h1[0], dev.raw.h1[16])
    assert np.all(np.isfinite(dev.ln_evidence)) and np.all(dev.n_finite == dev.n_inside)


def test_gaussian_prior_has_a_prior_problem_per_problem(rs):
    from victor_amd.priors import GaussianPrior
    prior = GaussianPrior(["fsigma8", "beta"], [0.45, 0.4], cov=[[0.05 ** 2, 0.5 * 0.05 * 0.04], [0.5 * 0.05 * 0.04, 0.04 ** 2]])
    qs = proposals(NAMES4, 16)
    kw = dict(bins=4, pairs=[("beta", "sigma_v")], chunk=7, min_ess=2.0)
    dev, ref, _ = both_routes(rs, PARAMS, qs, "16 mocks with a Gaussian prior", prior=prior, **kw)
    plain = rs.importance_posterior(PARAMS, qs, n=N23, **kw)
    assert not same_bytes(dev.ln_max, plain.ln_max)
    assert dev.prior_ln_max.shape == dev.prior_total.shape == dev.prior_error.shape == (16,) and len(set(dev.prior_total)) == 16
    assert same_bytes(dev.prior_ln_max, ref.prior_ln_max)
    assert np.all(np.abs(dev.prior_total - ref.prior_total) <= sum_bound("total", dev.n_chunks, N23) * ref.prior_total)
    want = (dev.ln_max + np.log(dev.raw.total)) - (dev.prior_ln_max + np.log(dev.prior_total))
    assert same_bytes(dev.ln_evidence, want)
    assert np.all(np.abs(dev.ln_evidence - ref.ln_evidence) <= 4 * sum_bound("total", dev.n_chunks, N23))


def test_tail_held_entries_a_short_and_an_empty_problem(rs):
    """``tail={"size": 5}``: the held entries agree as bytes between the routes.  Problem 3's proposal sits in the lowest corner of
    the box and no point of its 23 falls inside: NO_FINITE on both routes, sums of zeros.  Problem 5's sits on three lower faces
    and keeps fewer than 6 points: SHORT."""
    from victor_amd import ProposalSet
    qs = proposals(NAMES4, 16)
    mean = qs.mean.copy()
    mean[3] = mean[5] = [PARAMS[n]["prior"]["min"] for n in NAMES4]
    mean[5, 1] = qs.mean[5, 1]
    qs = ProposalSet(NAMES4, mean, qs.cov)
    for chunk in (7, 64):
        dev, ref, _ = both_routes(rs, PARAMS, qs, f"tail of 5, chunk {chunk}", bins=4, chunk=chunk, min_ess=1.0, tail={"size": 5})
        t = dev.tail
        assert t.size == 5 and t.lnpost.shape == (16, 6) and 0 < dev.n_inside[5] < 6 and t.count[5] == dev.n_finite[5] == dev.n_inside[5]
        assert t.status[5] == t.SHORT and np.all(t.index[5, t.count[5]:] == -1) and np.all(t.lnpost[5, t.count[5]:] == -np.inf)
        assert dev.n_inside[3] == 0 and dev.status[3] == dev.NO_FINITE and t.status[3] == t.NO_FINITE and t.count[3] == 0
        assert dev.ln_evidence[3] == -np.inf and dev.arg_max[3] == -1 and not np.any(dev.raw.h1[3]) and np.all(np.isnan(dev.mean[3]))
        full = np.flatnonzero(dev.n_finite >= 6)
        assert len(full) == 14 and np.all(t.count[full] == 6) and np.all(np.isin(t.status[full], (t.OK, t.HIGH_K)))
        assert np.all(np.diff(t.lnpost[full], axis=1) <= 0) and same_bytes(t.lnpost[:, 0], dev.ln_max) and same_bytes(t.index[:, 0], dev.arg_max)


def test_paired_model_mocks(tmp_path):
    """The route that was refused: every mock with its own real-space CCF, device against the definition over
    log_likelihood_pairs; a GaussianProposal is refused as before."""
    import victor_amd
    from tests.test_paired_realisations import NUMBERS, paired_boss_options, write_boss_model_stack
    from victor_amd.utils import InputError
    fit = victor_amd.CCFFit(*paired_boss_options(tmp_path, number=NUMBERS[0], model_file=write_boss_model_stack(tmp_path)))
    paired, shared = fit.realisations(NUMBERS, paired_model=True), fit.realisations(NUMBERS)
    block = {n: PARAMS[n] for n in ("fsigma8", "sigma_v")}
    fixed = {"beta": 0.37, "epsilon": 1.0}
    qs = proposals(["fsigma8", "sigma_v"], 3)
    kw = dict(fixed=fixed, bins=5, pairs=[("fsigma8", "sigma_v")], chunk=7, min_ess=2.0)
    dev, ref, rec = both_routes(paired, block, qs, "paired-model mocks", **kw)
    assert dev.n_problems == 3 and np.all(dev.n_finite == N23) and np.all(np.isfinite(dev.ln_evidence))
    other = shared.importance_posterior(block, qs, n=N23, **kw)   # the same mocks against the fit's one model: other likelihoods
    assert not same_bytes(other.ln_max, dev.ln_max) and same_bytes(other._sample.x, dev._sample.x)
    with pytest.raises(InputError, match="have no cross mode"):
        paired.importance_posterior(block, victor_amd.GaussianProposal(qs.names, qs.mean[0], qs.cov[0]), n=N23, **kw)
    again = paired.importance_posterior(block, qs, n=N23, **kw)    # (after the shared object used the engine)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(again.raw, name), getattr(dev.raw, name)), name


def test_identical_proposals_equal_the_shared_route(rs):
    """Every problem under one narrow proposal, no point outside: the own route (pairs mode, lists per problem) against the
    shared route (cross mode) given the same proposal and seed - exact fields as bytes, sums at the bound of two runs.

    The bits of a theory vector depend on the rows of the launch that forms it (tests/launch_shapes.py: point-major below
    ``cells_min`` rows, then ranges of ``cpi0`` cells up to ``band1`` rows), so exact fields can agree only where both routes
    launch inside one band: the own route's chunk of 5 points is 80 rows (48 in its last chunk), the shared route's chunk is the
    whole sample, 23 rows - all from ``cells_min`` up and below ``band1``."""
    from tests import launch_shapes as LS
    from tests.test_gpu_importance import definition
    from tests.test_importance import abs_sums
    from victor_amd import GaussianProposal
    t = LS.thresholds()
    assert t["cells_min"] <= 3 * 16 < 5 * 16 < t["band1"] and t["cells_min"] <= N23 < t["band1"]
    qs = proposals(NAMES2, 16, scale=0.2, spread=0.0)              # (narrow: lnpost spans less than 17 over the sample)
    q = GaussianProposal(NAMES2, qs.mean[0], qs.cov[0])
    kw = dict(n=N23, seed=3, fixed=FIXED2, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")], min_ess=2.0, tail={"size": 5})
    own, shared = rs.importance_posterior(PARAMS, qs, chunk=5, **kw), rs.importance_posterior(PARAMS, q, chunk=N23, **kw)
    assert np.all(own.n_inside == N23) and shared.n_inside == N23 and same_bytes(own._sample.x[:, 5], shared._sample.x)
    assert same_bytes(own._sample.lno[:, 9], shared._sample.lno) and own.n_chunks == 5 and shared.n_chunks == 1
    ref, rec = definition(rs, PARAMS, q=q, chunk=N23, **kw)
    lnpost = rec.chunks[0] + ref._sample.lno[:, None]
    assert np.all(lnpost.max(axis=0) - lnpost.min(axis=0) < 17)    # the two-run bound's condition (tests/test_grid.py)
    compare(own, shared, abs_sums(ref, rec.chunks), "own route against the shared route", chunks=[own.n_chunks, shared.n_chunks])
    for name in ("lnpost", "index", "count"):
        assert same_bytes(getattr(own.tail, name), getattr(shared.tail, name)), name


# ------------------------------------------------------------------ cuts, and what the C ABI refuses -----------------------
def test_cuts_and_refusals_of_the_c_abi(stack, rs):
    from victor_amd.utils import InputError
    qs = proposals(NAMES2, 16)
    kw = dict(fixed=FIXED2, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=5)
    h = Handle(stack, rs, PARAMS, NAMES2, qs, **kw)
    try:
        assert h.lib.vk_is_result(h.h, *([None] * 11)) == -1 and "reached 0 of 23" in h.error()
        assert h.run(0, N23) == 0, h.error()
        whole = h.result()
        assert h.run(0, 10) == 0, h.error()
        assert h.lib.vk_is_result(h.h, *([None] * 11)) == -1 and "reached 10 of 23" in h.error()
        assert h.lib.vk_is_set_predictive(h.h, 1) == -1 and "keeps no predictive sums" in h.error()
        assert h.run(5, 5) == -1 and "first must be 0" in h.error()
        assert h.run(10, 13) == 0, h.error()
        cut = h.result()
        for name in EXACT + SUMS:
            assert same_bytes(getattr(whole, name), getattr(cut, name)), ("10 + 13", name)
        assert np.all(whole.n_finite == h.sample.n_inside) and np.all(whole.total > 0)
    finally:
        h.close()

    # an index of which outside the realisations, a list entry outside its chunk, entries out of order, an offset past the chunk:
    # refused at create with text, nothing is launched
    def outside(lists):
        lists.entries[9, 0, 6] = 5                                # chunk 1 holds points 0 .. 4 of its own

    def disorder(lists):
        at = int(np.flatnonzero(np.diff(lists.offsets[0, 9, :8]) >= 2)[0])
        e = lists.offsets[0, 9, at]
        lists.entries[9, 0, [e, e + 1]] = lists.entries[9, 0, [e + 1, e]]

    def overrun(lists):
        lists.offsets[4, 9, 6] = 4                                # the last chunk has three points

    def decrease(lists):
        lists.offsets[1, 2, 3] = lists.offsets[1, 2, 2] - 1

    for spoil, text in ((outside, "outside its chunk"), (disorder, "outside its chunk"), (overrun, "end inside the chunk"),
                        (decrease, "of problem 2 is wrong")):
        with pytest.raises(InputError, match=text):
            Handle(stack, rs, PARAMS, NAMES2, qs, spoil=spoil, **kw)
    for bad in (16, -1):
        which = np.arange(16)
        which[11] = bad
        with pytest.raises(InputError, match=f"realisation index {bad} of problem 11 is outside 0..15"):
            Handle(stack, rs, PARAMS, NAMES2, qs, which=which, **kw)
    h = Handle(stack, rs, PARAMS, NAMES2, qs, **kw)                # the context is as usable as before
    try:
        assert h.run(0, N23) == 0, h.error()
        fresh = h.result()
        for name in EXACT + SUMS:
            assert same_bytes(getattr(whole, name), getattr(fresh, name)), ("after the refusals", name)
    finally:
        h.close()
    # which is honoured: the problems reversed over the realisations give the reversed problems' likelihoods at the same points
    same = proposals(NAMES2, 16, spread=0.0)
    a = Handle(stack, rs, PARAMS, NAMES2, same, **kw)
    try:
        assert a.run(0, N23) == 0, a.error()
        forward = a.result()
    finally:
        a.close()
    b = Handle(stack, rs, PARAMS, NAMES2, same, which=np.arange(16)[::-1], **kw)
    try:
        assert b.run(0, N23) == 0, b.error()
        backward = b.result()
    finally:
        b.close()
    for name in EXACT + SUMS:
        assert same_bytes(getattr(forward, name), getattr(backward, name)[::-1]), ("which reversed", name)
    assert len(set(forward.ln_max)) == 16
