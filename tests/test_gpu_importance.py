"""Importance-sampled posteriors reduced on the GPU (victor_amd/importance.py, vk_is_run) against the NumPy loop that defines them
(device=False: one log_likelihood_batch / Realisations.log_likelihood call per chunk): rows bit for bit with epsilon sampled;
maxima, arg max, counts and statuses as bytes, sums at the derived bounds of tests/test_importance.py; against one independent
evaluation of the whole sample with a plain log-sum-exp; the prior; cuts of vk_is_run; the refusals of the C ABI.  The samples
hold 23 kept points: a reduction goes wrong at chunk cuts, at empty cells and at a problem count that crosses a wave, not at
size."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases, tolerances
from tests.test_chains import same_bytes
from tests.test_importance import EXACT, SUMS, Recorder, abs_sums, assert_exact, assert_sums, sum_bound, terms_of
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
SYNTH = {"fsigma8": {"prior": {"min": 0.3, "max": 0.6}, "ref": {"loc": 0.45, "scale": 0.02}, "proposal": 0.02},
         "sigma_v": {"prior": {"min": 300.0, "max": 420.0}, "ref": {"loc": 360.0, "scale": 10.0}, "proposal": 10.0},
         "epsilon": {"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0, "scale": 0.02}, "proposal": 0.02}}
CENTRE = {"fsigma8": 0.46, "beta": 0.38, "sigma_v": 370.0, "epsilon": 1.0}
WIDTH = {"fsigma8": 0.06, "beta": 0.04, "sigma_v": 35.0, "epsilon": 0.04}
RANGES = {"fsigma8": (0.35, 0.6), "epsilon": (0.95, 1.05)}
G23 = 23


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def synth():
    import victor_amd
    return victor_amd.CCFFit(*cases.synth_options(2))


@pytest.fixture(scope="module")
def boss():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


@pytest.fixture(scope="module")
def stack():
    import victor_amd
    return victor_amd.CCFFit(*stack_options())


@pytest.fixture(scope="module")
def rs(stack):
    return stack.realisations()


def sample_of(block, names, seed=5, kept=G23, draws=None):
    """``dict(sample=, ln_proposal=)`` of a correlated Gaussian proposal over ``names`` (in the block's sampled order), cut behind
    its ``kept``-th point inside the box: G = ``kept`` (23 by default) whatever the generator draws, and some points outside the
    box before it.  ``draws``: the points drawn before the cut, 200 for up to 23 kept points and four per kept point above."""
    from victor_amd import GaussianProposal
    d = len(names)
    cov = np.diag([WIDTH[n] ** 2 for n in names])
    for j in range(1, d):
        cov[0, j] = cov[j, 0] = 0.4 * WIDTH[names[0]] * WIDTH[names[j]]
    q = GaussianProposal(names, [CENTRE[n] for n in names], cov)
    if draws is None:
        draws = 200 if kept <= G23 else 4 * kept
    pts = GaussianProposal.draw(q.mean, q.chol, None, draws, seed)
    lo, hi = (np.array([block[n]["prior"][k] for n in names]) for k in ("min", "max"))
    inside = np.all((pts >= lo) & (pts <= hi), axis=1)
    end = int(np.flatnonzero(np.cumsum(inside) == kept)[0]) + 1
    assert inside[:end].sum() == kept
    pts = pts[:end]
    return dict(sample=pts, ln_proposal=GaussianProposal.ln_density(pts, q.mean, q.chol, None))


def definition(obj, params, **kw):
    """The definition route over the object's own evaluation, its lnL kept chunk by chunk."""
    one = obj.log_likelihood if hasattr(obj, "fit") else obj.log_likelihood_batch
    rec = Recorder(lambda batch: one(batch)[0])
    return obj.importance_posterior(params, device=False, evaluate=rec, **kw), rec


def both_routes(obj, params, what, **kw):
    """The device route and the definition route of one call, compared: exact outputs as bytes, sums at the bound."""
    dev = obj.importance_posterior(params, **kw)
    ref, rec = definition(obj, params, **kw)
    assert dev.n_problems == ref.n_problems and dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks
    assert dev.n_inside == ref.n_inside == G23 and dev.n_drawn == ref.n_drawn >= G23
    assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status), what
    assert_sums(dev.raw, ref.raw, abs_sums(ref, rec.chunks), dev.n_chunks, what, dev._layout, dev._sample.x)
    for name in dev.names:
        assert same_bytes(dev.best[name], ref.best[name])
    return dev, ref


class Handle:
    """A raw vk_is handle of a call's arguments (victor_amd.importance.create_handle), for what the public route does not expose."""

    def __init__(self, fit, params, names, realisations=None, fixed=None, bins=4, ranges=None, pairs=None, chunk=7, prior=None, spoil=None, kept=G23):
        from victor_amd import importance as I
        from victor_amd.fitting import _Sampled
        q = _Sampled("importance_posterior", "sampled", params, fixed)
        assert q.names == names
        self.layout = I.resolve_layout("test", q.names, q.lo, q.hi, bins, ranges, pairs)
        s = sample_of(params, names, kept=kept)
        inside = np.all((s["sample"] >= q.lo) & (s["sample"] <= q.hi), axis=1)
        kept = s["sample"][inside]
        self.sample = I.Sample(kept, kept.mean(axis=0), s["ln_proposal"][inside], len(inside), q.lo, q.hi, q.prior(prior, fit))
        self.lists = I.Lists(self.layout, self.sample.x, chunk)
        if spoil is not None:
            spoil(self.lists)
        self.R = 1 if realisations is None else len(realisations)
        self.fixed = {k: float(v) for k, v in q.fixed_all.items()}
        self.lib, self.h, _ = I.create_handle(q, fit, realisations, {}, q.fit_options(fit, {}), self.layout, self.sample, self.lists, self.fixed)

    def run(self, first, count):
        return self.lib.vk_is_run(self.h, first, count)

    def error(self):
        return (self.lib.vk_is_last_error(self.h) or b"").decode()

    def result(self):
        from victor_amd import importance as I
        return I.read_result(self.lib, self.h, self.layout, self.R, self.sample.lnop is not None)

    def rows(self, first, count):
        out = np.empty((count, 12))
        rc = self.lib.vk_is_rows(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0, self.error()
        return out

    def close(self):
        self.lib.vk_is_destroy(self.h)


def host_rows(fit, handle):
    batch = dict(handle.fixed)
    batch.update({n: np.ascontiguousarray(handle.sample.x[:, j]) for j, n in enumerate(handle.layout.names)})
    return np.ascontiguousarray(fit._fit_rows(batch, fit._merged({})), dtype=np.float64)


# ------------------------------------------------------------------ device route against the definition route ---------------
@pytest.mark.parametrize("chunk", [7, 23, 64])
def test_synthetic_fit_with_epsilon_sampled(synth, chunk):
    """N = 80, d = 3 with epsilon; a cut inside the sample (7), one exact chunk (23), a chunk larger than G (64); a pair and, at
    6 bins over 23 points, empty cells."""
    names = ["fsigma8", "sigma_v", "epsilon"]
    assert len(synth.s) * len(np.atleast_1d(synth.poles_s)) == 80
    kw = dict(bins=6, ranges=RANGES, pairs=[("epsilon", "fsigma8")], chunk=chunk, min_ess=2.0, **sample_of(SYNTH, names))
    dev, ref = both_routes(synth, SYNTH, f"synthetic (fsigma8, sigma_v, epsilon), chunk {chunk}", **kw)
    assert dev.names == names and dev.n_chunks == -(-G23 // chunk) and dev.n_finite[0] == G23 and np.isfinite(dev.ln_evidence[0])
    counts = terms_of(dev._layout, dev._sample.x)
    assert np.any(counts["h1"] == 0) and np.any(counts["h2"] == 0) and counts["h1"].sum() == 3 * G23
    assert np.any(dev.outside_mass > 0)                           # (points below and above the sub-ranges)
    plain = synth.importance_posterior(SYNTH, device=False, **kw)  # the definition over log_likelihood_batch itself
    for name in EXACT + SUMS:
        assert same_bytes(getattr(plain.raw, name), getattr(ref.raw, name)), name
    if chunk == 7:
        h = Handle(synth, SYNTH, names, bins=6, ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=7)
        try:
            want = host_rows(synth, h)
            got = np.concatenate([h.rows(g0, min(7, G23 - g0)) for g0 in range(0, G23, 7)])
            assert same_bytes(got, want), np.argwhere(got != want)[:4]          # epsilon sampled: the host's own pow
            assert len(set(want[:, 3])) == G23                                  # (23 epsilons, 23 apar)
        finally:
            h.close()


def test_boss_fit_four_parameters(boss):
    """beta-dependent data and covariance, all four parameters of the cobaya block."""
    names = ["fsigma8", "beta", "sigma_v", "epsilon"]
    dev, ref = both_routes(boss, PARAMS, "BOSS, four parameters, chunk 7", bins=4, pairs=[("fsigma8", "beta")], chunk=7, min_ess=2.0,
                           **sample_of(PARAMS, names))
    assert dev.status[0] in (dev.OK, dev.LOW_ESS) and dev.n_finite[0] == G23 and dev.cov.shape == (1, 4, 4)


@pytest.mark.parametrize("chunk", [7, 23])
def test_sixteen_realisations(rs, chunk):
    names = ["fsigma8", "epsilon"]
    dev, ref = both_routes(rs, PARAMS, f"16 realisations (fsigma8, epsilon), chunk {chunk}", fixed={"beta": 0.37, "sigma_v": 380.0}, bins=5,
                           ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=chunk, min_ess=2.0, **sample_of(PARAMS, names))
    assert dev.n_problems == 16 and np.all(dev.n_finite == G23) and len(set(dev.ln_max)) == 16 and dev.mean.shape == (16, 2)


@pytest.mark.parametrize("chunk", [7, 23])
def test_seventy_problems_cross_a_wave(stack, chunk):
    """R = 70: problems r and r + 16 are the same realisation and agree byte for byte in every output."""
    rs70 = stack.realisations(np.arange(70) % 16)
    ip = rs70.importance_posterior(PARAMS, fixed={"beta": 0.37, "sigma_v": 380.0}, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")],
                                   chunk=chunk, **sample_of(PARAMS, ["fsigma8", "epsilon"]))
    assert ip.n_problems == 70
    for name in EXACT + SUMS:
        a = getattr(ip.raw, name)
        for r in range(70 - 16):
            assert same_bytes(a[r], a[r + 16]), (name, r)
    assert same_bytes(ip.ln_evidence[:16], ip.ln_evidence[16:32]) and len(set(ip.ln_max[:16])) == 16


def test_gaussian_prior(boss, rs):
    from victor_amd.priors import GaussianPrior
    names = ["fsigma8", "beta", "sigma_v", "epsilon"]
    prior = GaussianPrior(["fsigma8", "beta"], [0.45, 0.4], cov=[[0.05 ** 2, 0.5 * 0.05 * 0.04], [0.5 * 0.05 * 0.04, 0.04 ** 2]])
    kw = dict(bins=4, pairs=[("beta", "sigma_v")], chunk=7, min_ess=2.0, **sample_of(PARAMS, names))
    dev, ref = both_routes(boss, PARAMS, "BOSS with a Gaussian prior", prior=prior, **kw)
    plain = boss.importance_posterior(PARAMS, **kw)
    assert not same_bytes(dev.ln_max, plain.ln_max)
    assert same_bytes(dev.prior_ln_max, ref.prior_ln_max)
    assert abs(dev.prior_total - ref.prior_total) <= sum_bound("total", dev.n_chunks, G23) * ref.prior_total
    want = (dev.ln_max[0] + np.log(dev.raw.total[0])) - (dev.prior_ln_max + np.log(dev.prior_total))
    assert same_bytes(dev.ln_evidence[0], want) and abs(dev.ln_evidence[0] - ref.ln_evidence[0]) <= 4 * sum_bound("total", dev.n_chunks, G23)
    # against every realisation: one prior for all, its own problem once
    both_routes(rs, PARAMS, "16 realisations with a Gaussian prior", prior=GaussianPrior(["fsigma8"], [0.45], sigma=[0.05]),
                fixed={"beta": 0.37, "sigma_v": 380.0}, bins=5, chunk=7, min_ess=2.0, **sample_of(PARAMS, ["fsigma8", "epsilon"]))


# ------------------------------------------------------------------ against an independent evaluation ----------------------
def lnl_bound(fit, batch, lnl):
    """The per-point bound of tests/tolerances.py on lnL of two evaluation orders (64 ulps), as assert_same_lnl forms it."""
    return 0.51 * tolerances.chi2_bound(fit, batch, ulps=64) + 16 * tolerances.U * (np.abs(lnl) + 1000.0)


def independent(ip, m, lnl, bound, what):
    """Problem ``m`` of ``ip`` against lnL of the whole sample from ONE call, reduced by a plain NumPy log-sum-exp."""
    B = float(np.max(bound))
    lnpost = lnl + ip._sample.lno
    top = lnpost.max()
    ln_z = top + np.log(np.exp(lnpost - top).sum()) - np.log(ip.n_drawn)
    allowed = B + sum_bound("total", ip.n_chunks, ip.n_inside) + 64 * tolerances.U * (1.0 + abs(ln_z))
    tolerances._record(f"importance ln_evidence {what}", abs(ip.ln_evidence[m] - ln_z) / allowed)
    assert abs(ip.ln_evidence[m] - ln_z) <= allowed, (what, ip.ln_evidence[m] - ln_z, allowed)
    assert ip.arg_max[m] == int(np.argmax(lnpost)) or lnpost[ip.arg_max[m]] >= top - B


def test_data_vector_against_one_batch_call_and_logsumexp(boss):
    names = ["fsigma8", "beta", "sigma_v", "epsilon"]
    ip = boss.importance_posterior(PARAMS, bins=4, chunk=7, **sample_of(PARAMS, names))
    batch = {n: np.ascontiguousarray(ip._sample.x[:, j]) for j, n in enumerate(names)}
    lnl = boss.log_likelihood_batch(batch)[0]
    independent(ip, 0, lnl, lnl_bound(boss, batch, lnl), "BOSS data vector")


def test_realisations_against_one_call_and_logsumexp(rs):
    """Problems 0, 7 and 15: the bound needs the realisation's own data vector, a fit each."""
    import victor_amd
    fixed = {"beta": 0.37, "sigma_v": 380.0}
    ip = rs.importance_posterior(PARAMS, fixed=fixed, bins=5, chunk=7, **sample_of(PARAMS, ["fsigma8", "epsilon"]))
    batch = dict(fixed, **{n: np.ascontiguousarray(ip._sample.x[:, j]) for j, n in enumerate(ip.names)})
    lnl = rs.log_likelihood(batch)[0]
    assert lnl.shape == (G23, 16)
    for m in (0, 7, 15):
        one = victor_amd.CCFFit(*stack_options(simulation_number=m))
        independent(ip, m, lnl[:, m], lnl_bound(one, batch, lnl[:, m]), f"realisation {m}")


# ------------------------------------------------------------------ cuts, and what the C ABI refuses -----------------------
def test_cuts_and_refusals_of_the_c_abi(rs, stack):
    from victor_amd.utils import InputError
    names = ["fsigma8", "epsilon"]
    kw = dict(realisations=rs, fixed={"beta": 0.37, "sigma_v": 380.0}, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=7)
    h = Handle(stack, PARAMS, names, **kw)
    try:
        assert h.lib.vk_is_result(h.h, *([None] * 11)) == -1 and "reached 0 of 23" in h.error()
        assert h.run(0, G23) == 0, h.error()
        whole, _ = h.result()
        assert h.run(0, 1 << 40) == 0, h.error()                                # the same call twice (count past the end: to G)
        again, _ = h.result()
        assert h.run(0, 14) == 0, h.error()
        assert h.lib.vk_is_result(h.h, *([None] * 11)) == -1 and "reached 14 of 23" in h.error()     # a result before the end
        assert h.run(7, 7) == -1 and "first must be 0" in h.error()             # not where the run stands
        assert h.run(15, 5) == -1 and "multiple of the chunk" in h.error()
        assert h.run(14, 3) == -1 and "whole chunks" in h.error()
        assert h.run(23, 7) == -1 and h.run(-7, 7) == -1 and h.run(14, 0) == -1
        fewer, more = stack.realisations(np.arange(8)), stack.realisations(np.arange(24) % 16)
        fewer._plan({})                                                         # another realisation count on the context
        assert h.run(14, 9) == -1 and "holds 8 realisations" in h.error()
        more._plan({})
        assert h.run(14, 9) == -1 and "holds 24 realisations, the sample was made for 16" in h.error()
        out = np.empty((7, 12))
        assert h.lib.vk_is_rows(h.h, 0, 7, out.ctypes.data_as(C.POINTER(C.c_double))) == -1 and "holds 24" in h.error()
        rs._plan({})
        assert h.lib.vk_is_rows(h.h, 20, 7, out.ctypes.data_as(C.POINTER(C.c_double))) == -1 and "count <= chunk" in h.error()
        assert h.run(14, 9) == 0, h.error()                                     # every refusal left the handle where it stood
        cut, _ = h.result()
        for name in EXACT + SUMS:
            assert same_bytes(getattr(whole, name), getattr(again, name)), ("twice", name)
            assert same_bytes(getattr(whole, name), getattr(cut, name)), ("14 + 9", name)
        assert np.all(whole.n_finite == G23)
    finally:
        h.close()

    # a list entry outside its chunk, an entry out of order, an offset past the chunk: refused at create, nothing is launched
    def outside(lists):
        lists.entries[0, 8] = 7                                   # chunk 1 holds points 0 .. 6 of its own

    def disorder(lists):
        at = int(np.flatnonzero(np.diff(lists.offsets[0, :7]) >= 2)[0])
        e = lists.offsets[0, at]
        lists.entries[0, [e, e + 1]] = lists.entries[0, [e + 1, e]]

    def overrun(lists):
        lists.offsets[3, 6] = 3                                   # the last chunk has two points

    for spoil, text in ((outside, "outside its chunk"), (disorder, "outside its chunk"), (overrun, "end inside the chunk")):
        with pytest.raises(InputError, match=text):
            Handle(stack, PARAMS, names, spoil=spoil, **kw)
    h = Handle(stack, PARAMS, names, **kw)                         # the context is as usable as before
    try:
        assert h.run(0, G23) == 0, h.error()
        fresh, _ = h.result()
        for name in EXACT + SUMS:
            assert same_bytes(getattr(whole, name), getattr(fresh, name)), ("after the refusals", name)
    finally:
        h.close()


def test_refusals_with_a_context(rs, tmp_path):
    import victor_amd
    from tests.test_paired_realisations import NUMBERS, paired_boss_options, write_boss_model_stack
    from victor_amd.utils import InputError
    s = sample_of(PARAMS, ["fsigma8", "beta", "sigma_v", "epsilon"])
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        rs.importance_posterior(PARAMS, beta_interpolation="likelihood", **s)
    paired = victor_amd.CCFFit(*paired_boss_options(tmp_path, number=NUMBERS[0], model_file=write_boss_model_stack(tmp_path)))
    with pytest.raises(InputError, match="paired_model"):
        paired.realisations(NUMBERS, paired_model=True).importance_posterior(PARAMS, **s)
