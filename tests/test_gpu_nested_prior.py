"""Nested sampling under a Gaussian prior, stepped on the GPU (``prior=``; vk_nprior_set, the NestedPriorArgs instantiations of
vk_kernel_nested.h) against the NumPy loop that defines it (``device=False``).  With epsilon fixed both
routes launch the same rows and take the same decisions on lnL + ln prior, so the dead record (lnL, chi2, ln prior, x), the final
live points, the counters and the evidence are compared byte for byte.  The shapes are the smallest that reach what each case is
there for:

  P1  the BOSS data vector, a correlated prior; L = 258, K = 129: the second trip of the select kernel's strided loops with two
      lanes, the third workgroup of the per-walker kernels with one lane; the prior changes which points die
  P2  three mocks, a ``sigma=`` prior; 9 iterations = 7 + extend(2): across a block of 8; problems end inside a workgroup;
      ``prior_norm`` "exact" and "nested"
  P3  the same with every mock's own model (``paired_model=True``: the realisation index of a row travels)
  P4  block-diagonal joint mocks with a dispersion per block, a correlated prior over a shared and a per-block name, d = 7
  P5  a fit that blends in beta, the prior on beta: ln prior at the point's own beta under the doubled launch
  P6  the raw handle: set, run, clear, run; the refusals of the two entry points
  P7  P2 with epsilon sampled (d = 4), held to rounding by the rule of tests/test_gpu_nested.py (its
      ``test_device_route_with_epsilon_sampled``: a seed whose smallest margin on the definition route exceeds MARGIN of
      tests/test_gpu_chains.py, then identical decisions and lnL / chi2 within ``chi2_bound``)

No assertion is on elapsed time."""

import faulthandler

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_chains import MARGIN
from tests.test_gpu_nested import BYTES, EPS1, PARAMS, exercised
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PRIOR_BYTES = BYTES + ("dead_lnprior", "lnprior", "ln_evidence_unnormalised", "ln_prior_norm", "ln_prior_norm_error")


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
def rs3(stack):
    return stack.realisations([0, 1, 2])


@pytest.fixture(scope="module")
def boss():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


def sigma_v_prior():
    from victor_amd.priors import GaussianPrior
    return GaussianPrior("sigma_v", 300.0, sigma=40.0)


def correlated_prior(names=("fsigma8", "sigma_v")):
    from victor_amd.priors import GaussianPrior
    return GaussianPrior(list(names), [0.7, 300.0], cov=[[0.04, 1.6], [1.6, 1600.0]])


def same_run(dev, ref, what):
    assert dev.n_iter == ref.n_iter and dev.names == ref.names and dev.prior_norm == ref.prior_norm, what
    for a in PRIOR_BYTES:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)


def both(obj, params, what, **kw):
    ref = obj.nested_sampling(params, device=False, **kw)
    dev = obj.nested_sampling(params, **kw)
    same_run(dev, ref, what)
    assert dev.decision_margin is None and ref.decision_margin is not None
    assert same_bytes(ref.dead_lnprior, ref.prior.lnprior(ref.dead_x)) and same_bytes(ref.lnprior, ref.prior.lnprior(ref.x)), what
    return dev, ref


def under_the_prior(ref, what):
    """The definition route's run is one the prior matters to (conditions on the inputs, not on the code under test): both
    outcomes of a step in every problem, the dead record increasing in lnpost."""
    print(what, "acceptance", ref.acceptance, "stuck", ref.n_stuck, "margin", ref.decision_margin, "ln Z", ref.ln_evidence,
          "ln norm", ref.ln_prior_norm, ref.prior_norm)
    assert np.all((0 < ref.n_accept) & (ref.n_accept < ref.n_steps)), what
    post = (ref.dead_lnl + ref.dead_lnprior).transpose(1, 0, 2).reshape(ref.R, -1)
    assert np.all(np.isfinite(post)) and np.all(np.diff(post, axis=1) >= 0), what


def orders_differ(ns):
    """Iterations in which the K points lowest in lnpost were not the K lowest in lnL, read off the record: a point died while
    one of smaller lnL lived on - to die later or to be among the final live points."""
    n = 0
    for r in range(ns.R):
        later = ns.lnl[r].min()
        for t in range(ns.n_iter - 1, -1, -1):
            n += bool(ns.dead_lnl[t, r].max() > later)
            later = min(later, ns.dead_lnl[t, r].min())
    return n


# ------------------------------------------------------------------ P1 .. P5: the device route is the definition route ----------
def test_p1_data_vector_correlated_prior_past_one_trip(boss):
    kw = dict(fixed=EPS1, n_live=258, batch=129, steps=2, n_iter=3, seed=2, prior=correlated_prior())
    dev, ref = both(boss, PARAMS, "P1", **kw)
    assert dev.R == 1 and dev.dead_lnprior.shape == (3, 1, 129) and dev.lnprior.shape == (1, 258) and dev.prior_norm == "nested"
    under_the_prior(ref, "P1")
    assert orders_differ(ref) > 0                            # otherwise the run could not tell lnpost from lnL
    plain = boss.nested_sampling(PARAMS, **dict(kw, prior=None))
    assert plain.dead_lnprior is None and not same_bytes(plain.dead_lnl, dev.dead_lnl) and same_bytes(plain.start_points(), dev.start_points())


def test_p2_mocks_sigma_prior_across_a_block_and_both_normalisations(rs3):
    kw = dict(fixed=EPS1, n_live=48, batch=24, steps=2, seed=1, prior=sigma_v_prior())
    ref = rs3.nested_sampling(PARAMS, device=False, n_iter=9, **kw)
    dev = rs3.nested_sampling(PARAMS, n_iter=7, **kw).extend(2)
    same_run(dev, ref, "P2: 7 + 2")
    assert dev.prior_norm == "exact" and dev.ln_prior_norm_error == 0.0 and dev.dead_lnprior.shape == (9, 3, 24)
    under_the_prior(ref, "P2")
    assert not same_bytes(dev.dead_lnl[:, 0], dev.dead_lnl[:, 1])
    own = rs3.nested_sampling(PARAMS, n_iter=9, prior_norm="nested", **kw)
    assert own.prior_norm == "nested" and own.ln_prior_norm_error > 0.0
    for a in ("ln_evidence_unnormalised", "dead_lnl", "dead_lnprior", "dead_x", "x", "weights"):
        assert same_bytes(getattr(own, a), getattr(dev, a)), a
    assert same_bytes(own.ln_evidence, own.ln_evidence_unnormalised - own.ln_prior_norm)
    assert abs(own.ln_prior_norm - dev.ln_prior_norm) <= 4.0 * own.ln_prior_norm_error


def test_p3_paired_models(tmp_path):
    import victor_amd
    from tests.test_paired_realisations import NUMBERS, paired_boss_options
    paired = victor_amd.CCFFit(*paired_boss_options(tmp_path, number=NUMBERS[0])).realisations(NUMBERS, paired_model=True)
    assert len(NUMBERS) == 3
    dev, ref = both(paired, PARAMS, "P3", fixed=EPS1, n_live=48, batch=24, steps=2, n_iter=2, seed=1, prior=sigma_v_prior())
    under_the_prior(ref, "P3")


def test_p4_joint_mocks_with_a_per_block_name_in_the_prior(tmp_path):
    import victor_amd
    from tests.test_joint_realisations import dsplit_stacks
    from victor_amd.joint import JointFit, per_block
    jr = JointFit([victor_amd.CCFFit(*o) for o in dsplit_stacks(tmp_path, 5)]).realisations()
    prior = correlated_prior(("fsigma8", "sigma_v@2"))
    dev, ref = both(jr, per_block(PARAMS, ["sigma_v"], 5), "P4", fixed=EPS1, n_live=16, batch=8, steps=2, n_iter=2, seed=1, prior=prior)
    assert dev.R == 5 and dev.names == ["fsigma8", "beta"] + [f"sigma_v@{q}" for q in range(5)] and dev.prior_norm == "nested"
    assert np.all(dev.prior.precision[[1, 2, 3, 5, 6]] == 0.0) and dev.prior.precision[0, 4] != 0.0
    under_the_prior(ref, "P4")


def test_p5_prior_on_beta_in_a_fit_that_blends_in_beta():
    import victor_amd
    from victor_amd.priors import GaussianPrior
    model, data = cases.boss_options("config")
    fit = victor_amd.CCFFit(model, dict(data, beta_interpolation="likelihood"))
    assert fit.fit_options["beta_interpolation"] == "likelihood" and not fit.fixed_data
    dev, ref = both(fit, PARAMS, "P5", fixed=EPS1, n_live=16, batch=8, steps=2, n_iter=3, seed=1, prior=GaussianPrior("beta", 0.33, sigma=0.04))
    under_the_prior(ref, "P5")
    # ln prior is that of the point's own beta: the sampled values are not nodes of the data vector's beta grid
    j = dev.names.index("beta")
    assert not np.isin(dev.dead_x[..., j], fit.beta_ccf).any()
    assert same_bytes(dev.dead_lnprior, -0.5 * ((1.0 / (0.04 * 0.04)) * (dev.dead_x[..., j] - 0.33) * (dev.dead_x[..., j] - 0.33)))


# ------------------------------------------------------------------ P6: the raw handle ------------------------------------------
class Raw:
    """A raw vk_nested handle against the BOSS data vector: R = 1, L = 16, K = 8, S = 1."""
    L, K, S, scale = 16, 8, 1, 0.3

    def __init__(self, fit):
        from victor_amd import _native as N
        from victor_amd.fitting import _Sampled
        self.N = N
        self.q = q = _Sampled("nested_sampling", "sampled", PARAMS, EPS1)
        self.d = len(q.names)
        mid = 0.5 * (q.lo + q.hi)
        batch = dict({k: float(v) for k, v in q.fixed_all.items()}, **{n: np.full(self.K, mid[j]) for j, n in enumerate(q.names)})
        self.h = None
        self.lib, self.h, _ = q.create("vk_nested_create", fit, None, {}, q.fit_options(fit, {}), batch, np.zeros(self.K, dtype=np.int32),
                                       shape=(self.L, self.K, self.S, self.scale))
        rng = np.random.default_rng(7)
        self.x0 = np.ascontiguousarray(q.lo + rng.random((1, self.L, self.d)) * (q.hi - q.lo))
        self.pick, self.dz = rng.random((1, 1, self.K)), rng.standard_normal((1, self.S, 1, self.K, self.d))

    def error(self):
        return (self.lib.vk_nested_last_error(self.h) or b"").decode()

    def start(self):
        return self.lib.vk_nested_start(self.h, self.N.as_dp(self.x0))

    def begin(self, first=0):
        return self.lib.vk_nested_begin(self.h, 1, self.N.as_dp(self.pick), self.N.as_dp(self.dz), first, 1)

    def finish(self):
        out = [np.empty((1, 1, self.K)), np.empty((1, 1, self.K)), np.empty((1, 1, self.K, self.d)), np.empty((1, self.L))]
        assert self.lib.vk_nested_finish(self.h, *[self.N.as_dp(a) for a in out]) == 0, self.error()
        return out

    def record(self, n=1, give=(True, True)):
        dead, live = np.empty((1, 1, self.K)), np.empty((1, self.L))
        rc = self.lib.vk_nprior_record(self.h, n, self.N.as_dp(dead) if give[0] else None, self.N.as_dp(live) if give[1] else None)
        return rc, dead, live

    def state(self):
        x = np.empty((1, self.L, self.d))
        assert self.lib.vk_nested_state(self.h, self.N.as_dp(x), None, None, None, None, None) == 0, self.error()
        return x

    def close(self):
        if self.h:
            self.lib.vk_nested_destroy(self.h)
            self.h = None


def test_p6_raw_handle_set_clear_and_refusals(boss):
    a, b = Raw(boss), Raw(boss)
    try:
        dp = a.N.as_dp
        prior = a.q.prior(correlated_prior(), boss)
        # the refusals that need no run: one pointer NULL; a record without a prior, and without a start
        assert a.lib.vk_nprior_set(a.h, dp(prior.mu), None) == -1 and "both given or both NULL" in a.error()
        assert a.lib.vk_nprior_set(a.h, None, dp(prior.pp)) == -1 and "both given or both NULL" in a.error()
        bad = prior.mu.copy()
        bad[0] = np.nan
        assert a.lib.vk_nprior_set(a.h, dp(bad), dp(prior.pp)) == -1 and "not finite" in a.error()
        assert a.record()[0] == -1 and "has no prior" in a.error()
        # set, then a run
        assert a.lib.vk_nprior_set(a.h, dp(prior.mu), dp(prior.pp)) == 0, a.error()
        assert a.record()[0] == -1 and "have no start" in a.error()
        assert a.begin() == -1 and "have no start" in a.error()
        assert a.start() == 0, a.error()
        rc, _, live0 = a.record(0, give=(False, True))
        assert rc == 0 and same_bytes(live0, prior.lnprior(a.x0)), a.error()
        assert a.begin() == 0, a.error()
        assert a.lib.vk_nprior_set(a.h, None, None) == -1 and "awaiting vk_nested_finish" in a.error()      # a block in flight
        assert a.record()[0] == -1 and "awaiting vk_nested_finish" in a.error()
        dl, dc, dx, live = a.finish()                                             # ... and the handle is usable: the block ends
        assert a.record(2)[0] == -1 and "had 1 iterations" in a.error()
        rc, dead_lp, live_lp = a.record()
        assert rc == 0, a.error()
        assert same_bytes(dead_lp, prior.lnprior(dx)) and same_bytes(live_lp, prior.lnprior(a.state()))
        post = dl[0, 0] + dead_lp[0, 0]
        assert np.all(np.diff(post) >= 0) and np.all((live + live_lp).min() >= post[-1])
        # a change of prior ends the start; cleared, the handle is one that never had a prior
        assert a.lib.vk_nprior_set(a.h, None, None) == 0, a.error()
        assert a.begin(1) == -1 and "have no start" in a.error()
        assert a.record()[0] == -1 and "has no prior" in a.error()
        assert a.start() == 0 and a.begin() == 0, a.error()
        assert b.start() == 0 and b.begin() == 0, b.error()
        cleared, never = a.finish() + [a.state()], b.finish() + [b.state()]
        for got, want in zip(cleared, never):
            assert same_bytes(got, want)
        assert not same_bytes(never[2], dx)                  # (the run under the prior killed other points)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ P7: epsilon sampled -----------------------------------------
def test_p7_epsilon_sampled(rs3):
    """The rule of tests/test_gpu_nested.py::test_device_route_with_epsilon_sampled: the seed is the first whose smallest margin
    on the definition route (here of lnL + ln prior) exceeds MARGIN, chosen before the device route runs."""
    import victor_amd
    ref = None
    for seed in range(8):
        kw = dict(n_live=48, batch=24, steps=2, n_iter=2, seed=seed, prior=sigma_v_prior())
        ref = rs3.nested_sampling(PARAMS, device=False, **kw)
        print("seed", seed, "smallest margin (definition route):", ref.decision_margin)
        if ref.decision_margin > MARGIN:
            break
    assert ref.decision_margin > MARGIN, ref.decision_margin     # a condition on the inputs, not on the code under test
    dev = rs3.nested_sampling(PARAMS, **kw)
    assert dev.names == ["fsigma8", "beta", "sigma_v", "epsilon"]
    for a in ("dead_x", "x", "n_accept", "n_steps", "n_stuck", "samples", "dead_lnprior", "lnprior", "ln_prior_norm"):
        assert same_bytes(getattr(dev, a), getattr(ref, a)), a                       # identical decisions and order
    for m in range(3):
        fit = victor_amd.CCFFit(*stack_options(simulation_number=m))
        x = np.concatenate([ref.dead_x[:, m].reshape(-1, 4), ref.x[m]])
        bound = chi2_bound(fit, {n: x[:, j] for j, n in enumerate(ref.names)})
        assert_same_chi2(np.concatenate([dev.dead_chi2[:, m].ravel(), dev.chi2[m]]), np.concatenate([ref.dead_chi2[:, m].ravel(), ref.chi2[m]]),
                         bound, what="nested sampling under a prior, epsilon sampled: device vs definition route")
        assert_same_lnl(np.concatenate([dev.dead_lnl[:, m].ravel(), dev.lnl[m]]), np.concatenate([ref.dead_lnl[:, m].ravel(), ref.lnl[m]]),
                        bound, what="nested sampling under a prior, epsilon sampled: device vs definition route")
