"""Best fits and Metropolis chains of joint fits on the GPU: ``JointFit`` / ``JointRealisations`` ``.best_fit`` and
``.sample_chains`` (``vk_fit_create_joint`` / ``vk_chain_create_joint``; DESIGN.md sections 7a and 7b), block-diagonal and under
one joint covariance (fixed, or gridded in beta), against the joint data vector and against every joint realisation.

The cases are the smallest that reach every route: three density-split blocks (``cases.dsplit_options(q)``, q = 0, 1, 2) with
stacks of 5 realisations - their data do not depend on beta, which is therefore fixed (a parameter the likelihood ignores is a
flat direction): d = 3 with epsilon sampled (S = 4 rows per problem) and d = 2 without - and the BOSS pair under a covariance
gridded on 31 beta slices with stacks of 4 realisations (the slice sort and the log-det factor; d = 4, S = 5).
"""
import ctypes as C
import faulthandler
import gc
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_chains import assert_pooled, assert_sums, same_bytes
from tests.test_gpu_joint_cov import joint_bound, oracle_joint
from tests.test_joint_cov import boss_joint_cov_file, correlated
from tests.test_joint_realisations import boss_stacks, dsplit_stacks, with_number
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
BETA = 0.4                # the density-split blocks ignore beta: fixed at the cobaya block's reference value
MARGIN = 1e-6             # as tests/test_gpu_chains.py: the decision margin the epsilon-sampled comparisons need
# Seeds of the epsilon-sampled comparisons: the first of 0, 1, 2, ... whose smallest decision margin on the definition route
# exceeds MARGIN, picked with the definition route alone (70 steps, W = 2), before the device route was looked at.
# Observed smallest margins: dsplit_cov 5.3e-3 (seeds 1 .. 3: 6.5e-3, 2.2e-2, 1.3e-2), boss_grid 5.8e-3 (2.5e-1, 1.0e-2, 7.6e-3),
# dsplit_diag 1.4e-2 (1.3e-2, 4.9e-3, 1.1e-3).
SEEDS = {"dsplit_cov": 0, "boss_grid": 0, "dsplit_diag": 0}
# Best fits against scipy: positions are asserted (1e-3 of the prior widths, as tests/test_gpu_best_fit.py) where scipy's
# Nelder-Mead through log_likelihood_pairs agrees with itself that well from the two start simplices x0 + step and x0 - step.
# Density-split cases: the two runs end within 1e-7 of each width of each other (lnL equal to 1e-12).  BOSS pair under the
# gridded covariance: they end 0.07 / 0.08 / 0.21 / 0.01 of the widths apart (mock 0: lnL 541.508 and 559.954; mock 3: 549.023
# and 540.581) - the kinked ridge in beta of DESIGN.md section 7a - so there the requirement is on lnL alone.
SCIPY_POSITIONS = {"dsplit_cov": True, "boss_grid": False, "dsplit_diag": True}
GAUSS = {"form": "gaussian"}
HISTORY = ("pivot", "chain", "x", "n_accept", "acceptance", "lnl_chain", "chi2_chain")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle as vo
    return vo


def fits_of(opts):
    import victor_amd
    return [victor_amd.CCFFit(*o) for o in opts]


class Case:
    """A joint fit of stacked blocks with its realisations, and what its checks need: per-realisation joint fits (for the
    bounds, which read the realisation's own data vector) and the oracle's restatement."""

    def __init__(self, name, tmp):
        from victor_amd.joint import JointFit
        self.name = name
        self.likelihood = None
        if name.startswith("dsplit"):
            self.opts = dsplit_stacks(tmp, 5)[:3]
            self.fits = fits_of(self.opts)
            self.names = ["fsigma8", "sigma_v", "epsilon"]
            self.fixed = {"beta": BETA}
            self.covariance = correlated([f.covmat for f in self.fits]) if name == "dsplit_cov" else None
            self.cov_array, self.beta_grid = self.covariance, None
        else:
            self.opts = boss_stacks(tmp, 4)
            self.fits = fits_of(self.opts)
            self.names = ["fsigma8", "beta", "sigma_v", "epsilon"]
            self.fixed = {}
            self.covariance = boss_joint_cov_file(os.path.join(str(tmp), "joint_cov.npy"))
            self.likelihood = GAUSS                      # (the BOSS options' own form is sellentin: the oracle restates this one)
            src = np.load(os.path.join(self.covariance["dir"], self.covariance["data_file"]), allow_pickle=True).item()
            self.cov_array, self.beta_grid = src["covmat"], src["beta"]
            assert len(self.beta_grid) == 31
        self.joint = JointFit(self.fits, covariance=self.covariance, likelihood=self.likelihood)
        self.jr = self.joint.realisations()
        self.lo = np.array([PARAMS[n]["prior"]["min"] for n in self.names], dtype=float)
        self.hi = np.array([PARAMS[n]["prior"]["max"] for n in self.names], dtype=float)
        self.width = self.hi - self.lo
        self._single = {}

    def without(self, *fixed):
        return [n for n in self.names if n not in fixed]

    def of(self, m):
        """The joint fit of realisation m's own data vectors (fresh fits)."""
        from victor_amd.joint import JointFit
        if m not in self._single:
            self._single[m] = JointFit(fits_of(with_number(self.opts, m)), covariance=self.covariance, likelihood=self.likelihood)
        return self._single[m]

    def bound_of(self, joint, pts):
        """The rounding bound of chi2 at ``pts``: joint_bound under a covariance, block-diagonal the sum of the blocks' own."""
        if self.covariance is not None:
            return joint_bound(joint, pts)
        return sum(chi2_bound(f, pts) for f in joint.fits)

    def bound(self, m, pts):
        return self.bound_of(self.of(m), pts)

    def points(self, x, names=None, **more):
        pts = {n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(names or self.names)}
        pts.update({k: np.full(len(x), float(v)) for k, v in dict(self.fixed, **more).items() if k not in pts})
        return pts

    def oracle_at(self, oracle, m, point):
        """(lnL, chi2) of realisation m at ``point`` (name -> float) from the oracle's blocks."""
        ofits = [oracle.OracleFit(*o) for o in with_number(self.opts, m)]
        if self.covariance is None:
            each = [of.log_likelihood(dict(point)) for of in ofits]
            return sum(e[0] for e in each), sum(e[1] for e in each)
        theory = [[of.theory_multipole_vector(of.s, dict(point), of.poles_s)] for of in ofits]
        ol, oc = oracle_joint(ofits, theory, [point], self.cov_array, self.beta_grid, self.likelihood or GAUSS)
        return ol[0], oc[0]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory.mktemp(name))
        return made[name]
    return get


def history_bounds(c, ch, data=False, **fixed):
    """The chi2 bound of every kept sample: (n_kept, R, W)."""
    n, R, W, d = ch.chain.shape
    out = np.empty((n, R, W))
    for m in range(R):
        pts = c.points(ch.chain[:, m].reshape(n * W, d), ch.names, **fixed)
        out[:, m] = (c.bound_of(c.joint, pts) if data else c.bound(m, pts)).reshape(n, W)
    return out


def same_walk(dev, ref, what):
    """Positions, decisions and accept counts of two routes, bit for bit."""
    assert dev.chain.shape == ref.chain.shape, what
    for a in ("pivot", "chain", "x", "n_accept", "acceptance"):
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)
    assert dev.n_steps == ref.n_steps and dev.n_kept == ref.n_kept


# ------------------------------------------------------------------ 1. chains, epsilon fixed: the bytes of the definition route
@pytest.mark.parametrize("name,data", [("dsplit_cov", False), ("boss_grid", False), ("dsplit_diag", False), ("dsplit_cov", True)])
def test_device_route_is_the_definition_route_bit_for_bit_with_epsilon_fixed(case, name, data):
    """Both routes make the same launches on the same rows: the same bytes, not a tolerance.  70 steps
    cross the block of 64."""
    c = case(name)
    target = c.joint if data else c.jr
    kw = dict(walkers=8 if data else 2, seed=2, fixed=dict(c.fixed, epsilon=1.0))
    ref = target.sample_chains(PARAMS, 70, device=False, **kw)
    dev = target.sample_chains(PARAMS, 70, **kw)
    R = 1 if data else len(c.jr)
    assert dev.names == c.without("epsilon") and dev.chain.shape == (70, R, kw["walkers"], len(c.names) - 1)
    print(name, "data" if data else "mocks", "acceptance of the definition route:", ref.acceptance)
    assert 0.02 < ref.acceptance.mean() < 0.98
    for a in HISTORY:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (name, a)
    assert same_bytes(dev.lnl, ref.lnl) and same_bytes(dev.chi2, ref.chi2)
    assert dev.decision_margin is None and ref.decision_margin is not None


# ------------------------------------------------------------------ 2. chains, epsilon sampled
@pytest.mark.parametrize("name", ["dsplit_cov", "boss_grid", "dsplit_diag"])
def test_device_route_with_epsilon_sampled(case, name):
    c = case(name)
    kw = dict(walkers=2, seed=SEEDS[name], fixed=c.fixed)
    ref = c.jr.sample_chains(PARAMS, 70, device=False, **kw)
    print(name, "smallest decision margin (definition route):", ref.decision_margin)
    assert ref.decision_margin > MARGIN, ref.decision_margin            # a condition on the inputs, not on the code under test
    dev = c.jr.sample_chains(PARAMS, 70, **kw)
    assert dev.names == c.names
    same_walk(dev, ref, name)
    bound = history_bounds(c, ref)
    assert_same_chi2(dev.chi2_chain, ref.chi2_chain, bound, what=f"{name} chains: device vs definition route")
    assert_same_lnl(dev.lnl_chain, ref.lnl_chain, bound, what=f"{name} chains: device vs definition route")


# ------------------------------------------------------------------ 3. every kept sample is what the likelihood says
@pytest.mark.parametrize("name", ["dsplit_cov", "boss_grid", "dsplit_diag"])
def test_every_kept_sample_is_what_the_likelihood_says(case, oracle, name):
    c = case(name)
    ch = c.jr.sample_chains(PARAMS, 40, walkers=2, seed=5, burn=10, thin=3, fixed=c.fixed)
    n, R, W, d = ch.chain.shape
    assert n == 10 and ch.n_kept == 10
    t, m, w = (a.ravel() for a in np.indices((n, R, W)))
    pts = c.points(ch.chain[t, m, w])
    lnl, chi2 = c.jr.log_likelihood_pairs(pts, m.astype(np.int32))
    bound = np.empty(len(t))
    for k in range(R):
        bound[m == k] = c.bound(k, {key: v[m == k] for key, v in pts.items()})
    assert_same_chi2(ch.chi2_chain[t, m, w], chi2, bound, what=f"{name}: kept samples vs log_likelihood_pairs")
    assert_same_lnl(ch.lnl_chain[t, m, w], lnl, bound, what=f"{name}: kept samples vs log_likelihood_pairs")
    i = len(t) // 2 + 3                      # the oracle: a wrongly formed row (AP factors, beta, a fixed parameter) would show here
    ol, oc = c.oracle_at(oracle, int(m[i]), {key: float(v[i]) for key, v in pts.items()})
    got_l, got_c = ch.lnl_chain[t[i], m[i], w[i]], ch.chi2_chain[t[i], m[i], w[i]]
    assert abs(ol - got_l) <= 1e-9 * abs(ol) and abs(oc - got_c) <= 1e-9 * abs(oc), (name, ol, got_l, oc, got_c)


# ------------------------------------------------------------------ 4. best fits of every mock
def tight(c, fixed=()):
    """The tolerances of tests/test_gpu_best_fit.py's tight(): 1e-7 of each width, 1e-10 in lnL."""
    return dict(xtol={n: 1e-7 * w for n, w in zip(c.names, c.width) if n not in fixed}, ftol=1e-10, max_iter=3000, restarts=2)


def scipy_best(c, neg_lnl, x0, sign=1.0):
    """scipy's Nelder-Mead from the start simplex of the device search (vertex j: x0 + proposal_j e_j; ``sign=-1``: another
    simplex, x0 - proposal_j e_j), in box-normalised coordinates, with the tolerances of tight() - the construction of
    tests/test_gpu_best_fit.py's scipy_best over this case's parameters."""
    from scipy.optimize import minimize

    def f(u):
        x = c.lo + u * c.width
        if np.any(x < c.lo) or np.any(x > c.hi):
            return np.inf
        v = neg_lnl(x)
        return v if np.isfinite(v) else np.inf
    x0 = np.asarray(x0, dtype=float)
    step = sign * np.array([PARAMS[n]["proposal"] for n in c.names], dtype=float)
    sim = [x0.copy()]
    for j in range(len(x0)):
        v = x0.copy()
        v[j] = x0[j] + step[j] if c.lo[j] <= x0[j] + step[j] <= c.hi[j] else x0[j] - step[j]
        sim.append(v)
    sim = (np.array(sim) - c.lo) / c.width
    r = minimize(f, sim[0], method="Nelder-Mead",
                 options=dict(initial_simplex=sim, xatol=1e-7, fatol=1e-10, maxiter=20000, maxfev=20000))
    return c.lo + r.x * c.width, -r.fun


@pytest.mark.parametrize("name", ["dsplit_cov", "boss_grid", "dsplit_diag"])
def test_best_fits_of_every_mock(case, oracle, name):
    """Against scipy's Nelder-Mead through ``log_likelihood_pairs`` from the same start simplex: lnL no lower than scipy's
    (to 1e-6) in every case, and the position within 1e-3 of the prior widths in the density-split cases.  For the BOSS pair the
    positions are printed, not asserted: the definition side does not determine them there (SCIPY_POSITIONS above: scipy from
    two start simplices ends 0.2 of a width and 18 in lnL apart), so the requirement is on lnL alone."""
    c = case(name)
    R = len(c.jr)
    bf = c.jr.best_fit(PARAMS, fixed=c.fixed, **tight(c))
    again = c.jr.best_fit(PARAMS, fixed=c.fixed, **tight(c))
    assert bf.names == c.names and bf.x.shape == (R, len(c.names)) and np.all(bf.status == bf.CONVERGED), bf.status
    for a in ("x", "lnl", "chi2", "status", "n_iter", "n_evals"):
        assert getattr(bf, a).tobytes() == getattr(again, a).tobytes(), a
    start = np.array([PARAMS[n]["ref"]["loc"] for n in c.names])
    for k in (0, R - 1):
        def neg(x, k=k):
            return -c.jr.log_likelihood_pairs(c.points(x[None, :]), [k])[0][0]
        x_s, lnl_s = scipy_best(c, neg, start)
        print(name, "mock", k, "lnL device", bf.lnl[k], "scipy", lnl_s, "position difference / width", (bf.x[k] - x_s) / c.width)
        assert bf.lnl[k] >= lnl_s - 1e-6, (name, k, bf.lnl[k], lnl_s)
        if SCIPY_POSITIONS[name]:
            assert np.all(np.abs(bf.x[k] - x_s) <= 1e-3 * c.width), (name, k, (bf.x[k] - x_s) / c.width)
    # the reported (lnL, chi2) are those of the reported point
    pts = c.points(bf.x)
    lnl, chi2 = c.jr.log_likelihood_pairs(pts, np.arange(R))
    bound = np.array([c.bound(m, {key: v[m:m + 1] for key, v in pts.items()})[0] for m in range(R)])
    assert_same_chi2(bf.chi2, chi2, bound, what=f"{name}: best fit vs log_likelihood_pairs")
    assert_same_lnl(bf.lnl, lnl, bound, what=f"{name}: best fit vs log_likelihood_pairs")
    ol, oc = c.oracle_at(oracle, 1, bf.point(1))
    assert abs(ol - bf.lnl[1]) <= 1e-9 * abs(ol) and abs(oc - bf.chi2[1]) <= 1e-9 * abs(oc), (name, ol, bf.lnl[1], oc, bf.chi2[1])


# ------------------------------------------------------------------ 5. noise-free recovery
def test_noise_free_joint_realisations_recover_their_points(case, tmp_path):
    from victor_amd.joint import JointFit
    c = case("dsplit_cov")
    rng = np.random.default_rng(5)
    truth = c.lo + c.width * (0.2 + 0.6 * rng.random((5, len(c.names))))
    pts = c.points(truth)
    opts = []
    for q, ((model, data), fit) in enumerate(zip(c.opts, c.fits)):
        t = fit.theory_vector_batch(pts)
        data = cases.clone(data)
        ccf = data["redshift_space_ccf"]
        stack = dict(np.load(ccf["data_file"], allow_pickle=True).item())
        n_s = len(fit.s)
        for j, key in enumerate(ccf["ccf_keys"][1:]):
            stack[key] = t[:, j * n_s:(j + 1) * n_s].reshape(np.shape(stack[key]))
        ccf["data_file"] = str(tmp_path / f"noise_free_q{q}.npy")
        np.save(ccf["data_file"], stack, allow_pickle=True)
        opts.append((model, data))
    fits = fits_of(opts)
    for covariance in (c.covariance, None):
        jr = JointFit(fits, covariance=covariance).realisations()
        at_truth = jr.log_likelihood_pairs(pts, np.arange(5))[0]
        bf = jr.best_fit(PARAMS, fixed=c.fixed, **tight(c))
        print("noise-free, covariance" if covariance is not None else "noise-free, block-diagonal", "chi2", bf.chi2,
              "position difference / width", np.abs(bf.x - truth).max(axis=0) / c.width)
        assert np.all(bf.status == bf.CONVERGED), bf.status
        assert np.all(bf.chi2 <= 1e-6), bf.chi2
        assert np.all(bf.lnl >= at_truth - 1e-6), (bf.lnl, at_truth)


# ------------------------------------------------------------------ 6. the data vectors: best fit and profile
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_data_vector_joint_best_fit_and_profile(case, name):
    from victor_amd import InputError
    c = case(name)
    grid = np.array([0.35, 0.47, 0.6])
    prof = c.joint.best_fit(PARAMS, fixed=dict(c.fixed, fsigma8=grid), **tight(c, ["fsigma8"]))
    assert len(prof) == 3 and prof.names == ["sigma_v", "epsilon"] and np.array_equal(prof.params["fsigma8"], grid)
    assert np.all(prof.status == prof.CONVERGED), prof.status
    pts = c.points(prof.x, prof.names, fsigma8=0.0)
    pts["fsigma8"] = grid
    lnl, chi2 = c.joint.log_likelihood_batch(pts)
    bound = c.bound_of(c.joint, pts)
    assert_same_chi2(prof.chi2, chi2, bound, what=f"{name}: profile vs log_likelihood_batch")
    assert_same_lnl(prof.lnl, lnl, bound, what=f"{name}: profile vs log_likelihood_batch")
    free = c.joint.best_fit(PARAMS, fixed=c.fixed, **tight(c))
    assert len(free) == 1 and free.status[0] == free.CONVERGED and free.names == c.names
    one = c.points(free.x)
    lnl, chi2 = c.joint.log_likelihood_batch(one)
    bound = c.bound_of(c.joint, one)
    assert_same_chi2(free.chi2, chi2, bound, what=f"{name}: data-vector best fit vs log_likelihood_batch")
    assert_same_lnl(free.lnl, lnl, bound, what=f"{name}: data-vector best fit vs log_likelihood_batch")
    with pytest.raises(InputError, match="outside"):
        c.joint.best_fit(PARAMS, fixed=c.fixed, start={"sigma_v": 600.0})


# ------------------------------------------------------------------ 7. workflow and cuts
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_best_fit_then_chains_cuts_and_a_dropped_joint_fit(case, name):
    from victor_amd.joint import JointFit
    c = case(name)
    joint = JointFit(fits_of(c.opts), covariance=c.covariance)      # (its own: the fixture's must outlive this test)
    jr = joint.realisations()
    kw = dict(walkers=2, burn=8, fixed=c.fixed)
    bf = jr.best_fit(PARAMS, fixed=c.fixed)
    whole = jr.sample_chains(PARAMS, 70, start=bf, **kw)
    lean = jr.sample_chains(PARAMS, 70, start=bf, keep_chain=False, **kw)
    ch = jr.sample_chains(PARAMS, 40, start=bf, **kw)
    data = joint.sample_chains(PARAMS, 10, walkers=4, fixed=c.fixed)
    data_whole = joint.sample_chains(PARAMS, 70, walkers=4, fixed=c.fixed)
    del joint, jr
    gc.collect()
    ch.extend(30)
    data.extend(60)
    attrs = HISTORY + ("lnl", "chi2", "mean", "cov", "sum1", "sum2", "rhat")
    for a in attrs:
        assert same_bytes(getattr(ch, a), getattr(whole, a)), ("40 + 30", a)
        assert same_bytes(getattr(data, a), getattr(data_whole, a)), ("data vector, 10 + 60", a)
    assert whole.n_kept == 62 and lean.chain is None
    for a in ("x", "lnl", "chi2", "mean", "cov", "n_accept", "sum1", "sum2", "pivot"):
        assert same_bytes(getattr(lean, a), getattr(whole, a)), ("keep_chain=False", a)
    for m in range(len(bf)):
        assert_sums(lean.sum1[m], lean.sum2[m], whole.chain[:, m], whole.pivot[m], f"{name}: device sums, realisation {m}")
        assert_pooled(lean.mean[m], lean.cov[m], whole.chain[:, m], whole.pivot[m], whole.n_kept * 2.0 ** -52, f"{name}: realisation {m}")


def test_a_call_on_another_lead_engine_leaves_live_chains_their_covariance(case):
    """Which engine leads a joint evaluation depends on the call's options (the Simpson rule, the matter model), and the
    covariance tables are uploaded once per lead engine: a call with other options between ``sample_chains`` and ``extend``
    must not release the tables the chains' handle reads."""
    from victor_amd.joint import JointFit
    c = case("dsplit_cov")
    joint = JointFit(fits_of(c.opts), covariance=c.covariance)
    jr = joint.realisations()
    kw = dict(walkers=2, fixed=c.fixed)
    whole, data_whole = jr.sample_chains(PARAMS, 70, **kw), joint.sample_chains(PARAMS, 70, **kw)
    ch, data = jr.sample_chains(PARAMS, 40, **kw), joint.sample_chains(PARAMS, 40, **kw)
    assert len(joint._handles) == 1
    pts = c.points(whole.x[:, 0])
    default = joint.log_likelihood_batch(pts)
    other = joint.log_likelihood_batch(pts, simpson_even="avg")                 # another lead engine, its own tables
    jr.log_likelihood_pairs(pts, np.arange(5), simpson_even="avg")
    third = joint.sample_chains(PARAMS, 3, simpson_even="avg", **kw)            # a second Chains on the other engine
    assert len(joint._handles) == 2 and not same_bytes(default[1], other[1])
    ch.extend(30)
    data.extend(30)
    third.extend(3)
    for a in HISTORY + ("lnl", "chi2"):
        assert same_bytes(getattr(ch, a), getattr(whole, a)), ("mocks", a)
        assert same_bytes(getattr(data, a), getattr(data_whole, a)), ("data vector", a)
    assert same_bytes(joint.log_likelihood_batch(pts)[1], default[1])


# ------------------------------------------------------------------ 8. the C ABI's refusals
def test_c_abi_guards(case):
    """Every refusal of vk_fit_create_joint / vk_chain_create_joint that one device and these fixtures can reach: NULL and the
    text in err; on a handle, VK_E_ARG and the text through *_last_error; a valid call on the same contexts then succeeds.
    (Contexts on different devices are tried where a second device is visible.  The LDS refusal cannot be reached here: under a
    covariance vk_joint_cov_create refuses such a joint vector first, and block-diagonal it takes a data vector of more than
    140 bins, which no fixture has.)"""
    from victor_amd import _native as N
    from victor_amd.engine import Engine
    c = case("dsplit_cov")
    joint, jr, fits = c.joint, c.jr, c.fits
    engines, opts = joint._plan_cov({})
    lead = engines[0]
    lib = lead._lib
    h = joint._joint_handle(lead)
    jr._upload(engines)
    i32 = C.POINTER(C.c_int32)
    R, names = 2, ["fsigma8", "sigma_v"]
    lo, hi = N.f64(c.lo[:2]), N.f64(c.hi[:2])
    cols = np.array([N.ROW_COLUMNS[n] for n in names], dtype=np.int32)
    x0 = N.f64(np.array([[0.47, 380.0], [0.5, 350.0]]))
    rows = N.f64(fits[0]._fit_rows({"fsigma8": x0[:, 0], "sigma_v": x0[:, 1], "beta": BETA, "epsilon": 1.0}, fits[0].model))
    good = [e._ctx for e in engines]

    def create(entry, ctxs, hh=h, which=(0, 4), k=None):
        cc = (C.c_void_p * len(ctxs))(*ctxs)
        w = None if which is None else np.array(which, dtype=np.int32)
        err = C.create_string_buffer(512)
        out = getattr(lib, entry)(cc, len(ctxs) if k is None else k, hh, C.byref(opts), R, 2, cols.ctypes.data_as(i32), N.as_dp(lo),
                                  N.as_dp(hi), N.as_dp(rows), 1.0, None if w is None else w.ctypes.data_as(i32), err, len(err))
        return out, err.value.decode()

    nodata = Engine(fits[1], None, device=fits[1]._device, matter_model=fits[1].matter_model,
                    simpson_even=fits[1]._simpson_rule(fits[1].model["simpson_even"]))
    boss = case("boss_grid")                                      # a block of another size: a BOSS block's context
    other_size = boss.joint._plan_cov({})[0][1]._ctx
    boss_n = len(boss.fits[1].s) * len(boss.fits[1].poles_s)
    assert boss_n != 120
    for entry, destroy in (("vk_fit_create_joint", lib.vk_fit_destroy), ("vk_chain_create_joint", lib.vk_chain_destroy)):
        for hh in (h, None):
            out, text = create(entry, [good[0], None, good[2]], hh)
            assert not out and "context 1 is NULL" in text, text
            out, text = create(entry, [good[0], nodata._ctx, good[2]], hh)
            assert not out and "context 1 was created without a data vector" in text, text
            out, text = create(entry, good, hh, which=(0, 5))
            assert not out and "outside 0..4" in text, text
        out, text = create(entry, good[:2])
        assert not out and "2 contexts for 3 blocks" in text, text
        out, text = create(entry, [good[0], other_size, good[2]])
        assert not out and "block 1 has 120 entries, its context %d" % boss_n in text, text
        out, text = create(entry, [good[1], good[0], good[2]])
        assert not out and "not the context the handle was created with" in text, text
        engines[1].set_realisations(np.empty((0, 120)))
        engines[1]._real_owner = None
        out, text = create(entry, good)
        assert not out and "no realisations are set on context 1" in text, text
        engines[1].set_realisations(jr.blocks[1].blocks[:4])
        out, text = create(entry, good, None)
        assert not out and "context 1 holds 4 realisations, context 0 holds 5" in text, text
        out, text = create(entry, good, which=None)               # the data vectors need no realisations
        assert out, text
        destroy(out)
        jr._upload(engines)
        if lib.vk_device_count() > 1:
            other = Engine(fits[1], fits[1]._fit_side(), device=1, matter_model=fits[1].matter_model,
                           simpson_even=fits[1]._simpson_rule(fits[1].model["simpson_even"]))
            out, text = create(entry, [good[0], other._ctx, good[2]])
            assert not out and "same device" in text, text
        out, text = create(entry, good)
        assert out, text
        destroy(out)
    # on a handle: the realisations of a block are gone when the run starts
    step, xtol = N.f64(np.array([0.02, 10.0])), N.f64(np.array([1e-6, 1e-3]))
    x, lnl, chi2 = np.empty((R, 2)), np.empty(R), np.empty(R)
    status, n_iter, n_evals = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.int32), np.empty(R, dtype=np.int64)

    def run(f):
        return lib.vk_fit_run(f, N.as_dp(x0), N.as_dp(step), N.as_dp(xtol), 1e-8, 400, 0, N.as_dp(x), N.as_dp(lnl), N.as_dp(chi2),
                              status.ctypes.data_as(i32), n_iter.ctypes.data_as(i32), n_evals.ctypes.data_as(C.POINTER(C.c_int64)))
    f, text = create("vk_fit_create_joint", good)
    ch, text2 = create("vk_chain_create_joint", good)
    assert f and ch, (text, text2)
    engines[2].set_realisations(np.empty((0, 120)))
    engines[2]._real_owner = None
    assert run(f) == -1 and "no realisations are set on context 2" in lib.vk_fit_last_error(f).decode()
    assert lib.vk_chain_start(ch, N.as_dp(x0)) == -1 and "no realisations are set on context 2" in lib.vk_chain_last_error(ch).decode()
    far = N.f64(np.array([[0.47, 380.0], [0.5, 900.0]]))
    jr._upload(engines)
    assert lib.vk_chain_start(ch, N.as_dp(far)) == -1 and "outside the box" in lib.vk_chain_last_error(ch).decode()
    assert run(f) == 0, lib.vk_fit_last_error(f).decode()
    assert np.all(np.isfinite(lnl)) and np.all(status == 0), (lnl, status)
    assert lib.vk_chain_start(ch, N.as_dp(x0)) == 0, lib.vk_chain_last_error(ch).decode()
    want = jr.log_likelihood_pairs(c.points(x, names, epsilon=1.0), [0, 4])
    assert_same_lnl(lnl, want[0], np.array([c.bound(m, c.points(x[i:i + 1], names, epsilon=1.0))[0] for i, m in enumerate((0, 4))]),
                    what="vk_fit_run on a joint handle vs log_likelihood_pairs")
    lib.vk_fit_destroy(f)
    lib.vk_chain_destroy(ch)
    # the Python layer answers as before
    bf = jr.best_fit(PARAMS, fixed=dict(c.fixed, epsilon=1.0), max_iter=5)
    assert len(bf) == 5 and np.all(bf.status == bf.MAX_ITER)


# ------------------------------------------------------------------ 9. the host entry point the samplers share their launches with
@pytest.mark.parametrize("name", ["dsplit_cov", "boss_grid"])
def test_the_pairs_mode_entry_point_returns_the_same_bits_around_a_sampler_run(case, name):
    c = case(name)
    R = len(c.jr)
    hp = cases.halton_params(23, with_beta=True)
    which = (np.arange(23) * 3) % R
    before = c.jr.log_likelihood_pairs(hp, which)
    cross = c.jr.log_likelihood(hp)
    c.jr.best_fit(PARAMS, fixed=c.fixed, max_iter=20)
    c.jr.sample_chains(PARAMS, 5, walkers=2, fixed=c.fixed)
    after = c.jr.log_likelihood_pairs(hp, which)
    for a, b in zip(before, after):
        assert same_bytes(a, b)
    for a, b in zip(before, cross):
        assert same_bytes(a, b[np.arange(23), which])                  # (and pairs mode still returns cross mode's bits)
