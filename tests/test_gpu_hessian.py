"""Hessians and Laplace covariances on the GPU (``laplace`` of ``CCFFit`` / ``Realisations`` / ``JointFit`` /
``JointRealisations``, ``best_fit(covariance=True)``; vk_fit_hessian): the values of the stencil against the
single-point paths at :func:`victor_amd.laplace.stencil_points`, with chunk edges inside problems; A, the status, the Hessian and
the covariance against the NumPy statement from the device's own values, byte for byte; A against the oracle; the prior's
contribution; the widest joint stencil (d = 10, a row set per block) against the host route; the faces of the box; and the best
fit that carries its covariance into correlated chains.

Shapes: the fixed-covariance BOSS stack as noise-free realisations of known points (the construction of
tests/test_gpu_best_fit.py: truths in the inner 60 % of the box, so every stencil lies inside it and the maximum is the truth) -
R = 16 with d = 4 (rows_max 80 against M = 33) and R = 70 with d = 1 (M = 3, more than one workgroup of the rows kernel and 70
workgroups of the assemble kernel); the data vector with R = 1 (rows_max 5 < M = 33); the five density-split blocks.
"""

import faulthandler
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_joint_blocks import blocks_bound
from tests.test_gpu_priors import BETA, Five, boss_prior, joint_prior, resolved, same_run
from tests.test_realisations import REAL, stack_options
from tests.tolerances import U, _tau, assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "beta", "sigma_v", "epsilon"]
LO = np.array([PARAMS[n]["prior"]["min"] for n in NAMES], dtype=float)
HI = np.array([PARAMS[n]["prior"]["max"] for n in NAMES], dtype=float)
STEP = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
OUT = ("values", "a", "hessian", "cov", "status", "step", "lnpost", "chi2", "x")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class NoiseFree:
    """86 noise-free realisations of the fixed-covariance stack: 16 at random points of the inner 60 % of the box, then 70 that
    differ in sigma_v alone (the other parameters at ``common``).  With ``truth`` (n, 4): a stack of those truths instead."""

    def __init__(self, tmp, truth=None):
        import victor_amd
        self.base = victor_amd.CCFFit(*stack_options(fixed=True))
        if truth is None:
            rng = np.random.default_rng(5)
            self.truth = LO + (HI - LO) * (0.2 + 0.6 * rng.random((86, 4)))
            self.common = self.truth[16].copy()
            self.truth[16:, [0, 1, 3]] = self.common[[0, 1, 3]]
        else:
            self.truth, self.common = np.array(truth, dtype=float), None
        t = self.base.theory_vector_batch({n: self.truth[:, j] for j, n in enumerate(NAMES)})
        n_s = len(self.base.s)
        s = np.load(os.path.join(REAL, "stack_fixed.npy"), allow_pickle=True).item()
        path = str(tmp / "noise_free.npy")
        np.save(path, dict(s, monopole=t[:, :n_s], quadrupole=t[:, n_s:2 * n_s]), allow_pickle=True)
        self.data = t
        self.fit = victor_amd.CCFFit(*stack_options(fixed=True, data_file=path))
        assert self.fit.fixed_data and self.fit.fixed_covmat

    def bound(self, batch, which):
        """tests/tolerances.chi2_bound for rows against realisation ``which[i]`` (fixed data, fixed covariance): the same
        formula, 64 u |r|^T |P| (|r| + 2 tau), with the realisation's data vector for d - plus the term that formula, being first
        order in the residual, drops: theory entries that move by |dt_k| <= 64 u tau_k change chi2 by 2 r^T P dt + dt^T P dt, and
        at a noise-free truth r is exactly 0, so (64 u)^2 tau^T |P| tau is all that is left."""
        t = self.fit.theory_vector_batch(batch)
        absr = np.abs(t - self.data[which])
        tau, absP = _tau(self.fit), np.abs(self.fit.icov)
        return 64 * U * np.einsum("ij,jk,ik->i", absr, absP, absr + 2.0 * tau[None, :]) + (64 * U) ** 2 * (tau @ absP @ tau)


@pytest.fixture(scope="module")
def noise_free(tmp_path_factory):
    return NoiseFree(tmp_path_factory.mktemp("noise_free"))


def against_the_mirror(lap, lo, hi, what):
    """A, status, hess and cov of the device against the NumPy statement on the device's own values."""
    from victor_amd import laplace as L
    m = L.assemble(lap.values, lap.x, lap.step, lo, hi)
    assert np.array_equal(lap.status, m.status), (what, lap.status, m.status)
    assert same_bytes(lap.a, m.a), (what, "A", np.nanmax(np.abs(lap.a - m.a)))
    # FP64 division and square root are correctly rounded at the compiler's defaults: the same bytes
    assert same_bytes(lap.hessian, m.hess), (what, "hess", np.nanmax(np.abs(lap.hessian - m.hess)))
    assert same_bytes(lap.cov, m.cov), (what, "cov", np.nanmax(np.abs(lap.cov - m.cov) / np.abs(m.cov)))
    assert same_bytes(lap.lnpost, lap.values[:, 0])
    return m


def same_laplace(a, b, what, rows=slice(None)):
    for name in OUT:
        u, v = getattr(a, name), getattr(b, name)
        if u is None and v is None:
            continue
        assert same_bytes(u[rows], v[rows]), (what, name)


# ------------------------------------------------------------------ 1. values and the statistic -----------------------------
def test_noise_free_realisations_d4(noise_free):
    """R = 16, d = 4: rows_max = 80 against M = 33 - seven chunks, every chunk edge inside a problem."""
    from victor_amd import laplace as L
    nf = noise_free
    rs = nf.fit.realisations(list(range(16)))
    at = {n: nf.truth[:16, j] for j, n in enumerate(NAMES)}
    lap = rs.laplace(PARAMS, at, keep_values=True)
    assert lap.names == NAMES and lap.values.shape == (16, 33) and lap.cov.shape == (16, 4, 4)
    assert same_bytes(lap.step, np.tile(STEP, (16, 1)))                      # the inner 60 %: no step is shrunk
    pts = L.stencil_points(lap.x, lap.step, LO, HI)
    which = np.repeat(np.arange(16, dtype=np.int32), 33)
    batch = {n: np.ascontiguousarray(pts.reshape(-1, 4)[:, j]) for j, n in enumerate(NAMES)}
    lnl, chi2 = rs.log_likelihood_pairs(batch, which)
    assert_same_lnl(lap.values.ravel(), lnl, nf.bound(batch, which), what="stencil values vs log_likelihood_pairs, R 16 d 4")
    assert_same_chi2(lap.chi2, chi2.reshape(16, 33)[:, 0], nf.bound(batch, which).reshape(16, 33)[:, 0], what="centre chi2, R 16 d 4")
    assert np.all(lap.status == lap.OK), lap.status
    assert np.all(np.swapaxes(lap.a, 1, 2) == lap.a) and np.all(np.linalg.eigvalsh(lap.a) > 0)
    against_the_mirror(lap, LO, HI, "R 16 d 4")
    print("sigma at the truths:", lap.sigma[:3], "condition of A:", np.linalg.cond(lap.a)[:3])
    assert np.all(lap.sigma > 0) and np.all(np.abs(np.einsum("rjj->rj", lap.corr) - 1) < 1e-12)
    assert np.all(np.isfinite(lap.ln_evidence)) and np.all(lap.lnprior == 0) and same_bytes(lap.lnl, lap.lnpost)
    again = rs.laplace(PARAMS, at, keep_values=True)
    same_laplace(lap, again, "two identical calls")
    assert rs.laplace(PARAMS, at).values is None


def test_seventy_problems_d1(noise_free):
    """R = 70, d = 1: M = 3, rows_max = 280 - one chunk of 210 rows, four workgroups of the rows kernel, 70 of the assemble kernel."""
    from victor_amd import laplace as L
    nf = noise_free
    numbers = list(range(16, 86))
    rs = nf.fit.realisations(numbers)
    fixed = {n: float(nf.common[j]) for j, n in enumerate(NAMES) if n != "sigma_v"}
    lap = rs.laplace(PARAMS, {"sigma_v": nf.truth[16:, 2]}, fixed=fixed, keep_values=True)
    assert lap.names == ["sigma_v"] and lap.values.shape == (70, 3) and lap.cov.shape == (70, 1, 1)
    pts = L.stencil_points(lap.x, lap.step, LO[2:3], HI[2:3])
    assert same_bytes(pts[:, :, 0], np.stack([lap.x[:, 0], lap.x[:, 0] + 10.0, lap.x[:, 0] - 10.0], axis=1))
    which = np.repeat(np.arange(70, dtype=np.int32), 3)
    batch = dict(fixed, sigma_v=np.ascontiguousarray(pts.reshape(-1)))
    lnl, _ = rs.log_likelihood_pairs(batch, which)
    full = {n: (np.full(210, batch[n]) if np.ndim(batch[n]) == 0 else batch[n]) for n in NAMES}
    assert_same_lnl(lap.values.ravel(), lnl, nf.bound(full, np.asarray(numbers)[which]), what="stencil values vs log_likelihood_pairs, R 70 d 1")
    assert np.all(lap.status == lap.OK) and np.all(lap.a > 0)
    against_the_mirror(lap, LO[2:3], HI[2:3], "R 70 d 1")
    assert np.array_equal(lap.params["beta"], np.full(70, fixed["beta"]))


def test_data_vector_d4():
    """R = 1: rows_max = 5 < M = 33 - seven chunks of one problem."""
    import victor_amd
    from victor_amd import laplace as L
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    at = {"fsigma8": 0.47, "beta": 0.37, "sigma_v": 380.0, "epsilon": 1.0}
    lap = fit.laplace(PARAMS, at, keep_values=True)
    assert lap.values.shape == (1, 33)
    pts = L.stencil_points(lap.x, lap.step, LO, HI)[0]
    batch = {n: np.ascontiguousarray(pts[:, j]) for j, n in enumerate(NAMES)}
    lnl, chi2 = fit.log_likelihood_batch(batch)
    assert_same_lnl(lap.values[0], lnl, chi2_bound(fit, batch), what="stencil values vs log_likelihood_batch, data vector")
    against_the_mirror(lap, LO, HI, "data vector")
    one = fit.log_likelihood(at)
    assert abs(lap.lnl[0] - one[0]) <= 1e-9 * abs(one[0]) and abs(lap.chi2[0] - one[1]) <= 1e-9 * abs(one[1])
    again = fit.laplace(PARAMS, at, keep_values=True)
    same_laplace(lap, again, "two identical calls, data vector")


# ------------------------------------------------------------------ 2. against the oracle ------------------------------------
def test_against_the_oracle():
    """Mock 5 of the fixed-covariance stack, beta fixed, d = 3: 19 oracle evaluations at the same stencil.  An entry of A
    combines four values (the diagonal: v0 twice), each within the parity figure 1e-9 of tests/test_gpu_best_fit.py."""
    import victor_amd
    from victor_amd import laplace as L
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle as vo
    rs = victor_amd.CCFFit(*stack_options(fixed=True)).realisations([5])
    names = ["fsigma8", "sigma_v", "epsilon"]
    at = {"fsigma8": 0.45, "sigma_v": 390.0, "epsilon": 1.01}
    lap = rs.laplace(PARAMS, at, fixed={"beta": 0.4}, keep_values=True)
    assert lap.names == names and lap.values.shape == (1, 19) and lap.status[0] != lap.AT_BOUND
    j = [NAMES.index(n) for n in names]
    pts = L.stencil_points(lap.x, lap.step, LO[j], HI[j])[0]
    ofit = vo.OracleFit(*stack_options(fixed=True, simulation_number=5))
    v = np.array([ofit.log_likelihood(dict({n: float(p[i]) for i, n in enumerate(names)}, beta=0.4))[0] for p in pts])
    want = L.assemble(v[None], lap.x, lap.step, LO[j], HI[j])
    tol = 4 * 1e-9 * np.max(np.abs(v))
    print("max |dA|", np.max(np.abs(lap.a - want.a)), "tolerance", tol, "A", lap.a[0])
    assert np.all(np.abs(lap.a - want.a) <= tol)


# ------------------------------------------------------------------ 3. the prior ---------------------------------------------
def prior_term(lap0, lap1, precision, what):
    """A(with the prior) - A(without) = h_j h_k P_jk to 16 u max|v|: the lnL bits are those of the same launches, each of the
    <= 4 values of an entry carries one rounding of lnL + lp, and the combination <= 8 more."""
    assert same_bytes(lap0.step, lap1.step) and same_bytes(lap0.x, lap1.x)
    assert not np.any(lap0.status == lap0.AT_BOUND) and not np.any(lap0.status == lap0.NOT_FINITE)
    hh = lap0.step[:, :, None] * lap0.step[:, None, :]
    got, want = lap1.a - lap0.a, hh * precision
    tol = 16 * U * max(np.max(np.abs(lap1.values)), np.max(np.abs(lap0.values)))
    print(what, "max |dA - h h P|", np.max(np.abs(got - want)), "tolerance", tol)
    assert np.all(np.abs(got - want) <= tol), what
    assert np.any(np.abs(want) > 100 * tol), "the prior is invisible at this tolerance: the test does not reach it"


def test_prior_on_a_single_fit():
    import victor_amd
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    at = {"fsigma8": 0.47, "beta": 0.37, "sigma_v": 380.0, "epsilon": 1.0}
    r = resolved(boss_prior(), NAMES)
    lap0 = fit.laplace(PARAMS, at, keep_values=True)
    lap1 = fit.laplace(PARAMS, at, prior=boss_prior(), keep_values=True)
    prior_term(lap0, lap1, r.precision, "single fit")
    assert lap1.ln_evidence is None and same_bytes(lap1.lnprior, r.lnprior(lap1.x)) and lap1.lnprior[0] < 0
    assert same_bytes(lap1.lnl, lap1.lnpost - lap1.lnprior)
    from victor_amd import laplace as L
    pts = L.stencil_points(lap1.x, lap1.step, LO, HI)
    assert same_bytes(lap1.values, lap0.values + r.lnprior(pts))          # the same lnL bits, one addition each
    against_the_mirror(lap1, LO, HI, "single fit under a prior")


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    made = {}

    def get(cov):
        if cov not in made:
            made[cov] = Five(tmp_path_factory.mktemp("five_cov" if cov else "five_diag"), cov)
        return made[cov]
    return get


def blocked(names=("sigma_v",)):
    from victor_amd.joint import per_block
    return per_block(PARAMS, list(names), 5)


def test_prior_on_the_density_split_joint(five):
    c = five(True)
    names = ["fsigma8"] + [f"sigma_v@{q}" for q in range(5)]
    at = dict({"fsigma8": 0.47}, **{f"sigma_v@{q}": 340.0 + 15.0 * q for q in range(5)})
    fixed = {"beta": BETA, "epsilon": 1.0}
    r = resolved(joint_prior(), names)
    lap0 = c.joint.laplace(blocked(), at, fixed=fixed, keep_values=True)
    lap1 = c.joint.laplace(blocked(), at, fixed=fixed, prior=joint_prior(), keep_values=True)
    assert lap0.names == names and lap0.values.shape == (1, 73)
    prior_term(lap0, lap1, r.precision, "density-split joint")
    assert r.precision[2, 4] != 0 and not np.any(r.precision[0])            # correlated on sigma_v@1, sigma_v@3; none on fsigma8


# ------------------------------------------------------------------ 4. joint, per block, widest ------------------------------
TEN = [f"fsigma8@{q}" for q in range(5)] + [f"sigma_v@{q}" for q in range(5)]


@pytest.mark.parametrize("data", [True, False], ids=["data", "mocks"])
def test_ten_per_block_parameters(five, data):
    """d = 10, M = 201: the data (rows_max 11: nineteen chunks) and 3 joint mocks (rows_max 33), values and A against the host
    route (``device=False``: the same stencil through log_likelihood_batch / log_likelihood_pairs and the NumPy statement)."""
    from victor_amd import laplace as L
    c = five(True)
    block = blocked(("fsigma8", "sigma_v"))
    fixed = {"beta": BETA, "epsilon": 1.0}
    R = 1 if data else 3
    target = c.joint if data else c.joint.realisations([0, 1, 2])
    at = {n: (0.44 + 0.015 * q if n.startswith("fsigma8") else 350.0 + 12.0 * q) + 0.01 * np.arange(R) * (1 if n.startswith("fsigma8") else 100)
          for q in range(5) for n in (f"fsigma8@{q}", f"sigma_v@{q}")}
    dev = target.laplace(block, at, fixed=fixed, keep_values=True)
    assert dev.names == TEN and dev.values.shape == (R, 201) and dev.a.shape == (R, 10, 10)
    from victor_amd.laplace import laplace
    host = laplace(c.joint, block, at, fixed=fixed, keep_values=True, realisations=None if data else target, device=False)
    lo = np.array([PARAMS[n.partition("@")[0]]["prior"]["min"] for n in TEN], dtype=float)
    hi = np.array([PARAMS[n.partition("@")[0]]["prior"]["max"] for n in TEN], dtype=float)
    pts = L.stencil_points(dev.x, dev.step, lo, hi)
    bound = np.empty((R, 201))
    for m in range(R):
        batch = dict({n: np.ascontiguousarray(pts[m, :, j]) for j, n in enumerate(TEN)}, **{k: np.full(201, v) for k, v in fixed.items()})
        bound[m] = blocks_bound(c.joint if data else c.of(m), batch)
    assert_same_lnl(dev.values.ravel(), host.values.ravel(), bound.ravel(), what=f"d 10 stencil values, {'data' if data else 'mocks'}")
    against_the_mirror(dev, lo, hi, "d 10")
    # an entry of A is a combination of four values with coefficients of magnitude <= 1
    per_value = 0.51 * bound + 16 * U * (np.abs(host.values) + 1000.0)
    tol = 4 * per_value.max(axis=1)[:, None, None]
    ok = (dev.status != dev.AT_BOUND) & (dev.status != dev.NOT_FINITE)
    assert np.array_equal(ok, (host.status != host.AT_BOUND) & (host.status != host.NOT_FINITE)) and np.all(ok)
    print("d 10 status", dev.status, "max |dA|", np.max(np.abs(dev.a - host.a)), "tolerance", tol.ravel())
    assert np.all(np.abs(dev.a - host.a) <= tol)


# ------------------------------------------------------------------ 5. the faces of the box ----------------------------------
def test_faces(noise_free):
    nf = noise_free
    rs = nf.fit.realisations([0, 1, 2])
    h = STEP[2]
    at = {n: nf.truth[:3, j].copy() for j, n in enumerate(NAMES)}
    inner = rs.laplace(PARAMS, at, keep_values=True)
    at["sigma_v"][1] = HI[2] - h / 2
    at["sigma_v"][2] = HI[2] - h / 16
    lap = rs.laplace(PARAMS, at, keep_values=True)
    assert lap.status.tolist() == [lap.OK, lap.OK, lap.AT_BOUND], lap.status
    assert lap.step[1, 2] == 0.999 * (HI[2] - at["sigma_v"][1]) and lap.step[2, 2] == h and lap.step[0, 2] == h
    assert np.all(np.isnan(lap.cov[2])) and np.all(np.isnan(lap.hessian[2])) and np.all(np.isnan(lap.a[2]))
    assert np.all(lap.values[2] == lap.values[2, 0]) and np.isfinite(lap.values[2, 0])        # every row of the problem at x
    assert np.all(np.isfinite(lap.cov[1])) and np.all(np.linalg.eigvalsh(lap.a[1]) > 0)
    same_laplace(lap, inner, "the problem beside a flagged one", rows=slice(0, 1))           # the other problems: unaffected
    at["sigma_v"][2] = nf.truth[2, 2]
    moved = rs.laplace(PARAMS, at, keep_values=True)
    assert moved.status.tolist() == [lap.OK] * 3
    same_laplace(lap, moved, "the problems beside a flagged one", rows=slice(0, 2))
    against_the_mirror(lap, LO, HI, "faces")


# ------------------------------------------------------------------ 6. best_fit(covariance=True) ------------------------------
def test_best_fit_carries_its_covariance_into_chains():
    import victor_amd
    rs = victor_amd.CCFFit(*stack_options(fixed=True)).realisations([0, 5, 11])
    fixed = {"epsilon": 1.0}                   # (epsilon fixed: both chain routes launch the same bytes, tests/test_gpu_chains.py)
    plain = rs.best_fit(PARAMS, fixed=fixed)
    bf = rs.best_fit(PARAMS, fixed=fixed, covariance=True)
    for a in ("x", "lnl", "chi2", "lnpost", "lnprior", "status", "n_iter", "n_evals"):
        assert same_bytes(getattr(bf, a), getattr(plain, a)), a
    assert plain.laplace is None and plain.cov is None and plain.sigma is None
    assert bf.cov is bf.laplace.cov and bf.sigma is bf.laplace.sigma and bf.cov.shape == (3, 3, 3)
    lap = rs.laplace(PARAMS, bf, fixed=fixed)
    same_laplace(bf.laplace, lap, "best_fit(covariance=True) vs laplace(at=bf)")
    print("status", lap.status, "sigma", lap.sigma)
    kept = rs.best_fit(PARAMS, fixed=fixed, covariance={"refine": 1, "keep_values": True, "step": {"sigma_v": 5.0}})
    again = rs.laplace(PARAMS, bf, fixed=fixed, refine=1, keep_values=True, step={"sigma_v": 5.0})
    same_laplace(kept.laplace, again, "covariance={...} vs laplace(...)")
    assert kept.laplace.values.shape == (3, 19)
    kw = dict(walkers=4, seed=2, fixed=fixed, start=bf, proposal=bf)
    ref = rs.sample_chains(PARAMS, 12, device=False, **kw)
    dev = rs.sample_chains(PARAMS, 12, **kw)
    same_run(dev, ref, "chains with correlated proposals")
    widths = rs.sample_chains(PARAMS, 12, **dict(kw, proposal=None))
    if np.any(lap.ok):
        assert not same_bytes(widths.chain, dev.chain), "the proposal changed nothing"
