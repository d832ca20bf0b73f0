"""Fisher matrices from model-vector Jacobians on the GPU (``fisher`` of ``CCFFit`` / ``Realisations`` / ``JointFit`` /
``JointRealisations``; vk_fit_fisher): the stencil's theory vectors against ``theory_vector_batch`` at
:func:`victor_amd.fisher.stencil_points`, with chunk edges inside problems; D, fisher, A, cov and the status against the NumPy
statement on the device's own vectors, byte for byte; the device against the definition route (``device=False``: other launch
shapes) and against the oracle at the derived bound of tests/fisher_bounds.py; blended covariance slices; the five density-split
blocks under one covariance and block-diagonal, with the 10 x 10 prior; the faces of the box; and no effect on other calls.

Shapes - the smallest at which the kernels can still go wrong (N entries, M = 2 d + 1 rows per problem, S = max(4, d + 1) rows of
a problem in the handle's largest launch, rows_max = R S):
  1. the fixed-covariance BOSS stack (tests/test_gpu_hessian.py's noise-free construction), d = 4, R = 16: N = 60, M = 9, S = 5,
     144 rows in 2 chunks of 80 + 64 - the edge inside problem 8; 3 workgroups of the rows kernel, 16 of the assemble kernel
  2. the same stack, d = 1, R = 70: N = 60, M = 3 < S = 4, 210 rows in 1 chunk of a buffer of 280; 4 workgroups of the rows
     kernel, 70 of the assemble kernel
  3. the beta-gridded BOSS data-vector handle, R = 1: N = 60, d = 4 (M = 9, S = 5: 2 chunks of 5 + 4) and d = 3 (M = 7, S = 4:
     2 chunks of 4 + 3); the centre's beta between two nodes, on a node, outside the grid
  4. the five density-split blocks, d = 10, R = 3: N = 600 (five segments of 120), M = 21, S = 11, 63 rows in 2 chunks of
     33 + 30 - the edge inside problem 1; 96 KiB of LDS in the assemble kernel (above the 64 KiB default)
  6. the oracle: the BOSS data-vector handle at d = 2 (M = 5) and the isotropic synthetic fit (N = 80) at d = 3 (M = 7)
  7. three problems of the stack, one of them a sixteenth of a step from a face
"""

import faulthandler
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.fisher_bounds import assert_same_fisher, same_theory_delta
from tests.test_chains import same_bytes
from tests.test_gpu_hessian import HI, LO, NAMES, PARAMS, STEP, NoiseFree
from tests.test_gpu_parity import RTOL
from tests.test_gpu_priors import BETA, Five
from tests.test_gpu_ten_parameters import TEN, full_prior
from tests.tolerances import assert_same_theory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("fisher", "a", "cov", "status", "step", "x", "vectors", "jacobian", "model", "sigma")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def noise_free(tmp_path_factory):
    return NoiseFree(tmp_path_factory.mktemp("noise_free_fisher"))


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    made = {}

    def get(cov):
        if cov not in made:
            made[cov] = Five(tmp_path_factory.mktemp("fisher_five_cov" if cov else "fisher_five_diag"), cov)
        return made[cov]
    return get


def box(names):
    base = [n.partition("@")[0] for n in names]
    return (np.array([PARAMS[b]["prior"]["min"] for b in base], dtype=float),
            np.array([PARAMS[b]["prior"]["max"] for b in base], dtype=float))


def against_the_mirror(res, fit, what, prior_pp=None):
    """D, fisher, A, cov and the status of the device against the NumPy statement on the device's own vectors; returns the
    statement's result and the precision's blocks."""
    from victor_amd import fisher as F
    lo, hi = box(res.names)
    R = len(res)
    blocks = F.host_blocks(fit, res.params, R)
    assert same_bytes(res.scale, F.resolve_scale(fit, {})), (what, "scale", res.scale)
    m = F.assemble(res.vectors, res.x, res.step, lo, hi, blocks, res.scale, prior_pp)
    assert np.array_equal(res.status, m.status), (what, res.status, m.status)
    assert same_bytes(res.fisher, m.fisher), (what, "fisher", np.nanmax(np.abs(res.fisher - m.fisher)))
    assert same_bytes(res.a, m.a), (what, "A", np.nanmax(np.abs(res.a - m.a)))
    # FP64 division and square root are correctly rounded at the compiler's defaults: the same bytes
    assert same_bytes(res.cov, m.cov), (what, "cov", np.nanmax(np.abs(res.cov - m.cov) / np.abs(m.cov)))
    given = (m.status == F.OK) | (m.status == F.NOT_POSDEF)
    assert same_bytes(res.jacobian[given], (m.D / (2.0 * res.step[:, None, :]))[given]), (what, "D")
    assert same_bytes(res.model, res.vectors[:, 0])
    return m, blocks


def against_the_definition_route(dev, host, m, blocks, what):
    """``fisher`` of the device against ``device=False`` at the bound of tests/fisher_bounds.py, delta the bound
    ``assert_same_theory`` grants two evaluation orders.  ``cov`` is compared through ``fisher`` only: its conditioning is the
    problem's own (printed)."""
    assert same_bytes(dev.x, host.x) and same_bytes(dev.step, host.step) and np.array_equal(dev.status, host.status), what
    assert_same_theory(dev.vectors, host.vectors, what=f"{what}: stencil vectors, device vs definition route")
    delta = same_theory_delta(host.vectors)
    margin = assert_same_fisher(dev.fisher, host.fisher, m.D, blocks, dev.step, dev.scale, delta, what=f"{what}: device vs definition route")
    print(what, "worst margin of fisher", margin, "condition of A:", np.linalg.cond(dev.a), "status", dev.status)


def same_result(a, b, what, rows=slice(None)):
    for name in OUT:
        u, v = getattr(a, name), getattr(b, name)
        if u is None and v is None:
            continue
        assert same_bytes(u[rows], v[rows]), (what, name)
    assert a.scale == b.scale


# ------------------------------------------------------------------ 1. vectors and the statistic ----------------------------
def test_fixed_covariance_stack_d4(noise_free):
    """R = 16, d = 4: rows_max = 80 against R M = 144 - two chunks, the edge inside problem 8."""
    from victor_amd import fisher as F
    nf = noise_free
    rs = nf.fit.realisations(list(range(16)))
    at = {n: nf.truth[:16, j] for j, n in enumerate(NAMES)}
    res = rs.fisher(PARAMS, at, keep_vectors=True)
    assert res.names == NAMES and res.vectors.shape == (16, 9, 60) and res.jacobian.shape == (16, 60, 4) and res.cov.shape == (16, 4, 4)
    assert same_bytes(res.step, np.tile(STEP, (16, 1)))                      # the inner 60 %: no step is shrunk
    pts = F.stencil_points(res.x, res.step, LO, HI)
    batch = {n: np.ascontiguousarray(pts.reshape(-1, 4)[:, j]) for j, n in enumerate(NAMES)}
    assert_same_theory(res.vectors.reshape(-1, 60), nf.fit.theory_vector_batch(batch), what="stencil vectors vs theory_vector_batch, R 16 d 4")
    assert np.all(res.status == res.OK), res.status
    assert np.all(np.swapaxes(res.fisher, 1, 2) == res.fisher) and np.all(np.linalg.eigvalsh(res.a) > 0)
    m, blocks = against_the_mirror(res, nf.fit, "R 16 d 4")
    assert np.all(res.sigma > 0) and np.all(res.conditional_sigma <= res.sigma * (1 + 1e-12))
    again = rs.fisher(PARAMS, at, keep_vectors=True)
    same_result(res, again, "two identical calls")
    bare = rs.fisher(PARAMS, at)
    assert bare.vectors is None and bare.jacobian is None
    for name in ("fisher", "a", "cov", "status"):
        assert same_bytes(getattr(bare, name), getattr(res, name)), name
    assert_same_theory(bare.model, res.model, what="centre vectors: theory_vector_batch vs the stencil's")
    # the realisations only supply R: the data-vector handle of the same fit gives the same bytes
    same_result(res, nf.fit.fisher(PARAMS, at, keep_vectors=True), "realisation handle vs data-vector handle")
    host = F.fisher(nf.fit, PARAMS, at, keep_vectors=True, realisations=rs, device=False)
    against_the_definition_route(res, host, m, blocks, "R 16 d 4")


def test_seventy_problems_d1(noise_free):
    """R = 70, d = 1: M = 3 < S = 4 - one chunk of 210 rows in a buffer of 280, four workgroups of the rows kernel, 70 of the
    assemble kernel."""
    from victor_amd import fisher as F
    nf = noise_free
    rs = nf.fit.realisations(list(range(16, 86)))
    fixed = {n: float(nf.common[j]) for j, n in enumerate(NAMES) if n != "sigma_v"}
    res = rs.fisher(PARAMS, {"sigma_v": nf.truth[16:, 2]}, fixed=fixed, keep_vectors=True)
    assert res.names == ["sigma_v"] and res.vectors.shape == (70, 3, 60) and res.cov.shape == (70, 1, 1)
    pts = F.stencil_points(res.x, res.step, LO[2:3], HI[2:3])
    assert same_bytes(pts[:, :, 0], np.stack([res.x[:, 0], res.x[:, 0] + 10.0, res.x[:, 0] - 10.0], axis=1))
    batch = dict(fixed, sigma_v=np.ascontiguousarray(pts.reshape(-1)))
    assert_same_theory(res.vectors.reshape(-1, 60), nf.fit.theory_vector_batch(batch), what="stencil vectors vs theory_vector_batch, R 70 d 1")
    assert np.all(res.status == res.OK) and np.all(res.fisher > 0)
    against_the_mirror(res, nf.fit, "R 70 d 1")
    assert same_bytes(res.sigma, res.conditional_sigma) or np.allclose(res.sigma, res.conditional_sigma, rtol=1e-14)
    assert np.array_equal(res.params["beta"], np.full(70, fixed["beta"]))


# ------------------------------------------------------------------ 3. blended covariance slices ----------------------------
@pytest.fixture(scope="module")
def boss():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


def test_data_vector_handle_under_a_gridded_covariance(boss):
    """R = 1 on the data-vector handle, covariance gridded in beta: the centre's beta strictly between two nodes (the slices are
    blended), exactly on a node, and outside the grid (fixed: the box of the sampled beta lies inside the grid)."""
    from victor_amd import fisher as F
    fit = boss
    grid = np.asarray(fit.beta_covmat, dtype=float)
    assert not fit.fixed_covmat and grid[0] < 0.2 and grid[-1] > 0.6
    point = {"fsigma8": 0.47, "sigma_v": 380.0, "epsilon": 1.0}
    node = float(grid[13])
    for tag, beta, sampled, want_t in (("between", 0.37, True, None), ("node", node, True, 0.0), ("outside", 0.12, False, 0.0),
                                       ("above", 0.7, False, 0.0)):
        lo_t = fit._bracket(beta)
        assert (lo_t[1] != 0.0) if want_t is None else (lo_t[1] == 0.0), (tag, lo_t)
        if sampled:
            res = fit.fisher(PARAMS, dict(point, beta=beta), keep_vectors=True)
            assert res.names == NAMES and res.vectors.shape == (1, 9, 60)
        else:
            res = fit.fisher(PARAMS, point, fixed={"beta": beta}, keep_vectors=True)
            assert res.names == ["fsigma8", "sigma_v", "epsilon"] and res.vectors.shape == (1, 7, 60)
        m, blocks = against_the_mirror(res, fit, f"gridded covariance, beta {tag}")
        print("beta", tag, beta, "bracket", lo_t, "status", res.status, "sigma", res.sigma)
        if tag in ("between", "node"):
            assert res.status[0] == res.OK
            host = F.fisher(fit, PARAMS, dict(point, beta=beta), keep_vectors=True, device=False)
            against_the_definition_route(res, host, m, blocks, f"gridded covariance, beta {tag}")
        if tag == "between":
            # the blend was used: either slice alone gives other bytes
            one = F.assemble(res.vectors, res.x, res.step, LO, HI, [F.Block(0, np.asarray(fit.icov)[lo_t[0]])], res.scale)
            assert not same_bytes(one.fisher, res.fisher)
            same_result(res, fit.fisher(PARAMS, dict(point, beta=beta), keep_vectors=True), "two identical calls, data vector")


# ------------------------------------------------------------------ 4. the five density-split blocks, d = 10 ----------------
def ten_block():
    from victor_amd.joint import per_block
    return per_block(PARAMS, ["fsigma8", "sigma_v"], 5)


def ten_points(R):
    return {n: (0.44 + 0.015 * q if n.startswith("fsigma8") else 350.0 + 12.0 * q) + 0.01 * np.arange(R) * (1 if n.startswith("fsigma8") else 100)
            for q in range(5) for n in (f"fsigma8@{q}", f"sigma_v@{q}")}


@pytest.mark.parametrize("cov", [True, False], ids=["joint_cov", "block_diagonal"])
def test_five_blocks_ten_parameters(five, cov):
    """d = 10, R = 3 joint mocks: M = 21 against S = 11 - two chunks of 33 + 30 rows, the edge inside problem 1; N = 600 in five
    segments, one theory launch per block and chunk; under the joint covariance (one padded 600 x 608 matrix) and block-diagonal
    (five 120 x 120 matrices)."""
    from victor_amd import fisher as F
    c = five(cov)
    fixed = {"beta": BETA, "epsilon": 1.0}
    target = c.joint.realisations([0, 1, 2])
    at = ten_points(3)
    res = target.fisher(ten_block(), at, fixed=fixed, keep_vectors=True)
    assert res.names == TEN and res.vectors.shape == (3, 21, 600) and res.fisher.shape == (3, 10, 10)
    assert np.all(res.status == res.OK), res.status
    m, blocks = against_the_mirror(res, c.joint, f"d 10 cov {cov}")
    assert len(blocks) == (1 if cov else 5)
    # every block's segment of a row is that block's own theory vector at its own parameters
    pts = F.stencil_points(res.x, res.step, *box(TEN)).reshape(63, 10)
    batch = dict({n: np.ascontiguousarray(pts[:, j]) for j, n in enumerate(TEN)}, **fixed)
    assert_same_theory(res.vectors.reshape(63, 600), F.host_vectors(c.joint, batch, {}), what=f"d 10 cov {cov}: segments vs theory_vector_batch")
    if not cov:
        # block-diagonal with per-block parameters: the information of fsigma8@q, sigma_v@q' vanishes for q != q' exactly
        for q in range(5):
            for p in range(5):
                if p != q:
                    assert res.fisher[0, q, 5 + p] == 0.0 and res.fisher[0, q, p] == 0.0
    host = F.fisher(c.joint, ten_block(), at, fixed=fixed, keep_vectors=True, realisations=target, device=False)
    against_the_definition_route(res, host, m, blocks, f"d 10 cov {cov}")
    same_result(res, c.joint.fisher(ten_block(), at, fixed=fixed, keep_vectors=True), "joint mocks vs the joint data-vector handle")


def test_five_blocks_under_the_ten_parameter_prior(five):
    """The 10 x 10 correlated prior of tests/test_gpu_ten_parameters.py: ``fisher`` keeps its bytes (the likelihood's
    information), A is the prior-free A plus ``Lambda_jk (h_j h_k)`` - one rounded product, one rounded sum per entry, byte for
    byte.  (Stated forwards: subtracting the term from the rounded sum does not give the prior-free bytes back in general,
    fl(fl(u + w) - w) != u.)"""
    from victor_amd import fisher as F
    from tests.test_gpu_priors import resolved
    c = five(True)
    fixed = {"beta": BETA, "epsilon": 1.0}
    at = ten_points(1)
    free = c.joint.fisher(ten_block(), at, fixed=fixed, keep_vectors=True)
    post = c.joint.fisher(ten_block(), at, fixed=fixed, keep_vectors=True, prior=full_prior())
    r = resolved(full_prior(), TEN)
    assert same_bytes(post.vectors, free.vectors) and same_bytes(post.fisher, free.fisher) and same_bytes(post.step, free.step)
    hh = free.step[:, :, None] * free.step[:, None, :]
    term = F.lambda_matrix(r.pp, 10)[None] * hh
    assert same_bytes(post.a, free.a + term) and not same_bytes(post.a, free.a)
    assert np.allclose(F.lambda_matrix(r.pp, 10), r.precision, rtol=1e-12, atol=0) and np.all(r.precision != 0)
    against_the_mirror(post, c.joint, "d 10 under the prior", r.pp)
    assert np.all(post.status == post.OK) and np.all(post.sigma <= free.sigma * (1 + 1e-12)) and np.all(post.conditional_sigma <= free.conditional_sigma)


# ------------------------------------------------------------------ 6. against the oracle ------------------------------------
def test_against_the_oracle(boss):
    """The same stencil through oracle/victor_oracle.py, one BOSS point (d = 2: 5 oracle evaluations) and one synthetic point
    (d = 3: 7): ``fisher`` of the NumPy statement on the oracle's vectors, at the bound of tests/fisher_bounds.py with delta the
    tolerance the parity tests grant a theory vector against the oracle: ``RTOL max|t|`` (tests/test_gpu_parity.py, ``vec_close``,
    lines 49-51, RTOL = 1e-9, line 21)."""
    import victor_amd
    from victor_amd import fisher as F
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle as vo
    synth = victor_amd.CCFFit(*cases.synth_options(2))
    runs = (("boss", boss, vo.OracleFit(*cases.boss_options("config")), {"fsigma8": 0.47, "sigma_v": 380.0}, {"beta": 0.37, "epsilon": 1.0}),
            ("synthetic", synth, vo.OracleFit(*cases.synth_options(2)), {"fsigma8": 0.5, "sigma_v": 330.0, "epsilon": 1.02}, {"beta": BETA}))
    for tag, fit, ofit, at, fixed in runs:
        res = fit.fisher(PARAMS, at, fixed=fixed, keep_vectors=True)
        names = list(at)
        assert res.names == names and res.status[0] == res.OK
        lo, hi = box(names)
        pts = F.stencil_points(res.x, res.step, lo, hi)[0]
        v = np.array([ofit.theory_multipole_vector(ofit.s, dict({n: float(p[i]) for i, n in enumerate(names)}, **fixed), ofit.poles_s)
                      for p in pts])
        delta = RTOL * float(np.max(np.abs(v)))
        assert np.max(np.abs(res.vectors[0] - v)) <= delta, (tag, np.max(np.abs(res.vectors[0] - v)), delta)
        blocks = F.host_blocks(fit, res.params, 1)
        want = F.assemble(v[None], res.x, res.step, lo, hi, blocks, res.scale)
        margin = assert_same_fisher(res.fisher, want.fisher, want.D, blocks, res.step, res.scale, delta, what=f"{tag}: device vs oracle")
        print(tag, "fisher vs the oracle: worst margin", margin, "sigma", res.sigma, "condition of A", np.linalg.cond(res.a))


# ------------------------------------------------------------------ 7. the faces of the box ----------------------------------
def test_faces(noise_free):
    nf = noise_free
    rs = nf.fit.realisations([0, 1, 2])
    h = STEP[2]
    at = {n: nf.truth[:3, j].copy() for j, n in enumerate(NAMES)}
    inner = rs.fisher(PARAMS, at, keep_vectors=True)
    at["sigma_v"][1] = HI[2] - h / 2
    at["sigma_v"][2] = HI[2] - h / 16
    res = rs.fisher(PARAMS, at, keep_vectors=True)
    assert res.status.tolist() == [res.OK, res.OK, res.AT_BOUND], res.status
    assert res.step[1, 2] == 0.999 * (HI[2] - at["sigma_v"][1]) and res.step[2, 2] == h and res.step[0, 2] == h
    assert np.all(np.isnan(res.cov[2])) and np.all(np.isnan(res.fisher[2])) and np.all(np.isnan(res.a[2]))
    assert all(same_bytes(res.vectors[2, m], res.vectors[2, 0]) for m in range(9)) and np.all(np.isfinite(res.vectors[2, 0]))   # every row at x
    assert not same_bytes(res.vectors[1, 1], res.vectors[1, 0])
    assert np.all(np.isfinite(res.cov[1])) and np.all(np.linalg.eigvalsh(res.a[1]) > 0)
    same_result(res, inner, "the problem beside a flagged one", rows=slice(0, 1))           # the other problems: unaffected
    wide = rs.fisher(PARAMS, at, shrink=32, keep_vectors=True)                             # down to h / 32: the third one is shrunk, too
    assert wide.status.tolist() == [res.OK] * 3 and wide.step[2, 2] == 0.999 * (HI[2] - at["sigma_v"][2])
    against_the_mirror(res, nf.fit, "faces")
    against_the_mirror(wide, nf.fit, "faces, shrink 32")


# ------------------------------------------------------------------ 8. no effect on other calls ------------------------------
def test_other_calls_are_unaffected(noise_free):
    """best_fit and laplace on the same fit object give the same bytes before and after a fisher call."""
    nf = noise_free
    rs = nf.fit.realisations([0, 1, 2])
    at = {n: nf.truth[:3, j] for j, n in enumerate(NAMES)}
    kw = dict(max_iter=40)

    def others():
        bf = rs.best_fit(PARAMS, start=at, **kw)
        lap = rs.laplace(PARAMS, at, keep_values=True)
        one = nf.fit.laplace(PARAMS, {n: float(v[0]) for n, v in at.items()}, keep_values=True)
        lnl = nf.fit.log_likelihood_batch(at)
        return bf, lap, one, lnl
    before = others()
    rs.fisher(PARAMS, at, keep_vectors=True)
    nf.fit.fisher(PARAMS, at)
    after = others()
    for name in ("x", "lnl", "chi2", "status", "n_iter", "n_evals"):
        assert same_bytes(getattr(after[0], name), getattr(before[0], name)), ("best_fit", name)
    for k in (1, 2):
        for name in ("values", "a", "hessian", "cov", "status", "lnpost", "chi2"):
            assert same_bytes(getattr(after[k], name), getattr(before[k], name)), ("laplace", k, name)
    assert same_bytes(after[3][0], before[3][0]) and same_bytes(after[3][1], before[3][1])
