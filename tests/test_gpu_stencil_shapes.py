"""The two stencil calls - ``laplace`` (vk_fit_hessian) and ``fisher`` (vk_fit_fisher) - across the evaluator's batch-size regimes,
through every status of their assemble kernels, and at the LDS ceiling of the Fisher assemble kernel (DESIGN.md section 7a,
"Launch shapes under test").  The shapes are the rows of ``STENCILS`` in tests/launch_shapes.py; tests/test_launch_shapes.py
holds every row to the thresholds of the sources without a GPU.

Both calls cut their R M stencil rows into chunks of R S rows, S = max(4, d + 1), each chunk an evaluation launch of its own, the
last one shorter - so one call crosses regimes.  What every ``laplace`` row asserts:
  (a) chunk by chunk, the device's values (and the centres' chi2) in BYTES against one host call of exactly that chunk's rows -
      ``log_likelihood_batch`` / ``log_likelihood_pairs`` of ``laplace.stencil_points``: the row count and the position of every
      row in the launch are then those of the device's own launch (the check of tests/test_gpu_launch_shapes.py on final chain
      positions; epsilon is fixed in every row for it).  On the single-fit data routes the host call's kernel instance and
      fused / unfused is asserted against what the table predicts.
  (b) ``a``, ``hessian``, ``cov``, ``status``, ``lnpost`` in bytes against the NumPy statement on the device's own values.
  (c) the device against ``device=False``, which evaluates all R M rows in ONE host call (other launch shapes): values at
      ``chi2_bound`` / ``NoiseFree.bound`` / ``blocks_bound``, ``a`` at the four-value formula of
      tests/test_gpu_hessian.py::test_ten_per_block_parameters.  No new tolerance.
  (d) the status: ``OK`` everywhere at noise-free truths (H7); on the data routes, whose centres are Halton points around the
      notebook's point and need not be maxima, the NumPy statement's status (b) and at least three quarters ``OK``.
and every ``fisher`` row: (a) the stencil vectors chunk by chunk in bytes against ``fisher.host_vectors`` (``theory_vector_batch``
per block) of the chunk's rows in one call; (b), (c) ``against_the_mirror`` and ``against_the_definition_route`` of
tests/test_gpu_fisher.py; every status ``OK``.

Centres lie in the inner 60 % of the box, so no step is shrunk at a face.
"""

import faulthandler
import os
import re

import numpy as np
import pytest

from tests import cases
from tests import launch_shapes as LS
from tests.test_chains import same_bytes
from tests.test_gpu_fisher import against_the_definition_route, against_the_mirror as fisher_mirror, same_result
from tests.test_gpu_hessian import NoiseFree, against_the_mirror as hessian_mirror, same_laplace
from tests.test_gpu_joint_blocks import blocks_bound
from tests.test_gpu_priors import BETA, Five
from tests.test_gpu_ten_parameters import TEN
from tests.test_joint_cov import boss_joint_cov_file, boss_pair_options
from tests.test_realisations import stack_options
from tests.tolerances import U, assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
T = LS.thresholds()
IDS = {}                                                     # test function -> its case ids (tests/test_launch_shapes.py reads it)
CENTRE = {"fsigma8": 0.47, "beta": 0.37, "sigma_v": 380.0}   # the notebook's point (tests/cases.NOTEBOOK_POINT)
# The centres fill this fraction of the inner 60 % of the box, around CENTRE.  The data vector's lnL is kinked in beta at the
# nodes of its covariance grid, and with the default step in beta a stencil centred outside about
# 0.345 .. 0.385 reads NOT_POSDEF: at 0.15 (beta 0.352 .. 0.388) some 4 % of the data-vector problems do, at 0.25 a quarter.  The
# ten per-block parameters of J8 are all OK at 0.05 and half NOT_POSDEF at 0.25; at 0.12 three of 24 are.
SPREAD, SPREAD_PER_BLOCK = 0.15, 0.12
NAMES3 = ["fsigma8", "beta", "sigma_v"]
EPS = {"epsilon": 1.0}


def table(name, *rows):
    """Parametrise over every variant of the given rows of ``STENCILS``: ids "<row>-<call>-<route>-R<problems>"."""
    vs = [dict(v, row=row) for row in rows for v in LS.stencil_variants(LS.STENCILS[row])]
    IDS[name] = [f"{v['row']}-{v['call']}-{v['route']}-R{v['R']}" for v in vs]
    return pytest.mark.parametrize("v", vs, ids=IDS[name])


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def box(names):
    base = [n.partition("@")[0] for n in names]
    return (np.array([PARAMS[b]["prior"]["min"] for b in base], dtype=float),
            np.array([PARAMS[b]["prior"]["max"] for b in base], dtype=float))


def steps(names):
    return np.array([PARAMS[n.partition("@")[0]]["proposal"] for n in names], dtype=float)


def inner(names):
    lo, hi = box(names)
    return lo + 0.2 * (hi - lo), lo + 0.8 * (hi - lo)


def centres(names, R):
    """(R, d) centres: the Halton set of ``cases.halton_params`` mapped into the fraction ``SPREAD`` of the inner 60 % of the
    box around ``CENTRE`` (a per-block parameter "name@q": uniform random numbers, ``SPREAD_PER_BLOCK``) - and inside that
    inner box, which is asserted."""
    lo, hi = box(names)
    hp = cases.halton_params(R, with_beta=True)
    unit = {"fsigma8": (hp["fsigma8"] - 0.05) / 1.45, "sigma_v": (hp["sigma_v"] - 100.0) / 400.0, "beta": (hp["beta"] - 0.2) / 0.4}
    more = np.random.default_rng(11).random((R, 10))
    x = np.empty((R, len(names)))
    for j, n in enumerate(names):
        base, _, q = n.partition("@")
        u, spread = (unit[base], SPREAD) if not q else (more[:, (int(q) + (5 if base == "sigma_v" else 0)) % 10], SPREAD_PER_BLOCK)
        x[:, j] = CENTRE[base] + spread * 0.6 * (hi[j] - lo[j]) * (u - 0.5)
    ilo, ihi = inner(names)
    assert np.all((x >= ilo) & (x <= ihi)), "a centre outside the inner 60 % of the box"
    return x


def full(names, pts, fixed):
    """The batch of ``pts`` (n, d): every sampled and fixed value as an (n,) array."""
    batch = {k: np.full(len(pts), float(v)) for k, v in fixed.items()}
    batch.update({n: np.ascontiguousarray(pts[:, j]) for j, n in enumerate(names)})
    return batch


def launch_is(fit, n, what):
    """The last evaluation of the single fit's engine against what the row count predicts (tests/launch_shapes.py)."""
    from tests.test_gpu_predictive import engine_of
    eng = engine_of(fit)
    instance, is_fused = eng.last_instance(), eng.last_fused()
    assert instance.startswith("cells") == (LS.cells_range(n, T) != 0), (what, n, instance)
    assert is_fused == LS.fused(n, T) and instance.endswith("+fused") == LS.fused(n, T), (what, n, instance)
    return instance


# ------------------------------------------------------------------ the fits ---------------------------------------------------------
@pytest.fixture(scope="module")
def data_fit():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


class Truths(NoiseFree):
    """A noise-free stack of 513 truths, built as tests/test_gpu_hessian.py builds its 86: random points of the inner 60 % of
    the box, epsilon at 1 (fixed in every row of the table)."""

    def __init__(self, tmp, n=513):
        lo, hi = box(NAMES3 + ["epsilon"])
        truth = lo + (hi - lo) * (0.2 + 0.6 * np.random.default_rng(7).random((n, 4)))
        truth[:, 3] = 1.0
        super().__init__(tmp, truth)


@pytest.fixture(scope="module")
def truths(tmp_path_factory):
    return Truths(tmp_path_factory.mktemp("noise_free_513"))


@pytest.fixture(scope="module")
def noise_free(tmp_path_factory):
    return NoiseFree(tmp_path_factory.mktemp("noise_free_status"))


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    made = {}

    def get(cov):
        if cov not in made:
            made[cov] = Five(tmp_path_factory.mktemp("stencil_five_cov" if cov else "stencil_five_diag"), cov)
        return made[cov]
    return get


@pytest.fixture(scope="module")
def boss_grid(tmp_path_factory):
    import victor_amd
    from victor_amd.joint import JointFit
    tmp = tmp_path_factory.mktemp("stencil_boss_grid")
    return JointFit([victor_amd.CCFFit(*o) for o in boss_pair_options()], covariance=boss_joint_cov_file(str(tmp / "joint_cov.npy")))


# ------------------------------------------------------------------ what every row does ----------------------------------------------
def laplace_row(v, target, fit, block, names, fixed, x, bound_of, what, realisations=None, single=None, all_ok=False):
    """(a) - (d) of the module docstring.  ``target``: what ``laplace`` is called on; ``fit``: the fit of the definition route;
    ``bound_of(batch, which)``: the chi2 bound of rows; ``single``: the single fit whose engine's launches are asserted."""
    from victor_amd import laplace as L
    R, d, M = v["R"], v["d"], LS.points("laplace", v["d"])
    assert len(names) == d and x.shape == (R, d)
    lo, hi = box(names)
    at = {n: x[:, j] for j, n in enumerate(names)}
    dev = target.laplace(block, at, fixed=fixed, keep_values=True)
    if single is not None:
        print(what, "the device route's last chunk:", launch_is(single, LS.chunks(v)[-1], what + ", device route"))
    assert dev.names == names and dev.values.shape == (R, M) and dev.a.shape == (R, d, d)
    assert same_bytes(dev.step, np.tile(steps(names), (R, 1)))                # the inner 60 %: no step is shrunk
    pts = L.stencil_points(dev.x, dev.step, lo, hi).reshape(R * M, d)
    which = np.repeat(np.arange(R, dtype=np.int32), M)
    # (a) chunk by chunk, in bytes
    values, g0 = dev.values.ravel(), 0
    for n in LS.chunks(v):
        rows = slice(g0, g0 + n)
        batch = full(names, pts[rows], fixed)
        lnl, chi2 = realisations.log_likelihood_pairs(batch, which[rows]) if realisations is not None else fit.log_likelihood_batch(batch)
        if single is not None:
            print(what, "chunk at", g0, "of", n, "rows:", launch_is(single, n, what))
        diff = lnl != values[rows]
        assert same_bytes(lnl, values[rows]), (what, "values of the chunk at", g0, int(diff.sum()), float(np.nanmax(np.abs(lnl - values[rows]))))
        centre = np.flatnonzero(np.arange(g0, g0 + n) % M == 0)
        assert same_bytes(chi2[centre], dev.chi2[(g0 + centre) // M]), (what, "centre chi2 of the chunk at", g0)
        g0 += n
    assert g0 == R * M
    # (b) the statistic against the NumPy statement on the device's own values
    m = hessian_mirror(dev, lo, hi, what)
    # (c) against the definition route: one host call of all R M rows
    host = L.laplace(fit, block, at, fixed=fixed, keep_values=True, realisations=realisations, device=False)
    bound = np.asarray(bound_of(full(names, pts, fixed), which)).reshape(R, M)
    assert_same_lnl(dev.values.ravel(), host.values.ravel(), bound.ravel(), what=f"{what}: stencil values, device vs definition route")
    assert_same_chi2(dev.chi2, host.chi2, bound[:, 0], what=f"{what}: centre chi2, device vs definition route")
    per_value = 0.51 * bound + 16 * U * (np.abs(host.values) + 1000.0)          # an entry of A combines four values
    tol = 4 * per_value.max(axis=1)[:, None, None]
    given = (dev.status != dev.AT_BOUND) & (dev.status != dev.NOT_FINITE)
    assert np.array_equal(given, (host.status != host.AT_BOUND) & (host.status != host.NOT_FINITE)) and np.all(given), (what, dev.status)
    print(what, "max |dA|", float(np.max(np.abs(dev.a - host.a))), "smallest tolerance", float(tol.min()))
    assert np.all(np.abs(dev.a - host.a) <= tol), what
    # (d) the status
    n_ok = int(np.sum(dev.status == dev.OK))
    print(what, "status: OK", n_ok, "of", R, "; NOT_POSDEF", int(np.sum(dev.status == dev.NOT_POSDEF)))
    if all_ok:
        assert n_ok == R, (what, dev.status)
    else:
        assert np.array_equal(dev.status, m.status) and 4 * n_ok >= 3 * R, (what, n_ok, R)
    return dev


def fisher_row(v, target, fit, block, names, fixed, x, what, realisations=None):
    from victor_amd import fisher as F
    R, d, M = v["R"], v["d"], LS.points("fisher", v["d"])
    lo, hi = box(names)
    at = {n: x[:, j] for j, n in enumerate(names)}
    dev = target.fisher(block, at, fixed=fixed, keep_vectors=True)
    N = dev.vectors.shape[2]
    assert dev.names == names and dev.vectors.shape == (R, M, N) and dev.fisher.shape == (R, d, d)
    assert same_bytes(dev.step, np.tile(steps(names), (R, 1)))
    pts = F.stencil_points(dev.x, dev.step, lo, hi).reshape(R * M, d)
    # (a) chunk by chunk, in bytes: each block's segment is that block's own theory_vector_batch of the chunk's rows
    vectors, g0 = dev.vectors.reshape(R * M, N), 0
    for n in LS.chunks(v):
        rows = slice(g0, g0 + n)
        got = F.host_vectors(fit, full(names, pts[rows], fixed), {})
        assert same_bytes(got, vectors[rows]), (what, "vectors of the chunk at", g0, int(np.sum(got != vectors[rows])),
                                                float(np.nanmax(np.abs(got - vectors[rows]))))
        g0 += n
    assert g0 == R * M
    # (b), (c)
    m, blocks = fisher_mirror(dev, fit, what)
    host = F.fisher(fit, block, at, fixed=fixed, keep_vectors=True, realisations=realisations, device=False)
    against_the_definition_route(dev, host, m, blocks, what)
    assert np.all(dev.status == dev.OK), (what, dev.status)
    return dev


# ------------------------------------------------------------------ 1. laplace: H rows ------------------------------------------------
@table("test_laplace_on_the_data_vector", "H1", "H2", "H3", "H4", "H5", "H6")
def test_laplace_on_the_data_vector(data_fit, v):
    what = f"{v['row']} R = {v['R']} d = {v['d']}"
    names = NAMES3 if v["d"] == 3 else ["sigma_v"]
    fixed = dict(EPS) if v["d"] == 3 else dict(EPS, fsigma8=CENTRE["fsigma8"], beta=CENTRE["beta"])
    x = centres(names, v["R"])
    laplace_row(v, data_fit, data_fit, PARAMS, names, fixed, x, lambda batch, which: chi2_bound(data_fit, batch), what, single=data_fit)


@table("test_laplace_on_noise_free_mocks", "H7")
def test_laplace_on_noise_free_mocks(truths, v):
    nf = truths
    rs = nf.fit.realisations(list(range(v["R"])))
    lap = laplace_row(v, rs, nf.fit, PARAMS, NAMES3, dict(EPS), nf.truth[:v["R"], :3], nf.bound, f"{v['row']} R = {v['R']}", realisations=rs, all_ok=True)
    assert np.all(np.linalg.eigvalsh(lap.a) > 0)


# ------------------------------------------------------------------ 2. fisher: F rows -------------------------------------------------
@table("test_fisher_on_the_data_vector", "F1", "F2", "F3", "F4")
def test_fisher_on_the_data_vector(data_fit, v):
    fisher_row(v, data_fit, data_fit, PARAMS, NAMES3, dict(EPS), centres(NAMES3, v["R"]), f"{v['row']} R = {v['R']}")


# ------------------------------------------------------------------ 3. joint fits: J rows ---------------------------------------------
def joint_case(v, five, boss_grid):
    """(joint fit, params block, sampled names, fixed) of a J row."""
    from victor_amd.joint import per_block
    if v["route"] == "boss_grid":
        return boss_grid, PARAMS, NAMES3, dict(EPS)
    joint = five(v["route"] == "five_cov").joint
    if v["d"] == 10:
        return joint, per_block(PARAMS, ["fsigma8", "sigma_v"], 5), TEN, {"beta": BETA, "epsilon": 1.0}
    return joint, PARAMS, ["fsigma8", "sigma_v"], {"beta": BETA, "epsilon": 1.0}


@table("test_joint_fits", "J6", "J7", "J8")
def test_joint_fits(five, boss_grid, v):
    what = f"{v['row']} {v['call']} {v['route']} R = {v['R']} d = {v['d']}"
    joint, block, names, fixed = joint_case(v, five, boss_grid)
    x = centres(names, v["R"])
    if v["call"] == "fisher":
        res = fisher_row(v, joint, joint, block, names, fixed, x, what)
        assert res.vectors.shape[2] == joint.n_data
    else:
        laplace_row(v, joint, joint, block, names, fixed, x, lambda batch, which: blocks_bound(joint, batch), what)


# ------------------------------------------------------------------ 4. the status branches on the device ------------------------------
def failing_pivot(a):
    """(c, value): the first Cholesky pivot of A that fails ``> 0`` and its value in the NumPy statement's order of operations
    (victor_amd.laplace.assemble); (-1, nan) for a positive definite A."""
    S = np.array(a, dtype=float)
    d = len(S)
    for c in range(d):
        if not S[c, c] > 0.0:
            return c, float(S[c, c])
        lcc = np.sqrt(S[c, c])
        col = S[:, c] / lcc
        for j in range(c + 1, d):
            for k in range(c + 1, j + 1):
                S[j, k] = S[j, k] - col[j] * col[k]
    return -1, float("nan")


def test_hessian_not_finite_beside_ok(tmp_path):
    """The covariance of tests/test_gpu_realisations.py::test_guard_positions_match_the_single_path - a last slice whose blends
    have a determinant of sign -1 over part of the last beta interval, where lnL is -inf - on the data-vector handle with beta
    sampled up to the grid's last node: eight problems, every other one with a stencil that reaches that part."""
    import victor_amd
    from victor_amd import laplace as L
    cov = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    stack = np.array(cov["covmat"], dtype=float)
    w, vec = np.linalg.eigh(stack[-1])
    flipped = stack[-1] - 1.25 * w[5] * np.outer(vec[:, 5], vec[:, 5]) - 5.0 * w[40] * np.outer(vec[:, 40], vec[:, 40])
    stack[-1] = 0.5 * (flipped + flipped.T)
    path = str(tmp_path / "cov_two_negative.npy")
    np.save(path, {"beta": cov["beta"], "covmat": stack}, allow_pickle=True)
    model, data = cases.boss_options("config")
    data["covariance_matrix"]["data_file"] = path
    fit = victor_amd.CCFFit(model, data)
    g = np.asarray(cov["beta"], dtype=float)
    # where lnL fails, by the host entry point: one stretch of the last interval
    scan = g[-2] + (g[-1] - g[-2]) * np.linspace(0.0, 1.0, 201)
    lnl, _ = fit.log_likelihood_batch(dict(fsigma8=np.full(201, 0.47), sigma_v=np.full(201, 380.0), epsilon=np.full(201, 1.0), beta=scan))
    bad = np.flatnonzero(np.isneginf(lnl))
    assert len(bad) > 20 and np.array_equal(bad, np.arange(bad[0], bad[-1] + 1)) and bad[0] > 5 and bad[-1] < 195, bad
    b_lo, b_hi = scan[bad[0]], scan[bad[-1]]
    h = 0.004
    assert b_hi - b_lo > 2 * h
    block = dict(PARAMS, beta=dict(PARAMS["beta"], prior={"dist": "uniform", "min": 0.2, "max": float(g[-1])}))
    mid = 0.5 * (b_lo + b_hi)
    flagged = np.array([mid, b_lo - 0.5 * h, mid + 0.25 * h, b_lo - 0.25 * h])           # the centre itself, or only beta + h
    # clear of it: every value of the stencil is finite (the blends with the last slice fail in other intervals, too)
    # on the definition route
    cand = np.concatenate([np.linspace(0.41, 0.59, 19), flagged])
    step = {"beta": h}
    host = L.laplace(fit, block, {"fsigma8": 0.47, "beta": cand, "sigma_v": 380.0}, fixed=EPS, step=step, device=False)
    assert np.all(host.status[19:] == host.NOT_FINITE), host.status
    clear = cand[:19][host.status[:19] != host.NOT_FINITE][:4]
    assert len(clear) == 4, ("fewer than four centres whose stencil is finite", host.status)
    beta = np.stack([clear, flagged], axis=1).ravel()                                     # clear, flagged, clear, flagged, ...
    at = {"fsigma8": np.full(8, 0.47), "beta": beta, "sigma_v": np.full(8, 380.0)}
    lap = fit.laplace(block, at, fixed=EPS, step=step, keep_values=True)
    lo, hi = box(NAMES3)
    hi[1] = g[-1]
    assert same_bytes(lap.step[:, 1], np.full(8, h))                                      # no step is shrunk: no face is near
    m = hessian_mirror(lap, lo, hi, "NOT_FINITE beside OK")
    want = np.tile([lap.OK, lap.NOT_FINITE], 4)
    print("statuses", lap.status, "values not finite per problem", np.sum(~np.isfinite(lap.values), axis=1))
    assert np.array_equal(m.status == lap.NOT_FINITE, want == lap.NOT_FINITE) and np.array_equal(lap.status == lap.NOT_FINITE, want == lap.NOT_FINITE)
    assert np.all(np.isin(lap.status[0::2], (lap.OK, lap.NOT_POSDEF)))           # (a data-vector centre need not be a maximum)
    assert np.any(lap.status == lap.OK) and np.any(lap.status == lap.NOT_FINITE)
    assert np.isneginf(lap.values[1, 0]) and np.isfinite(lap.values[3, 0]) and np.isneginf(lap.values[3, L.at_axis(1, 0)])
    for p in range(8):
        nan = [bool(np.all(np.isnan(getattr(lap, k)[p]))) for k in ("a", "hessian", "cov")]
        if want[p] == lap.NOT_FINITE:
            assert all(nan), (p, nan)
        else:
            assert np.all(np.isfinite(lap.a[p])) and np.all(np.isfinite(lap.hessian[p])), p
    # the problems beside the flagged ones keep their bytes in a call whose other problems are clear
    moved = fit.laplace(block, dict(at, beta=np.stack([clear, clear], axis=1).ravel()), fixed=EPS, step=step, keep_values=True)
    assert not np.any(moved.status == lap.NOT_FINITE)
    same_laplace(lap, moved, "the problems beside the flagged ones", rows=slice(0, 8, 2))


@pytest.mark.parametrize("d", [1, 4])
def test_hessian_not_posdef_beside_ok(noise_free, d):
    """Noise-free mocks centred away from their truths, where lnL is not concave: the centres are picked on the definition
    route - ``NOT_POSDEF`` in the NumPy statement by a pivot a thousand times further below zero than the bound on an entry of A
    between two evaluation orders - and run on the device beside problems at their truths.  d = 4: the break at a pivot other
    than the first for at least one problem."""
    from victor_amd import laplace as L
    nf = noise_free
    names = ["sigma_v"] if d == 1 else NAMES3 + ["epsilon"]
    cols = [2] if d == 1 else [0, 1, 2, 3]
    numbers = np.arange(16, 86) if d == 1 else np.arange(16)
    fixed = {n: float(nf.common[j]) for j, n in enumerate(NAMES3 + ["epsilon"]) if n not in names}
    lo, hi = box(names)
    ilo, ihi = inner(names)
    # candidates: every mock at the truths of other mocks (all in the inner 60 %) and at mixtures of them with its own
    pool_numbers, pool_x = [], []
    for shift in (1, 3, 5, 7, 9, 11):
        other = nf.truth[numbers][:, cols][(np.arange(len(numbers)) + shift) % len(numbers)]
        for wgt in (1.0, 0.6):
            pool_numbers.append(numbers)
            pool_x.append((1.0 - wgt) * nf.truth[numbers][:, cols] + wgt * other)
    pool_numbers, pool_x = np.concatenate(pool_numbers), np.clip(np.concatenate(pool_x), ilo, ihi)
    rs_pool = nf.fit.realisations(pool_numbers)
    host = L.laplace(nf.fit, PARAMS, {n: pool_x[:, j] for j, n in enumerate(names)}, fixed=fixed, keep_values=True, realisations=rs_pool, device=False)
    M = L.n_points(d)
    pts = L.stencil_points(host.x, host.step, lo, hi).reshape(-1, d)
    bound = nf.bound(full(names, pts, fixed), np.repeat(pool_numbers, M)).reshape(-1, M)
    entry = 4 * (0.51 * bound + 16 * U * (np.abs(host.values) + 1000.0)).max(axis=1)      # the bound on an entry of A
    pivots = [failing_pivot(a) if s == host.NOT_POSDEF else (-1, np.nan) for a, s in zip(host.a, host.status)]
    clear = [i for i, (c, value) in enumerate(pivots) if c >= 0 and value < -1000.0 * entry[i]]
    first = [i for i in clear if pivots[i][0] == 0][:4]
    later = [i for i in clear if pivots[i][0] > 0][:4]
    print("d", d, "candidates", len(pool_x), "NOT_POSDEF", int(np.sum(host.status == host.NOT_POSDEF)), "clearly:", len(clear),
          "; picked at the first pivot", first, "at a later pivot", [(i, pivots[i][0]) for i in later])
    assert first or later, "no candidate is clearly not positive definite: the test does not reach the branch"
    if d == 4:
        assert later, "no candidate breaks at a pivot other than the first"
    picked = first + later
    # the device: the picked problems between problems at their truths
    n_ok = len(picked) + 1
    own = numbers[:n_ok]
    run_numbers = np.empty(len(picked) + n_ok, dtype=int)
    run_x = np.empty((len(run_numbers), d))
    run_numbers[0::2], run_x[0::2] = own, nf.truth[own][:, cols]
    run_numbers[1::2], run_x[1::2] = pool_numbers[picked], pool_x[picked]
    rs = nf.fit.realisations(run_numbers)
    lap = rs.laplace(PARAMS, {n: run_x[:, j] for j, n in enumerate(names)}, fixed=fixed, keep_values=True)
    m = hessian_mirror(lap, lo, hi, f"NOT_POSDEF beside OK, d {d}")                       # a, hessian, cov, status: the statement's bytes
    want = np.tile([lap.OK, lap.NOT_POSDEF], n_ok)[:len(run_numbers)]
    assert np.array_equal(lap.status, want), (lap.status, want)
    for p in np.flatnonzero(want == lap.NOT_POSDEF):
        c, value = failing_pivot(lap.a[p])
        print("d", d, "problem", p, "breaks at pivot", c, "of value", value, "(definition route:", pivots[picked[p // 2]], ")")
        assert c == pivots[picked[p // 2]][0] and np.all(np.isfinite(lap.a[p])) and np.all(np.isfinite(lap.hessian[p])) and np.all(np.isnan(lap.cov[p]))
    assert np.all(np.isfinite(lap.cov[want == lap.OK]))
    # the OK problems keep the bytes of a call in which every problem is at its truth
    run_x[1::2] = nf.truth[run_numbers[1::2]][:, cols]
    calm = rs.laplace(PARAMS, {n: run_x[:, j] for j, n in enumerate(names)}, fixed=fixed, keep_values=True)
    assert np.all(calm.status == calm.OK)
    same_laplace(lap, calm, "the problems beside the flagged ones", rows=slice(0, len(run_numbers), 2))


@pytest.mark.parametrize("order", ["last", "first"])
def test_fisher_not_posdef_for_a_parameter_the_model_ignores(data_fit, order):
    """The Kaiser model does not read sigma_v (oracle/victor_oracle.py, the ``rsd in ("kaiser", ...)`` branch): sampled, its two
    stencil vectors are equal in bytes, its column of D is exactly zero and the Cholesky loop breaks - at the last pivot with
    sigma_v last among the sampled names, at the first with sigma_v first.  A Gaussian prior on sigma_v makes the same call OK."""
    from victor_amd import GaussianPrior
    kw = {"rsd_model": "kaiser"}
    names = NAMES3 if order == "last" else ["sigma_v", "fsigma8", "beta"]
    block = {n: PARAMS[n] for n in names + ["epsilon"]}
    j = names.index("sigma_v")
    R = 3
    at = {"fsigma8": 0.47 + 0.02 * np.arange(R), "beta": 0.37 + 0.015 * np.arange(R), "sigma_v": 380.0 - 20.0 * np.arange(R)}
    res = data_fit.fisher(block, at, fixed=EPS, keep_vectors=True, **kw)
    assert res.names == names and res.vectors.shape == (R, 7, 60)
    plus, minus = res.vectors[:, 1 + 2 * j], res.vectors[:, 2 + 2 * j]
    assert same_bytes(plus, minus) and same_bytes(plus, res.vectors[:, 0]) and np.all(res.jacobian[:, :, j] == 0.0)
    assert not same_bytes(res.vectors[:, 1 + 2 * ((j + 1) % 3)], res.vectors[:, 0])
    m, _ = fisher_mirror(res, data_fit, f"kaiser, sigma_v {order}")                        # fisher, a, cov, status: the statement's bytes
    assert np.all(res.status == res.NOT_POSDEF), res.status
    pivots = [failing_pivot(a) for a in res.a]
    print("kaiser, sigma_v", order, "breaks at", pivots)
    assert all(c == j and value == 0.0 for c, value in pivots)
    assert np.all(np.isfinite(res.fisher)) and np.all(np.isfinite(res.a)) and np.all(np.isnan(res.cov))
    assert np.all(res.fisher[:, j, :] == 0.0) and np.all(res.fisher[:, :, j] == 0.0)
    prior = GaussianPrior(["sigma_v"], [375.0], cov=[[400.0]])
    post = data_fit.fisher(block, at, fixed=EPS, keep_vectors=True, prior=prior, **kw)
    from tests.test_gpu_priors import resolved
    fisher_mirror(post, data_fit, f"kaiser under a prior, sigma_v {order}", resolved(prior, names).pp)
    assert np.all(post.status == post.OK) and np.all(np.isfinite(post.cov)) and same_bytes(post.fisher, res.fisher) and same_bytes(post.vectors, res.vectors)


def test_fisher_not_finite_beside_ok(data_fit):
    """A per-problem ``fixed`` array whose fsigma8 is NaN for every other problem: their vectors are not finite."""
    names = ["beta", "sigma_v"]
    R = 6
    fs8 = np.where(np.arange(R) % 2 == 1, np.nan, 0.47 + 0.01 * np.arange(R))
    at = {"beta": 0.37 + 0.01 * np.arange(R), "sigma_v": 380.0 - 10.0 * np.arange(R)}
    res = data_fit.fisher(PARAMS, at, fixed=dict(EPS, fsigma8=fs8), keep_vectors=True)
    assert res.names == names and res.vectors.shape == (R, 5, 60)
    fisher_mirror(res, data_fit, "NOT_FINITE beside OK")
    want = np.where(np.isnan(fs8), res.NOT_FINITE, res.OK)
    assert np.array_equal(res.status, want), res.status
    flagged = want == res.NOT_FINITE
    assert np.all(np.any(~np.isfinite(res.vectors[flagged]), axis=(1, 2))) and np.all(np.isfinite(res.vectors[~flagged]))
    for k in ("fisher", "a", "cov"):
        assert np.all(np.isnan(getattr(res, k)[flagged])) and np.all(np.isfinite(getattr(res, k)[~flagged])), k
    calm = data_fit.fisher(PARAMS, at, fixed=dict(EPS, fsigma8=0.47 + 0.01 * np.arange(R)), keep_vectors=True)
    assert np.all(calm.status == calm.OK)
    same_result(res, calm, "the problems beside the flagged ones", rows=slice(0, R, 2))


# ------------------------------------------------------------------ 5. the LDS ceiling of the Fisher assemble kernel ------------------
@pytest.fixture(scope="module")
def boss_blocks():
    """Block-diagonal joint fits of n fixed-covariance BOSS fits from the same options."""
    import victor_amd
    from victor_amd.joint import JointFit
    fits = [victor_amd.CCFFit(*stack_options(fixed=True)) for _ in range(max(c["blocks"] for c in LS.CEILING.values()))]
    return lambda n: JointFit(fits[:n])


def ceiling_case(case):
    """(params block, sampled names, fixed, centres) of a ceiling case: fsigma8 and beta shared, a sigma_v per block for the
    first d - 2 blocks, the other blocks' fixed."""
    from victor_amd.joint import per_block
    nb, d, R = case["blocks"], case["d"], case["R"]
    names = ["fsigma8", "beta"] + [f"sigma_v@{q}" for q in range(d - 2)]
    fixed = dict(EPS, **{f"sigma_v@{q}": 380.0 for q in range(d - 2, nb)})
    return per_block(PARAMS, ["sigma_v"], nb), names, fixed, centres(names, R)


def test_fisher_at_the_lds_ceiling(boss_blocks):
    c = LS.CEILING["accepted"]
    joint = boss_blocks(c["blocks"])
    block, names, fixed, x = ceiling_case(c)
    N = c["blocks"] * LS.BOSS_N
    assert joint.n_data == N and LS.fisher_lds_doubles(N, c["d"], T) <= T["kFisherLdsDoubles"]
    print("dynamic LDS of the assemble kernel:", 8 * LS.fisher_lds_doubles(N, c["d"], T), "bytes in", c["blocks"], "segments")
    v = dict(call="fisher", d=c["d"], R=c["R"])
    res = fisher_row(v, joint, joint, block, names, fixed, x, f"LDS ceiling, {c['blocks']} blocks d = {c['d']}")
    assert res.vectors.shape == (c["R"], 21, N)
    # block-diagonal: sigma_v@q meets block q alone, so the information between two blocks' own parameters vanishes exactly
    assert np.all(res.fisher[:, 2, 3:] == 0.0) and np.all(res.fisher[:, 2, 2] > 0.0)


def test_fisher_past_the_lds_ceiling_is_refused(boss_blocks):
    from victor_amd.utils import InputError
    c = LS.CEILING["refused"]
    joint = boss_blocks(c["blocks"])
    block, names, fixed, x = ceiling_case(c)
    N = c["blocks"] * LS.BOSS_N
    assert LS.fisher_lds_doubles(N, c["d"], T) > T["kFisherLdsDoubles"]
    with pytest.raises(InputError) as err:
        joint.fisher(block, {n: x[:, j] for j, n in enumerate(names)}, fixed=fixed)
    text = str(err.value)
    limit = (T["kFisherLdsDoubles"] - 3 * T["kMaxP"] ** 2) // 2
    want = f"vk_fit_fisher: a theory vector of {N} entries with {c['d']} parameters needs more than 160 KiB of LDS (entries x parameters <= {limit})"
    assert re.search(re.escape(want), text), text
    assert N * c["d"] > limit >= LS.CEILING["accepted"]["blocks"] * LS.BOSS_N * LS.CEILING["accepted"]["d"]
    # the same seventeen blocks with one parameter fewer run
    b = LS.CEILING["below"]
    block, names, fixed, x = ceiling_case(b)
    res = joint.fisher(block, {n: x[:, j] for j, n in enumerate(names)}, fixed=fixed, keep_vectors=True)
    assert res.vectors.shape == (b["R"], 19, N) and np.all(res.status == res.OK)
    fisher_mirror(res, joint, f"{b['blocks']} blocks d = {b['d']}")
