"""Posterior-predictive sums of an importance sample on the GPU (``predictive=True``: vk_is_set_predictive, vk_is_predict_kernel)
against the NumPy route that defines them (``device=False, predictive=True``: rule 6 of victor_amd/importance.py over the
object's own likelihood call and ``theory_vector_batch``).  Counts, maxima, pivots and statuses are compared as bytes; the sums
are held to the two-route bound derived in tests/test_importance_predictive.py plus the per-point theory tolerance of
tests/tolerances.py (``assert_same_theory``: two evaluation orders of a theory vector differ by dT = 512 u tau 4 max(1, |T|)
per entry), which moves a term ``w v`` by ``w dT`` and a term ``(w v) v`` by ``2 w |v| dT + w dT^2``.  The scale A of the bound -
the sum of the absolute terms - and those allowances come from one evaluation of the whole sample under the run's final maxima.

Shapes: the synthetic fit (N = 80) with 3 mocks, 200 draws in chunks of 64 (four chunks, the last partial), the data vector
(R = 1: lanes cover entry groups), R = 70 from repeated mocks (past one wave of problems; repeated mocks give identical
columns), epsilon sampled and fixed, a Gaussian prior, a mock without a finite point; the beta-dependent BOSS fit; joint fits
under one covariance, block-diagonal with a sigma_v per block, and the joint data vector of two blocks of DIFFERENT N through
the module function.  With ``predictive=None`` everything ``vk_is_result`` returned before is the same bytes."""

import faulthandler
import os

import numpy as np
import pytest

from tests import cases, tolerances
from tests.test_chains import same_bytes
from tests.test_gpu_importance import CENTRE, WIDTH
from tests.test_gpu_joint_importance import OWN, own_blocks
from tests.test_gpu_joint_sampled import BETA, Case
from tests.test_importance import EXACT, SUMS
from tests.test_importance_predictive import PRED, predictive_bound
from tests.test_joint_realisations import write_stacks
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
SYNTH = {"fsigma8": {"prior": {"min": 0.3, "max": 0.6}, "ref": {"loc": 0.45, "scale": 0.02}, "proposal": 0.02},
         "sigma_v": {"prior": {"min": 300.0, "max": 420.0}, "ref": {"loc": 360.0, "scale": 10.0}, "proposal": 10.0},
         "epsilon": {"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0, "scale": 0.02}, "proposal": 0.02}}


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def run(obj, params, proposal=None, **kw):
    """The public route of ``obj``: the method of a fit, its realisations or a joint fit's realisations, or for a JointFit (R =
    1) the module function."""
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import JointFit
    if isinstance(obj, JointFit):
        return importance_posterior(obj, params, proposal, **kw)
    return obj.importance_posterior(params, proposal, **kw)


def proposal(names, shrink=4.0):
    """A correlated Gaussian well inside the box (the widths of tests/test_gpu_importance.py over ``shrink``): nearly every draw
    is kept, so the draws fix the chunks."""
    from victor_amd import GaussianProposal
    base = [n.partition("@")[0] for n in names]
    cov = np.diag([(WIDTH[b] / shrink) ** 2 for b in base])
    for j in range(1, len(names)):
        cov[0, j] = cov[j, 0] = 0.4 * WIDTH[base[0]] * WIDTH[base[j]] / shrink ** 2
    return GaussianProposal(names, [CENTRE[b] for b in base], cov)


def whole_sample(obj, ip, fixed):
    """``(lnl, chi2 (G, R), theory (G, N))`` of the kept points from one call each."""
    from victor_amd.fisher import host_vectors
    from victor_amd.joint import JointFit
    batch = {k: np.full(ip.n_inside, float(v)) for k, v in (fixed or {}).items()}
    batch.update({n: np.ascontiguousarray(ip._sample.x[:, j]) for j, n in enumerate(ip.names)})
    if hasattr(obj, "log_likelihood_pairs"):
        lnl, chi2 = obj.log_likelihood(batch)
        fit = obj.joint if hasattr(obj, "joint") else obj.fit
    else:
        lnl, chi2 = obj.log_likelihood_batch(batch)
        fit = obj
    assert isinstance(fit, JointFit) or hasattr(fit, "theory_vector_batch")
    return lnl.reshape(ip.n_inside, -1), chi2.reshape(ip.n_inside, -1), host_vectors(fit, batch, {})


def scales(ip, lnl, chi2, theory):
    """Per accumulator of rule 6 ``(A, the theory allowance)``: the sums of the absolute terms under the run's final maxima, and
    what a theory vector that differs by dT per entry moves them by (module docstring)."""
    acc = ip.raw
    with np.errstate(invalid="ignore"):
        lnpost = lnl + ip._sample.lno[:, None]
        lnpost = np.where(np.isfinite(lnpost), lnpost, -np.inf)
        w = np.where(acc.n_finite[None, :] > 0, np.exp(lnpost - np.where(acc.n_finite > 0, acc.ln_max, 0.0)[None, :]), 0.0)
        v = np.where(np.isfinite(theory), theory - acc.pivot_t[None, :], 0.0)
        a = np.where(w > 0, chi2 - acc.pivots[0][None, :], 0.0)
        b = np.where(w > 0, lnl - acc.pivots[1][None, :], 0.0)
    dT = 512 * tolerances.U * 2.0 * 4.0 * max(1.0, float(np.max(np.abs(np.where(np.isfinite(theory), theory, 0.0)))))
    A = {"pt": w.T @ np.abs(v), "ptt": w.T @ (v * v), "dev": np.stack([(w * np.abs(a)).sum(0), (w * a * a).sum(0), (w * np.abs(b)).sum(0), (w * b * b).sum(0)])}
    total = w.sum(axis=0)
    extra = {"pt": dT * total[:, None] * np.ones_like(A["pt"]), "ptt": 2.0 * dT * A["pt"] + dT * dT * total[:, None], "dev": np.zeros_like(A["dev"])}
    return A, extra


def both_routes(obj, params, what, fixed=None, **kw):
    """The device route and the definition route of one call with ``predictive=True``, compared; the device route once more
    without it.  Returns ``(dev, ref)``."""
    dev = run(obj, params, predictive=True, fixed=fixed, **kw)
    ref = run(obj, params, predictive=True, device=False, fixed=fixed, **kw)
    off = run(obj, params, fixed=fixed, **kw)
    assert off.predictive is None and not hasattr(off.raw, "pt")
    for name in EXACT + SUMS:                                    # predictive on or off: what vk_is_result returned before
        assert same_bytes(getattr(dev.raw, name), getattr(off.raw, name)), (what, name)
    assert dev.n_problems == ref.n_problems and dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks and dev.n_inside == ref.n_inside
    for name in EXACT:
        assert same_bytes(getattr(dev.raw, name), getattr(ref.raw, name)), (what, name)
    assert same_bytes(dev.status, ref.status), what
    assert same_bytes(dev.raw.pivot_t, ref.raw.pivot_t) and same_bytes(dev.raw.pivots, ref.raw.pivots), what
    assert np.all(np.isfinite(dev.raw.pivot_t)) and np.any(dev.raw.pivot_t != 0)
    A, extra = scales(ref, *whole_sample(obj, ref, fixed))
    worst = 0.0
    for name in PRED:
        got, want = getattr(dev.raw, name), getattr(ref.raw, name)
        assert got.shape == want.shape == A[name].shape and np.all(np.isfinite(got)) and np.all(np.isfinite(want)), (what, name)
        second = np.zeros(got.shape, dtype=bool)
        if name == "ptt":
            second[...] = True
        if name == "dev":
            second[1::2] = True
        rel = np.where(second, predictive_bound(True, dev.n_chunks, dev.n_inside, True), predictive_bound(False, dev.n_chunks, dev.n_inside, True))
        bound = rel * A[name] * (1.0 + 64 * tolerances.U) + extra[name]
        diff = np.abs(got - want)
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
        print(f"{what}: {name} worst |device - definition| / bound = {ratio.max():.3e} (without the theory allowance "
              f"{np.max(np.where(rel * A[name] > 0, diff / np.where(rel * A[name] > 0, rel * A[name], 1.0), 0.0)):.3e})")
        worst = max(worst, float(ratio.max()))
    tolerances._record(f"importance predictive sums {what}", worst)
    assert worst <= 1.0, (what, worst)
    # two device runs give the same bytes
    again = run(obj, params, predictive=True, fixed=fixed, **kw)
    for name in PRED + ("pivot_t", "pivots"):
        assert same_bytes(getattr(dev.raw, name), getattr(again.raw, name)), (what, name)
    # the read-out: both routes alike, NaN exactly where no point was finite, the likelihood at the mean from a pairs call
    p, q = dev.predictive, ref.predictive
    ok = dev.status != dev.NO_FINITE
    N = dev.raw.pivot_t.size
    assert p.mean.shape == p.std.shape == (dev.n_problems, N)
    for name in ("mean", "std", "mean_chi2", "var_chi2", "mean_lnl", "var_lnl", "chi2_at_mean", "lnl_at_mean", "p_d", "p_v", "dic"):
        a, b = getattr(p, name), getattr(q, name)
        assert np.all(np.isnan(a[~ok])) and np.all(np.isfinite(a[ok])), (what, name)
        assert np.allclose(a[ok], b[ok], rtol=1e-9, atol=1e-9), (what, name)
    assert np.all(p.std[ok] >= 0) and np.all(p.var_lnl[ok] >= 0)
    return dev, ref


def at_mean(obj, ip, fixed):
    """lnL and chi2 of problem r at ``ip.mean[r]`` from a direct pairs call (the data vector: a batch call)."""
    ok = np.flatnonzero(ip.status != ip.NO_FINITE)
    batch = {k: np.full(len(ok), float(v)) for k, v in (fixed or {}).items()}
    batch.update({n: np.ascontiguousarray(ip.mean[ok, j]) for j, n in enumerate(ip.names)})
    if hasattr(obj, "log_likelihood_pairs"):
        return ok, obj.log_likelihood_pairs(batch, ok.astype(np.int32))
    return ok, obj.log_likelihood_batch(batch)


def assert_at_mean(obj, ip, fixed):
    ok, (lnl, chi2) = at_mean(obj, ip, fixed)
    assert same_bytes(ip.predictive.lnl_at_mean[ok], lnl) and same_bytes(ip.predictive.chi2_at_mean[ok], chi2)
    assert same_bytes(ip.predictive.p_d[ok], -2.0 * ip.predictive.mean_lnl[ok] + 2.0 * lnl)


# ------------------------------------------------------------------ 1. the synthetic fit, N = 80 ---------------------------
@pytest.fixture(scope="module")
def synth_rs(tmp_path_factory):
    """The synthetic fit against a stack of 3 mocks, and the same with mock 1 scaled out of every chi-square's range."""
    import victor_amd
    tmp = tmp_path_factory.mktemp("synth_stack")
    opts = write_stacks(tmp, [cases.synth_options(2)], 3, tag="synth")[0]
    fit = victor_amd.CCFFit(*opts)
    assert len(fit.s) * len(np.atleast_1d(fit.poles_s)) == 80
    path = opts[1]["redshift_space_ccf"]["data_file"]
    stack = np.load(path, allow_pickle=True).item()
    for key in ("monopole", "quadrupole"):
        stack[key] = np.array(stack[key])
        stack[key][1] *= 1e170                                    # its residual squared overflows: chi2 = inf, lnL = -inf
    lost = os.path.join(str(tmp), "synth_lost.npy")
    np.save(lost, stack, allow_pickle=True)
    model, data = cases.clone(opts[0]), cases.clone(opts[1])
    data["redshift_space_ccf"]["data_file"] = lost
    return fit, victor_amd.CCFFit(model, data)


SYNTH_KW = dict(n=200, seed=3, chunk=64, bins=6, min_ess=2.0)


@pytest.mark.parametrize("eps", ["sampled", "fixed"])
def test_synthetic_fit_three_mocks(synth_rs, eps):
    fit, _ = synth_rs
    names = ["fsigma8", "sigma_v"] + (["epsilon"] if eps == "sampled" else [])
    fixed = {"beta": BETA} if eps == "sampled" else {"beta": BETA, "epsilon": 1.01}
    rs = fit.realisations()
    dev, ref = both_routes(rs, SYNTH, f"synthetic, 3 mocks, epsilon {eps}", fixed=fixed, proposal=proposal(names), **SYNTH_KW)
    assert dev.n_problems == 3 and dev.n_chunks == 4 and dev.n_inside % 64 != 0 and np.all(dev.status == dev.OK)
    assert set(dev.predictive.multipoles) == {0, 2} and dev.predictive.multipoles[2][0].shape == (3, 40)
    assert len({dev.predictive.dic[r] for r in range(3)}) == 3
    assert_at_mean(rs, dev, fixed)


def test_synthetic_data_vector(synth_rs):
    """R = 1: a wave's lanes are 64 entry groups of one problem; the data-vector route keeps its vectors for the kernel."""
    fit, _ = synth_rs
    names = ["fsigma8", "sigma_v", "epsilon"]
    dev, ref = both_routes(fit, SYNTH, "synthetic data vector", fixed={"beta": BETA}, proposal=proposal(names), **SYNTH_KW)
    assert dev.n_problems == 1 and dev.n_chunks == 4
    assert_at_mean(fit, dev, {"beta": BETA})


def test_seventy_problems_from_repeated_mocks(synth_rs):
    fit, _ = synth_rs
    names = ["fsigma8", "sigma_v", "epsilon"]
    rs70 = fit.realisations(np.arange(70) % 3)
    dev, ref = both_routes(rs70, SYNTH, "synthetic, R = 70", fixed={"beta": BETA}, proposal=proposal(names), **SYNTH_KW)
    assert dev.n_problems == 70
    for name in ("pt", "ptt"):
        a = getattr(dev.raw, name)
        for r in range(70 - 3):
            assert same_bytes(a[r], a[r + 3]), (name, r)
    assert same_bytes(dev.raw.dev[:, :67], dev.raw.dev[:, 3:]) and same_bytes(dev.predictive.dic[:67], dev.predictive.dic[3:])
    assert not same_bytes(dev.raw.pt[0], dev.raw.pt[1])


def test_gaussian_prior_and_a_mock_without_a_finite_point(synth_rs):
    from victor_amd.priors import GaussianPrior
    fit, lost = synth_rs
    names = ["fsigma8", "sigma_v", "epsilon"]
    prior = GaussianPrior(["fsigma8"], [0.45], sigma=[0.03])
    kw = dict(fixed={"beta": BETA}, proposal=proposal(names), **SYNTH_KW)
    rs = fit.realisations()
    dev, ref = both_routes(rs, SYNTH, "synthetic with a Gaussian prior", prior=prior, **kw)
    plain = run(rs, SYNTH, predictive=True, **kw)
    assert dev.raw.pt.shape == (3, 80) and dev.raw.dev.shape == (4, 3)          # the prior's own problem keeps no such sums
    assert not same_bytes(dev.raw.pt, plain.raw.pt) and same_bytes(dev.raw.pivot_t, plain.raw.pivot_t)
    # D carries no prior term: the deviance pivots are the likelihood's, prior or not
    assert same_bytes(dev.raw.pivots, plain.raw.pivots)
    dev, ref = both_routes(lost.realisations(), SYNTH, "synthetic, mock 1 without a finite point", **kw)
    assert list(dev.status == dev.NO_FINITE) == [False, True, False] and dev.n_finite[1] == 0
    assert np.all(dev.raw.pt[1] == 0) and np.all(dev.raw.ptt[1] == 0) and np.all(dev.raw.dev[:, 1] == 0)
    assert np.all(np.isnan(dev.predictive.mean[1])) and np.isnan(dev.predictive.dic[1]) and np.all(np.isfinite(dev.predictive.mean[[0, 2]]))


# ------------------------------------------------------------------ 2. the beta-dependent BOSS fit -------------------------
def test_boss_fit_three_golden_mocks():
    import victor_amd
    names = ["fsigma8", "beta", "sigma_v", "epsilon"]
    rs = victor_amd.CCFFit(*stack_options()).realisations([0, 1, 2])
    dev, ref = both_routes(rs, PARAMS, "BOSS, 3 golden mocks", proposal=proposal(names), n=128, seed=4, chunk=48, bins=5, min_ess=2.0)
    assert dev.n_problems == 3 and dev.n_chunks == 3 and dev.n_inside % 48 != 0
    assert_at_mean(rs, dev, None)


# ------------------------------------------------------------------ 3. joint fits ------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory.mktemp(name))
        return made[name]
    return get


JOINT_KW = dict(n=96, seed=6, chunk=40, bins=5, min_ess=2.0)


def test_three_blocks_under_one_covariance(case):
    c = case("dsplit_cov")
    jr = c.joint.realisations([0, 1, 2])
    dev, ref = both_routes(jr, PARAMS, "dsplit under one covariance, 3 joint mocks", fixed=c.fixed, proposal=proposal(c.names), **JOINT_KW)
    p = dev.predictive
    sizes = [len(f.s) * len(np.atleast_1d(f.poles_s)) for f in c.joint.fits]
    assert dev.n_problems == 3 and dev.n_chunks == 3 and p.mean.shape == (3, sum(sizes)) and p.multipoles is None
    assert [b.stop - b.start for b in p.blocks] == sizes and p.blocks[1].start == sizes[0]
    assert same_bytes(p.multipoles_of(2)[0][0], p.mean[:, p.blocks[2].start:p.blocks[2].start + len(c.joint.fits[2].s)])
    assert_at_mean(jr, dev, c.fixed)
    # the joint data vector under the covariance, through the module function
    both_routes(c.joint, PARAMS, "dsplit under one covariance, joint data vector", fixed=c.fixed, proposal=proposal(c.names), **JOINT_KW)


def test_block_diagonal_with_a_velocity_dispersion_per_block(case):
    c = case("dsplit_diag")
    params = own_blocks(OWN)
    jr = c.joint.realisations([0, 1, 2])
    dev, ref = both_routes(jr, params, "dsplit block-diagonal, sigma_v per block", fixed=c.fixed, proposal=proposal(OWN), **JOINT_KW)
    assert dev.names == OWN and dev.n_problems == 3
    # the blocks' own values reach the blocks' own vectors: the band differs from one sigma_v for all
    shared = jr.importance_posterior(PARAMS, predictive=True, fixed=c.fixed, proposal=proposal(c.names), **JOINT_KW)
    assert not np.allclose(shared.predictive.mean, dev.predictive.mean, rtol=1e-6, atol=0)
    assert_at_mean(jr, dev, c.fixed)


def test_joint_data_vector_of_blocks_with_different_lengths(tmp_path):
    """Block 1 keeps the first 28 of its 40 s bins (N = 120 and 84): the segments' offsets in the pivot vector and the sums, and
    in the block-diagonal workspace whose stride follows the longer block."""
    import victor_amd
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import JointFit
    first = victor_amd.CCFFit(*cases.dsplit_options(0))
    model, data = (cases.clone(v) for v in cases.dsplit_options(1))
    ccf = data["redshift_space_ccf"]
    src = np.load(os.path.join(data["dir"], ccf["data_file"]), allow_pickle=True).item()
    n_s, keep = len(src["s"]), 28
    cut = dict(src)
    for key in ccf["ccf_keys"]:
        cut[key] = np.asarray(src[key])[..., :keep]
    ccf["data_file"] = os.path.join(str(tmp_path), "short.npy")
    np.save(ccf["data_file"], cut, allow_pickle=True)
    cov = np.load(os.path.join(data["dir"], data["covariance_matrix"]["data_file"]), allow_pickle=True).item()
    idx = np.concatenate([ell * n_s + np.arange(keep) for ell in range(len(ccf["ccf_keys"]) - 1)])
    data["covariance_matrix"]["data_file"] = os.path.join(str(tmp_path), "short_cov.npy")
    np.save(data["covariance_matrix"]["data_file"], dict(cov, covmat=np.asarray(cov["covmat"])[np.ix_(idx, idx)]), allow_pickle=True)
    second = victor_amd.CCFFit(model, data)
    joint = JointFit([first, second])
    sizes = [len(f.s) * len(np.atleast_1d(f.poles_s)) for f in joint.fits]
    assert sizes == [3 * n_s, 3 * keep] and sizes[0] != sizes[1]
    names = ["fsigma8", "sigma_v", "epsilon"]
    fixed = {"beta": BETA}
    dev, ref = both_routes(joint, PARAMS, "joint data vector, blocks of different N", fixed=fixed, proposal=proposal(names), **JOINT_KW)
    p = dev.predictive
    assert p.mean.shape == (1, sum(sizes)) and [(b.start, b.stop) for b in p.blocks] == [(0, sizes[0]), (sizes[0], sum(sizes))]
    # each block's segment of the pivot vector is that block's own theory vector at point 0 (a batch of one point may take
    # another launch shape than the chunk did: the theory tolerance, not bytes)
    x0 = {n: np.array([dev._sample.x[0, j]]) for j, n in enumerate(names)}
    x0["beta"] = np.array([BETA])
    tolerances.assert_same_theory(dev.raw.pivot_t[:sizes[0]], first.theory_vector_batch(x0)[0], "pivot segment of block 0")
    tolerances.assert_same_theory(dev.raw.pivot_t[sizes[0]:], second.theory_vector_batch(x0)[0], "pivot segment of block 1")
    assert not np.allclose(dev.raw.pivot_t[:sizes[1]], dev.raw.pivot_t[sizes[0]:], rtol=1e-3, atol=0)      # (the blocks differ)
    assert set(p.multipoles_of(1)) == {0, 2, 4} and p.multipoles_of(1)[4][0].shape == (1, keep)
    ok, (lnl, chi2) = at_mean(joint, dev, fixed)
    assert same_bytes(p.lnl_at_mean, lnl) and same_bytes(p.chi2_at_mean, chi2)
    assert importance_posterior(joint, PARAMS, fixed=fixed, proposal=proposal(names), **JOINT_KW).predictive is None
