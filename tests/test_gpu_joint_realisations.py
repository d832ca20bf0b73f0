"""JointFit.realisations() on the GPU (JointRealisations, vk_joint_cov_eval_realisations).

Value contract: entry [p, m] equals JointFit([CCFFit(model_q, data_q with simulation_number=numbers[m]) for q],
covariance=same, likelihood=same).log_likelihood_batch(point p), with (-inf, inf) in the same places.  Against the oracle
restatement of the joint vector (tests/test_gpu_joint_cov.py: OracleFit with simulation_number=m per block) the bound is RTOL;
against the per-realisation JointFit - the same theory vectors, the joint chi-square summed for other rows of another kernel -
the derived bound of tests/tolerances.py; pairs mode returns the bits of cross mode.  Fixtures: per-block stacks written from the
goldens with a fixed seed (tests/test_joint_realisations.py: write_stacks)."""

import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_joint_cov import _gridded_points, joint_bound, oracle_joint
from tests.test_joint_cov import boss_joint_cov_file, correlated
from tests.test_joint_realisations import boss_stacks, dsplit_stacks, with_number
from tests.tolerances import assert_same_chi2, assert_same_lnl

pytestmark = pytest.mark.gpu
RTOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"gaussian": {}, "sellentin": {"nmocks": 1000}, "hartlap": {"nmocks": 1000}, "percival": {"nmocks": 1000, "nparams": 4}}


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


def like(form):
    return dict({"form": form}, **FORMS[form])


def points_dict(pts):
    return {k: np.array([p[k] for p in pts]) for k in pts[0]}


def fits_of(opts):
    import victor_amd
    return [victor_amd.CCFFit(*o) for o in opts]


def release(fits):
    for f in fits:
        f._engine = None


def per_realisation(opts, numbers, params, covariance, likelihood=None, bounds=True):
    """(lnl, chi2, bound), each (n_points, len(numbers)): one JointFit of fresh CCFFits per realisation number."""
    from victor_amd.joint import JointFit
    out = []
    for m in numbers:
        fits = fits_of(with_number(opts, m))
        joint = JointFit(fits, covariance=covariance, likelihood=likelihood)
        lnl, chi2 = joint.log_likelihood_batch(params)
        b = joint_bound(joint, params) if bounds and covariance is not None else np.zeros(len(lnl))
        out.append((lnl, chi2, b))
        joint._release_handle()
        release(fits)
    return tuple(np.stack([o[i] for o in out], axis=1) for i in range(3))


def oracle_entries(oracle, opts, pts, numbers, cov, beta_grid, lk):
    """(lnl, chi2) [len(pts)][len(numbers)] of the joint vector restated from OracleFit blocks with simulation_number=m; each
    block's theory vector once per point (it does not depend on the realisation)."""
    base = [oracle.OracleFit(*o) for o in opts]
    theory = [[of.theory_multipole_vector(of.s, dict(p), of.poles_s) for p in pts] for of in base]
    ol, oc = np.empty((len(pts), len(numbers))), np.empty((len(pts), len(numbers)))
    for j, m in enumerate(numbers):
        ofits = [oracle.OracleFit(*o) for o in with_number(opts, m)]
        ol[:, j], oc[:, j] = oracle_joint(ofits, theory, pts, cov, beta_grid, lk)
    return ol, oc


def assert_oracle(lnl, chi2, ol, oc, what):
    failed = ~np.isfinite(oc)
    assert np.array_equal(~np.isfinite(chi2), failed), what
    assert np.all(np.isneginf(lnl[failed])) and np.all(np.isposinf(chi2[failed])), what
    ok = ~failed
    assert np.max(np.abs(chi2[ok] / oc[ok] - 1)) < RTOL, what
    assert np.max(np.abs(lnl[ok] - ol[ok]) / np.abs(oc[ok])) < RTOL, what


def assert_per_realisation(lnl, chi2, want_l, want_c, bound, what):
    assert np.array_equal(np.isinf(chi2), np.isinf(want_c)) and np.array_equal(np.isinf(lnl), np.isinf(want_l)), what
    assert_same_chi2(chi2, want_c, bound, what=what)
    assert_same_lnl(lnl, want_l, bound, what=what)


def dsplit_case(tmp_path, n_real=37):
    opts = dsplit_stacks(tmp_path, n_real)
    fits = fits_of(opts)
    return opts, fits, correlated([f.covmat for f in fits])


def boss_case(tmp_path, n_real, indefinite=False):
    opts = boss_stacks(tmp_path, n_real)
    spec = boss_joint_cov_file(str(tmp_path / f"cov_{indefinite}.npy"), indefinite_last=indefinite)
    src = np.load(os.path.join(spec["dir"], spec["data_file"]), allow_pickle=True).item()
    return opts, fits_of(opts), spec, src


def test_dsplit_fixed_covariance_against_the_oracle_and_per_realisation_fits(tmp_path, oracle):
    from victor_amd.joint import JointFit
    opts, fits, cov = dsplit_case(tmp_path)
    hp = cases.halton_params(21)
    jr = JointFit(fits, covariance=cov).realisations()
    lnl, chi2 = jr.log_likelihood(hp)
    assert lnl.shape == chi2.shape == (21, 37) and np.all(np.isfinite(chi2))
    pick = [0, 16, 17, 36]
    pts = [cases.point(hp, i) for i in (0, 9, 20)]
    ol, oc = oracle_entries(oracle, opts, pts, pick, cov, None, like("gaussian"))
    assert_oracle(lnl[[0, 9, 20]][:, pick], chi2[[0, 9, 20]][:, pick], ol, oc, "dsplit cross mode vs oracle")
    wl, wc, bound = per_realisation(opts, range(37), hp, cov)
    assert_per_realisation(lnl, chi2, wl, wc, bound, "dsplit cross mode vs per-realisation JointFit")
    one_l, one_c = jr.log_likelihood(cases.point(hp, 4))                # (a batch of one: another theory launch)
    assert one_c.shape == (37,)
    assert_same_chi2(one_c, chi2[4], bound[4], what="dsplit one point vs the batch")
    assert_same_lnl(one_l, lnl[4], bound[4], what="dsplit one point vs the batch")
    assert jr.chi_squared(hp).tobytes() == chi2.tobytes()


@pytest.mark.parametrize("indefinite", [False, True])
def test_boss_gridded_covariance_against_the_oracle_and_per_realisation_fits(tmp_path, oracle, indefinite):
    from victor_amd.joint import JointFit
    opts, fits, spec, src = boss_case(tmp_path, 19, indefinite)
    pts = _gridded_points(fits[0].beta_covmat)
    params = points_dict(pts)
    jr = JointFit(fits, covariance=spec, likelihood=like("gaussian")).realisations()     # (the BOSS options' own form: sellentin)
    lnl, chi2 = jr.log_likelihood(params)
    assert chi2.shape == (len(pts), 19)
    failed = ~np.isfinite(chi2)
    assert failed.any() == indefinite and (~failed).sum() > 10 * 19
    assert np.array_equal(failed, np.repeat(failed[:, :1], 19, axis=1))     # a failed covariance fails the point
    pick = [0, 7, 18]
    sel = [0, 5, len(pts) - 7, len(pts) - 4, len(pts) - 3, len(pts) - 1]    # box, below the grid, blended, last slice, blended
    ol, oc = oracle_entries(oracle, opts, [pts[i] for i in sel], pick, src["covmat"], src["beta"], like("gaussian"))
    assert_oracle(lnl[sel][:, pick], chi2[sel][:, pick], ol, oc, f"boss gridded cross mode vs oracle, indefinite={indefinite}")
    wl, wc, bound = per_realisation(opts, range(19), params, spec, like("gaussian"))
    assert_per_realisation(lnl, chi2, wl, wc, bound, f"boss gridded vs per-realisation JointFit, indefinite={indefinite}")


@pytest.mark.parametrize("form", list(FORMS))
def test_every_likelihood_form(tmp_path, oracle, form):
    from victor_amd.joint import JointFit
    opts, fits, cov = dsplit_case(tmp_path, 5)
    hp = cases.halton_params(6)
    lnl, chi2 = JointFit(fits, covariance=cov, likelihood=like(form)).realisations().log_likelihood(hp)
    pts = [cases.point(hp, i) for i in range(6)]
    ol, oc = oracle_entries(oracle, opts, pts, [0, 4], cov, None, like(form))
    assert_oracle(lnl[:, [0, 4]], chi2[:, [0, 4]], ol, oc, f"dsplit {form} vs oracle")
    wl, wc, bound = per_realisation(opts, range(5), hp, cov, like(form))
    assert_per_realisation(lnl, chi2, wl, wc, bound, f"dsplit {form} vs per-realisation JointFit")
    release(fits)
    bopts, boss, spec, src = boss_case(tmp_path, 4, indefinite=True)
    bpts = _gridded_points(boss[0].beta_covmat)
    bl, bc = JointFit(boss, covariance=spec, likelihood=like(form)).realisations().log_likelihood(points_dict(bpts))
    sel = [1, len(bpts) - 5, len(bpts) - 4, len(bpts) - 1]
    ol, oc = oracle_entries(oracle, bopts, [bpts[i] for i in sel], [1, 3], src["covmat"], src["beta"], like(form))
    assert_oracle(bl[sel][:, [1, 3]], bc[sel][:, [1, 3]], ol, oc, f"boss gridded {form} vs oracle")
    wl, wc, bound = per_realisation(bopts, range(4), points_dict(bpts), spec, like(form))
    assert_per_realisation(bl, bc, wl, wc, bound, f"boss gridded {form} vs per-realisation JointFit")


@pytest.mark.parametrize("case", ["fixed", "gridded"])
def test_pairs_mode_returns_the_bits_of_cross_mode(tmp_path, case):
    from victor_amd.joint import JointFit
    if case == "fixed":
        opts, fits, cov = dsplit_case(tmp_path, 20)
        params = cases.halton_params(23)
    else:
        opts, fits, cov, _ = boss_case(tmp_path, 20, indefinite=True)
        params = points_dict(_gridded_points(fits[0].beta_covmat))
    joint = JointFit(fits, covariance=cov)
    n = len(next(iter(params.values())))
    assert n % 16 != 0
    rng = np.random.default_rng(5)
    for numbers in ([4], list(range(17)), None):
        jr = joint.realisations(numbers)
        lnl, chi2 = jr.log_likelihood(params)
        k = len(jr)
        which = rng.integers(0, k, n)
        which[:3] = which[0]                                                # repeated indices
        pl, pc = jr.log_likelihood_pairs(params, which)
        assert pl.shape == (n,)
        assert pc.tobytes() == chi2[np.arange(n), which].tobytes(), (case, k)
        assert pl.tobytes() == lnl[np.arange(n), which].tobytes(), (case, k)
        # one point: against every realisation, and against some of them as pairs of one point (the same theory launch)
        p0 = cases.point(params, n - 1)
        one_l, one_c = jr.log_likelihood(p0)
        for m in {0, k // 2, k - 1}:
            sl, sc = jr.log_likelihood_pairs(p0, [m])
            assert sc.tobytes() == one_c[m:m + 1].tobytes() and sl.tobytes() == one_l[m:m + 1].tobytes(), (case, k, m)
        # the same realisation for every point, repeated
        rl, rc = jr.log_likelihood_pairs(params, np.full(n, k - 1))
        assert rc.tobytes() == chi2[:, k - 1].tobytes() and rl.tobytes() == lnl[:, k - 1].tobytes()


def test_block_diagonal_against_per_realisation_joint_fits(tmp_path):
    from victor_amd.joint import JointFit
    from victor_amd import _native as N
    for opts, params in ((dsplit_stacks(tmp_path, 9), cases.halton_params(20)),
                         (boss_stacks(tmp_path, 9), cases.halton_params(20, with_beta=True))):
        fits = fits_of(opts)
        jr = JointFit(fits).realisations()
        bad = {k: v.copy() for k, v in params.items()}
        bad["sigma_v"][3] = np.nan
        lnl, chi2 = jr.log_likelihood(bad)
        assert np.all(np.isneginf(lnl[3])) and np.all(np.isposinf(chi2[3]))
        wl, wc, _ = per_realisation(opts, range(9), bad, None)
        assert np.array_equal(np.isinf(chi2), np.isinf(wc))
        rows = fits[0]._fit_rows(bad, fits[0].model)
        good = np.isfinite(rows[:, N.P_SIGMAV])
        bound = None
        for m in range(9):
            mf = fits_of(with_number(opts, m))
            from tests.tolerances import chi2_bound
            b = sum(chi2_bound(f, {k: v[good] for k, v in bad.items()}) for f in mf)
            release(mf)
            bound = b[:, None] if bound is None else np.concatenate([bound, b[:, None]], axis=1)
        assert_same_chi2(chi2[good], wc[good], bound, what="block-diagonal realisations vs per-realisation JointFit")
        assert_same_lnl(lnl[good], wl[good], bound, what="block-diagonal realisations vs per-realisation JointFit")
        which = np.arange(20) % 9
        pl, pc = jr.log_likelihood_pairs(bad, which)                       # each block's pairs are its cross bits
        assert pc.tobytes() == chi2[np.arange(20), which].tobytes() and pl.tobytes() == lnl[np.arange(20), which].tobytes()
        release(fits)


def test_outputs_above_256_mb_are_chunked(tmp_path):
    from victor_amd.joint import JointFit
    opts, fits, spec, _ = boss_case(tmp_path, 1000)
    n = 34000                                           # 34000 x 1000 doubles = 272 MB per output: two launches
    params = cases.halton_params(n, with_beta=True)
    jr = JointFit(fits, covariance=spec).realisations()
    lnl, chi2 = jr.log_likelihood(params)
    assert chi2.shape == (n, 1000) and np.all(np.isfinite(chi2)) and np.all(np.isfinite(lnl))
    rng = np.random.default_rng(3)
    p = np.concatenate([rng.integers(0, n, 3000), [0, 33553, 33554, n - 1]])
    m = np.concatenate([rng.integers(0, 1000, 3000), [0, 999, 0, 999]])
    # (the pairs call is another batch: its theory launch may take another kernel variant, so the bound is the generic one)
    pl, pc = jr.log_likelihood_pairs({k: v[p] for k, v in params.items()}, m)
    bound = assert_same_chi2(pc, chi2[p, m], n_data=120, what="chunked cross mode vs pairs")
    assert_same_lnl(pl, lnl[p, m], bound, what="chunked cross mode vs pairs")
    # pairs mode over the whole batch (one launch): the same theory batch up to its chunking
    which = rng.integers(0, 1000, n)
    wl, wc = jr.log_likelihood_pairs(params, which)
    bound = assert_same_chi2(wc, chi2[np.arange(n), which], n_data=120, what="chunked cross mode vs whole-batch pairs")
    assert_same_lnl(wl, lnl[np.arange(n), which], bound, what="chunked cross mode vs whole-batch pairs")


def test_repeated_calls_instance_name_and_c_abi_guards(tmp_path):
    from victor_amd import _native as N
    from victor_amd.joint import JointFit
    opts, fits, cov = dsplit_case(tmp_path, 20)
    params = cases.halton_params(100)
    joint = JointFit(fits, covariance=cov)
    jr = joint.realisations()
    lnl, chi2 = jr.log_likelihood(params)
    again = jr.log_likelihood(params)
    assert again[0].tobytes() == lnl.tobytes() and again[1].tobytes() == chi2.tobytes()
    assert fits[0]._get_engine().last_instance().endswith("+joint_real_chi2")
    # the plain joint covariance fit on the same engines still works and does not disturb the realisations
    joint.log_likelihood_batch(params)
    assert fits[0]._get_engine().last_instance().endswith("+joint_chi2")
    assert jr.log_likelihood(params)[1].tobytes() == chi2.tobytes()
    # C ABI guards
    engines, opts_blk = joint._plan_cov({})
    lead = engines[0]
    lib = lead._lib
    h = joint._joint_handle(lead)
    rows = N.f64(fits[0]._fit_rows(params, fits[0].model))
    out = np.empty((len(rows), 20))
    ctxs = (C.c_void_p * 5)(*[e._ctx for e in engines])

    def call(cc, k, which=None, hh=h, n=len(rows)):
        w = None if which is None else np.ascontiguousarray(which, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        return lib.vk_joint_cov_eval_realisations(hh, cc, k, C.byref(opts_blk), N.as_dp(rows), n, w, N.as_dp(out), None)
    assert call(ctxs, 5) == 0
    assert call(ctxs, 5, hh=None) == -1
    assert call(ctxs, 4) == -1
    assert call(None, 5) == -1
    assert call(ctxs, 5, n=-1) == -1
    which = np.zeros(len(rows))
    which[7] = 20
    assert call(ctxs, 5, which) == -1
    assert "outside 0..19" in lib.vk_last_error(lead._ctx).decode()
    engines[3].set_realisations(np.empty((0, 120)))                       # none
    engines[3]._real_owner = None
    assert call(ctxs, 5) == -1
    assert "no realisations are set on context 3" in lib.vk_last_error(lead._ctx).decode()
    engines[3].set_realisations(jr.blocks[3].blocks)
    engines[2].set_realisations(jr.blocks[2].blocks[:19])                 # different n_real
    engines[2]._real_owner = None
    assert call(ctxs, 5) == -1
    assert "context 2 holds 19 realisations, context 0 holds 20" in lib.vk_last_error(lead._ctx).decode()
    # the Python layer uploads again and answers as before
    l2, c2 = jr.log_likelihood(params)
    assert c2.tobytes() == chi2.tobytes() and l2.tobytes() == lnl.tobytes()
