"""Joint fit under one covariance across the data vectors on the GPU (JointFit(covariance=...), vk_joint_cov_eval_device_async).

Value contract: the reference's CCFFit applied to the concatenated vector - r = concat_q (t_q - d_q(beta)), chi2 = r^T Psi(beta) r
with the precision slices blended by the bracket rule, -1/2 log det C(beta) for a beta-dependent covariance, the likelihood
forms with p = NT.  The oracle answers below are restated here with NumPy from OracleFit theory and data vectors (OracleFit's
own likelihood form takes p from its block).  Against the oracle and the reference the bound is the parity bound of the
other parity tests (RTOL); against other GPU evaluation orders it is the derived bound of tests/tolerances.py."""

import ctypes as C
import faulthandler
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_joint_cov import boss_joint_cov_file, boss_pair_options, correlated
from tests.tolerances import U, _tau, assert_same_chi2, assert_same_lnl, chi2_bound

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


def restated_form(lk, chisq, factor, nd):
    """ccf_fit.py:455-473 with p = nd, the joint vector's length."""
    form, n = lk["form"].lower(), lk.get("nmocks", 1)
    if form == "sellentin":
        return -n * np.log(1 + chisq / (n - 1)) / 2 + factor
    if form == "hartlap":
        return -0.5 * chisq * (n - nd - 2) / (n - 1) + factor
    if form == "percival":
        npar = lk["nparams"]
        B = (n - nd - 2) / ((n - nd - 1) * (n - nd - 4))
        m = npar + 2 + (n - 1 + B * (nd - npar)) / (1 + B * (nd - npar))
        return -m * np.log(1 + chisq / (n - 1)) / 2 + factor
    return -0.5 * chisq + factor


def oracle_theory(oracle, opts, pts):
    """[block][point] theory vectors and the block oracles (one theory evaluation per block and point, shared by the forms)."""
    ofits = [oracle.OracleFit(*o) for o in opts]
    return ofits, [[of.theory_multipole_vector(of.s, dict(p), of.poles_s) for p in pts] for of in ofits]


def oracle_joint(ofits, theory, pts, cov, beta_grid, lk):
    """(lnl, chi2) of the joint vector, restated: cov is (NT, NT) or (n_beta, NT, NT) on beta_grid."""
    nd = cov.shape[-1]
    icov = np.linalg.inv(cov)
    lnl, chi2 = np.empty(len(pts)), np.empty(len(pts))
    for i, p in enumerate(pts):
        beta = p.get("beta", None)
        r = np.concatenate([theory[q][i] - of.data_vector(beta) for q, of in enumerate(ofits)])
        factor = 0.0
        if cov.ndim == 2:
            c = r @ np.linalg.solve(cov, r)
        else:
            g = beta_grid
            if beta < g.min():
                lo, t = 0, 0.0
            elif beta > g.max():
                lo, t = len(g) - 1, 0.0
            elif beta in g:
                lo, t = int(np.where(g == beta)[0][0]), 0.0
            else:
                lo = int(np.where(g < beta)[0][-1])
                t = (beta - g[lo]) / (g[-1] - g[lo])
            P = icov[lo] if t == 0.0 else (1 - t) * icov[lo] + t * icov[-1]
            C_ = cov[lo] if t == 0.0 else (1 - t) * cov[lo] + t * cov[-1]
            c = r @ P @ r
            sign, ld = np.linalg.slogdet(C_)
            if sign != 1:
                lnl[i], chi2[i] = -np.inf, np.inf
                continue
            factor = -0.5 * ld
        lnl[i] = restated_form(lk, c, factor, nd)
        chi2[i] = c
    bad = ~np.isfinite(lnl)
    lnl[bad], chi2[bad] = -np.inf, np.inf
    return lnl, chi2


def joint_bound(joint, params, ulps=64):
    """tests/tolerances.chi2_bound for the joint vector: |P| (blended as the slices are) against |r| and the blocks' tau."""
    from victor_amd import _native as N
    fit = joint.fits[0]
    rows = fit._fit_rows(params, fit._merged({}))
    t = np.concatenate([f.theory_vector_batch(rows) for f in joint.fits], axis=1)
    beta = rows[:, N.P_BETA]
    d = np.array([joint.multipole_datavector(b if not joint.fixed_data else None) for b in beta])
    absr = np.abs(t - d)
    v = absr + 2.0 * np.concatenate([_tau(f) for f in joint.fits])[None, :]
    absP = np.abs(joint.icov)
    if joint.fixed_covmat:
        amp = np.einsum("ij,jk,ik->i", absr, absP, v)
    else:
        amp = np.empty(len(rows))
        for i in range(len(rows)):
            lo, w = joint._bracket(beta[i]) if np.isfinite(beta[i]) else (0, 0.0)
            P = absP[lo] if w == 0.0 else (1 - w) * absP[lo] + w * absP[-1]
            amp[i] = absr[i] @ P @ v[i]
    return ulps * U * amp


def points_dict(pts):
    return {k: np.array([p[k] for p in pts]) for k in pts[0]}


def sub(params, sl):
    return {k: v[sl] for k, v in params.items()}


def test_blockdiag_covariance_reproduces_the_reference_and_the_block_path():
    import scipy.linalg as sl
    import victor_amd
    from victor_amd.joint import JointFit
    fits = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(5)]
    joint = JointFit(fits, covariance=sl.block_diag(*[f.covmat for f in fits]))
    g, meta = cases.golden_outputs()
    pts = meta["synth_points"][:len(g["dsplit_chi2"])]
    lnl, chi2 = joint.log_likelihood_batch(points_dict(pts))
    assert np.max(np.abs(chi2 / g["dsplit_chi2"] - 1)) < RTOL
    assert np.max(np.abs(lnl / g["dsplit_lnl"] - 1)) < RTOL
    one = joint.log_likelihood(pts[0])
    assert abs(one[1] / g["dsplit_chi2"][0] - 1) < RTOL
    hp = cases.halton_params(16384)
    lnl, chi2 = joint.log_likelihood_batch(hp)
    assert fits[0]._get_engine().last_instance().endswith("+joint_chi2")
    plain_l, plain_c = JointFit(fits).log_likelihood_batch(hp)
    bound = sum(chi2_bound(f, hp) for f in fits)
    assert_same_chi2(chi2, plain_c, bound, what="joint covariance blockdiag vs block-diagonal path")
    assert_same_lnl(lnl, plain_l, bound, what="joint covariance blockdiag vs block-diagonal path")


def test_correlated_fixed_covariance_against_the_oracle(oracle):
    import victor_amd
    from victor_amd.joint import JointFit
    opts = [cases.dsplit_options(q) for q in range(5)]
    fits = [victor_amd.CCFFit(*o) for o in opts]
    cov = correlated([f.covmat for f in fits])
    g, meta = cases.golden_outputs()
    hp = cases.halton_params(64)
    pts = list(meta["synth_points"][:6]) + [cases.point(hp, i) for i in range(64)]
    ofits, theory = oracle_theory(oracle, opts, pts)
    for form in FORMS:
        joint = JointFit(fits, covariance=cov, likelihood=like(form))
        lnl, chi2 = joint.log_likelihood_batch(points_dict(pts))
        ol, oc = oracle_joint(ofits, theory, pts, cov, None, like(form))
        assert np.all(np.isfinite(oc))
        assert np.max(np.abs(chi2 / oc - 1)) < RTOL, form
        assert np.max(np.abs(lnl - ol) / np.abs(oc)) < RTOL, form
        # the correlation matters: the block-diagonal answer is another one
        assert np.max(np.abs(JointFit(fits).log_likelihood_batch(points_dict(pts))[1] / chi2 - 1)) > 1e-3


def _gridded_points(beta_grid):
    hp = cases.halton_params(24, with_beta=True)
    pts = [cases.point(hp, i) for i in range(24)]
    base = dict(pts[0])
    for b in (beta_grid[0] - 0.03, beta_grid[0], beta_grid[5], 0.5 * (beta_grid[5] + beta_grid[6]), beta_grid[-1],
              beta_grid[-1] + 0.02, 0.5 * (beta_grid[-2] + beta_grid[-1])):
        pts.append(dict(base, beta=float(b)))
    return pts


def test_correlated_gridded_covariance_against_the_oracle(oracle, tmp_path):
    import victor_amd
    from victor_amd.joint import JointFit
    opts = boss_pair_options()
    fits = [victor_amd.CCFFit(*o) for o in opts]
    pts = _gridded_points(fits[0].beta_covmat)
    ofits, theory = oracle_theory(oracle, opts, pts)
    for indefinite in (False, True):
        spec = boss_joint_cov_file(str(tmp_path / f"cov_{indefinite}.npy"), indefinite_last=indefinite)
        src = np.load(os.path.join(spec["dir"], spec["data_file"]), allow_pickle=True).item()
        for form in FORMS:
            joint = JointFit(fits, covariance=spec, likelihood=like(form))
            lnl, chi2 = joint.log_likelihood_batch(points_dict(pts))
            ol, oc = oracle_joint(ofits, theory, pts, src["covmat"], src["beta"], like(form))
            failed = ~np.isfinite(oc)
            assert np.array_equal(~np.isfinite(chi2), failed), (form, indefinite, np.where(~np.isfinite(chi2))[0], np.where(failed)[0])
            assert np.all(np.isneginf(lnl[failed])) and np.all(np.isposinf(chi2[failed]))
            assert failed.any() == indefinite and (~failed).sum() > 10
            ok = ~failed
            assert np.max(np.abs(chi2[ok] / oc[ok] - 1)) < RTOL, (form, indefinite)
            assert np.max(np.abs(lnl[ok] - ol[ok]) / np.abs(oc[ok])) < RTOL, (form, indefinite)


def test_seventeen_beta_dependent_blocks_against_the_oracle(oracle, tmp_path):
    """More blocks than the 16 rows of a tile: every block's PCHIP piece of the data at beta is found (the per-row tables of the
    kernel hold blocks x 16 entries, more than one pass of the workgroup's 256 threads).  17 BOSS-style blocks (N = 60, NT = 1020)
    alternate between data.npy and patchy_data.npy; the covariance has six of the 31 beta slices."""
    import victor_amd
    from victor_amd.joint import JointFit
    pair = boss_pair_options()
    q_of = [q % 2 for q in range(17)]
    fits = [victor_amd.CCFFit(*pair[q]) for q in q_of]
    src = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    pick = np.arange(0, 31, 6)
    beta_grid = np.asarray(src["beta"], dtype=float)[pick]
    slices = np.array([correlated([c] * 17) for c in src["covmat"][pick]])
    np.save(tmp_path / "cov17.npy", {"beta": beta_grid, "covmat": slices}, allow_pickle=True)
    spec = {"dir": str(tmp_path), "data_file": "cov17.npy", "cov_key": "covmat", "fixed_beta": False, "beta_key": "beta"}
    hp = cases.halton_params(12, with_beta=True)
    pts = [cases.point(hp, i) for i in range(12)]
    pts += [dict(pts[0], beta=float(b)) for b in (beta_grid[0] - 0.03, beta_grid[2], 0.5 * (beta_grid[2] + beta_grid[3]),
                                                   beta_grid[-1] + 0.02)]
    ofits2, theory2 = oracle_theory(oracle, pair, pts)
    ofits, theory = [ofits2[q] for q in q_of], [theory2[q] for q in q_of]
    for form in ("gaussian", "percival"):
        joint = JointFit(fits, covariance=spec, likelihood=like(form))
        assert joint.n_data == 1020
        lnl, chi2 = joint.log_likelihood_batch(points_dict(pts))
        ol, oc = oracle_joint(ofits, theory, pts, slices, beta_grid, like(form))
        assert np.all(np.isfinite(oc)) and np.all(np.isfinite(chi2))
        assert np.max(np.abs(chi2 / oc - 1)) < RTOL, form
        assert np.max(np.abs(lnl - ol) / np.abs(oc)) < RTOL, form


@pytest.mark.parametrize("case", ["fixed", "gridded"])
def test_one_block_equals_the_single_fit(case):
    import victor_amd
    from victor_amd.joint import JointFit
    if case == "fixed":
        fit = victor_amd.CCFFit(*cases.dsplit_options(0))
        cov = fit.covmat
        params = cases.halton_params(1000)
    else:
        fit = victor_amd.CCFFit(*cases.boss_options())
        cov = {"dir": cases.GOLDEN, "data_file": "boss/cov.npy", "cov_key": "covmat", "fixed_beta": False, "beta_key": "beta"}
        params = cases.halton_params(1000, with_beta=True)
        params["beta"] = np.concatenate([fit.beta_covmat[:40 - 9], params["beta"][31:]])    # on every grid value as well
    bound = chi2_bound(fit, params)
    for form in FORMS:
        lnl, chi2 = JointFit([fit], covariance=cov, likelihood=like(form)).log_likelihood_batch(params)
        sl_, sc = fit.log_likelihood_batch(params, likelihood=like(form))
        assert_same_chi2(chi2, sc, bound, what=f"one-block joint vs CCFFit, {case}, {form}")
        assert_same_lnl(lnl, sl_, bound, what=f"one-block joint vs CCFFit, {case}, {form}")


@pytest.mark.parametrize("case", ["fixed", "gridded"])
def test_sizes_repeats_and_nan_guard(case, tmp_path):
    import victor_amd
    from victor_amd.joint import JointFit
    if case == "fixed":
        fits = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(5)]
        joint = JointFit(fits, covariance=correlated([f.covmat for f in fits]))
        params = cases.halton_params(16389)
    else:
        fits = [victor_amd.CCFFit(*o) for o in boss_pair_options()]
        joint = JointFit(fits, covariance=boss_joint_cov_file(str(tmp_path / "c.npy")))
        params = cases.halton_params(16389, with_beta=True)
    lnl, chi2 = joint.log_likelihood_batch(params)
    assert np.all(np.isfinite(lnl)) and np.all(np.isfinite(chi2))
    again = joint.log_likelihood_batch(params)
    assert again[0].tobytes() == lnl.tobytes() and again[1].tobytes() == chi2.tobytes()   # repeated call: same bits
    assert fits[0]._get_engine().last_instance().endswith("+joint_chi2")
    for n in (1, 17, 1000):
        part = sub(params, slice(0, n))
        pl, pc = joint.log_likelihood_batch(part)
        bound = joint_bound(joint, part)
        assert_same_chi2(pc, chi2[:n], bound, what=f"joint covariance {case}: {n} points vs 16389")
        assert_same_lnl(pl, lnl[:n], bound, what=f"joint covariance {case}: {n} points vs 16389")
    tail = sub(params, slice(16389 - 40, 16389))
    tl, tc = joint.log_likelihood_batch(tail)
    assert_same_chi2(tc, chi2[-40:], joint_bound(joint, tail), what=f"joint covariance {case}: tail")
    one = joint.log_likelihood(cases.point(params, 5))
    assert_same_chi2(one[1], chi2[5], joint_bound(joint, sub(params, slice(5, 6))), what=f"joint covariance {case}: one point")
    bad = sub(params, slice(0, 9))
    bad = {k: v.copy() for k, v in bad.items()}
    bad["sigma_v"][3] = np.nan
    if case == "gridded":
        bad["beta"][6] = np.nan
    bl, bc = joint.log_likelihood_batch(bad)
    failed = [3, 6] if case == "gridded" else [3]
    assert np.all(np.isneginf(bl[failed])) and np.all(np.isposinf(bc[failed]))
    good = [i for i in range(9) if i not in failed]
    assert np.all(np.isfinite(bl[good]))
    assert_same_chi2(bc[good], chi2[good], joint_bound(joint, sub(params, good)), what=f"joint covariance {case}: NaN neighbours")


def test_c_abi_rejects_bad_joint_covariance_calls():
    import victor_amd
    from victor_amd import _native as N
    from victor_amd.joint import JointFit
    fits = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(2)]
    joint = JointFit(fits, covariance=correlated([f.covmat for f in fits]))
    joint.log_likelihood_batch(cases.halton_params(4))
    engines, opts = joint._plan_cov({})
    lead = engines[0]
    lib = lead._lib
    h = joint._joint_handle(lead)
    n = 8
    d_rows, d_out, d_ws = lead.alloc(n * N.VK_NPAR), lead.alloc(2 * n), lead.alloc(lib.vk_joint_cov_workspace_doubles(h, n))
    ctxs = (C.c_void_p * 2)(*[e._ctx for e in engines])
    swapped = (C.c_void_p * 2)(engines[1]._ctx, engines[0]._ctx)
    other = victor_amd.CCFFit(*cases.boss_options())._get_engine()
    wrong_n = (C.c_void_p * 2)(engines[0]._ctx, other._ctx)
    call = lambda hh, cc, k, rows, m, out, ws: lib.vk_joint_cov_eval_device_async(hh, cc, k, C.byref(opts), rows, m, out, None, ws)   # noqa: E731
    assert call(None, ctxs, 2, d_rows, n, d_out, d_ws) == -1
    assert call(h, ctxs, 1, d_rows, n, d_out, d_ws) == -1                  # block count
    assert call(h, swapped, 2, d_rows, n, d_out, d_ws) == -1               # lead is not the handle's
    assert call(h, wrong_n, 2, d_rows, n, d_out, d_ws) == -1               # N of a block
    assert call(h, ctxs, 2, None, n, d_out, d_ws) == -1                    # buffers
    assert call(h, ctxs, 2, d_rows, n, None, d_ws) == -1
    assert call(h, ctxs, 2, d_rows, n, d_out, None) == -1
    assert call(h, ctxs, 2, d_rows, -1, d_out, d_ws) == -1
    assert call(h, None, 2, d_rows, n, d_out, d_ws) == -1
    assert lib.vk_joint_cov_workspace_doubles(None, n) == 0
    # tables
    t = N.vk_joint_cov_tables()
    out = C.c_void_p()
    assert lib.vk_joint_cov_create(lead._ctx, C.byref(t), C.byref(out)) == -1 and not out.value      # no blocks
    bn = np.array([120, 120], dtype=np.int32)
    prec = np.eye(240)
    beta = np.array([0.3, 0.2])
    t.n_blocks, t.block_n, t.prec = 2, bn.ctypes.data_as(C.POINTER(C.c_int32)), N.as_dp(prec)
    t.n_beta, t.beta = 2, N.as_dp(beta)
    assert lib.vk_joint_cov_create(lead._ctx, C.byref(t), C.byref(out)) == -1                        # no logdet / eig
    ld, eig = np.zeros(2), np.ones((2, 240))
    t.logdet, t.eig = N.as_dp(ld), N.as_dp(eig)
    assert lib.vk_joint_cov_create(lead._ctx, C.byref(t), C.byref(out)) == -1                        # grid decreasing
    msg = lib.vk_last_error(lead._ctx).decode()
    assert "beta grid must be strictly" in msg, msg
    assert lib.vk_joint_cov_create(None, C.byref(t), C.byref(out)) == -1
    t.n_blocks = 33                                                                                  # above the 32-block cap
    assert lib.vk_joint_cov_create(lead._ctx, C.byref(t), C.byref(out)) == -1
    # the context still works
    for p in (d_rows, d_out, d_ws):
        lead.free(p)
    lnl, chi2 = joint.log_likelihood_batch(cases.halton_params(4))
    assert np.all(np.isfinite(lnl))
