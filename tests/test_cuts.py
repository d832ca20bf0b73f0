"""Scale cuts (victor_amd/cuts.py) without a GPU: how a cut resolves to entries of the data vector, the refusals, the per-cut
tables against hand-sliced golden covariances, and the NumPy definition ``cut_likelihood`` against the oracle and against a
value computed by hand."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_realisations import stack_options
from tests.tolerances import U, _quadratic_bound, assert_same_chi2, assert_same_lnl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"gaussian": {}, "sellentin": {"nmocks": 1000}, "hartlap": {"nmocks": 1000}, "percival": {"nmocks": 1000, "nparams": 4}}


def boss_fit(fixed_cov=False):
    import victor_amd
    model, data = cases.boss_options("config")
    if fixed_cov:
        data["covariance_matrix"].update(data_file="boss/cov_fixed.npy", fixed_beta=True)
    return victor_amd.CCFFit(model, data)


def test_a_cut_resolves_to_increasing_entries_of_the_multipole_major_vector():
    from victor_amd import ScaleCut
    fit = boss_fit()
    n_s = len(fit.s)
    assert list(fit.poles_s) == [0, 2] and n_s == 30
    assert np.array_equal(ScaleCut().resolve(fit), np.arange(60))
    assert np.array_equal(ScaleCut(s_min=fit.s[7]).resolve(fit), np.r_[7:30, 37:60])
    assert np.array_equal(ScaleCut(s_max=fit.s[4]).resolve(fit), np.r_[0:5, 30:35])
    assert np.array_equal(ScaleCut(poles=[0]).resolve(fit), np.arange(30))
    assert np.array_equal(ScaleCut(poles=2).resolve(fit), np.arange(30, 60))
    assert np.array_equal(ScaleCut(s_min=fit.s[3], s_max=fit.s[10]).resolve(fit), np.r_[3:11, 33:41])
    assert np.array_equal(ScaleCut(s_min=fit.s[5], s_max=fit.s[5]).resolve(fit), [5, 35])
    mask = np.zeros(60, dtype=bool)
    mask[[1, 2, 17, 44, 59]] = True
    idx = ScaleCut(mask=mask).resolve(fit)
    assert np.array_equal(idx, [1, 2, 17, 44, 59]) and idx.dtype == np.int32
    # bounds between two bins select by value
    assert np.array_equal(ScaleCut(s_min=0.5 * (fit.s[6] + fit.s[7]), poles=[0]).resolve(fit), np.arange(7, 30))


def test_refusals():
    from victor_amd import InputError, ScaleCut
    from victor_amd.cuts import cut_tables
    fit = boss_fit()
    with pytest.raises(InputError, match="given alone"):
        ScaleCut(s_min=10.0, mask=np.ones(60, dtype=bool))
    with pytest.raises(InputError, match="keeps no entry"):
        ScaleCut(mask=np.zeros(60, dtype=bool)).resolve(fit)
    with pytest.raises(InputError, match="select no s bin"):
        ScaleCut(s_min=fit.s[-1] + 1.0).resolve(fit)
    with pytest.raises(InputError, match="select no s bin"):
        ScaleCut(s_min=fit.s[4] + 0.1, s_max=fit.s[5] - 0.1).resolve(fit)
    with pytest.raises(InputError, match="subset"):
        ScaleCut(poles=[0, 4]).resolve(fit)
    with pytest.raises(InputError, match="subset"):
        ScaleCut(poles=[0, 0]).resolve(fit)
    for bad in (np.ones(59, dtype=bool), np.ones(60), np.ones((2, 30), dtype=bool)):
        with pytest.raises(InputError, match="boolean array of length 60"):
            ScaleCut(mask=bad).resolve(fit)
    with pytest.raises(InputError, match="keep the same entries"):
        cut_tables(fit, [ScaleCut(), ScaleCut(poles=[0]), ScaleCut(s_min=fit.s[0])])
    for bad in ([], [None], ["all"]):
        with pytest.raises(InputError, match="non-empty list"):
            cut_tables(fit, bad)
    # the routes that are out of scope, before any device call
    rs = fit.scale_cuts([ScaleCut(), ScaleCut(poles=[0])])
    assert len(rs) == 2 and rs.shape == (2, 1)
    with pytest.raises(InputError, match="fisher"):
        rs.fisher({}, None)
    with pytest.raises(InputError, match="predictive"):
        rs.sample_chains({}, 10, predictive=True)
    with pytest.raises(InputError, match="predictive"):
        rs.importance_posterior({}, predictive=True)
    with pytest.raises(InputError, match="beta_interpolation"):
        rs.log_likelihood({"fsigma8": 0.47, "beta": 0.37, "sigma_v": 380, "epsilon": 1.0}, beta_interpolation="likelihood")
    import victor_amd
    with pytest.raises(InputError, match="broker"):
        victor_amd.CCFFit(*cases.boss_options("config"), broker="cuts-test").scale_cuts([ScaleCut()])
    with pytest.raises(InputError, match="leading axis"):
        rs.unflatten(np.zeros(3))
    assert rs.unflatten(np.zeros((2, 5))).shape == (2, 1, 5)


@pytest.mark.parametrize("fixed_cov", [False, True])
def test_cut_tables_are_the_inverse_and_log_dets_of_the_hand_sliced_covariance(fixed_cov):
    from victor_amd import ScaleCut
    from victor_amd.cuts import cut_tables, pack_cut_tables
    from victor_amd.engine import covariance_logdets
    fit = boss_fit(fixed_cov)
    raw = np.load(os.path.join(cases.GOLDEN, "boss", "cov_fixed.npy" if fixed_cov else "cov.npy"), allow_pickle=True).item()
    cov = np.asarray(raw["covmat"], dtype=float)
    mask = np.zeros(60, dtype=bool)
    mask[[0, 3, 4, 29, 30, 41, 58]] = True
    cuts = [ScaleCut(), ScaleCut(s_min=fit.s[7]), ScaleCut(poles=[0]), ScaleCut(s_min=fit.s[5], s_max=fit.s[5]), ScaleCut(mask=mask)]
    hand = [np.arange(60), np.r_[7:30, 37:60], np.arange(30), np.array([5, 35]), np.array([0, 3, 4, 29, 30, 41, 58])]
    tables = cut_tables(fit, cuts)
    assert [t.n for t in tables] == [60, 46, 30, 2, 7]
    for t, idx in zip(tables, hand):
        assert np.array_equal(t.idx, idx)
        sub = cov[np.ix_(idx, idx)][None] if fixed_cov else np.stack([c[np.ix_(idx, idx)] for c in cov])
        assert t.cov.tobytes() == np.ascontiguousarray(sub).tobytes()
        assert t.prec.tobytes() == np.linalg.inv(sub).tobytes()
        if fixed_cov:
            assert t.logdet is None and t.eig is None
        else:
            logdet, eig = covariance_logdets(sub, np.asarray(raw["beta"], dtype=float))
            assert t.logdet.tobytes() == logdet.tobytes() and t.eig.tobytes() == eig.tobytes()
    # the all-entries cut is the fit's own precision
    assert tables[0].prec.tobytes() == (fit.icov[None] if fixed_cov else fit.icov).tobytes()
    # ... and a cut's precision is NOT a sub-block of it
    assert not np.allclose(tables[1].prec[0], (fit.icov if fixed_cov else fit.icov[0])[np.ix_(hand[1], hand[1])], rtol=1e-3)
    # packed at the fixed strides of the full N
    nb = 0 if fixed_cov else len(raw["beta"])
    n_keep, index, prec, logdet, eig = pack_cut_tables(tables, 60, nb)
    assert n_keep.dtype == index.dtype == np.int32 and list(n_keep) == [60, 46, 30, 2, 7]
    assert index.shape == (5, 60) and prec.shape == (5, max(nb, 1), 3600)
    for k, t in enumerate(tables):
        assert np.array_equal(index[k, : t.n], t.idx) and not index[k, t.n:].any()
        assert prec[k, :, : t.n * t.n].tobytes() == t.prec.reshape(max(nb, 1), -1).tobytes() and not prec[k, :, t.n * t.n:].any()
        if nb:
            assert np.array_equal(logdet[k], t.logdet, equal_nan=True) and np.array_equal(eig[k, :, : t.n], t.eig)
    assert (logdet is None and eig is None) if fixed_cov else (logdet.shape == (5, nb) and eig.shape == (5, nb, 60))


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("fixed_cov", [False, True])
def test_cut_likelihood_of_the_all_entries_cut_is_the_oracle_likelihood(form, fixed_cov):
    """The same theory vector through the oracle's CCFFit.log_likelihood and through cut_likelihood with every entry kept: the
    same formulas on the same inverse, so the two differ by the rounding of one quadratic form each ((2 N + 5) u |r|^T |P| |r|,
    tests/tolerances._quadratic_bound) and of the log determinant (assert_same_lnl's offset term)."""
    from victor_amd import ScaleCut
    from victor_amd.cuts import cut_likelihood, cut_tables
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle as vo
    model, data = cases.boss_options("config")
    if fixed_cov:
        data["covariance_matrix"].update(data_file="boss/cov_fixed.npy", fixed_beta=True)
    data["likelihood"] = dict({"form": form}, **FORMS[form])
    import victor_amd
    fit = victor_amd.CCFFit(cases.clone(model), cases.clone(data))
    ofit = vo.OracleFit(model, data)
    tables = cut_tables(fit, [ScaleCut()])[0]
    g = np.asarray(fit.beta_ccf, dtype=float)
    rng = np.random.default_rng(11)
    for beta in (g[4], 0.5 * (g[9] + g[10]), g[0] - 0.01, 0.37, g[-1] + 0.02):
        d = ofit.data_vector(beta)
        theory = d + rng.normal(size=60) * np.sqrt(np.diag(fit.get_interpolated_covariance(beta)))
        ofit.theory_multipole_vector = lambda *a, _t=theory, **k: _t
        want = ofit.log_likelihood({"fsigma8": 0.47, "beta": beta, "sigma_v": 380.0, "epsilon": 1.0})
        got = cut_likelihood(fit, theory, d, beta, tables, fit.fit_options)
        r = np.abs(theory - d)
        bound = 2 * _quadratic_bound(r, np.abs(fit.get_interpolated_precision(beta)), np.zeros(60))
        assert np.isfinite(want[1]) and want[1] > 10
        assert_same_chi2(got[1], want[1], bound, what=f"cut_likelihood vs oracle, {form}")
        assert_same_lnl(got[0], want[0], bound, what=f"cut_likelihood vs oracle, {form}")


def test_cut_likelihood_counts_the_entries_kept_and_fails_where_the_reference_rule_does():
    from victor_amd import ScaleCut
    from victor_amd.cuts import cut_likelihood, cut_tables
    fit = boss_fit(fixed_cov=True)
    t16 = cut_tables(fit, [ScaleCut(s_min=fit.s[3], s_max=fit.s[10])])[0]
    assert t16.n == 16
    d = fit.multipole_datavector(0.37)
    theory = d + 0.01 * np.cos(np.arange(60))
    r = (theory - d)[t16.idx]
    chi2 = float(r @ np.linalg.inv(fit.covmat[np.ix_(t16.idx, t16.idx)]) @ r)
    hart = {"likelihood": {"form": "hartlap", "nmocks": 1000}}
    lnl, c = cut_likelihood(fit, theory, d, 0.37, t16, hart)
    assert c == chi2
    by_hand = -0.5 * chi2 * (982.0 / 999.0)                       # (1000 - 16 - 2) / (1000 - 1): n_k = 16, not N = 60
    assert abs(lnl - by_hand) <= 4 * U * abs(by_hand)
    assert abs(lnl - (-0.5 * chi2 * (938.0 / 999.0))) > 1e-3 * abs(lnl)
    perc = {"likelihood": {"form": "percival", "nmocks": 1000, "nparams": 4}}
    B = 982.0 / (983.0 * 980.0)
    m = 4 + 2 + (999.0 + B * 12.0) / (1 + B * 12.0)
    by_hand = -m * np.log(1 + chi2 / 999.0) / 2
    assert abs(cut_likelihood(fit, theory, d, 0.37, t16, perc)[0] - by_hand) <= 8 * U * abs(by_hand)
    # failures: a NaN in the theory vector; on a gridded covariance a NaN beta and a blend whose determinant is not positive
    bad = theory.copy()
    bad[t16.idx[3]] = np.nan
    assert cut_likelihood(fit, bad, d, 0.37, t16, hart) == (-np.inf, np.inf)
    bad = theory.copy()
    bad[0] = np.nan                                               # (an entry the cut drops does not fail it)
    assert cut_likelihood(fit, bad, d, 0.37, t16, hart) == (lnl, chi2)
    grid = boss_fit()
    tg = cut_tables(grid, [ScaleCut(poles=[0])])[0]
    assert cut_likelihood(grid, theory, d, np.nan, tg, hart) == (-np.inf, np.inf)
    g = np.asarray(grid.beta_covmat, dtype=float)
    flipped = cut_tables(grid, [ScaleCut(poles=[0])])[0]
    w, v = np.linalg.eigh(flipped.cov[-1])
    flipped.cov[-1] = flipped.cov[-1] - 2.0 * w[3] * np.outer(v[:, 3], v[:, 3])       # one negative eigenvalue: sign -1
    assert cut_likelihood(grid, theory, d, g[-1], flipped, hart) == (-np.inf, np.inf)
    assert np.isfinite(cut_likelihood(grid, theory, d, g[2], flipped, hart)[0])


def test_the_header_declares_vk_set_cuts_and_the_abi_version_stays():
    from victor_amd import _native as N
    with open(os.path.join(ROOT, "include", "victor_hip.h")) as fh:
        header = fh.read()
    assert "#define VK_ABI_VERSION 22\n" in header and N.VK_ABI_VERSION == 22
    assert ("int vk_set_cuts(vk_ctx* ctx, int32_t n_cuts, const int32_t* n_keep, const int32_t* index, const double* prec, "
            "const double* logdet,\n                const double* eig);") in header
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert N.SYMBOLS["vk_set_cuts"] == (C.c_int, [C.c_void_p, C.c_int32, ip, ip, dp, dp, dp])
