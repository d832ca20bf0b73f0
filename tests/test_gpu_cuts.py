"""Scale cuts on the GPU (victor_amd/cuts.py, vk_set_cuts, csrc/vk_kernel_real_cuts.h): K cuts x R realisations as K R problems.

1. the kernel against its NumPy definition (``cut_likelihood`` fed the device's own theory vectors and the same tables), at a
   bound formed per (point, cut, realisation) from the cut's blended |P| and the gathered r, tau and dd;
2. pairs mode returns the bits of cross mode for every (cut, realisation); the matrix-core and vector-ALU builds agree;
3. the all-entries cut against the plain realisation route;
4. s cuts against the route users take today: sliced files, a sliced ``CCFFit`` and its ``realisations()``;
5. residency: plain and cut objects on one engine, and the refusals, each leaving the context or handle usable;
6. every device loop against its own definition route, by the helper of that loop's own GPU test.
"""

import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

from tests import cases, tolerances
from tests import fit_definition as FD
from tests.test_chains import same_bytes
from tests.test_realisations import REAL, stack_options
from tests.tolerances import U, assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
PARAMS2 = {n: PARAMS[n] for n in ("fsigma8", "sigma_v")}              # d = 2
FIXED = {"beta": 0.37, "epsilon": 1.0}
FORMS = {"gaussian": {}, "sellentin": {"nmocks": 1000}, "hartlap": {"nmocks": 1000}, "percival": {"nmocks": 1000, "nparams": 4}}
NUMBERS = {1: [6], 5: [0, 1, 2, 3, 4], 16: list(range(16)), 18: list(range(16)) + [3, 9]}     # 18: two tiles, the second partial


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def stack_fit(fixed=False, form="gaussian"):
    import victor_amd
    model, data = stack_options(fixed=fixed)
    data["likelihood"] = dict({"form": form}, **FORMS[form])
    return victor_amd.CCFFit(model, data)


def five_cuts(fit):
    """n_k = 60 (all entries), 46 (Np 48: three row blocks), 30 (two row blocks), 16 (exactly one), 2 (heavy padding)."""
    from victor_amd import ScaleCut
    s = fit.s
    return [ScaleCut(), ScaleCut(s_min=s[7]), ScaleCut(poles=[0]), ScaleCut(s_min=s[3], s_max=s[10]), ScaleCut(s_min=s[5], s_max=s[5])]


def three_cuts(fit):
    from victor_amd import ScaleCut
    return [ScaleCut(), ScaleCut(s_min=fit.s[7]), ScaleCut(poles=[0])]


def rows_of(fit, n):
    """n rows of the prior box with a beta on a grid value, one between grid values, a NaN parameter and - at n = 70 - a beta
    below the grid and a NaN beta."""
    from victor_amd import _native as N
    g = np.load(os.path.join(REAL, "stack.npy"), allow_pickle=True).item()["beta"]
    hp = cases.halton_params(n, with_beta=True)
    hp["beta"][0] = g[4]
    hp["beta"][1] = 0.5 * (g[9] + g[10])
    if n > 3:
        hp["beta"][3] = g[0] - 0.01
    rows = np.array(fit._fit_rows(hp, fit.model), dtype=float)
    rows[2, N.P_FSIGMA8] = np.nan
    if n > 3:
        rows[6, N.P_BETA] = np.nan
    return rows


def cut_bounds(rs, rows):
    """(n, K R): (2 n_k + 5) u |r|^T |P_k| |r| + 2 (|P_k| |r|) . dd + 64 u |r|^T |P_k| (|r| + 2 tau) - the terms of
    tolerances._quadratic_bound and chi2_bound with the cut's blended |P| and the gathered r, tau and dd (the data's Horner
    rounding, 8 u sum_p |c_p| |db|^p; 0 for a fixed data vector).  0 where the row must fail."""
    from victor_amd import _native as N
    fit = rs.fit
    theory = fit.theory_vector_batch(rows)
    tau = tolerances._tau(fit)
    K, R = rs.shape
    out = np.zeros((len(rows), K * R))
    for p, row in enumerate(rows):
        beta = row[N.P_BETA]
        if not np.all(np.isfinite(theory[p])) or (not np.isfinite(beta) and not (fit.fixed_data and fit.fixed_covmat)):
            continue
        lo, w = (0, 0.0) if fit.fixed_covmat else fit._bracket(beta)
        for m in range(R):
            d = rs.data_at(m, beta)
            dd = np.zeros(len(d))
            if not fit.fixed_data:
                g = np.asarray(fit.beta_ccf, dtype=float)
                kb = max([i for i in range(1, len(g) - 1) if beta >= g[i]], default=0)
                c = np.abs(rs.blocks[m].reshape(len(g) - 1, -1, 4)[kb])
                dd = 8 * U * (c @ (abs(beta - g[kb]) ** np.arange(4)))
            for k, t in enumerate(rs.tables):
                absP = tolerances._blend_abs(t.prec, lo, w)
                r = np.abs(theory[p] - d)[t.idx]
                out[p, k * R + m] = tolerances._quadratic_bound(r, absP, dd[t.idx]) + 64 * U * (r @ absP @ (r + 2 * tau[t.idx]))
    return out


def against_definition(rs, rows, what):
    K, R = rs.shape
    lnl, chi2 = rs.log_likelihood(rows)
    want_l, want_c = rs.log_likelihood(rows, device=False)
    assert lnl.shape == chi2.shape == want_l.shape == want_c.shape == (len(rows), K, R)
    bound = cut_bounds(rs, rows).reshape(len(rows), K, R)
    failed = np.isposinf(want_c)
    assert np.array_equal(np.isposinf(chi2), failed) and np.array_equal(np.isneginf(lnl), failed), what
    assert np.array_equal(np.isneginf(want_l), failed) and np.all(np.isfinite(chi2[~failed])) and np.all(np.isfinite(lnl[~failed]))
    assert failed[2].all() and not failed[:2].any(), what                      # the NaN parameter; the rows in front of it
    assert_same_chi2(chi2, want_c, bound, what=f"cuts kernel vs definition, {what}")
    assert_same_lnl(lnl, want_l, bound, what=f"cuts kernel vs definition, {what}")
    return lnl, chi2


# ------------------------------------------------------------------ 1. the kernel against its definition -------------------------
@pytest.mark.parametrize("fixed, R, n, form", [(False, 1, 3, "gaussian"), (False, 5, 70, "hartlap"), (False, 16, 3, "percival"),
                                                 (False, 18, 70, "sellentin"), (True, 1, 70, "hartlap"), (True, 5, 3, "sellentin"),
                                                 (True, 16, 70, "gaussian"), (True, 18, 3, "percival")])
def test_kernel_against_its_definition(fixed, R, n, form):
    fit = stack_fit(fixed, form)
    rs = fit.realisations(NUMBERS[R]).scale_cuts(five_cuts(fit))
    assert len(rs) == 5 * R and rs.shape == (5, R) and [t.n for t in rs.tables] == [60, 46, 30, 16, 2]
    rows = rows_of(fit, n)
    lnl, chi2 = against_definition(rs, rows, f"{'fixed' if fixed else 'gridded'}, R = {R}, n = {n}, {form}")
    if n > 3 and not fixed:
        assert np.isposinf(chi2[6]).all() and np.isfinite(chi2[3]).all()          # the NaN beta; the beta below the grid
    if form in ("hartlap", "percival") and fixed:                                 # n_k enters, by hand (no log-det term): cut 3, n_k = 16
        ok = np.isfinite(chi2[:, 3, 0])
        c = chi2[ok, 3, 0]

        def by_hand(nd):
            if form == "hartlap":
                return -0.5 * c * (1000 - nd - 2) / 999.0
            B = (1000 - nd - 2) / ((1000 - nd - 1) * (1000 - nd - 4))
            return -(4 + 2 + (999.0 + B * (nd - 4)) / (1 + B * (nd - 4))) * np.log(1 + c / 999.0) / 2
        # hartlap: three roundings; percival: the logarithm of 1 + chi2 / 999 carries the rounding of its argument, u / log(1 + x),
        # below 100 u for chi2 > 10 as here, and each side its own two ulps of log
        assert np.all(c > 10)
        assert np.allclose(lnl[ok, 3, 0], by_hand(16), rtol=1e-14 if form == "hartlap" else 2e-14, atol=0)
        assert not np.allclose(lnl[ok, 3, 0], by_hand(60), rtol=1e-3)
    if R == 18:                                                                   # a repeated number: the same bits in both tiles
        assert same_bytes(chi2[:, :, 16], chi2[:, :, 3]) and same_bytes(lnl[:, :, 17], lnl[:, :, 9])


def test_three_multipoles_a_gather_with_holes_and_the_fit_as_one_block():
    """N = 120 (l = 0, 2, 4), R = 1 through ``fit.scale_cuts``: l = {0, 4} is a non-contiguous gather, the mask has holes."""
    import victor_amd
    from victor_amd import ScaleCut
    fit = victor_amd.CCFFit(*cases.synth_options(3))
    assert len(fit.s) * len(fit.poles_s) == 120
    mask = np.zeros(120, dtype=bool)
    mask[[0, 1, 5, 17, 39, 40, 47, 80, 81, 83, 119]] = True
    rs = fit.scale_cuts([ScaleCut(poles=[0, 4]), ScaleCut(mask=mask), ScaleCut(), ScaleCut(s_min=fit.s[11], poles=[2])])
    assert rs.shape == (4, 1) and [t.n for t in rs.tables] == [80, 11, 120, 29]
    hp = cases.halton_params(70)
    rows = np.array(fit._fit_rows(hp, fit.model), dtype=float)
    rows[2, 0] = np.nan
    lnl, chi2 = against_definition(rs, rows, "synthetic, N = 120, R = 1")
    plain = fit.log_likelihood_batch(rows)
    bound = chi2_bound(fit, rows, ulps=64)
    ok = np.isfinite(plain[1])
    assert_same_chi2(chi2[ok, 2, 0], plain[1][ok], bound[ok], what="synthetic all-entries cut vs the fit's own route")
    assert_same_lnl(lnl[ok, 2, 0], plain[0][ok], bound[ok], what="synthetic all-entries cut vs the fit's own route")


# ------------------------------------------------------------------ 2. pairs == cross; MFMA against the VALU twin --------------
def test_pairs_mode_has_the_bits_of_cross_mode_and_the_valu_twin_agrees():
    from victor_amd import _native as N
    fit = stack_fit()
    rs = fit.realisations(NUMBERS[18]).scale_cuts(three_cuts(fit))
    assert len(rs) == 54
    rows = rows_of(fit, 70)[:54]
    which = ((np.arange(54) * 7) % 54).astype(np.int32)                           # every (k, m) once
    assert len(set(which)) == 54
    cross = rs.log_likelihood(rows)
    pairs = rs.log_likelihood_pairs(rows, which)
    assert pairs[0].shape == pairs[1].shape == (54,)
    for got, full in zip(pairs, cross):
        assert same_bytes(got, full.reshape(54, 54)[np.arange(54), which])
    assert rs.fit._get_engine().last_instance().endswith("like_real_cuts<true>")
    bound = cut_bounds(rs, rows).reshape(54, 3, 18)
    try:
        N.set_knob("VICTOR_HIP_REAL_VALU", "1")
        valu = rs.log_likelihood(rows)
        assert rs.fit._get_engine().last_instance().endswith("like_real_cuts<false>")
        valu_pairs = rs.log_likelihood_pairs(rows, which)
    finally:
        N.set_knob("VICTOR_HIP_REAL_VALU", None)
    assert_same_chi2(valu[1], cross[1], bound, what="cuts kernel: VALU twin vs MFMA")
    assert_same_lnl(valu[0], cross[0], bound, what="cuts kernel: VALU twin vs MFMA")
    assert same_bytes(valu_pairs[1], valu[1].reshape(54, 54)[np.arange(54), which])
    from victor_amd import InputError
    with pytest.raises(InputError):
        rs.log_likelihood_pairs(rows, np.full(54, 54))


# ------------------------------------------------------------------ 3. the all-entries cut against the plain route -------------
@pytest.mark.parametrize("fixed", [False, True])
def test_all_entries_cut_against_the_plain_route(fixed):
    import victor_amd
    fit = stack_fit(fixed)
    plain = fit.realisations(NUMBERS[5])
    rs = plain.scale_cuts(three_cuts(fit))
    hp = cases.halton_params(70, with_beta=True)
    lnl, chi2 = rs.log_likelihood(hp)
    want_l, want_c = plain.log_likelihood(hp)
    for m in range(5):
        single = victor_amd.CCFFit(*stack_options(fixed=fixed, simulation_number=m))
        bound = chi2_bound(single, hp, ulps=64)
        assert_same_chi2(chi2[:, 0, m], want_c[:, m], bound, what="all-entries cut vs plain realisations")
        assert_same_lnl(lnl[:, 0, m], want_l[:, m], bound, what="all-entries cut vs plain realisations")
        single._engine = None
    assert not np.allclose(chi2[:, 1], chi2[:, 0], rtol=1e-3)


# ------------------------------------------------------------------ 4. s cuts against sliced files ----------------------------
@pytest.mark.parametrize("first, last", [(7, 29), (3, 10)])
def test_s_cuts_against_the_sliced_files_users_write_today(tmp_path, first, last):
    import victor_amd
    from victor_amd import ScaleCut
    fit = stack_fit()
    keep = np.arange(first, last + 1)
    idx = np.concatenate([keep, 30 + keep])
    stack = np.load(os.path.join(REAL, "stack.npy"), allow_pickle=True).item()
    cov = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    data_path, cov_path = str(tmp_path / "stack_cut.npy"), str(tmp_path / "cov_cut.npy")
    np.save(data_path, dict(stack, s=stack["s"][keep], monopole=stack["monopole"][..., keep], quadrupole=stack["quadrupole"][..., keep]),
            allow_pickle=True)
    np.save(cov_path, dict(cov, covmat=np.ascontiguousarray(cov["covmat"][:, idx][:, :, idx])), allow_pickle=True)

    def sliced(m):
        model, data = stack_options(data_file=data_path, simulation_number=m)
        data["covariance_matrix"]["data_file"] = cov_path
        data["likelihood"] = dict(fit.fit_options["likelihood"])
        return victor_amd.CCFFit(model, data)
    numbers = [0, 5, 11]
    rs = fit.realisations(numbers).scale_cuts([ScaleCut(), ScaleCut(s_min=fit.s[first], s_max=fit.s[last])])
    assert rs.tables[1].n == len(idx) and np.array_equal(rs.tables[1].idx, idx)
    hp = cases.halton_params(70, with_beta=True)
    lnl, chi2 = rs.log_likelihood(hp)
    want_l, want_c = sliced(0).realisations(numbers).log_likelihood(hp)
    for j, m in enumerate(numbers):
        single = sliced(m)
        bound = chi2_bound(single, hp)
        assert_same_chi2(chi2[:, 1, j], want_c[:, j], bound, what=f"s cut {first}..{last} vs sliced files")
        assert_same_lnl(lnl[:, 1, j], want_l[:, j], bound, what=f"s cut {first}..{last} vs sliced files")
        single._engine = None


# ------------------------------------------------------------------ 5. residency and refusals ---------------------------------
def raw_handle(entry, rs, n_rows_per_problem=1):
    """(lib, handle, names) of ``entry`` over the cut object's problems, as the drivers create it."""
    from victor_amd.fitting import _Sampled
    q = _Sampled("best_fit", "fitted", PARAMS2, FIXED)
    R = len(rs) * n_rows_per_problem
    x0 = np.tile(0.5 * (q.lo + q.hi), (R, 1))
    batch = dict(q.fixed_all)
    batch.update({n: np.ascontiguousarray(x0[:, j]) for j, n in enumerate(q.names)})
    which = (np.arange(R) // n_rows_per_problem).astype(np.int32)
    lib, h, _ = q.create(entry, rs.fit, rs, {}, q.fit_options(rs.fit, {}), batch, which)
    return lib, h, q, x0


def test_residency_on_one_engine():
    fit = stack_fit()
    plain = fit.realisations(NUMBERS[5])
    rs = plain.scale_cuts(three_cuts(fit))
    hp = cases.halton_params(16, with_beta=True)
    before = plain.log_likelihood(hp)
    cut = rs.log_likelihood(hp)
    after = plain.log_likelihood(hp)                                             # (clears the cuts: vk_set_realisations)
    assert before[0].shape == (16, 5) and cut[0].shape == (16, 3, 5)
    assert same_bytes(after[0], before[0]) and same_bytes(after[1], before[1])
    again = rs.log_likelihood(hp)                                                # ... and the reverse
    assert same_bytes(again[0], cut[0]) and same_bytes(again[1], cut[1])
    eng = fit._get_engine()
    assert eng.last_instance().endswith("like_real_cuts<true>")
    eng.set_cuts()                                                               # released: the uncut values of the same blocks
    l, c = eng.eval_realisations(eng.make_opts(fit.model, fit.fit_options), fit._fit_rows(hp, fit.model), 5)
    assert same_bytes(l, before[0]) and same_bytes(c, before[1])
    eng._real_owner = None
    # an index past the problems; indices that do not increase
    from victor_amd import InputError
    with pytest.raises(InputError, match="outside 0..14|out of range"):
        rs.log_likelihood_pairs(hp, np.full(16, 15))
    n_keep, index, prec, logdet, eig = rs._packed
    bad = index.copy()
    bad[1, 3] = bad[1, 2]
    with pytest.raises(InputError, match="increase strictly"):
        eng.set_cuts(n_keep, bad, prec, logdet, eig)
    eng._real_owner = None
    assert same_bytes(rs.log_likelihood(hp)[1], cut[1])                          # the context is usable after the refusal


def test_cuts_and_table_sets_refuse_each_other(tmp_path):
    import victor_amd
    from victor_amd import InputError
    from tests.test_paired_realisations import NUMBERS as PAIRED, paired_boss_options
    fit = victor_amd.CCFFit(*paired_boss_options(tmp_path))
    paired = fit.realisations(PAIRED, paired_model=True)
    with pytest.raises(InputError, match="paired_model"):
        paired.scale_cuts(three_cuts(fit))
    hp = cases.halton_params(6, with_beta=True)
    which = np.arange(6) % 3
    want = paired.log_likelihood_pairs(hp, which)                               # the sets are resident now
    eng = fit._get_engine()
    rs = fit.realisations(PAIRED).scale_cuts(three_cuts(fit))
    with pytest.raises(InputError, match="vk_set_model_realisations"):
        eng.set_cuts(*rs._packed)
    assert same_bytes(paired.log_likelihood_pairs(hp, which)[1], want[1])
    cut = rs.log_likelihood(hp)                                                  # clears the sets, then sets the cuts
    with pytest.raises(InputError, match="vk_set_cuts"):
        eng.set_model_realisations(*paired._sets_of[id(eng)])
    assert same_bytes(rs.log_likelihood(hp)[1], cut[1])
    eng.set_cuts()
    with pytest.raises(InputError, match="vk_set_realisations comes first|no realisations"):
        fresh = victor_amd.CCFFit(*stack_options())
        fresh._get_engine().set_cuts(*rs._packed)


def test_refusals_leave_the_handle_usable():
    from victor_amd import _native as N
    fit = stack_fit()
    rs = fit.realisations(NUMBERS[5]).scale_cuts(three_cuts(fit))
    dp, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    # Fisher on a best-fit handle
    lib, h, q, x0 = raw_handle("vk_fit_create", rs)
    try:
        d = len(q.names)
        steps = np.tile(0.01 * (q.hi - q.lo), (15, 1))
        out = [np.empty((15, d, d)) for _ in range(3)]
        c, status = C.c_double(), np.empty(15, dtype=np.int32)
        rc = lib.vk_fit_fisher(h, N.as_dp(N.f64(x0)), N.as_dp(N.f64(steps)), None, *[N.as_dp(a) for a in out], C.byref(c), status.ctypes.data_as(i32))
        assert rc == -1 and "vk_set_cuts" in lib.vk_fit_last_error(h).decode()
        x, lnl, chi2 = np.empty((15, d)), np.empty(15), np.empty(15)
        n_iter, n_evals = np.empty(15, dtype=np.int32), np.empty(15, dtype=np.int64)
        rc = lib.vk_fit_run(h, N.as_dp(N.f64(x0)), N.as_dp(N.f64(steps[0])), N.as_dp(N.f64(1e-3 * steps[0])), 1e-6, 5, 0, N.as_dp(x),
                            N.as_dp(lnl), N.as_dp(chi2), status.ctypes.data_as(i32), n_iter.ctypes.data_as(i32),
                            n_evals.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == 0 and np.all(np.isfinite(lnl)), lib.vk_fit_last_error(h)
    finally:
        lib.vk_fit_destroy(h)
    # predictive sums on a chain handle
    lib, h, q, x0 = raw_handle("vk_chain_create", rs, 2)
    try:
        assert lib.vk_chain_set_predictive(h, 1) == -1 and "vk_set_cuts" in lib.vk_chain_last_error(h).decode()
        assert lib.vk_chain_set_predictive(h, 0) == 0
        assert lib.vk_chain_start(h, N.as_dp(N.f64(x0))) == 0, lib.vk_chain_last_error(h)
    finally:
        lib.vk_chain_destroy(h)
    # predictive sums on an importance handle
    from tests.test_gpu_importance import G23, Handle
    ih = Handle(fit, PARAMS2, ["fsigma8", "sigma_v"], realisations=rs, fixed=FIXED)
    try:
        assert ih.lib.vk_is_set_predictive(ih.h, 1) == -1 and "vk_set_cuts" in ih.error()
        assert ih.run(0, G23) == 0, ih.error()
    finally:
        ih.close()
    # the beta blend at create of a handle over realisations; joint evaluations against realisations
    from victor_amd.fitting import _Sampled
    from victor_amd import InputError
    qq = _Sampled("best_fit", "fitted", PARAMS2, FIXED)
    with pytest.raises(InputError, match="beta_interpolation"):
        rs.best_fit(PARAMS2, fixed=FIXED, beta_interpolation="likelihood")
    eng = fit._get_engine()
    opts = eng.make_opts(fit.model, fit.fit_options)
    opts.reserved |= 1                                                            # VK_OPT_BETA_BLEND
    err = C.create_string_buffer(512)
    cols = np.array([N.ROW_COLUMNS[n] for n in qq.names], dtype=np.int32)
    base = np.ascontiguousarray(fit._fit_rows(dict(FIXED, fsigma8=np.full(15, 0.45), sigma_v=np.full(15, 380.0)), fit.model))
    which = np.arange(15, dtype=np.int32)
    h = eng._lib.vk_fit_create(eng._ctx, C.byref(opts), 15, 2, cols.ctypes.data_as(i32), N.as_dp(N.f64(qq.lo)), N.as_dp(N.f64(qq.hi)),
                               N.as_dp(base), 1.0, which.ctypes.data_as(i32), err, len(err))
    assert not h and "vk_set_cuts" in err.value.decode()
    ctxs = (C.c_void_p * 1)(eng._ctx)
    plain = eng.make_opts(fit.model, fit.fit_options)
    h = eng._lib.vk_fit_create_joint(ctxs, 1, None, C.byref(plain), 15, 2, cols.ctypes.data_as(i32), N.as_dp(N.f64(qq.lo)),
                                     N.as_dp(N.f64(qq.hi)), N.as_dp(base), 1.0, which.ctypes.data_as(i32), err, len(err))
    assert not h and "vk_set_cuts" in err.value.decode()
    # ... while the same calls over the context's own data vector are served: they read nothing the cuts changed
    assert eng._lib.vk_joint_eval_device_async(ctxs, 1, C.byref(plain), None, 0, None, None, None) == 0
    h = eng._lib.vk_fit_create(eng._ctx, C.byref(opts), 15, 2, cols.ctypes.data_as(i32), N.as_dp(N.f64(qq.lo)), N.as_dp(N.f64(qq.hi)),
                               N.as_dp(base), 1.0, None, err, len(err))
    assert h, err.value.decode()
    eng._lib.vk_fit_destroy(h)
    hp = cases.halton_params(4, with_beta=True)
    assert np.all(np.isfinite(rs.log_likelihood(hp)[1]))                          # the context is usable


def test_the_fit_s_own_routes_do_not_notice_resident_cuts():
    """The cuts stay resident on the fit's engine after a ``CutRealisations`` call.  Everything over the fit's own data vector -
    its Fisher forecast, predictive sums from chains and from an importance sample, the loops of a ``beta_interpolation:
    likelihood`` fit, a plain ``JointFit`` over it - creates handles without realisation indices and returns the bytes it
    returned before."""
    import victor_amd
    from tests.test_gpu_importance_predictive import proposal
    from victor_amd.joint import JointFit
    names = ["fsigma8", "sigma_v"]
    at = {"fsigma8": 0.47, "sigma_v": 380.0}
    hp = cases.halton_params(16, with_beta=True)

    def own_routes(fit, other):
        fi = fit.fisher(PARAMS2, at, fixed=FIXED)
        ch = fit.sample_chains(PARAMS2, 40, walkers=4, seed=1, fixed=FIXED, predictive=True)
        ip = fit.importance_posterior(PARAMS2, proposal(names), n=128, seed=3, fixed=FIXED, min_ess=2.0, predictive=True)
        jl = JointFit([fit, other]).log_likelihood_batch(hp)
        return [fi.fisher, fi.cov, ch.chain, ch.predictive.mean, ch.predictive.mean_chi2, ip.ln_evidence, ip.predictive.mean_chi2,
                ip.predictive.dic, jl[0], jl[1]]
    fit, other = stack_fit(), stack_fit()
    before = own_routes(fit, other)
    cr = fit.scale_cuts(three_cuts(fit))
    cut = cr.log_likelihood(hp)
    assert fit._get_engine().last_instance().endswith("like_real_cuts<true>")          # resident now, and they stay
    after = own_routes(fit, other)
    assert len(before) == len(after) == 10
    for i, (a, b) in enumerate(zip(before, after)):
        assert same_bytes(np.asarray(a), np.asarray(b)), i
    assert same_bytes(cr.log_likelihood(hp)[1], cut[1])                                 # (still resident: no re-upload was needed)
    # a fit whose own option is 'likelihood': chi_squared of its cut object uploads the cuts; its blended loops go on
    model, data = stack_options()
    blend = victor_amd.CCFFit(model, dict(data, beta_interpolation="likelihood"))
    kw = dict(fixed=dict(FIXED, beta=0.3712), max_iter=40)
    bf0 = blend.best_fit(PARAMS2, **kw)
    c = blend.scale_cuts(three_cuts(blend)).chi_squared(hp)
    assert c.shape == (16, 3, 1) and np.all(np.isfinite(c))
    bf1 = blend.best_fit(PARAMS2, **kw)
    assert same_bytes(bf0.x, bf1.x) and same_bytes(bf0.lnl, bf1.lnl) and same_bytes(bf0.chi2, bf1.chi2)


# ------------------------------------------------------------------ 6. the device loops ---------------------------------------
@pytest.fixture(scope="module")
def rs15():
    """K = 3 cuts x R = 5 mocks: 15 problems, not a multiple of the tile."""
    fit = stack_fit()
    return fit.realisations(NUMBERS[5]).scale_cuts(three_cuts(fit))


class Flat:
    """The cut object as the helpers of the importance tests address a ``Realisations``: ``log_likelihood`` with the problem
    axis flat."""

    def __init__(self, rs):
        self.fit, self.numbers = rs.fit, rs.numbers
        self.log_likelihood = rs._cross
        self.log_likelihood_pairs = rs.log_likelihood_pairs
        self.importance_posterior = rs.importance_posterior


def test_best_fit_is_its_definition_route(rs15):
    from tests.test_gpu_fit_definition import same_fit
    kw = dict(fixed=FIXED, restarts=1)
    ref = FD.best_fit(rs15, PARAMS2, **kw)
    dev = rs15.best_fit(PARAMS2, covariance=True, **kw)
    assert dev.names == ref.names == ["fsigma8", "sigma_v"] and ref.x.shape == (15, 2)
    assert np.all(ref.status == FD.ST_CONVERGED)
    same_fit(dev, ref, "best fits under cuts")
    x = rs15.unflatten(dev.x)
    assert x.shape == (3, 5, 2) and not np.allclose(x[0], x[2], rtol=1e-6)        # the cuts move the best fit
    assert dev.cov.shape == (15, 2, 2) and dev.sigma.shape == (15, 2) and np.isfinite(dev.sigma).any()
    lap = rs15.laplace(PARAMS2, dev, fixed=FIXED)
    assert lap.cov.shape == (15, 2, 2) and np.array_equal(np.isfinite(lap.cov), np.isfinite(dev.cov))


@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_chains_are_their_definition_route(rs15, move):
    from tests.test_gpu_chains import same_walk
    from tests.test_gpu_stretch import RUN, same_run
    if move == "stretch":
        ref = rs15.sample_chains(PARAMS2, 40, device=False, fixed=FIXED, **RUN)
        dev = rs15.sample_chains(PARAMS2, 40, fixed=FIXED, **RUN)
        same_run(dev, ref, "stretch ensembles under cuts")
    else:
        kw = dict(walkers=4, seed=2, fixed=FIXED)
        ref = rs15.sample_chains(PARAMS2, 80, device=False, **kw)
        dev = rs15.sample_chains(PARAMS2, 80, marginals=True, autocorr=True, **kw)
        assert dev.chain.shape == (80, 15, 4, 2) and 0.02 < ref.acceptance.mean() < 0.98
        same_walk(dev, ref, "Metropolis chains under cuts")
        assert same_bytes(dev.lnl_chain, ref.lnl_chain) and same_bytes(dev.chi2_chain, ref.chi2_chain)
        assert dev.marginals is not None and dev.autocorr is not None
    assert len({float(v) for v in dev.lnl[:, 0]}) == 15


def test_tempered_chains_run_under_cuts(rs15):
    kw = dict(walkers=4, seed=2, fixed=FIXED, temper={"rungs": 3})
    ref = rs15.sample_chains(PARAMS2, 30, device=False, **kw)
    dev = rs15.sample_chains(PARAMS2, 30, **kw)
    assert same_bytes(dev.chain, ref.chain) and same_bytes(dev.lnl_chain, ref.lnl_chain)


def test_nested_sampling_is_its_definition_route(rs15):
    from tests.test_gpu_nested import SMALL, both, exercised
    dev, ref = both(rs15, PARAMS2, "nested sampling under cuts", fixed=FIXED, **SMALL)
    exercised(ref, "nested sampling under cuts")
    assert dev.ln_evidence.shape == (15,) and len(set(dev.ln_evidence)) == 15


def test_grid_posterior_is_its_definition_route(rs15):
    from tests.test_gpu_grid import both_routes
    dev, ref = both_routes(rs15, PARAMS2, "grid 8 x 8 under cuts", bins=8, fixed=FIXED, ranges={"fsigma8": (0.35, 0.6), "sigma_v": (300.0, 460.0)},
                           pairs=[("fsigma8", "sigma_v")])
    assert dev.n_problems == 15 and np.all(dev.status == dev.OK) and len(set(dev.ln_max)) == 15


def test_importance_posterior_is_its_definition_route_and_the_all_entries_cut_is_the_plain_object(rs15):
    from tests.test_gpu_importance_predictive import proposal
    from tests.test_gpu_importance_tail import both_routes
    names = ["fsigma8", "sigma_v"]
    kw = dict(fixed=FIXED, n=512, seed=3, chunk=64, bins=6, min_ess=2.0)
    dev, ref = both_routes(Flat(rs15), PARAMS2, "importance sample of 512 under cuts", None, q=proposal(names), **kw)
    assert dev.n_problems == 15 and dev.mean.shape == (15, 2) and dev.tail is not None
    plain = rs15.fit.realisations(NUMBERS[5]).importance_posterior(PARAMS2, proposal(names), tail=True, **kw)
    assert plain.n_problems == 5 and plain.n_inside == dev.n_inside
    for name in ("ln_evidence", "ess", "mean", "sigma"):
        assert np.allclose(getattr(dev, name)[:5], getattr(plain, name), rtol=1e-9, atol=1e-12), name
        assert np.allclose(getattr(dev.tail, name)[:5], getattr(plain.tail, name), rtol=1e-9, atol=1e-12), name
    assert rs15.unflatten(dev.sigma).shape == (3, 5, 2)
    # a proposal per problem
    from victor_amd import ProposalSet
    bf = rs15.best_fit(PARAMS2, fixed=FIXED, covariance=True)
    own = rs15.importance_posterior(PARAMS2, ProposalSet.from_fits(bf, bf.laplace), n=128, seed=1, fixed=FIXED, min_ess=2.0)
    assert own.n_problems == 15 and np.all(np.isfinite(own.ln_evidence))
