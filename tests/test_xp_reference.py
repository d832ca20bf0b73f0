"""The extended-precision evaluation of the table contract (tests/xp_reference.py) on the CPU: against the FP64 oracle and the
reference's goldens at the 1e-10 end-to-end budget ("accuracy budget"), for every matter model of
victor_amd/velocity_tables.py, and the refined tables of the fast kernels against the vk_pp cubics at the bound
tests/tolerances.py assumes for them.  No GPU: the tables are host-built (engine.build_tables)."""

import os
import sys

import numpy as np
import pytest

from tests import cases
from tests import kernel_matrix as KM
from tests import xp_reference as X
from tests.tolerances import ULP, XP_TABLE_ULPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = 1e-10


@pytest.fixture(scope="module")
def vo():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import victor_oracle
    return victor_oracle


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    return str(tmp_path_factory.mktemp("xp_cpu"))


def _same(xp_t, want, what):
    xp_t = np.asarray(xp_t, dtype=float)
    want = np.asarray(want, dtype=float)
    assert np.max(np.abs(xp_t - want)) <= BUDGET * np.max(np.abs(want)), (what, float(np.max(np.abs(xp_t - want))))


def _against_oracle(fit, ora, rows, params, kw, what):
    """xp's theory vector, chi2 and lnL against the oracle's at BUDGET."""
    xp = X.XP(fit, kw)
    lnl, chi, th = xp.log_likelihood(rows)
    for i, p in enumerate(params):
        to = ora.theory_multipole_vector(ora.s, dict(p), ora.poles_s, **kw)
        _same(th[i], to, (what, i))
        lo, co = ora.log_likelihood(dict(p), **kw)
        assert abs(float(chi[i]) / co - 1) <= BUDGET, (what, i, float(chi[i]), co)
        assert abs(float(lnl[i]) - lo) <= BUDGET * (abs(lo) + co), (what, i, float(lnl[i]), lo)


def _recipe_cases():
    seen = {}
    for key, rc in KM.RECIPES.items():
        if rc.api == "xi":
            continue
        kws = [rc.kw] + ([dict(rc.kw, rsd_model="euclid_special")] if ",kaiser," in key else [])
        for kw in kws:
            seen.setdefault((rc.setup, tuple(sorted(kw.items()))), key)
    return sorted(seen.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("case", [c for c, _ in _recipe_cases()], ids=[k for _, k in _recipe_cases()])
def test_xp_against_the_oracle_on_every_recipe(case, vo, scratch):
    """The CPU-buildable inputs of every recipe of tests/kernel_matrix.py (KM.options, KM.points): one point each, the third
    (beta on a table knot) where the tables depend on beta."""
    import victor_amd
    st, kw = case
    kw = dict(kw)
    model, data = KM.options(st, scratch)
    fit = victor_amd.CCFFit(model, data)
    ora = vo.OracleFit(model, data)
    p = KM.points(fit, 3)
    i = 2 if not (fit.fixed_real_input and fit.fixed_data) else 0
    q = cases.point(p, i)
    rows = fit._fit_rows(p, fit._merged(kw))[i:i + 1]
    _against_oracle(fit, ora, rows, [q], kw, (st, kw))


def test_xp_against_the_reference_goldens():
    """The reference's outputs (tests/golden/ref_outputs.npz) on the BOSS configuration: theory vectors, chi2 and lnL of the default options, dispersion / kaiser / euclid_special / kaiser_approximation, the
    anisotropic sum, linear_bias (beta-dependent velocity tables) and empirical_corr."""
    import victor_amd
    g, meta = cases.golden_outputs()
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    pts = meta["boss_points"]
    rows = np.concatenate([fit._fit_rows(dict(q), fit.model) for q in pts])
    lnl, chi, th = X.XP(fit).log_likelihood(rows)
    _same(th, g["boss_config_theory"], "boss config")
    assert np.max(np.abs(chi.astype(float) / g["boss_config_chi2"] - 1)) <= BUDGET
    assert np.max(np.abs(lnl.astype(float) - g["boss_config_lnl"]) / (np.abs(g["boss_config_lnl"]) + g["boss_config_chi2"])) <= BUDGET
    for rsd in ("dispersion", "kaiser", "euclid_special"):
        kw = {"rsd_model": rsd}
        r3 = np.concatenate([fit._fit_rows(dict(q), fit._merged(kw)) for q in pts[:3]])
        _same(X.XP(fit, kw).theory(r3, sens=False).t, g[f"boss_{rsd}_theory"], rsd)
    kw = {"rsd_model": "kaiser", "kaiser_approximation": True}
    r3 = np.concatenate([fit._fit_rows(dict(q, M=1.1, Q=0.9), fit._merged(kw)) for q in pts[:3]])
    _same(X.XP(fit, kw).theory(r3, sens=False).t, g["boss_kaiser_approx_theory"], "kaiser_approximation")
    kw = {"assume_isotropic": False}
    r3 = np.concatenate([fit._fit_rows(dict(q), fit._merged(kw)) for q in pts[:3]])
    _same(X.XP(fit, kw).theory(r3, sens=False).t, g["boss_aniso_theory"], "anisotropic")
    # matter models and empirical_corr on the beta-dependent BOSS tables (test_oracle_golden.py: opt_boss_*)
    opt = {"lb": dict(matter_model="linear_bias"), "emp": dict(empirical_corr=True),
           "lb_emp": dict(matter_model="linear_bias", empirical_corr=True)}
    rsd = {"stream": {}, "disp": dict(rsd_model="dispersion"), "kaiser": dict(rsd_model="kaiser")}
    bpts = [dict(q, bias=2.1, Av=0.7, M=1.05, Q=0.95) for q in pts[:3]]
    checked = 0
    for b, bkw in opt.items():
        for r, rkw in rsd.items():
            key = f"opt_boss_{b}_{r}"
            if key not in g:
                continue
            kw = dict(bkw, **rkw)
            r3 = np.concatenate([fit._fit_rows(dict(q), fit._merged(kw)) for q in bpts])
            _same(X.XP(fit, kw).theory(r3, sens=False).t, g[key], key)
            checked += 1
    assert checked >= 4


@pytest.mark.parametrize("case", sorted(cases.SHIPPED_COMBINATIONS))
def test_xp_against_the_shipped_combination_goldens(case, tmp_path):
    """tests/golden/ref_outputs_more.npz: the remaining shipped file combinations, two likelihood forms."""
    import victor_amd
    g, meta = cases.golden_outputs("more")
    model, data, kw = cases.shipped_combination(case, tmp_path)
    fit = victor_amd.CCFFit(model, data)
    pts = meta["boss_points"][:4]
    rows = np.concatenate([fit._fit_rows(dict(q), fit._merged(kw)) for q in pts])
    th = X.XP(fit, kw).theory(rows, sens=False).t
    _same(th, g[f"{case}_theory"][:4], case)
    for form in ("sellentin", "gaussian"):
        kf = dict(kw, likelihood={"form": form, "nmocks": 1000, "nparams": 4})
        lnl, chi = X.chi2_from_theory(fit, th, rows, kf)
        assert np.max(np.abs(chi.astype(float) / g[f"{case}_{form}_chi2"][:4] - 1)) < BUDGET, form
        assert np.max(np.abs(lnl.astype(float) / g[f"{case}_{form}_lnl"][:4] - 1)) < BUDGET, form


def _matter_cases(tmp):
    from tests.test_host import _aniso_inputs
    boss = cases.boss_options("config")
    synth = cases.synth_options(3)
    model, data = _aniso_inputs(tmp)
    model["velocity_pdf"]["mean"]["model"] = "template"
    model["velocity_pdf"]["dispersion"] = {"model": "template", "template_keys": ["rsv", "sigmav"]}
    return {"template": (synth, {}), "linear_bias_fixed": (synth, {"matter_model": "linear_bias"}),
            "linear_bias_beta": (boss, {"matter_model": "linear_bias"}),
            "linear_bias_beta_empirical": (boss, {"matter_model": "linear_bias", "empirical_corr": True}),
            "velocity_template": ((model, data), {}), "empirical_corr": (synth, {"empirical_corr": True}),
            "empirical_corr_beta": (boss, {"empirical_corr": True})}


@pytest.mark.parametrize("rsd", ["streaming", "dispersion", "kaiser"])
@pytest.mark.parametrize("matter", ["template", "linear_bias_fixed", "linear_bias_beta", "linear_bias_beta_empirical",
                                    "velocity_template", "empirical_corr", "empirical_corr_beta"])
def test_velocity_tables_of_every_matter_model(matter, rsd, vo, tmp_path):
    """victor_amd/velocity_tables.py on its own: V1 / Da / V2 / Ge1 / Ge2, the linear-bias maps and the degree-6 beta tables of
    the empirical branch, read by xp exactly as the kernels read them, against the oracle's own construction at BUDGET."""
    import victor_amd
    (model, data), kw = _matter_cases(tmp_path)[matter]
    kw = dict(kw, rsd_model=rsd)
    fit = victor_amd.CCFFit(model, data)
    ora = vo.OracleFit(model, data)
    hp = cases.halton_params(4, with_beta=True)
    pts = [dict(cases.point(hp, i), bias=1.9, Av=0.6, M=1.05, Q=0.9) for i in (1, 3)]
    rows = np.concatenate([fit._fit_rows(dict(q), fit._merged(kw)) for q in pts])
    _against_oracle(fit, ora, rows, pts, kw, (matter, rsd))


# --------------------------------------------------------------------------------------------------- refined tables
def _uni_pieces(t, xp):
    """(left, width) of every interval of the refined grid."""
    if t.uni_lut_n:
        k = np.ctypeslib.as_array(t.uni_knots, shape=(t.uni_n + 1,)).astype(float)
        return k[:-1], np.diff(k)
    h = 1.0 / t.uni_inv_h
    return t.uni_u0 + h * np.arange(t.uni_n), np.full(t.uni_n, h)


@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("empirical", [False, True])
def test_refined_tables_reproduce_the_vk_pp_cubics(grid, empirical, scratch):
    """uni_xi, uni_xic, uni_sv_v, uni_v2, uni_da, uni_ge of the lattice (grid 0) and union-grid (grid 1) forms, at 8 points of
    every refined interval, against the vk_pp table xp reads: within XP_TABLE_ULPS ulps of the local magnitude - the largest
    |value| on the interval and its two neighbours (a narrow union-grid interval where V2 = r Delta delta crosses zero holds
    values far below the rounding of the cubic it was cut from); for xi^r at least 1, since the kernels sum (1 + xi^r) times the Gaussian weight and
    tests/tolerances.py charges the table error to that magnitude - the assumption XP_FAMILIES makes for the fast kernels."""
    import victor_amd
    from victor_amd import engine as E
    st = KM.Setup(nlr=3, nl=3, grid=grid)
    fit = victor_amd.CCFFit(*KM.options(st, scratch))
    kw = {"empirical_corr": empirical}
    xp = X.XP(fit, kw)
    t, keep = E.build_tables(fit, fit, fit._engine_key(fit._merged(kw)), fit._simpson_rule(fit.model["simpson_even"]))
    assert t.uni_n > 0
    left, width = _uni_pieces(t, xp)
    tau = np.linspace(0, 1, 8, endpoint=False)
    U = left[:, None] + width[:, None] * tau[None, :]                   # (uni_n, 8)
    lim = XP_TABLE_ULPS * ULP
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).astype(np.longdouble)     # noqa: E731

    def check(coef, ref, what, mask=None, floor=0.0):
        got = X._horner(coef[:, None, :], tau.astype(np.longdouble)[None, :])      # (uni_n, 8)
        mask = np.ones(ref.shape, bool) if mask is None else mask
        loc = np.max(np.where(mask, np.abs(ref), 0), axis=1)
        loc = np.maximum(loc, np.maximum(np.r_[loc[1:], 0], np.r_[0, loc[:-1]]))      # with the two neighbouring intervals
        mag = np.maximum(loc, floor)[:, None]
        bad = mask & (np.abs(got - ref) > lim * np.maximum(mag, np.finfo(float).tiny))
        assert not bad.any(), (what, float(np.max(np.abs(got - ref) / mag)) / ULP, np.argwhere(bad)[:3])

    xi, vr = xp.point_tables(0.4)
    Ul = U.astype(np.longdouble)
    # below a table's first knot the refined records hold its boundary value (the kernels clamp there)
    nl = t.n_ell_r
    uxi = arr(t.uni_xi, nl * t.uni_n * 4).reshape(nl, t.uni_n, 4)
    for l in range(nl):
        check(uxi[l], xi(l, Ul), f"uni_xi[{l}]", floor=1.0)
    uxc = arr(t.uni_xic, nl * t.uni_n * 4).reshape(nl, t.uni_n, 4)
    x0, x2, x4 = xi(0, Ul), xi(1, Ul), xi(2, Ul)
    for l, ref in enumerate([x0 - x2 / 2 + 3 * x4 / 8, 3 * x2 / 2 - 15 * x4 / 4, 35 * x4 / 8]):
        check(uxc[l], ref, f"uni_xic[{l}]", floor=1.0)
    svv = arr(t.uni_sv_v, t.uni_n * 8).reshape(t.uni_n, 2, 4)
    check(svv[:, 0], xp.sv(0, Ul), "uni_sv_v sigma_v")
    inside = Ul >= xp.vr_knots[0]                                         # V is never evaluated below u = 0.01
    check(svv[:, 1], vr(0, Ul), "uni_sv_v V1", inside)
    check(arr(t.uni_v2, t.uni_n * 4).reshape(t.uni_n, 4), vr(2, Ul), "uni_v2", inside)
    check(arr(t.uni_da, t.uni_n * 4).reshape(t.uni_n, 4), vr(1, Ul), "uni_da", inside)
    ge = arr(t.uni_ge, t.uni_n * 8).reshape(2, t.uni_n, 4)
    check(ge[0], vr(3, Ul), "uni_ge[0]", inside)
    check(ge[1], vr(4, Ul), "uni_ge[1]", inside)


@pytest.mark.parametrize("kw", [{}, {"empirical_corr": True, "rsd_model": "dispersion"}, {"matter_model": "linear_bias"}],
                         ids=["default", "linear_bias_empirical_dispersion", "linear_bias"])
def test_refined_beta_forms_reproduce_the_vk_pp_cubics(kw):
    """The beta forms of the refined tables on the BOSS tables (31 beta knots): uni_xi / uni_xic [l][k][i][4][4], uni_vb and
    uni_dab [k][i][4][4], uni_empb [3][k][i][4][7], evaluated at a knot, midway between two knots and outside both ends of
    the grid, against the vk_pp tables xp builds at that beta - the same bound as the fixed forms."""
    import victor_amd
    from victor_amd import engine as E
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    xp = X.XP(fit, kw)
    t, keep = E.build_tables(fit, fit, fit._engine_key(fit._merged(kw)), fit._simpson_rule(fit.model["simpson_even"]))
    assert t.uni_n > 0 and t.n_beta_r > 2
    nb, n = t.n_beta_r, t.uni_n
    left, width = _uni_pieces(t, xp)
    tau = np.linspace(0, 1, 8, endpoint=False)
    Ul = (left[:, None] + width[:, None] * tau[None, :]).astype(np.longdouble)
    inside = Ul >= xp.vr_knots[0]
    lim = XP_TABLE_ULPS * ULP
    arr = lambda p, m: np.ctypeslib.as_array(p, shape=(m,)).astype(np.longdouble)     # noqa: E731
    g = np.asarray(fit.beta, float)
    checked = 0
    for beta in (g[nb // 2], 0.5 * (g[3] + g[4]), g[0] - 0.03, g[-1] + 0.03):
        k, db = xp.beta_piece(xp.beta_r, np.longdouble(beta))
        xi, vr = xp.point_tables(beta)

        def check(coef_beta, ref, what, mask=None, floor=0.0):
            coef = X._horner(coef_beta, db)                                   # [..., 4] in powers of tau
            got = X._horner(coef[:, None, :], tau.astype(np.longdouble)[None, :])
            mask = np.ones(ref.shape, bool) if mask is None else mask
            loc = np.max(np.where(mask, np.abs(ref), 0), axis=1)
            loc = np.maximum(loc, np.maximum(np.r_[loc[1:], 0], np.r_[0, loc[:-1]]))
            mag = np.maximum(loc, floor)[:, None]
            bad = mask & (np.abs(got - ref) > lim * np.maximum(mag, np.finfo(float).tiny))
            assert not bad.any(), (what, beta, float(np.max(np.where(mask, np.abs(got - ref), 0) / mag)) / ULP)

        nl = t.n_ell_r
        uxi = arr(t.uni_xi, nl * (nb - 1) * n * 16).reshape(nl, nb - 1, n, 4, 4)[:, k]
        for l in range(nl):
            check(uxi[l], xi(l, Ul), f"uni_xi[{l}]", floor=1.0)
        if nl > 1:
            uxc = arr(t.uni_xic, nl * (nb - 1) * n * 16).reshape(nl, nb - 1, n, 4, 4)[:, k]
            x0, x2 = xi(0, Ul), xi(1, Ul)
            x4 = xi(2, Ul) if nl > 2 else 0 * x0
            for l, ref in enumerate([x0 - x2 / 2 + 3 * x4 / 8, 3 * x2 / 2 - 15 * x4 / 4, 35 * x4 / 8][:nl]):
                check(uxc[l], ref, f"uni_xic[{l}]", floor=1.0)
        if t.vr_beta_dep:
            check(arr(t.uni_vb, (nb - 1) * n * 16).reshape(nb - 1, n, 4, 4)[k], vr(0, Ul), "uni_vb", inside)
            check(arr(t.uni_dab, (nb - 1) * n * 16).reshape(nb - 1, n, 4, 4)[k], vr(1, Ul), "uni_dab", inside)
            if t.uni_empb:
                emp = arr(t.uni_empb, 3 * (nb - 1) * n * 28).reshape(3, nb - 1, n, 4, 7)[:, k]
                for j, name in enumerate(("V2", "Ge1", "Ge2")):
                    check(emp[j], vr(2 + j, Ul), f"uni_empb {name}", inside)
        checked += 1
    assert checked == 4


# --------------------------------------------------------------------------------------------------- xp's own precision
def _mp_cell(xp, row, s, mu, mp):
    """One (s, mu) cell of CCFModel.theory_xi - sum over the velocity nodes of the integrand, minus one - and its magnitude,
    evaluated with mpmath on the tables xp reads: an independent scalar restatement of xp_reference.XP._cells."""
    import bisect
    F = lambda v: mp.mpf(float(v))                    # noqa: E731  (every input is a double: exact)
    f = xp.flags
    S = {k: (v if k == "poison" else F(v)) for k, v in xp.scalars(np.asarray(row, float)).items()}
    row = [F(v) for v in row]
    from victor_amd import _native as N
    aperp, apar = row[N.P_APERP], row[N.P_APAR]
    if f["ap"]:
        eps = row[N.P_EPSILON]
        h = (1 - F(1e-10)) / 49
        ms = [F(1e-10) + j * h for j in range(49)] + [mp.mpf(1)]
        v = [apar * mp.sqrt((1 - m * m) * (eps * eps - 1) + 1) for m in ms]
        c = (mp.fsum(v) - (v[0] + v[-1]) / 2) * h
    else:
        c = row[N.P_ASTAR]
    S["c"] = c
    S["gD"] = S["G"] * 3 / c
    xi, vr = xp.point_tables(float(row[N.P_BETA]))

    def table(pp, var):
        knots = [F(k) for k in pp.knots]

        def ev(u):
            uc = min(max(u, knots[0]), knots[-1])
            i = min(max(bisect.bisect_right(knots, uc) - 1, 0), len(knots) - 2)
            cc = [F(x) for x in pp.coef[var][i]]
            dx = uc - knots[i]
            return ((cc[3] * dx + cc[2]) * dx + cc[1]) * dx + cc[0]
        return ev

    nlr = 1 if f["iso"] else xp.n_ell_r
    xis = [table(xi, l) for l in range(nlr)]
    V1, D1, V2, G1, G2 = (table(vr, j) for j in range(5))
    sv = table(xp.sv, 0)

    def vel(u):
        return V1(u) + S["av"] * V2(u) if f["empirical"] else V1(u)

    def xi_real(u, mu_r, r_par, s_perp):
        if f["from_data"]:
            rp, rt = r_par / apar, s_perp / aperp
            u = mp.sqrt(rp * rp + rt * rt)
            mu_r = rp / u
        x = xis[0](u)
        if nlr > 1:
            m2 = mu_r * mu_r
            x += xis[1](u) * (mp.mpf(3) / 2 * m2 - mp.mpf(1) / 2)
            if nlr > 2:
                x += xis[2](u) * ((35 * m2 - 30) * m2 + 3) / 8
        return x

    s, mu = F(s), F(mu)
    s_perp = s * aperp * mp.sqrt(1 - mu * mu)
    s_par = s * apar * mu
    rsd = f["rsd"]
    kais = rsd in (N.RSD["kaiser"], N.RSD["euclid_special"])
    nodes = [(mp.mpf(0), mp.mpf(1))] if kais else [(F(a), F(b)) for a, b in zip(xp.x, xp.w_x)]
    total, mag = mp.mpf(0), mp.mpf(0)
    for xk, wk in nodes:
        if rsd == N.RSD["streaming"]:
            r_par = s_par - xk * S["B"]
        elif rsd == N.RSD["dispersion"] or f["coord_shift"]:
            mfac = mp.mpf(1) if rsd == N.RSD["dispersion"] else S["M"]
            num = s_par - xk * S["B"] if rsd == N.RSD["dispersion"] else s_par

            def q_of(r2):
                r = mp.sqrt(r2)
                return -S["G"] * vel(r / c) / r
            r_par = num / (1 + mfac * q_of(s_par * s_par + s_perp * s_perp))
            for _ in range(f["niter"]):
                r_par = num / (1 + mfac * q_of(r_par * r_par + s_perp * s_perp))
        else:
            r_par = s_par
        r = mp.sqrt(s_perp * s_perp + r_par * r_par)
        mu_r = r_par / r
        u = r / c
        xir = xi_real(u, mu_r, r_par, s_perp)
        if rsd == N.RSD["streaming"]:
            sig = sv(u)
            z = (S["A"] * vel(u) * mu_r + xk) / sig
            g = wk / sig * mp.exp(-z * z / 2)
            total += g * (1 + xir)
            mag += abs(g) * (1 + abs(xir))
            continue
        q = -S["G"] * vel(u) / r
        Dq = G1(u) + S["av"] * G2(u) if f["empirical"] else D1(u)
        dq = -S["gD"] * Dq
        m2 = mu_r * mu_r
        if rsd == N.RSD["dispersion"]:
            sig = sv(u)
            z = xk / sig
            g = wk / (1 + q + m2 * (dq - q)) * mp.exp(-z * z / 2) / sig
            total += g * (1 + xir)
            mag += abs(g) * (1 + abs(xir))
        elif rsd == N.RSD["kaiser"] and not f["kaiser_approx"]:
            J = S["M"] * q + S["M"] * S["Q"] * m2 * (dq - q)
            total += (1 + S["M"] * xir) / (1 + J)
            mag += (1 + abs(S["M"] * xir)) / abs(1 + J)
        else:
            a, b = (1, 1) if rsd == N.RSD["kaiser"] else (3, 2)
            J = a * S["M"] * q + b * S["M"] * S["Q"] * m2 * (dq - q)
            total += 1 + (S["M"] * xir - J)
            mag += 1 + abs(S["M"] * xir) + abs(J)
    return total - 1, mag + 1


@pytest.mark.parametrize("setup, kw", [
    (KM.Setup(), {"rsd_model": "streaming"}),
    (KM.Setup(), {"rsd_model": "dispersion", "empirical_corr": True}),
    (KM.Setup(), {"rsd_model": "kaiser"}),
    (KM.Setup(), {"rsd_model": "kaiser", "kaiser_approximation": True}),
    (KM.Setup(), {"rsd_model": "euclid_special", "matter_model": "linear_bias"}),
    (KM.Setup(boss="config"), {"rsd_model": "streaming", "assume_isotropic": False}),
    (KM.Setup(nlr=2, from_data=True), {"rsd_model": "dispersion"}),
], ids=["streaming", "dispersion_empirical", "kaiser", "kaiser_approx", "euclid_linear_bias", "boss_streaming_beta",
        "from_data_dispersion"])
def test_xp_own_precision_against_mpmath(setup, kw, scratch):
    """A handful of cells of each RSD model recomputed with mpmath at 40 digits on the same tables (:func:`_mp_cell`): xp
    agrees to 1e-17 of each cell's magnitude, so the longdouble arithmetic the bounds rest on holds (a double leaking into
    xp_reference.py would show here as ~1e-16)."""
    mpmath = pytest.importorskip("mpmath")
    import victor_amd
    mp = mpmath.mp.clone() if hasattr(mpmath.mp, "clone") else mpmath.mp
    mp.dps = 40
    fit = victor_amd.CCFFit(*KM.options(setup, scratch))
    xp = X.XP(fit, kw)
    p = KM.points(fit, 3)
    rows = fit._fit_rows(dict(p, M=1.05, Q=0.9), fit._merged(kw))
    s = np.asarray(fit.s, float)
    cells = ((0, s[0], 0.0), (1, s[len(s) // 2], 0.37), (2, s[-1], 1.0), (0, s[len(s) // 3], 0.81))
    for i, sj, m in cells:
        th = xp.xi_smu(rows[i:i + 1], [sj], [m], sens=False)
        want, mag = _mp_cell(xp, rows[i], sj, m, mp)
        diff = abs(mp.mpf(str(th.t[0, 0, 0])) - want)
        assert diff <= mp.mpf("1e-17") * mag, (kw, i, sj, m, float(diff / mag))
