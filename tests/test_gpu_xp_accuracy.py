"""Every shipped theory kernel and chi-square kernel against the extended-precision evaluation of the table contract
(tests/xp_reference.py) at bounds derived from the documented errors of each kernel's arithmetic (tests/tolerances.py:
theory_xp_bound, chi2_xp_bound) - not at the flat 1e-9 of the oracle parity tests.

- theory layer: every THEORY recipe of tests/kernel_matrix.py (cells, fast, generic, K1x) on the recipe's first points, and for
  one recipe per family on the edge set (:func:`edge_rows`): beta on / between / outside the knots, sigma_v that saturates the
  Gaussian or flattens it, alpha that pushes r / c below the first knot or beyond the last, epsilon far from 1, fsigma8 = 0,
  Av and bias, kaiser M and Q, NaN rows (which must be NaN exactly where xp's are);
- chi-square layer: every chi-square kernel (fused, like_wide, like_tiled<8>, like, like_real<true / false>, the joint kernel
  with a gridded covariance) against ``chi2_from_theory`` on the GPU's own theory vectors, for the four likelihood forms;
- batch sizes at the point-major / cells switch (19, 20) and with partial tiles (33, 257).

xp results are cached per (setup, options, point); one xp point with its sensitivities costs 0.05 s (kaiser) to 1 s
(dispersion, anisotropic sigma_v) of one CPU core, which is what sizes the point sets.
"""

import faulthandler
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests import cases
from tests import kernel_matrix as KM
from tests import xp_reference as X
from tests.tolerances import (assert_chi2_xp, assert_theory_xp, chi2_bound, chi2_xp_bound, joint_chi2_xp_bound,
                              theory_xp_bound)
from victor_amd import _native

pytestmark = pytest.mark.gpu
N_XP = 2                      # recipe points held to xp per THEORY recipe
FORMS = {"gaussian": {"form": "Gaussian"}, "sellentin": {"form": "Sellentin", "nmocks": 1000},
         "hartlap": {"form": "Hartlap", "nmocks": 1000}, "percival": {"form": "Percival", "nmocks": 1000, "nparams": 4}}
# one recipe per kernel family that also runs the edge set
EDGE_RECIPES = ("cells<3,3,0,streaming,0>+fused", "fast<3,3,0,streaming,0>+fused", "cells<3,2,1,dispersion,0>+fused",
                "fast<3,2,0,dispersion,0>+fused", "cells<3,3,0,kaiser,0>+fused", "cells<1,2,0,streaming,0>+fused",
                "fast<1,2,0,dispersion,0>+fused", "generic<streaming,3,3>+like_wide", "generic<dispersion,2,2>+like_wide",
                "generic<kaiser,3,3>+like_wide", "cells<3,3,0,streaming,1>+fused")


@pytest.fixture(scope="module", autouse=True)
def time_limit():
    """The whole file under one time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(1700, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Inputs:
    """Fits, xp tables and xp results, built once per Setup / (Setup, options) / (Setup, options, row)."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.fits = {}
        self.xps = {}
        self.answers = {}

    def fit(self, st):
        if st not in self.fits:
            import victor_amd
            model, data = KM.options(st, self.tmp)
            self.fits[st] = victor_amd.CCFFit(model, data)
        return self.fits[st]

    def xp(self, st, kw):
        key = (st, tuple(sorted((k, str(v)) for k, v in kw.items())))
        if key not in self.xps:
            self.xps[key] = X.XP(self.fit(st), kw)
        return self.xps[key], key

    def theory(self, st, kw, rows):
        """xp Theory of ``rows`` (n, N) with sensitivities, cached per row."""
        xp, key = self.xp(st, kw)
        parts = []
        for row in np.atleast_2d(rows):
            k = (key, row.tobytes())
            if k not in self.answers:
                self.answers[k] = xp.theory(row[None], sens=True)
            parts.append(self.answers[k])
        return X.Theory(**{a: np.concatenate([getattr(p, a) for p in parts]) for a in vars(parts[0])})


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(str(tmp_path_factory.mktemp("xp_accuracy")))


@contextmanager
def knobs(**kv):
    for k, v in kv.items():
        _native.set_knob("VICTOR_HIP_" + k, v)
    try:
        yield
    finally:
        for k in kv:
            _native.set_knob("VICTOR_HIP_" + k, None)


def engine(fit, kw):
    return fit._get_engine(fit._engine_key(fit._merged(kw)))


def family(theory):
    """Kernel family of a theory instance string (tests/tolerances.py: XP_FAMILIES)."""
    fam, args = theory.split("<", 1)
    if fam in ("generic", "xi"):
        return "generic"
    mode = args.rstrip(">").split(",")[3]
    if mode.startswith("dispersion"):
        return "dispersion"
    if mode == "kaiser":
        return "kaiser"
    return fam


def edge_rows(fit, kw, base):
    """The edge set around the row ``base`` (see the module docstring)."""
    N = _native
    rows = []

    def put(**kv):
        r = base.copy()
        for k, v in kv.items():
            r[getattr(N, "P_" + k.upper())] = v
        r[N.P_EPSILON] = r[N.P_APERP] / r[N.P_APAR]
        rows.append(r)

    # test_gpu_parity.py::test_extreme_but_valid_parameters_vs_oracle
    put(fsigma8=1.5, sigmav=40.0, aperp=0.8, apar=1.2)
    put(fsigma8=0.05, sigmav=900.0, aperp=1.35, apar=0.7)
    put(fsigma8=3.0, sigmav=100.0, aperp=1.0, apar=1.0)
    put(fsigma8=0.0, sigmav=250.0, aperp=0.6, apar=1.5)
    # beta on the first, an interior and the last knot of each grid the fit's tables use - beta_r (real-space tables), beta_d
    # (data), beta_c (covariance) - just outside both ends of each, and midway between two knots; fixed tables: beta enters
    # only the growth term of linear_bias on a measured real-space ccf, two values of it
    grids = []
    if not fit.fixed_real_input:
        grids.append(fit.beta)
    if not fit.fixed_data:
        grids.append(fit.beta_ccf)
    if not fit.fixed_covmat:
        grids.append(fit.beta_covmat)
    betas = []
    for g in (np.asarray(g, float) for g in grids):
        betas += [g[0], g[len(g) // 2], g[-1], g[0] - 0.02, g[-1] + 0.02, 0.5 * (g[1] + g[2])]
    for b in (sorted(set(betas)) if grids else [0.3, 0.55]):
        put(beta=float(b))
    put(sigmav=8.0)                         # the Gaussian saturates at the outer velocity nodes (|z| > 37.7)
    put(sigmav=2500.0)
    put(aperp=0.45, apar=0.45)              # r / c below the first knot of every table (V clamped at u = 0.01) ...
    put(aperp=2.2, apar=2.2)                # ... and beyond the last
    put(aperp=1.45, apar=0.72)              # epsilon = 2
    put(av=2.5, bias=1.4)
    put(m=1.6, q=0.4)                       # kaiser: 1 + J stays well away from 0
    put(m=0.4, q=2.0)
    put(fsigma8=np.nan)
    put(beta=np.nan)
    return np.array(rows)


def gpu_theory(fit, kw, rows, theory_key, rc_knobs, chunk):
    """Theory vectors of ``rows`` in launches of ``chunk`` rows, each of which must run ``theory_key``."""
    out = []
    with knobs(**rc_knobs):
        for i in range(0, len(rows), chunk):
            part = rows[i:i + chunk]
            out.append(fit.theory_vector_batch(part, **kw))
            assert engine(fit, kw).last_instance() == theory_key + "+none", (engine(fit, kw).last_instance(), len(part))
    return np.concatenate(out)


def check_theory(key, rc, inputs, kw, edges):
    st = rc.setup
    fit = inputs.fit(st)
    theory, _ = KM.parse(key)
    fam = family(theory)
    rows = fit._fit_rows(KM.points(fit, rc.n), fit._merged(kw))
    got = gpu_theory(fit, kw, rows, theory, rc.knobs, rc.n)[:N_XP]
    th = inputs.theory(st, kw, rows[:N_XP])
    model = fit._merged(kw)
    ap = not model["velocity_independent_of_AP"]
    xp, _ = inputs.xp(st, kw)
    bound = theory_xp_bound(th, fam, xp.n_mu, xp.n_x, ap)
    assert_theory_xp(got, th, bound, what=f"{fam} {key} {kw}")
    if edges:
        er = edge_rows(fit, kw, rows[0])
        if rc.n >= KM.CELLS_N:                          # cells from 20 points on (one launch), point-major below (16 a launch)
            er = np.concatenate([er, rows[:max(0, 20 - len(er))]])
        chunk = len(er) if rc.n >= KM.CELLS_N else 16
        got = gpu_theory(fit, kw, er, theory, rc.knobs, chunk)
        th = inputs.theory(st, kw, er)
        assert_theory_xp(got, th, theory_xp_bound(th, fam, xp.n_mu, xp.n_x, ap), what=f"{fam} edges {key} {kw}")


def check_xi(key, rc, inputs):
    st = rc.setup
    fit = inputs.fit(st)
    p = KM.points(fit, rc.n)
    rows = fit._fit_rows(p, fit._merged(rc.kw))
    mu = np.linspace(0, 1, 17)
    s = np.asarray(fit.s)[::4]
    with knobs(**rc.knobs):
        got = fit.theory_xi_batch(s, mu, rows[:N_XP], **rc.kw)
        assert engine(fit, rc.kw).last_instance() == key, engine(fit, rc.kw).last_instance()
    xp, _ = inputs.xp(st, rc.kw)
    th = xp.xi_smu(rows[:N_XP], s, mu)
    ap = not fit._merged(rc.kw)["velocity_independent_of_AP"]
    n_x = 1 if rc.kw.get("rsd_model") in ("kaiser", "euclid_special") else xp.n_x
    assert_theory_xp(got, th, theory_xp_bound(th, "generic", 0, n_x, ap), what=f"generic K1x {key}")


@pytest.mark.parametrize("key", [k for k, r in KM.THEORY.items()])
def test_theory_against_xp(key, inputs):
    rc = KM.THEORY[key]
    if rc.api == "xi":
        check_xi(key, rc, inputs)
        return
    check_theory(key, rc, inputs, rc.kw, key in EDGE_RECIPES)
    if ",kaiser," in key:                                          # kModeKaiser serves euclid_special as well
        check_theory(key, rc, inputs, dict(rc.kw, rsd_model="euclid_special"), key in EDGE_RECIPES)


# ------------------------------------------------------------------------------------------------------------ chi-square
def check_chi2(fit, kw, rows, key, rc_knobs, what, xp=None):
    """The likelihood of ``rows`` (must run ``key``) against chi2_from_theory on the theory vectors the same launch returns -
    the vectors the chi-square kernel consumed, so the bound is the quadratic form's alone - and log_likelihood_batch's
    results equal to those bit for bit."""
    with knobs(**rc_knobs):
        lnl, chi2, th = fit._run(rows, kw, want_theory=True)
        assert engine(fit, kw).last_instance() == key, (engine(fit, kw).last_instance(), len(rows))
        plain = fit.log_likelihood_batch(rows, **kw)
        assert engine(fit, kw).last_instance() == key, (engine(fit, kw).last_instance(), len(rows))
    assert np.array_equal(plain[1], chi2) and np.array_equal(plain[0], lnl), what
    xp = xp or X.XP(fit, kw)
    want_l, want_c = X.chi2_from_theory(fit, th, rows, kw, xp=xp)
    bound = chi2_xp_bound(xp, th, rows)
    assert_chi2_xp(lnl, chi2, want_l, want_c, bound, what=what)


LIKE_KEYS = [k for k in KM.LIKE if "like_real" not in k] + ["cells<3,3,0,streaming,0>+fused", "fast<3,3,0,streaming,0>+fused",
                                                           "cells<1,2,0,streaming,0>+fused", "fast<1,2,0,dispersion,0>+fused"]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("key", LIKE_KEYS)
def test_chi2_against_xp(key, form, inputs):
    rc = KM.RECIPES[key]
    fit = inputs.fit(rc.setup)
    kw = dict(rc.kw, likelihood=FORMS[form])
    rows = fit._fit_rows(KM.points(fit, rc.n), fit._merged(kw))
    check_chi2(fit, kw, rows, key, rc.knobs, f"{key} {form}")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("key", [k for k in KM.LIKE if "like_real" in k])
def test_realisation_chi2_against_xp(key, form, inputs):
    """like_real<true / false>: every realisation's chi2 / lnL against chi2_from_theory on a fit of that realisation, with
    the theory vectors of a separate launch (so 64 ulps of tau on top, as tolerances.chi2_bound)."""
    import victor_amd
    rc = KM.RECIPES[key]
    st = rc.setup
    fit = inputs.fit(st)
    kw = dict(rc.kw, likelihood=FORMS[form])
    rows = fit._fit_rows(KM.points(fit, rc.n), fit._merged(kw))
    with knobs(**rc.knobs):
        lnl, chi2 = fit.realisations().log_likelihood(rows, **kw)
        assert engine(fit, kw).last_instance() == key, engine(fit, kw).last_instance()
        th = fit.theory_vector_batch(rows, **rc.kw)
        theory, _ = KM.parse(key)
        assert engine(fit, rc.kw).last_instance() == theory + "+none", engine(fit, rc.kw).last_instance()
    model, data = KM.options(st, inputs.tmp)
    for m in range(st.n_real):
        d = dict(data, redshift_space_ccf=dict(data["redshift_space_ccf"], simulation_number=m))
        single = victor_amd.CCFFit(model, d)
        xp = X.XP(single, kw)
        want_l, want_c = X.chi2_from_theory(single, th, rows, kw, xp=xp)
        bound = chi2_xp_bound(xp, th, rows, chi2_bound(single, rows, ulps=64, **rc.kw))
        assert_chi2_xp(lnl[:, m], chi2[:, m], want_l, want_c, bound, what=f"{key} {form} realisation {m}")
        single._engine = None


# the instances the BOSS configuration selects by batch size (victor_hip.hip: cells from 20 points on)
BATCH_INSTANCE = {19: "fast<1,2,0,streaming,0>+fused", 20: "cells<1,2,0,streaming,0>+fused",
                  33: "cells<1,2,0,streaming,0>+fused", 257: "cells<1,2,0,streaming,0>+fused"}


@pytest.mark.parametrize("n", sorted(BATCH_INSTANCE))
def test_batch_size_edges_against_xp(n, inputs):
    """The point-major / cells switch and partial tiles / workgroups on the BOSS tables (beta-dependent, blended covariance):
    every point's chi-square against xp on the theory vectors the same launch consumed, the theory of the first, the last and
    the tile-edge points against xp."""
    st = KM.Setup(boss="config")
    fit = inputs.fit(st)
    hp = cases.halton_params(n, with_beta=True)
    rows = fit._fit_rows(hp, fit.model)
    xp, _ = inputs.xp(st, {})
    lnl, chi2, th = fit._run(rows, {}, want_theory=True)
    inst = engine(fit, {}).last_instance()
    assert inst == BATCH_INSTANCE[n], (n, inst)
    want_l, want_c = X.chi2_from_theory(fit, th, rows, xp=xp)
    bound = chi2_xp_bound(xp, th, rows)
    assert_chi2_xp(lnl, chi2, want_l, want_c, bound, what=f"{inst} batch of {n}")
    pick = sorted({0, min(n - 1, 19), min(n - 1, 32), n - 1})
    t = inputs.theory(st, {}, rows[pick])
    fam = family(KM.parse(inst)[0])
    assert_theory_xp(th[pick], t, theory_xp_bound(t, fam, xp.n_mu, xp.n_x), what=f"{fam} batch of {n} {inst}")


def _block_theory(fits, rows):
    """The blocks' theory vectors of ``rows``, concatenated; every launch a theory kernel alone (``+none``)."""
    out = []
    for f in fits:
        out.append(f.theory_vector_batch(rows))
        assert f._get_engine().last_instance().endswith("+none"), f._get_engine().last_instance()
    return np.concatenate(out, axis=1)


def test_joint_chi2_against_xp(tmp_path):
    """The joint kernel (one full covariance across the blocks): a fixed covariance and the 17-block gridded case of
    test_gpu_joint_cov.py, both against chi2_from_theory on the blocks' own GPU theory vectors, for the four likelihood
    forms."""
    import victor_amd
    import scipy.linalg as sl
    from victor_amd.joint import JointFit
    from tests.test_gpu_joint_cov import boss_pair_options, correlated, like, points_dict
    pair = boss_pair_options()
    q_of = [q % 2 for q in range(17)]
    fits = [victor_amd.CCFFit(*pair[q]) for q in q_of]
    src = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    pick = np.arange(0, 31, 6)
    beta_grid = np.asarray(src["beta"], dtype=float)[pick]
    slices = np.array([correlated([c] * 17) for c in src["covmat"][pick]])
    np.save(tmp_path / "cov17.npy", {"beta": beta_grid, "covmat": slices}, allow_pickle=True)
    spec = {"dir": str(tmp_path), "data_file": "cov17.npy", "cov_key": "covmat", "fixed_beta": False, "beta_key": "beta"}
    hp = cases.halton_params(8, with_beta=True)
    pts = [cases.point(hp, i) for i in range(8)]
    pts += [dict(pts[0], beta=float(b)) for b in (beta_grid[0] - 0.03, beta_grid[2], 0.5 * (beta_grid[2] + beta_grid[3]),
                                                   beta_grid[-1] + 0.02)]
    rows = fits[0]._fit_rows(points_dict(pts), fits[0].model)
    th = _block_theory(fits, rows)
    xps = [X.XP(f) for f in fits]
    for cov, nb in ((spec, 17), (sl.block_diag(*[f.covmat[0] for f in fits[:3]]), 3)):
        name = f"{nb} blocks, " + ("gridded" if nb == 17 else "fixed")
        tt = th[:, :sum(x.N for x in xps[:nb])]
        for form in FORMS:
            joint = JointFit(fits[:nb], covariance=cov, likelihood=like(form))
            lnl, chi2 = joint.log_likelihood_batch(points_dict(pts))
            assert fits[0]._get_engine().last_instance().endswith("+joint_chi2"), fits[0]._get_engine().last_instance()
            want_l, want_c = X.chi2_from_theory(joint, tt, rows)
            bound = joint_chi2_xp_bound(joint, xps[:nb], tt, rows)
            assert_chi2_xp(lnl, chi2, want_l, want_c, bound, what=f"joint_chi2 {name} {form}", offset_scale=1e4)
            joint._release_handle()


@pytest.mark.parametrize("case", ["fixed", "gridded"])
def test_joint_realisation_chi2_against_xp(case, tmp_path):
    """The joint-realisation kernel (JointFit.realisations(), ``+joint_real_chi2``): every (point, realisation) entry against
    chi2_from_theory on a JointFit of that realisation's blocks, with the blocks' GPU theory vectors, for the four likelihood
    forms - five dsplit blocks under one fixed covariance, two BOSS blocks under a gridded one."""
    import victor_amd
    from victor_amd.joint import JointFit
    from tests.test_gpu_joint_cov import _gridded_points, like, points_dict
    from tests.test_joint_cov import boss_joint_cov_file, correlated
    from tests.test_joint_realisations import boss_stacks, dsplit_stacks, with_number
    n_real = 4
    if case == "fixed":
        opts = dsplit_stacks(tmp_path, n_real)
        fits = [victor_amd.CCFFit(*o) for o in opts]
        cov = correlated([f.covmat for f in fits])
        params = cases.halton_params(6)
    else:
        opts = boss_stacks(tmp_path, n_real)
        fits = [victor_amd.CCFFit(*o) for o in opts]
        cov = boss_joint_cov_file(str(tmp_path / "cov.npy"))
        params = points_dict(_gridded_points(fits[0].beta_covmat))
    rows = fits[0]._fit_rows(params, fits[0].model)
    th = _block_theory(fits, rows)
    per = []
    for m in range(n_real):
        fm = [victor_amd.CCFFit(*o) for o in with_number(opts, m)]
        per.append((fm, [X.XP(f) for f in fm]))
    for form in FORMS:
        joint = JointFit(fits, covariance=cov, likelihood=like(form))
        lnl, chi2 = joint.realisations().log_likelihood(params)
        assert fits[0]._get_engine().last_instance().endswith("+joint_real_chi2"), fits[0]._get_engine().last_instance()
        assert chi2.shape == (len(rows), n_real)
        for m, (fm, xps) in enumerate(per):
            jm = JointFit(fm, covariance=cov, likelihood=like(form))
            want_l, want_c = X.chi2_from_theory(jm, th, rows)
            bound = joint_chi2_xp_bound(jm, xps, th, rows)
            assert_chi2_xp(lnl[:, m], chi2[:, m], want_l, want_c, bound, what=f"joint_real_chi2 {case} {form} realisation {m}",
                           offset_scale=1e4)
        joint._release_handle()
