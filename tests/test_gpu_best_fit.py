"""Best-fit points on the GPU (victor_amd/fitting.py, vk_fit_run): recovery of known points from noise-free realisations, agreement
with scipy's Nelder-Mead driven through log_likelihood / log_likelihood_pairs, the reported point against the single-point paths
and the oracle, profiles, the prior box, determinism and independence of the batch, the iteration limit."""

import faulthandler
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_realisations import write_stack
from tests.test_realisations import REAL, stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "beta", "sigma_v", "epsilon"]
LO = np.array([PARAMS[n]["prior"]["min"] for n in NAMES], dtype=float)
HI = np.array([PARAMS[n]["prior"]["max"] for n in NAMES], dtype=float)
WIDTH = HI - LO


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


def tight(fixed=()):
    """Tight tolerances for the fitted parameters (every name but the fixed ones)."""
    return dict(xtol={n: 1e-7 * w for n, w in zip(NAMES, WIDTH) if n not in fixed}, ftol=1e-10, max_iter=3000, restarts=2)


def scipy_best(neg_lnl, x0):
    """scipy's Nelder-Mead from the same start simplex as the device search (vertex j: x0 + proposal_j e_j), in box-normalised
    coordinates - an affine map, under which Nelder-Mead takes the same steps - with the same tolerances (1e-7 of each width,
    1e-10 in lnL).  The same start matters: on the BOSS stack the maximum sits on a kink in beta, where Nelder-Mead can stall on
    the ridge, and a different start simplex stalls elsewhere."""
    from scipy.optimize import minimize

    def f(u):
        x = LO + u * WIDTH
        if np.any(x < LO) or np.any(x > HI):
            return np.inf
        v = neg_lnl(x)
        return v if np.isfinite(v) else np.inf
    x0 = np.asarray(x0, dtype=float)
    step = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
    sim = [x0.copy()]
    for j in range(len(x0)):
        v = x0.copy()
        v[j] = x0[j] + step[j] if x0[j] + step[j] <= HI[j] else x0[j] - step[j]
        sim.append(v)
    sim = (np.array(sim) - LO) / WIDTH
    r = minimize(f, sim[0], method="Nelder-Mead",
                 options=dict(initial_simplex=sim, xatol=1e-7, fatol=1e-10, maxiter=20000, maxfev=20000))
    return LO + r.x * WIDTH, -r.fun


def as_point(x):
    return {n: float(v) for n, v in zip(NAMES, x)}


def x_of(bf):
    return np.stack([bf.params[n] for n in NAMES], axis=1)


def test_noise_free_realisations_recover_their_points(tmp_path):
    import victor_amd
    base = victor_amd.CCFFit(*stack_options(fixed=True))
    rng = np.random.default_rng(5)
    truth = LO + WIDTH * (0.2 + 0.6 * rng.random((16, 4)))
    t = base.theory_vector_batch({n: truth[:, j] for j, n in enumerate(NAMES)})
    n_s = len(base.s)
    s = np.load(os.path.join(REAL, "stack_fixed.npy"), allow_pickle=True).item()
    path = str(tmp_path / "noise_free.npy")
    np.save(path, dict(s, monopole=t[:, :n_s], quadrupole=t[:, n_s:2 * n_s]), allow_pickle=True)
    rs = victor_amd.CCFFit(*stack_options(fixed=True, data_file=path)).realisations()
    bf = rs.best_fit(PARAMS, **tight())
    assert bf.names == NAMES and bf.x.shape == (16, 4)
    assert np.all(bf.status == bf.CONVERGED), bf.status
    assert np.all(bf.chi2 <= 1e-6), bf.chi2
    assert np.all(np.abs(x_of(bf) - truth) <= 1e-3 * WIDTH), np.abs(x_of(bf) - truth) / WIDTH
    assert np.all(bf.n_evals > 0) and np.all(bf.n_iter >= 1)


@pytest.fixture(scope="module")
def stack_fit():
    """The beta-dependent BOSS stack, Sellentin form with nmocks 1000: every realisation's best fit, twice."""
    import victor_amd
    opts = stack_options()
    like = opts[1]["likelihood"]
    assert like["form"].lower() == "sellentin" and like["nmocks"] == 1000
    rs = victor_amd.CCFFit(*opts).realisations()
    return rs, rs.best_fit(PARAMS, **tight()), rs.best_fit(PARAMS, **tight())


def test_realisations_against_scipy_and_the_single_point_paths(stack_fit, oracle):
    import victor_amd
    rs, bf, _ = stack_fit
    start = np.array([PARAMS[n]["ref"]["loc"] for n in NAMES])
    for k in (0, 5, 11):
        x_s, lnl_s = scipy_best(lambda x: -rs.log_likelihood_pairs(as_point(x), [k])[0][0], start)
        assert bf.lnl[k] >= lnl_s - 1e-6, (k, bf.lnl[k], lnl_s)
        assert np.all(np.abs(x_of(bf)[k] - x_s) <= 1e-3 * WIDTH), (k, (x_of(bf)[k] - x_s) / WIDTH)
    # the reported (lnL, chi2) are those of the reported point
    pts = {n: bf.params[n] for n in NAMES}
    lnl, chi2 = rs.log_likelihood_pairs(pts, np.arange(16))
    bound = np.array([chi2_bound(victor_amd.CCFFit(*stack_options(simulation_number=m)), bf.point(m))[0] for m in range(16)])
    assert_same_chi2(bf.chi2, chi2, bound, what="best fit vs log_likelihood_pairs")
    assert_same_lnl(bf.lnl, lnl, bound, what="best fit vs log_likelihood_pairs")
    # the oracle at point(i): a wrongly formed row (AP factors, beta, a fixed parameter) would show here
    ofit = oracle.OracleFit(*stack_options(simulation_number=5))
    ol, oc = ofit.log_likelihood(bf.point(5))
    assert abs(ol - bf.lnl[5]) <= 1e-9 * abs(ol) and abs(oc - bf.chi2[5]) <= 1e-9 * abs(oc), (ol, bf.lnl[5], oc, bf.chi2[5])


def test_data_vector_profile_and_box():
    import victor_amd
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    bf = fit.best_fit(PARAMS, **tight())
    assert len(bf) == 1 and bf.status[0] == bf.CONVERGED
    start = np.array([PARAMS[n]["ref"]["loc"] for n in NAMES])
    x_s, lnl_s = scipy_best(lambda x: -fit.log_likelihood(as_point(x))[0], start)
    assert bf.lnl[0] >= lnl_s - 1e-6 and np.all(np.abs(bf.x[0] - x_s) <= 1e-3 * WIDTH), (bf.x[0], x_s, bf.lnl[0], lnl_s)
    lnl, chi2 = fit.log_likelihood(bf.point(0))
    bound = chi2_bound(fit, bf.point(0))
    assert_same_chi2(bf.chi2, [chi2], bound, what="data-vector best fit vs log_likelihood")
    assert_same_lnl(bf.lnl, [lnl], bound, what="data-vector best fit vs log_likelihood")
    # a profile over fsigma8: eight problems in one run equal eight single-problem runs; none above the free maximum
    fs8 = np.linspace(0.3, 0.6, 8)
    prof = fit.best_fit(PARAMS, fixed={"fsigma8": fs8}, **tight(["fsigma8"]))
    assert prof.names == ["beta", "sigma_v", "epsilon"] and np.array_equal(prof.params["fsigma8"], fs8)
    assert np.all(prof.status == prof.CONVERGED)
    for i, v in enumerate(fs8):
        one = fit.best_fit(PARAMS, fixed={"fsigma8": float(v)}, **tight(["fsigma8"]))
        assert abs(one.lnl[0] - prof.lnl[i]) <= 1e-6, (v, one.lnl[0], prof.lnl[i])
    # Nelder-Mead from the cobaya start stalls on this likelihood's kinked ridge (it ends 0.23 in lnL below the profile's best
    # point, and scipy from the same start ends where it does): the free fit restarted from the profile's best point holds the
    # maximum - no profile point may lie above it
    best = int(np.argmax(prof.lnl))
    free = fit.best_fit(PARAMS, start=prof.point(best), **tight())
    assert free.status[0] == free.CONVERGED and free.lnl[0] >= bf.lnl[0] - 1e-6
    assert np.max(prof.lnl) <= free.lnl[0] + 1e-6, (prof.lnl, free.lnl)
    # sigma_v's prior narrowed to exclude the free optimum: the result stays inside, at the near face
    sv = float(bf.params["sigma_v"][0])
    lo, hi = (sv - 100.0, sv - 20.0) if sv > 300.0 else (sv + 20.0, sv + 100.0)
    narrow = dict(PARAMS, sigma_v=dict(PARAMS["sigma_v"], prior={"dist": "uniform", "min": lo, "max": hi}, ref={"loc": 0.5 * (lo + hi)}))
    box = fit.best_fit(narrow, **tight())
    got = float(box.params["sigma_v"][0])
    near = hi if sv > 300.0 else lo
    assert lo <= got <= hi and abs(got - near) <= 1e-2 * (hi - lo), (lo, hi, got)


def test_deterministic_and_independent_of_the_batch(stack_fit):
    import victor_amd
    rs, bf, again = stack_fit
    for a in ("x", "lnl", "chi2", "status", "n_iter", "n_evals"):
        assert getattr(bf, a).tobytes() == getattr(again, a).tobytes(), a
    sub = victor_amd.CCFFit(*stack_options()).realisations([11, 3]).best_fit(PARAMS, **tight())
    for i, k in enumerate((11, 3)):
        assert abs(sub.lnl[i] - bf.lnl[k]) <= 1e-6, (k, sub.lnl[i], bf.lnl[k])
        assert np.all(np.abs(sub.x[i] - bf.x[k]) <= 1e-3 * WIDTH), (k, sub.x[i], bf.x[k])


def test_iteration_limit(tmp_path):
    import victor_amd
    path = write_stack(str(tmp_path / "stack32.npy"), 32)
    rs = victor_amd.CCFFit(*stack_options(data_file=path)).realisations()
    bf = rs.best_fit(PARAMS, max_iter=3)
    assert len(bf) == 32 and np.all(bf.status == bf.MAX_ITER) and np.all(bf.n_iter == 3)
    start = {n: PARAMS[n]["ref"]["loc"] for n in NAMES}
    lnl0 = rs.log_likelihood(start)[0]
    assert np.all(bf.lnl >= lnl0), bf.lnl - lnl0
