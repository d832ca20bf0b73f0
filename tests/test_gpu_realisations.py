"""One parameter batch against many simulation realisations (victor_amd/realisations.py, vk_eval_realisations) on the GPU.

Value contract: entry [p, m] equals CCFFit(model, data with simulation_number=numbers[m]).log_likelihood(point p).  Against
the reference (tests/golden/realisations/ref.npz) and the oracle it is held to the parity bound of the other parity tests
(RTOL); against the single-realisation path on the GPU - the same theory vector, the chi-square summed in another order - to
tests/tolerances.chi2_bound.  Pairs mode returns the bits of cross mode."""

import faulthandler
import json
import os
import sys

import numpy as np
import pytest

from tests import cases
from tests.test_realisations import REAL, stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

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


def with_form(opts, form):
    model, data = opts
    data["likelihood"] = dict({"form": form}, **FORMS[form])
    return model, data


def single_path(opts_of, numbers, params, **kwargs):
    """(lnl, chi2, bound), each (n_points, len(numbers)): one CCFFit per realisation, log_likelihood_batch, chi2_bound."""
    import victor_amd
    out = []
    for m in numbers:
        fit = victor_amd.CCFFit(*opts_of(m))
        lnl, chi2 = fit.log_likelihood_batch(params, **kwargs)
        out.append((lnl, chi2, chi2_bound(fit, params)))
        fit._engine = None
        del fit
    return tuple(np.stack([o[i] for o in out], axis=1) for i in range(3))


def write_stack(path, n_real):
    """n_real realisations from the 16 of stack.npy (realisation m: number m % 16 scaled by 1 + (m // 16) / 100)."""
    s = np.load(os.path.join(REAL, "stack.npy"), allow_pickle=True).item()
    scale = (1.0 + (np.arange(n_real) // 16) / 100.0)[:, None, None]
    idx = np.arange(n_real) % 16
    np.save(path, dict(s, monopole=s["monopole"][idx] * scale, quadrupole=s["quadrupole"][idx] * scale), allow_pickle=True)
    return path


def test_cross_mode_boss_against_the_reference_the_oracle_and_the_single_path(oracle):
    import victor_amd
    g = np.load(os.path.join(REAL, "ref.npz"))
    meta = json.loads(str(g["meta_json"]))
    pts = meta["points"]
    batch = {k: np.array([p[k] for p in pts]) for k in pts[0]}
    for form in meta["forms"]:
        fit = victor_amd.CCFFit(*with_form(stack_options(), form))
        rs = fit.realisations()
        lnl, chi2 = rs.log_likelihood(batch)
        assert lnl.shape == chi2.shape == (len(pts), meta["n_real"])
        want_l, want_c = g[f"lnl_{form}"], g[f"chi2_{form}"]
        assert_same_chi2(chi2, want_c, RTOL * np.abs(want_c), what=f"realisations vs reference, {form}")
        assert_same_lnl(lnl, want_l, RTOL * np.abs(want_c), what=f"realisations vs reference, {form}")
        # the oracle, one fit per simulation_number (theory vector once per point)
        base = oracle.OracleFit(*with_form(stack_options(), form))
        theory = [base.theory_multipole_vector(base.s, dict(p), base.poles_s) for p in pts]
        for m in range(meta["n_real"]):
            ofit = oracle.OracleFit(*with_form(stack_options(simulation_number=m), form))
            for p, q in enumerate(pts):
                ofit.theory_multipole_vector = lambda *a, _t=theory[p], **k: _t
                ol, oc = ofit.log_likelihood(dict(q))
                assert abs(chi2[p, m] - oc) <= RTOL * abs(oc) and abs(lnl[p, m] - ol) <= RTOL * abs(ol), (form, p, m)
        sl, sc, bound = single_path(lambda m: with_form(stack_options(simulation_number=m), form), range(16), batch)
        assert_same_chi2(chi2, sc, bound, what=f"realisations vs single path, {form}")
        assert_same_lnl(lnl, sl, bound, what=f"realisations vs single path, {form}")


def test_64_realisations_256_points_against_the_oracle(tmp_path, oracle):
    import victor_amd
    path = write_stack(str(tmp_path / "stack64.npy"), 64)
    opts = stack_options(data_file=path)
    rs = victor_amd.CCFFit(*opts).realisations()
    hp = cases.halton_params(256, with_beta=True)
    lnl, chi2 = rs.log_likelihood(hp)
    assert chi2.shape == (256, 64) and np.all(np.isfinite(chi2))
    model_in = oracle.load_input(os.path.join(cases.GOLDEN, opts[0]["input_model_data_file"]))
    data_in = oracle.load_input(path)
    cov_in = oracle.load_input(os.path.join(cases.GOLDEN, opts[1]["covariance_matrix"]["data_file"]))
    base = oracle.OracleFit(*opts, model_input=model_in, data_input=data_in, cov_input=cov_in)
    theory = [base.theory_multipole_vector(base.s, cases.point(hp, p), base.poles_s) for p in range(256)]
    want = np.empty((2, 256, 64))
    for m in range(64):
        ofit = oracle.OracleFit(*stack_options(data_file=path, simulation_number=m), model_input=model_in, data_input=data_in,
                                cov_input=cov_in)
        for p in range(256):
            ofit.theory_multipole_vector = lambda *a, _t=theory[p], **k: _t
            want[:, p, m] = ofit.log_likelihood(cases.point(hp, p))
    assert_same_chi2(chi2, want[1], RTOL * np.abs(want[1]), what="64 realisations x 256 points vs oracle")
    assert_same_lnl(lnl, want[0], RTOL * np.abs(want[1]), what="64 realisations x 256 points vs oracle")


def test_pairs_mode_has_the_bits_of_cross_mode():
    import victor_amd
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    hp = cases.halton_params(64, with_beta=True)
    which = (np.arange(64) * 7) % 16
    cross = rs.log_likelihood(hp)
    pairs = rs.log_likelihood_pairs(hp, which)
    assert pairs[0].shape == pairs[1].shape == (64,)
    for got, full in zip(pairs, cross):
        assert np.array_equal(got, full[np.arange(64), which])
    sl, sc, bound = single_path(lambda m: stack_options(simulation_number=m), range(16), hp)
    assert_same_chi2(cross[1], sc, bound, what="cross vs single path")
    assert_same_lnl(cross[0], sl, bound, what="cross vs single path")
    # a subset: indices into rs.numbers
    sub = victor_amd.CCFFit(*stack_options()).realisations([9, 2, 14])
    got = sub.log_likelihood_pairs(hp, np.arange(64) % 3)
    pick = np.array([9, 2, 14])[np.arange(64) % 3]
    assert_same_chi2(got[1], cross[1][np.arange(64), pick], bound[np.arange(64), pick], what="pairs on a subset")
    from victor_amd import InputError
    with pytest.raises(InputError):
        sub.log_likelihood_pairs(hp, np.full(64, 3))


@pytest.mark.parametrize("case", ["gaussian", "hartlap", "percival", "fixed_cov", "likelihood_interp", "fixed_data"])
def test_options_against_the_single_path(case):
    import victor_amd
    if case in FORMS:
        opts_of = lambda m: with_form(stack_options(simulation_number=m), case)          # noqa: E731
    elif case == "fixed_cov":
        def opts_of(m):
            model, data = stack_options(simulation_number=m)
            data["covariance_matrix"].update(data_file="boss/cov_fixed.npy", fixed_beta=True)
            return model, data
    elif case == "fixed_data":
        opts_of = lambda m: stack_options(fixed=True, simulation_number=m)                # noqa: E731
    else:
        opts_of = lambda m: stack_options(simulation_number=m)                            # noqa: E731
    kw = {"beta_interpolation": "likelihood"} if case == "likelihood_interp" else {}
    hp = cases.halton_params(48, with_beta=True)
    rs = victor_amd.CCFFit(*opts_of(0)).realisations()
    lnl, chi2 = rs.log_likelihood(hp, **kw)
    sl, sc, bound = single_path(opts_of, range(16), hp, **kw)
    if kw:            # the blend of two evaluations at the bracketing grid betas: the larger of their bounds
        fit = victor_amd.CCFFit(*opts_of(0))
        g = fit.beta_ccf
        lo = np.array([np.where(g < b)[0][-1] for b in hp["beta"]])
        hi = np.array([np.where(g >= b)[0][0] for b in hp["beta"]])
        bound = np.maximum(chi2_bound(fit, dict(hp, beta=g[lo])), chi2_bound(fit, dict(hp, beta=g[hi])))[:, None]
    assert_same_chi2(chi2, sc, bound, what=f"realisations vs single path, {case}")
    assert_same_lnl(lnl, sl, bound, what=f"realisations vs single path, {case}")
    assert np.array_equal(rs.log_likelihood_pairs(hp, np.arange(48) % 16, **kw)[1], chi2[np.arange(48), np.arange(48) % 16])


def test_size_edges(tmp_path):
    import victor_amd
    hp = cases.halton_params(40, with_beta=True)
    full = victor_amd.CCFFit(*stack_options()).realisations()
    ref_l, ref_c = full.log_likelihood(hp)
    one = victor_amd.CCFFit(*stack_options()).realisations([5])                  # n_real = 1
    l1, c1 = one.log_likelihood(hp)
    assert c1.shape == (40, 1)
    bound = chi2_bound(full.fit, hp)
    assert_same_chi2(c1[:, 0], ref_c[:, 5], bound, what="n_real = 1")
    p0 = cases.point(hp, 3)                                                       # one point, dict of scalars
    l0, c0 = full.log_likelihood(p0)
    assert c0.shape == l0.shape == (16,)
    assert_same_chi2(c0, ref_c[3], bound[3], what="one point")
    assert full.chi_squared(p0).shape == (16,)
    path = write_stack(str(tmp_path / "stack37.npy"), 37)                         # n_real = 37: not a multiple of the tile
    rs = victor_amd.CCFFit(*stack_options(data_file=path)).realisations()
    l37, c37 = rs.log_likelihood(hp)
    assert c37.shape == (40, 37) and np.all(np.isfinite(c37))
    assert_same_chi2(c37[:, :16], ref_c, bound[:, None], what="n_real = 37, first 16")
    sl, sc, b37 = single_path(lambda m: stack_options(data_file=path, simulation_number=m), (16, 31, 32, 36), hp)
    assert_same_chi2(c37[:, [16, 31, 32, 36]], sc, b37, what="n_real = 37, last tile")
    assert_same_lnl(l37[:, [16, 31, 32, 36]], sl, b37, what="n_real = 37, last tile")


def test_guard_positions_match_the_single_path(tmp_path):
    """(-inf, inf) exactly where the single path returns it: a NaN parameter, a NaN beta, and a covariance whose blend has a
    determinant of sign -1 over part of the last beta interval (tests/test_gpu_parity.py builds the same covariance)."""
    import victor_amd
    cov = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    stack = np.array(cov["covmat"], dtype=float)
    w, v = np.linalg.eigh(stack[-1])
    flipped = stack[-1] - 1.25 * w[5] * np.outer(v[:, 5], v[:, 5]) - 5.0 * w[40] * np.outer(v[:, 40], v[:, 40])
    stack[-1] = 0.5 * (flipped + flipped.T)
    path = str(tmp_path / "cov_two_negative.npy")
    np.save(path, {"beta": cov["beta"], "covmat": stack}, allow_pickle=True)

    def opts_of(m):
        model, data = stack_options(simulation_number=m)
        data["covariance_matrix"]["data_file"] = path
        return model, data
    g = np.asarray(cov["beta"], dtype=float)
    betas = np.concatenate([g[-2] + (g[-1] - g[-2]) * np.linspace(0.02, 0.98, 49), [g[7], 0.5 * (g[3] + g[4])]])
    hp = dict(cases.halton_params(len(betas)), beta=betas)
    hp["fsigma8"][50] = np.nan
    rows = victor_amd.CCFFit(*opts_of(0))._fit_rows(hp, victor_amd.CCFFit(*opts_of(0)).model)
    rows = np.vstack([rows, rows[:1]])
    rows[-1, 5] = np.nan                                                          # beta
    rs = victor_amd.CCFFit(*opts_of(0)).realisations()
    lnl, chi2 = rs.log_likelihood(rows)
    sl, sc, _ = single_path(opts_of, (0, 9), rows)
    for j, m in enumerate((0, 9)):
        failed = np.isneginf(sl[:, j])
        assert 10 <= failed.sum() <= len(rows) - 10 and failed[50] and failed[-1]
        assert np.array_equal(np.isneginf(lnl[:, m]), failed) and np.array_equal(np.isposinf(chi2[:, m]), failed), m
        assert np.array_equal(np.isposinf(sc[:, j]), failed)
    assert np.array_equal(np.isneginf(lnl), np.repeat(np.isneginf(lnl[:, :1]), 16, axis=1))     # a guard fails the point
