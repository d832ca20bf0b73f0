"""Realisations (victor_amd/realisations.py) without a GPU: the per-realisation tables it uploads, its input errors, and the
reference pin of its fixtures (tests/golden/realisations/, tools/make_realisation_golden.py)."""

import json
import os
import sys

import numpy as np
import pytest

from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(cases.GOLDEN, "realisations")


def stack_options(fixed=False, simulation_number=0, data_file=None):
    """BOSS model against the 16-realisation stack (fixed: its fixed-data twin with the fixed covariance)."""
    model, data = cases.boss_options("config")
    ccf = data["redshift_space_ccf"]
    ccf["data_file"] = data_file or os.path.join(REAL, "stack_fixed.npy" if fixed else "stack.npy")
    if simulation_number is not None:
        ccf["simulation_number"] = simulation_number
    if fixed:
        ccf["reconstruction"] = False
        data["covariance_matrix"].update(data_file="boss/cov_fixed.npy", fixed_beta=True)
    return model, data


def _data_table(fit):
    from victor_amd import engine
    t, keep = engine.build_tables(fit, fit)
    n = engine.table_array_lengths(t)["data"]
    out = np.ctypeslib.as_array(t.data, shape=(n,)).copy()
    del keep
    return out


@pytest.mark.parametrize("fixed", [False, True])
def test_uploaded_tables_are_those_of_single_realisation_fits(fixed):
    import victor_amd
    rs = victor_amd.CCFFit(*stack_options(fixed)).realisations()
    assert list(rs.numbers) == list(range(16)) and rs.blocks.shape[0] == 16
    for i in (0, 7, 15):
        want = _data_table(victor_amd.CCFFit(*stack_options(fixed, simulation_number=i)))
        assert rs.blocks[i].tobytes() == want.tobytes(), i
    sub = victor_amd.CCFFit(*stack_options(fixed)).realisations([11, 3])
    assert list(sub.numbers) == [11, 3] and sub.blocks.tobytes() == rs.blocks[[11, 3]].tobytes()


def test_input_errors(tmp_path):
    import victor_amd
    from victor_amd import InputError
    with pytest.raises(InputError, match="simulation_number"):
        victor_amd.CCFFit(*cases.boss_options("config")).realisations()           # built without simulation_number
    fit = victor_amd.CCFFit(*stack_options())
    for bad in ([0, 16], [-1], [2.5], []):
        with pytest.raises(InputError):
            fit.realisations(bad)
    # the file as the fit was built from it, then replaced: no realisation axis / realisations of another shape
    stack = np.load(os.path.join(REAL, "stack.npy"), allow_pickle=True).item()
    path = os.path.join(str(tmp_path), "stack.npy")
    np.save(path, stack, allow_pickle=True)
    fit = victor_amd.CCFFit(*stack_options(data_file=path, simulation_number=3))
    assert len(fit.realisations()) == 16
    np.save(path, dict(stack, monopole=stack["monopole"][0], quadrupole=stack["quadrupole"][0]), allow_pickle=True)
    with pytest.raises(InputError, match="no realisation axis"):
        fit.realisations()
    np.save(path, dict(stack, monopole=stack["monopole"][:, :-1], quadrupole=stack["quadrupole"][:, :-1]), allow_pickle=True)
    with pytest.raises(InputError, match="Shape of a realisation"):
        fit.realisations()


@pytest.mark.reference
def test_oracle_looped_over_simulation_number_matches_the_reference_fixture():
    """ref.npz holds the reference's own (lnL, chi2) per (point, realisation); the oracle, one fit per simulation_number,
    reproduces them (its theory vector computed once per point: it does not depend on the realisation)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shim
    if not ref_shim.available():
        pytest.skip("reference not present")
    import victor_oracle as vo
    g = np.load(os.path.join(REAL, "ref.npz"))
    meta = json.loads(str(g["meta_json"]))
    pts = meta["points"]
    base = vo.OracleFit(*stack_options())
    theory = [base.theory_multipole_vector(base.s, dict(p), base.poles_s) for p in pts]
    for form in meta["forms"]:
        for m in range(meta["n_real"]):
            model, data = stack_options(simulation_number=m)
            data["likelihood"] = dict(data["likelihood"], form=form)
            ofit = vo.OracleFit(model, data)
            for p, q in enumerate(pts):
                ofit.theory_multipole_vector = lambda *a, _t=theory[p], **k: _t
                lnl, chi2 = ofit.log_likelihood(dict(q))
                want_l, want_c = g[f"lnl_{form}"][p, m], g[f"chi2_{form}"][p, m]
                assert abs(chi2 - want_c) <= 1e-12 * abs(want_c), (form, p, m)
                assert abs(lnl - want_l) <= 1e-12 * abs(want_l), (form, p, m)
