"""Realisations with each mock's own real-space CCF (``realisations(paired_model=True)``, victor_amd/realisations.py) without a
GPU: the table sets it stacks, its refusals - each before any call into the library - and the expansion of cross mode into
pairs.  The fixtures (a paired BOSS stack with beta-dependent tables, a paired synthetic stack with fixed ones) are written into
``tmp_path`` from files under tests/golden/; tests/test_gpu_paired_realisations.py shares them."""

import os

import numpy as np
import pytest

from tests import cases
from tests.test_realisations import stack_options

N_STACK = 16
NUMBERS = [5, 0, 9]          # not contiguous, not sorted: a simulation number taken for an index shows


def which_of(n):
    """Adjacent rows, and the ranges of one launch, differ in set."""
    return ((7 * np.arange(n)) % len(NUMBERS)).astype(np.int32)


def _factor(r, n=N_STACK):
    """Realisation m = base x (1 + 0.03 sin(0.7 m + r / 20)) for m >= 1; realisation 0 is the base unchanged."""
    m = np.arange(n)
    f = 1.0 + 0.03 * np.sin(0.7 * m[:, None] + np.asarray(r)[None, :] / 20.0)
    f[0] = 1.0
    return f


def write_boss_model_stack(tmp, n=N_STACK, name="boss_model_stack.npy"):
    base = np.load(os.path.join(cases.GOLDEN, "boss", "model.npy"), allow_pickle=True).item()
    f = _factor(base["r"], n)[:, None, :]                                       # (n, 1, n_r) over (n_beta, n_r)
    path = os.path.join(str(tmp), name)
    np.save(path, dict(base, monopole=base["monopole"][None] * f, quadrupole=base["quadrupole"][None] * f), allow_pickle=True)
    return path


def paired_boss_options(tmp, number=0, model_number="same", model_file=None):
    """BOSS tables (n_beta_r = 31, beta-dependent data vector and covariance): the 16-realisation data stack against a model
    file with 16 realisations of the real-space multipoles."""
    model, data = stack_options(simulation_number=number)
    model["input_model_data_file"] = model_file or write_boss_model_stack(tmp)
    if model_number is not None:
        model["realspace_ccf"]["simulation_number"] = number if model_number == "same" else model_number
    return model, data


def write_fixed_stacks(tmp, n=N_STACK):
    base = np.load(os.path.join(cases.GOLDEN, "synth", "model.npy"), allow_pickle=True).item()
    f = _factor(base["r"], n)
    mpath = os.path.join(str(tmp), "synth_model_stack.npy")
    np.save(mpath, dict(base, **{k: base[k][None] * f for k in ("monopole", "quadrupole", "hexadecapole")}), allow_pickle=True)
    d = np.load(os.path.join(cases.GOLDEN, "synth", "data3.npy"), allow_pickle=True).item()
    rng = np.random.default_rng(5)
    dpath = os.path.join(str(tmp), "synth_data_stack.npy")
    np.save(dpath, dict(d, **{k: d[k][None] * (1.0 + 0.02 * rng.standard_normal((n,) + d[k].shape))
                              for k in ("monopole", "quadrupole", "hexadecapole")}), allow_pickle=True)
    return mpath, dpath


def paired_fixed_options(tmp, number=0, files=None):
    """Fixed tables (n_beta_r = 0), three real-space multipoles, anisotropic sum: the only case that reaches the per-point copy."""
    mpath, dpath = files or write_fixed_stacks(tmp)
    model, data = cases.synth_options(3)
    model["input_model_data_file"] = mpath
    model["realspace_ccf"]["simulation_number"] = number
    data["redshift_space_ccf"].update(data_file=dpath, simulation_number=number)
    return model, data


def _xi_tables(model_like):
    from victor_amd import engine
    t, keep = engine.build_tables(model_like)
    n = engine.table_array_lengths(t)
    out = tuple(np.ctypeslib.as_array(p, shape=(n[k],)).copy() for k, p in (("xi.coef", t.xi.coef), ("uni_xi", t.uni_xi), ("uni_xic", t.uni_xic)))
    del keep
    return out


@pytest.mark.parametrize("fixture", ["boss", "fixed"])
def test_stacked_sets_are_the_tables_of_single_simulation_models(tmp_path, fixture):
    import victor_amd
    opts = paired_boss_options if fixture == "boss" else paired_fixed_options
    rs = victor_amd.CCFFit(*opts(tmp_path)).realisations(NUMBERS, paired_model=True)
    sets = rs.model_sets()
    assert all(s.shape[0] == len(NUMBERS) for s in sets)
    for i, number in enumerate(NUMBERS):
        want = _xi_tables(victor_amd.CCFModel(opts(tmp_path, number=number)[0]))
        for name, got, w in zip(("xi.coef", "uni_xi", "uni_xic"), sets, want):
            assert got[i].tobytes() == w.tobytes(), (name, number)
    assert sets[0][0].tobytes() != sets[0][1].tobytes()
    # a shared object of the same fit has none
    with pytest.raises(victor_amd.InputError):
        victor_amd.CCFFit(*opts(tmp_path)).realisations(NUMBERS).model_sets()


class _NoLibrary:
    """Stands where the engine would: any use is a call into the library."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the refusal")


def _no_library(monkeypatch):
    import victor_amd
    monkeypatch.setattr(victor_amd.CCFFit, "_get_engine", lambda self, *a, **k: _NoLibrary())


def test_refusals_come_before_any_library_call(tmp_path, monkeypatch):
    import victor_amd
    from victor_amd import InputError
    _no_library(monkeypatch)
    point = dict(cases.NOTEBOOK_POINT)
    # the model without an integer simulation_number
    with pytest.raises(InputError, match="realspace_ccf.simulation_number"):
        victor_amd.CCFFit(*stack_options()).realisations(paired_model=True)
    # a stack key without a realisation axis: the model file replaced after the fit was built
    path = write_boss_model_stack(tmp_path, name="replaced.npy")
    fit = victor_amd.CCFFit(*paired_boss_options(tmp_path, model_file=path))
    stack = np.load(path, allow_pickle=True).item()
    np.save(path, dict(stack, quadrupole=stack["quadrupole"][0]), allow_pickle=True)
    with pytest.raises(InputError, match=r"quadrupole in .*replaced\.npy has no realisation axis"):
        fit.realisations(paired_model=True)
    np.save(path, dict(stack, monopole=stack["monopole"][:, :, :-1]), allow_pickle=True)
    with pytest.raises(InputError, match=r"Shape of a realisation of monopole in .*replaced\.npy"):
        fit.realisations(paired_model=True)
    # another number of realisations than the data stack
    short = write_boss_model_stack(tmp_path, n=12, name="short.npy")
    with pytest.raises(InputError, match=r"monopole in .*short\.npy holds 12 realisations.*16"):
        victor_amd.CCFFit(*paired_boss_options(tmp_path, model_file=short)).realisations(paired_model=True)
    # linear_bias: the velocity tables follow xi^r_0 and differ between the simulations
    model, data = paired_boss_options(tmp_path)
    model["matter_ccf"]["model"] = "linear_bias"
    rs = victor_amd.CCFFit(model, data).realisations(NUMBERS, paired_model=True)
    with pytest.raises(InputError, match=r"vk_tables\.(vr\.coef|vr_emp|uni_vb|uni_sv_v) of simulation 5 differs"):
        rs.log_likelihood_pairs(point, [0])
    # another r grid in the file than the one the fit was built from
    path = write_boss_model_stack(tmp_path, name="regrid.npy")
    fit = victor_amd.CCFFit(*paired_boss_options(tmp_path, model_file=path))
    stack = np.load(path, allow_pickle=True).item()
    np.save(path, dict(stack, r=stack["r"] * 1.01), allow_pickle=True)
    rs = fit.realisations(NUMBERS, paired_model=True)
    with pytest.raises(InputError, match=r"vk_tables\.\S+ of simulation 5 differs"):
        rs.log_likelihood_pairs(point, [0])
    # the RSD models that are not covered
    rs = victor_amd.CCFFit(*paired_boss_options(tmp_path)).realisations(NUMBERS, paired_model=True)
    for rsd in ("dispersion", "kaiser", "euclid_special"):
        with pytest.raises(InputError, match="streaming"):
            rs.log_likelihood_pairs(point, [0], rsd_model=rsd)
    # a joint fit
    from victor_amd.joint import JointFit
    joint = JointFit([victor_amd.CCFFit(*paired_boss_options(tmp_path)), victor_amd.CCFFit(*paired_boss_options(tmp_path))])
    with pytest.raises(InputError, match="joint"):
        joint.realisations(paired_model=True)


class _Recorder:
    """An engine that records the pairs it is asked for and answers with numbers that name them."""

    def __init__(self):
        self.calls, self.sets, self.blocks = [], None, None
        self._real_owner = None

    def set_realisations(self, blocks):
        self.blocks = len(blocks)

    def set_model_realisations(self, *sets):
        self.sets = None if sets[0] is None else len(sets[0])

    def make_opts(self, model, fit_options=None):
        return None

    def eval_realisations(self, opts, rows, n_real, which=None):
        assert which is not None, "cross mode reached the device on a paired object"
        rows = np.asarray(rows).reshape(-1, 12)
        self.calls.append((rows.copy(), np.array(which)))
        v = 1000.0 * rows[:, 0] + np.asarray(which)
        return -v, 2 * v


def test_cross_mode_expands_to_pairs(tmp_path, monkeypatch):
    import victor_amd
    from victor_amd import realisations as R
    rec = _Recorder()
    monkeypatch.setattr(victor_amd.CCFFit, "_get_engine", lambda self, *a, **k: rec)
    monkeypatch.setattr(R, "PAIR_CHUNK", 7)                 # chunks of two whole points
    rs = victor_amd.CCFFit(*paired_boss_options(tmp_path)).realisations(NUMBERS, paired_model=True)
    P, n_real = 5, len(NUMBERS)
    params = {"fsigma8": 0.3 + 0.05 * np.arange(P), "beta": np.full(P, 0.37), "sigma_v": np.full(P, 380.0), "epsilon": np.ones(P)}
    lnl, chi2 = rs.log_likelihood(params)
    assert rec.blocks == n_real and rec.sets == n_real
    rows = np.concatenate([c[0] for c in rec.calls])
    which = np.concatenate([c[1] for c in rec.calls])
    assert len(rows) == P * n_real and [len(c[1]) for c in rec.calls] == [6, 6, 3]
    assert np.array_equal(which, np.tile(np.arange(n_real), P))
    assert np.array_equal(rows[:, 0], np.repeat(params["fsigma8"], n_real))
    assert lnl.shape == chi2.shape == (P, n_real)
    want = 1000.0 * params["fsigma8"][:, None] + np.arange(n_real)[None, :]
    assert np.array_equal(chi2, 2 * want) and np.array_equal(lnl, -want)
    # pairs go straight through, in one call
    rec.calls.clear()
    w = which_of(P)
    rs.log_likelihood_pairs(params, w)
    assert len(rec.calls) == 1 and np.array_equal(rec.calls[0][1], w)
    # a shared object that takes the engine over clears the sets; the paired one installs both again
    shared = rs.fit.realisations(NUMBERS)
    shared.log_likelihood_pairs(params, w)
    assert rec.sets is None
    rs.log_likelihood_pairs(params, w)
    assert rec.sets == n_real
