"""Joint fit under one covariance across the data vectors (victor_amd/joint.py ``covariance=``): host side, no GPU.

The covariance loader that CCFFit and JointFit share and the log-det helper of the covariance slices must leave CCFFit's arrays
and ``build_tables`` output bit for bit as they were; the joint covariance is read in both input forms and checked against
the joint vector's length; blocks that cannot share one launch are refused."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 0.5


def correlated(blocks, rho=RHO):
    """C_joint = L (K kron I) L^T, L = blockdiag(chol C_q), K_qq' = rho^|q - q'|: its diagonal blocks are exactly the C_q."""
    import scipy.linalg as sl
    n = blocks[0].shape[0]
    L = sl.block_diag(*[np.linalg.cholesky(c) for c in blocks])
    q = np.arange(len(blocks))
    K = rho ** np.abs(q[:, None] - q[None, :])
    return L @ np.kron(K, np.eye(n)) @ L.T


def boss_pair_options():
    """Two reconstructed BOSS-style blocks on the same model options: data.npy and patchy_data.npy."""
    a = cases.boss_options()
    b = cases.boss_options()
    b[1]["redshift_space_ccf"]["data_file"] = "boss/patchy_data.npy"
    return [a, b]


def boss_joint_cov_file(path, rho=RHO, indefinite_last=False):
    """The 31 beta slices of boss/cov.npy as correlated 120 x 120 joint slices, written as a covariance_matrix dict file.
    ``indefinite_last``: the last slice gets one negative eigenvalue, so that blends with it change sign part of the way."""
    src = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    slices = np.array([correlated([c, c], rho) for c in src["covmat"]])
    if indefinite_last:
        w, v = np.linalg.eigh(slices[-1])
        w[0] = -0.5 * w[0]
        slices[-1] = (v * w) @ v.T
    np.save(path, {"beta": src["beta"], "covmat": slices}, allow_pickle=True)
    return {"dir": os.path.dirname(path), "data_file": os.path.basename(path), "cov_key": "covmat", "fixed_beta": False,
            "beta_key": "beta"}


def old_logdets(covmat):
    """The slice loop as build_tables had it inline before it became engine.covariance_logdets."""
    import scipy.linalg as sl
    nb = len(covmat)
    logdet = np.empty(nb)
    eig = np.ones((nb, covmat.shape[-1]))
    for kk in range(nb):
        sign, ld = np.linalg.slogdet(covmat[kk])
        logdet[kk] = ld if sign == 1 else np.nan
        if kk < nb - 1 and sign == 1:
            try:
                eig[kk] = sl.eigh(covmat[-1], covmat[kk], eigvals_only=True)
            except np.linalg.LinAlgError:
                eig[kk] = np.nan
    return logdet, eig


def _table_array(t, name):
    from victor_amd import engine
    n = engine.table_array_lengths(t)[name]
    return np.ctypeslib.as_array(getattr(t, name), shape=(n,)).copy()


@pytest.mark.parametrize("which", ["boss", "synth3", "boss_fixed"])
def test_covariance_loader_and_logdet_helper_keep_ccffit_bits(which):
    import victor_amd
    from victor_amd import engine
    opts = {"boss": cases.boss_options(), "synth3": cases.synth_options(3)}.get(which)
    if which == "boss_fixed":
        opts = cases.boss_options()
        opts[1]["covariance_matrix"] = {"data_file": "boss/cov_fixed.npy", "cov_key": "covmat"}
    fit = victor_amd.CCFFit(*opts)
    src = np.load(os.path.join(cases.GOLDEN, opts[1]["covariance_matrix"]["data_file"]), allow_pickle=True).item()
    cov = np.asarray(src[opts[1]["covariance_matrix"]["cov_key"]], dtype=float)
    assert fit.covmat.tobytes() == cov.tobytes()
    assert fit.icov.tobytes() == np.linalg.inv(cov).tobytes()
    assert fit.fixed_covmat == (cov.ndim == 2)
    if cov.ndim == 3:
        assert fit.beta_covmat.tobytes() == np.asarray(src["beta"], dtype=float).tobytes()
    else:
        assert not hasattr(fit, "beta_covmat")
    t, keep = engine.build_tables(fit, fit)
    assert _table_array(t, "prec").tobytes() == np.linalg.inv(cov).tobytes()
    if cov.ndim == 3:
        logdet, eig = old_logdets(cov)
        assert _table_array(t, "logdet").tobytes() == logdet.tobytes()
        assert _table_array(t, "eig").tobytes() == eig.reshape(-1).tobytes()
        l2, e2 = engine.covariance_logdets(cov, fit.beta_covmat)
        assert l2.tobytes() == logdet.tobytes() and e2.tobytes() == eig.tobytes()
    else:
        assert t.n_beta_c == 0
    del keep


def test_joint_covariance_array_form():
    import scipy.linalg as sl
    import victor_amd
    from victor_amd.joint import JointFit
    fits = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(5)]
    cov = correlated([f.covmat for f in fits])
    joint = JointFit(fits, covariance=cov)
    assert joint.n_data == 600 and joint.fixed_covmat
    assert joint.get_interpolated_covariance().tobytes() == cov.tobytes()
    assert joint.get_interpolated_covariance(0.4).tobytes() == cov.tobytes()
    assert np.array_equal(joint.get_interpolated_precision(), np.linalg.inv(cov))
    assert np.array_equal(joint.multipole_datavector(), np.concatenate([f.multipole_datavector() for f in fits]))
    for q, f in enumerate(fits):                          # the diagonal blocks are the blocks' own covariances
        assert np.allclose(cov[120 * q:120 * (q + 1), 120 * q:120 * (q + 1)], f.covmat, rtol=1e-12, atol=0)
    assert joint.likelihood == fits[0].fit_options["likelihood"]
    assert JointFit(fits, covariance=cov, likelihood={"form": "hartlap", "nmocks": 2000}).likelihood["form"] == "hartlap"
    # default: block-diagonal, as before
    plain = JointFit(fits)
    assert plain.covariance is None
    assert np.array_equal(plain.get_interpolated_covariance(), sl.block_diag(*[f.covmat for f in fits]))
    with pytest.raises(victor_amd.InputError, match="Unexpected shape of \\(fixed\\) covariance matrix"):
        JointFit(fits, covariance=cov[:599, :599])
    with pytest.raises(victor_amd.InputError, match="Unexpected shape"):
        JointFit(fits[:4], covariance=cov)


def test_joint_covariance_dict_form_and_beta_grid(tmp_path):
    import victor_amd
    from victor_amd.joint import JointFit
    fits = [victor_amd.CCFFit(*o) for o in boss_pair_options()]
    spec = boss_joint_cov_file(str(tmp_path / "joint_cov.npy"))
    joint = JointFit(fits, covariance=spec)
    src = np.load(os.path.join(tmp_path, "joint_cov.npy"), allow_pickle=True).item()
    assert not joint.fixed_covmat and joint.n_data == 120
    assert joint.covmat.shape == (31, 120, 120) and np.array_equal(joint.beta_covmat, src["beta"])
    g = joint.beta_covmat
    # the bracket rule of ccf_fit.py:213-228: below / above the grid the first / last slice, on the grid that slice, else
    # slice lo blended with the LAST slice
    assert np.array_equal(joint.get_interpolated_covariance(g[0] - 0.1), src["covmat"][0])
    assert np.array_equal(joint.get_interpolated_covariance(g[-1] + 0.1), src["covmat"][-1])
    assert np.array_equal(joint.get_interpolated_covariance(g[7]), src["covmat"][7])
    b = 0.5 * (g[7] + g[8])
    t = (b - g[7]) / (g[-1] - g[7])
    assert np.array_equal(joint.get_interpolated_covariance(b), (1 - t) * src["covmat"][7] + t * src["covmat"][-1])
    assert np.array_equal(joint.multipole_datavector(b), np.concatenate([f.multipole_datavector(b) for f in fits]))
    with pytest.raises(victor_amd.InputError, match="Need to supply a valid value of beta"):
        joint.get_interpolated_covariance()
    # the log dets through the shared helper
    logdet, eig = old_logdets(src["covmat"])
    assert joint._logdet.tobytes() == logdet.tobytes() and joint._eig.tobytes() == eig.tobytes()
    # errors with the reference's messages
    bad = dict(src, beta=src["beta"][::-1].copy())
    np.save(tmp_path / "bad_grid.npy", bad, allow_pickle=True)
    with pytest.raises(victor_amd.InputError, match="Covariance beta grid must be strictly monotonically increasing"):
        JointFit(fits, covariance=dict(spec, data_file="bad_grid.npy"))
    np.save(tmp_path / "bad_shape.npy", dict(src, covmat=src["covmat"][:, :60, :60]), allow_pickle=True)
    with pytest.raises(victor_amd.InputError, match="Unexpected shape of \\(beta-varying\\) covariance matrix"):
        JointFit(fits, covariance=dict(spec, data_file="bad_shape.npy"))
    with pytest.raises(victor_amd.InputError, match="Key nokey not found"):
        JointFit(fits, covariance=dict(spec, cov_key="nokey"))
    with pytest.raises(victor_amd.InputError, match="not found"):
        JointFit(fits, covariance=dict(spec, data_file="missing.npy"))
    # fixed_beta (the default) wants one (NT, NT) matrix
    np.save(tmp_path / "fixed.npy", {"covmat": src["covmat"][3]}, allow_pickle=True)
    fixed = JointFit(fits, covariance={"dir": str(tmp_path), "data_file": "fixed.npy", "cov_key": "covmat"})
    assert fixed.fixed_covmat and np.array_equal(fixed.covmat, src["covmat"][3])
    # no beta_key: the data's own beta grid, as CCFFit
    np.save(tmp_path / "nogrid.npy", {"covmat": src["covmat"]}, allow_pickle=True)
    nogrid = JointFit(fits, covariance=dict(spec, data_file="nogrid.npy", beta_key=None))
    assert np.array_equal(nogrid.beta_covmat, fits[0].beta_ccf)


def test_joint_covariance_refuses_what_it_cannot_share(tmp_path):
    import victor_amd
    from victor_amd.joint import JointFit
    fits = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(2)]
    cov = correlated([f.covmat for f in fits])
    joint = JointFit(fits, covariance=cov)
    fits[1].model = dict(fits[1].model, rsd_model="dispersion")
    with pytest.raises(victor_amd.InputError, match="every block must share its model and fit options"):
        joint._plan_cov({})
    fits[1].model = dict(fits[0].model)
    fits[1].fit_options = dict(fits[1].fit_options, likelihood={"form": "hartlap", "nmocks": 100})
    fits[1].fit_options["beta_interpolation"] = "likelihood"
    with pytest.raises(victor_amd.InputError, match="every block must share"):
        joint._plan_cov({})
    fits[1].fit_options = dict(fits[0].fit_options)
    fits[1]._device = 1
    with pytest.raises(victor_amd.InputError, match="every block must live on the same device"):
        joint._plan_cov({})
    boss = [victor_amd.CCFFit(*o) for o in boss_pair_options()]
    jb = JointFit(boss, covariance=boss_joint_cov_file(str(tmp_path / "c.npy")))
    with pytest.raises(victor_amd.InputError, match="beta_interpolation 'likelihood'"):
        jb._plan_cov({"beta_interpolation": "likelihood"})
    with pytest.raises(victor_amd.InputError, match="likelihood= applies to a joint covariance only"):
        JointFit(fits, likelihood={"form": "gaussian"})


def test_joint_cov_tables_struct_matches_header(tmp_path):
    """The ctypes mirror of vk_joint_cov_tables has the C layout (a tiny C program against the header)."""
    from victor_amd import _native as N
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "victor_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(vk_joint_cov_tables), offsetof(vk_joint_cov_tables, block_n), offsetof(vk_joint_cov_tables, beta), '
                   'offsetof(vk_joint_cov_tables, eig));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = N.vk_joint_cov_tables
    assert out == [ctypes.sizeof(T), T.block_n.offset, T.beta.offset, T.eig.offset]


def test_joint_covariance_needs_a_beta_grid_when_the_blocks_grids_differ(tmp_path):
    """Blocks whose data sit on different beta grids: the covariance file must hold its own grid.  Whether beta_key is not
    given or names a key the file does not have, the loader's fall-back to a block's data grid is refused."""
    import victor_amd
    from victor_amd.joint import JointFit
    d = np.load(os.path.join(cases.GOLDEN, "boss", "patchy_data.npy"), allow_pickle=True).item()
    np.save(tmp_path / "shifted.npy", dict(d, beta=np.asarray(d["beta"]) + 1e-3), allow_pickle=True)
    a, b = boss_pair_options()
    b[1]["redshift_space_ccf"].update(data_file=str(tmp_path / "shifted.npy"), beta_key="beta")
    fits = [victor_amd.CCFFit(*a), victor_amd.CCFFit(*b)]
    assert not np.array_equal(fits[0].beta_ccf, fits[1].beta_ccf)
    spec = boss_joint_cov_file(str(tmp_path / "c.npy"))
    assert not JointFit(fits, covariance=spec).fixed_covmat                  # the file's own grid: accepted
    for key in (None, "no_such_key"):
        with pytest.raises(victor_amd.InputError, match="beta grids differ"):
            JointFit(fits, covariance=dict(spec, beta_key=key))

