"""JointFit.realisations() (victor_amd/joint.py, JointRealisations) without a GPU: the per-block tables it uploads, its input
errors, and the C ABI surface of vk_joint_cov_eval_realisations.

The fixtures are stacked data files with a realisation axis, one per block, written into tmp_path from the committed goldens
with a fixed seed (realisation m of block q: the block's golden multipoles times 1 + 0.02 N(0, 1))."""

import os
import re

import numpy as np
import pytest

from tests import cases
from tests.test_joint_cov import boss_joint_cov_file, boss_pair_options, correlated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_stacks(tmp_path, opts, n_real, seed=11, tag="stack"):
    """Copies of ``opts`` (a list of (model, data) blocks) whose data files are stacks of ``n_real`` realisations, written into
    ``tmp_path``; every block is built with simulation_number 0.  ``n_real`` may be a list (one count per block)."""
    rng = np.random.default_rng(seed)
    counts = n_real if isinstance(n_real, (list, tuple)) else [n_real] * len(opts)
    out = []
    for q, ((model, data), m) in enumerate(zip(opts, counts)):
        model, data = cases.clone(model), cases.clone(data)
        ccf = data["redshift_space_ccf"]
        src = np.load(os.path.join(data.get("dir", ""), ccf["data_file"]), allow_pickle=True).item()
        stack = dict(src)
        for key in ccf["ccf_keys"][1:]:
            a = np.asarray(src[key], dtype=float)
            stack[key] = a[None] * (1.0 + 0.02 * rng.standard_normal((m,) + a.shape))
        path = os.path.join(str(tmp_path), f"{tag}_q{q}.npy")
        np.save(path, stack, allow_pickle=True)
        ccf["data_file"] = path
        ccf["simulation_number"] = 0
        out.append((model, data))
    return out


def with_number(opts, m):
    """``opts`` with simulation_number m in every block."""
    out = []
    for model, data in opts:
        data = cases.clone(data)
        data["redshift_space_ccf"]["simulation_number"] = int(m)
        out.append((model, data))
    return out


def dsplit_stacks(tmp_path, n_real, seed=11):
    return write_stacks(tmp_path, [cases.dsplit_options(q) for q in range(5)], n_real, seed, tag="dsplit")


def boss_stacks(tmp_path, n_real, seed=12):
    return write_stacks(tmp_path, boss_pair_options(), n_real, seed, tag="boss")


def test_the_blocks_tables_are_those_of_their_realisations(tmp_path):
    import victor_amd
    from victor_amd.joint import JointFit
    for opts, cov in ((dsplit_stacks(tmp_path, 7), None), (boss_stacks(tmp_path, 7), "gridded")):
        fits = [victor_amd.CCFFit(*o) for o in opts]
        if cov == "gridded":
            cov = boss_joint_cov_file(str(tmp_path / "cov.npy"))
        else:
            cov = correlated([f.covmat for f in fits])
        for covariance in (cov, None):
            jr = JointFit(fits, covariance=covariance).realisations()
            assert len(jr) == 7 and list(jr.numbers) == list(range(7)) and len(jr.blocks) == len(fits)
            for q, fit in enumerate(fits):
                own = fit.realisations()
                assert jr.blocks[q].blocks.tobytes() == own.blocks.tobytes(), q
            sub = JointFit(fits, covariance=covariance).realisations([5, 2, 5])
            assert list(sub.numbers) == [5, 2, 5]
            for q, fit in enumerate(fits):
                assert sub.blocks[q].blocks.tobytes() == fit.realisations([5, 2, 5]).blocks.tobytes()


def test_input_errors(tmp_path):
    import victor_amd
    from victor_amd import InputError
    from victor_amd.joint import JointFit
    # a block built without simulation_number
    plain = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(2)]
    with pytest.raises(InputError, match="simulation_number"):
        JointFit(plain, covariance=correlated([f.covmat for f in plain])).realisations()
    with pytest.raises(InputError, match="simulation_number"):
        JointFit(plain).realisations()
    # blocks with different numbers of realisations: both counts named
    opts = write_stacks(tmp_path, [cases.dsplit_options(q) for q in range(3)], [5, 5, 7], tag="uneven")
    fits = [victor_amd.CCFFit(*o) for o in opts]
    joint = JointFit(fits, covariance=correlated([f.covmat for f in fits]))
    with pytest.raises(InputError, match=r"block 0 holds 5 realisations and block 2 holds 7"):
        joint.realisations()
    # a number that one block's file does not hold; numbers every file holds are fine
    with pytest.raises(InputError, match="simulation number 6 is out of range"):
        joint.realisations([0, 6])
    for bad in ([-1], [2.5], []):
        with pytest.raises(InputError):
            joint.realisations(bad)
    jr = joint.realisations([4, 0, 1])
    assert len(jr) == 3
    # a bad which: out of range, wrong length, not integers (checked before anything reaches the device)
    hp = cases.halton_params(4)
    for which in ([0, 1, 2, 3], [0, 1, -1, 0], [0, 1], [0.0, 1.0, 2.0, 0.0]):
        with pytest.raises(InputError, match="which|realisation index"):
            jr.log_likelihood_pairs(hp, which)
    # 'likelihood' beta interpolation with beta-dependent data under a joint covariance: JointFit's own refusal
    bopts = boss_stacks(tmp_path, 3)
    boss = [victor_amd.CCFFit(*o) for o in bopts]
    jb = JointFit(boss, covariance=boss_joint_cov_file(str(tmp_path / "c.npy"))).realisations()
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        jb.log_likelihood(cases.halton_params(4, with_beta=True), beta_interpolation="likelihood")
    # what JointFit._plan_cov refuses, refused the same way
    fits[1].model = dict(fits[1].model, rsd_model="dispersion")
    with pytest.raises(InputError, match="every block must share its model and fit options"):
        jr.log_likelihood(hp)


def test_the_entry_point_is_declared_exported_and_bound():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"int vk_joint_cov_eval_realisations\(vk_joint_cov\* h, vk_ctx\* const\* ctxs, int32_t n_ctx, "
                     r"const vk_eval_opts\* opts,\s+const double\* params, int64_t n, const int32_t\* which, double\* lnl, "
                     r"double\* chi2\);", header)
    assert "vk_joint_cov_eval_realisations" in N.SYMBOLS
    restype, argtypes = N.SYMBOLS["vk_joint_cov_eval_realisations"]
    assert len(argtypes) == 9
    lib = N.load()
    assert lib.vk_joint_cov_eval_realisations is not None
    assert int(re.search(r"#define VK_ABI_VERSION (\d+)", header).group(1)) == 22
    assert N.VK_ABI_VERSION == 22 and lib.vk_abi_version() == 22
    import victor
    import victor_amd
    assert victor.JointRealisations is victor_amd.JointRealisations is victor_amd.joint.JointRealisations
