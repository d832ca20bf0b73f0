"""Best fits and Metropolis chains of joint fits (``JointFit`` / ``JointRealisations`` ``.best_fit`` / ``.sample_chains``,
``vk_fit_create_joint`` / ``vk_chain_create_joint``): what needs no GPU - the refusals of the parameter block, raised before any
device call with the texts of the single-fit methods, and the declaration, export and binding of the two entry points.
"""
import os
import re

import numpy as np
import pytest

from tests import cases
from tests.test_joint_cov import correlated
from tests.test_joint_realisations import write_stacks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
ALL_FIXED = {"fsigma8": 0.5, "beta": 0.4, "sigma_v": 380.0, "epsilon": 1.0}
ALPHA = {"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0}, "proposal": 0.01}


def _no_device(fits):
    def boom(*a, **k):
        raise AssertionError("a joint best_fit / sample_chains reached the device before refusing its input")
    for f in fits:
        f._get_engine = boom
    return fits


@pytest.fixture(scope="module")
def joints(tmp_path_factory):
    """(JointFit, JointRealisations) of three density-split blocks with 5 realisations each, block-diagonal and correlated."""
    import victor_amd
    from victor_amd.joint import JointFit
    opts = write_stacks(tmp_path_factory.mktemp("joint_sampled"), [cases.dsplit_options(q) for q in range(3)], 5, tag="dsplit")
    fits = _no_device([victor_amd.CCFFit(*o) for o in opts])
    out = []
    for covariance in (None, correlated([f.covmat for f in fits])):
        joint = JointFit(fits, covariance=covariance)
        out.append((joint, joint.realisations()))
    return out


def test_parameter_block_refusals_come_before_any_device_call(joints):
    from victor_amd import InputError
    for joint, jr in joints:
        for target in (joint, jr):
            with pytest.raises(InputError, match="every parameter is fixed"):
                target.best_fit(PARAMS, fixed=ALL_FIXED)
            with pytest.raises(InputError, match="every parameter is fixed"):
                target.sample_chains(PARAMS, 10, fixed=ALL_FIXED)
            with pytest.raises(InputError, match="no column"):
                target.best_fit(dict(PARAMS, alpha=ALPHA))
            with pytest.raises(InputError, match="no column"):
                target.sample_chains(dict(PARAMS, alpha=ALPHA), 10)
            with pytest.raises(InputError, match="scatter needs a start"):
                target.sample_chains(PARAMS, 10, scatter=0.1)
            with pytest.raises(InputError, match="walkers must be >= 1"):
                target.sample_chains(PARAMS, 10, walkers=0)
            with pytest.raises(InputError, match="outside"):
                target.best_fit(PARAMS, start={"fsigma8": 1.6})
        with pytest.raises(InputError, match="fixed values must be scalars"):
            jr.best_fit(PARAMS, fixed={"fsigma8": np.linspace(0.3, 0.6, 5)})
        with pytest.raises(InputError, match="fixed values must be scalars"):
            jr.sample_chains(PARAMS, 10, fixed={"fsigma8": np.linspace(0.3, 0.6, 5)})
        with pytest.raises(InputError, match="fixed values must be scalars"):
            joint.sample_chains(PARAMS, 10, fixed={"fsigma8": np.linspace(0.3, 0.6, 5)})
        with pytest.raises(InputError, match="different lengths"):                  # (arrays give a profile on JointFit.best_fit)
            joint.best_fit(PARAMS, fixed={"fsigma8": np.linspace(0.3, 0.6, 4), "sigma_v": np.array([300.0, 400.0])})


def test_signatures_are_those_of_the_single_fit_methods():
    import inspect
    import victor_amd
    from victor_amd.joint import JointFit, JointRealisations
    for cls in (JointFit, JointRealisations):
        assert inspect.signature(cls.best_fit) == inspect.signature(victor_amd.CCFFit.best_fit)
        assert inspect.signature(cls.sample_chains) == inspect.signature(victor_amd.CCFFit.sample_chains)


def test_the_two_entry_points_are_declared_exported_and_bound():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    args = (r"\(vk_ctx\* const\* ctxs, int32_t n_ctx, vk_joint_cov\* cov, const vk_eval_opts\* opts,\s+int32_t %s, "
            r"int32_t n_params, const int32_t\* columns, const double\* lo, const double\* hi,\s+const double\* base_rows, "
            r"double alpha, const int32_t\* which, char\* err, size_t errlen\);")
    assert re.search(r"vk_fit\* vk_fit_create_joint" + args % "n_problems", header)
    assert re.search(r"vk_chain\* vk_chain_create_joint" + args % "n_chains", header)
    lib = N.load()
    for name in ("vk_fit_create_joint", "vk_chain_create_joint"):
        restype, argtypes = N.SYMBOLS[name]
        assert len(argtypes) == 14 and restype is N.SYMBOLS["vk_fit_create"][0]
        assert argtypes[3:] == N.SYMBOLS["vk_fit_create"][1][1:]                     # (after ctxs, n_ctx, cov: those of vk_fit_create)
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define VK_ABI_VERSION (\d+)", header).group(1)) == 22
    assert N.VK_ABI_VERSION == 22 and lib.vk_abi_version() == 22
