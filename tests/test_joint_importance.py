"""Importance-sampled posteriors of joint fits without a GPU (victor_amd/importance.py, JointRealisations.importance_posterior;
DESIGN.md section 7e): per-block names on the definition route (``evaluate=`` with ``n_blocks=``), the refusals that come before
the first evaluation, ``GaussianProposal.from_fits`` with ``@`` names, and the C ABI surface of ``vk_is_create_joint`` and
``vk_is_create_joint_blocks``.  The device route: tests/test_gpu_joint_importance.py."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests.test_chains import same_bytes
from tests.test_importance import EXACT, SUMS, Recorder, raiser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOINT = ("vk_is_create_joint", "vk_is_create_joint_blocks")
SPEC = {"prior": {"min": -1.0, "max": 1.0}, "ref": {"loc": 0.0, "scale": 0.1}, "proposal": 0.1}
BLOCK = {"a": SPEC, "b": {"prior": {"min": -1.0, "max": 2.0}, "ref": {"loc": 0.5, "scale": 0.1}, "proposal": 0.1}, "fixed_one": 2.5}


def lnl_of(a, b0, b1, b2):
    """Two problems on (a, b of block 0, 1, 2): each block a Gaussian in (a, its b), the second problem narrower."""
    q = sum(3.0 * (a - 0.2) ** 2 + (1.0 + k) * (b - 0.4 - 0.1 * k) ** 2 for k, b in enumerate((b0, b1, b2)))
    return np.stack([-0.5 * q, -1.5 * q], axis=1)


def per_block_evaluator(batch):
    assert set(batch) == {"a", "b@0", "b@1", "b@2", "fixed_one"} and np.all(batch["fixed_one"] == 2.5)
    return lnl_of(batch["a"], batch["b@0"], batch["b@1"], batch["b@2"])


def plain_evaluator(batch):
    assert set(batch) == {"a", "b0", "b1", "b2", "fixed_one"}
    return lnl_of(batch["a"], batch["b0"], batch["b1"], batch["b2"])


def proposal(names):
    from victor_amd import GaussianProposal
    return GaussianProposal(names, [0.2, 0.4, 0.5, 0.6], np.diag([0.4, 0.5, 0.4, 0.3]) ** 2)


def test_per_block_names_are_labels_on_the_definition_route():
    """``evaluate=`` with ``n_blocks=3``: the call runs, the callable sees the ``@`` keys, and every raw output equals, as bytes,
    that of the same call with the three columns under plain names."""
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import per_block
    block = per_block(BLOCK, ["b"], 3)
    names = ["a", "b@0", "b@1", "b@2"]
    assert [n for n in block if n != "fixed_one"] == names
    kw = dict(n=300, seed=3, bins=5, chunk=64, min_ess=2.0, device=False)
    rec = Recorder(per_block_evaluator)
    own = importance_posterior(None, block, proposal(names), evaluate=rec, n_blocks=3, pairs=[("b@2", "a")], **kw)
    assert own.names == names and own.n_problems == 2 and len(rec.chunks) == own.n_chunks > 1 and 100 < own.n_inside <= 300
    assert np.all(own.status == own.OK) and own.marginal("b@1").shape == (2, 5) and own.marginal2d("a", "b@2").shape == (2, 5, 5)
    plain_block = {"a": BLOCK["a"], "b0": BLOCK["b"], "b1": BLOCK["b"], "b2": BLOCK["b"], "fixed_one": 2.5}
    plain = importance_posterior(None, plain_block, proposal(["a", "b0", "b1", "b2"]), evaluate=plain_evaluator, pairs=[("b2", "a")], **kw)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(own.raw, name), getattr(plain.raw, name)), name
    assert same_bytes(own.ln_evidence, plain.ln_evidence) and same_bytes(own.cov, plain.cov)
    # a fixed per-block value reaches the callable under its own key, and a prior may name a per-block parameter
    from victor_amd.priors import GaussianPrior

    def fixed_too(batch):
        assert np.all(batch["c@1"] == 7.0)
        return per_block_evaluator({k: v for k, v in batch.items() if k != "c@1"})
    with_prior = importance_posterior(None, block, proposal(names), evaluate=fixed_too, n_blocks=3, fixed={"c@1": 7.0},
                                      prior=GaussianPrior(["b@1"], [0.5], sigma=[0.3]), **kw)
    assert not same_bytes(with_prior.ln_max, own.ln_max) and np.isfinite(with_prior.prior_ln_max)


def test_the_method_and_the_module_function():
    import victor_amd
    from victor_amd import importance
    assert hasattr(victor_amd.joint.JointRealisations, "importance_posterior")
    assert not hasattr(victor_amd.JointFit, "importance_posterior")            # (the joint data vector: the module function)
    sig = inspect.signature(victor_amd.joint.JointRealisations.importance_posterior)
    assert list(sig.parameters) == ["self", "params", "proposal", "n", "seed", "fixed", "prior", "bins", "ranges", "pairs", "chunk", "min_ess",
                                    "device", "evaluate", "sample", "ln_proposal", "kwargs"]
    other = inspect.signature(victor_amd.Realisations.importance_posterior)
    for (_, a), (_, b) in zip(list(sig.parameters.items())[3:], list(other.parameters.items())[3:]):
        assert (a.name, a.default, a.kind) == (b.name, b.default, b.kind)
    assert "n_blocks" in inspect.signature(importance.importance_posterior).parameters
    assert "no ``importance_posterior`` method" in importance.importance_posterior.__doc__


def test_abi_surface_of_the_joint_creators():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    for name in JOINT:
        assert re.search(r"\b%s\(" % name, header), f"include/victor_hip.h does not declare {name}"
        assert name in N.SYMBOLS, name
    ip, vpp = C.POINTER(C.c_int32), C.POINTER(C.c_void_p)
    single = N.SYMBOLS["vk_is_create"][1]
    assert len(single) == 21
    # the joint forms: contexts, their number and the covariance handle for the context; _blocks: param_block behind the columns
    assert N.SYMBOLS["vk_is_create_joint"] == (C.c_void_p, [vpp, C.c_int32, C.c_void_p] + single[1:])
    assert N.SYMBOLS["vk_is_create_joint_blocks"] == (C.c_void_p, [vpp, C.c_int32, C.c_void_p] + single[1:4] + [ip] + single[4:])
    for name, n_args in (("vk_is_create", 21), ("vk_is_create_joint", 23), ("vk_is_create_joint_blocks", 24)):
        decl = re.search(r"vk_is\* %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == n_args, (name, decl)


def test_library_exports_the_joint_creators():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in JOINT:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22


def test_the_new_refusals_come_before_the_first_evaluation():
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import per_block
    from victor_amd.utils import InputError
    block = per_block(BLOCK, ["b"], 3)
    names = ["a", "b@0", "b@1", "b@2"]

    def refused(match, block=block, q=None, **kw):
        with pytest.raises(InputError, match=match):
            importance_posterior(None, block, q if q is not None else proposal(names), device=False, evaluate=raiser, **kw)
    refused("per-block")                                                        # @ names without n_blocks or a joint fit
    refused("per-block", block=BLOCK, q=proposal(names), fixed={"c@0": 1.0})
    refused(r"b@2 names block 2 of 2", n_blocks=2)                              # name@q with q >= B
    refused(r"c@3 names block 3 of 3", n_blocks=3, fixed={"c@3": 1.0})
    refused("alpha is one scalar", n_blocks=3, fixed={"alpha@1": 1.0})
    refused("n_blocks must be an integer >= 1", n_blocks=0)
    refused("n_blocks must be an integer >= 1", n_blocks=2.5)
    eps = per_block(dict(BLOCK, epsilon=SPEC), ["epsilon"], 2)
    refused("epsilon cannot be sampled per block", block=eps, n_blocks=2)        # a sampled epsilon@q
    with pytest.raises(InputError, match="n_blocks goes with an evaluate callable"):
        importance_posterior(object(), block, proposal(names), n_blocks=3)     # (a fit knows its blocks)
    # a fixed epsilon@q is fine
    seen = []

    def fine(batch):
        seen.append(sorted(batch))
        return -0.5 * (batch["a"] ** 2 + batch["b"] ** 2)
    from victor_amd import GaussianProposal
    ip = importance_posterior(None, BLOCK, GaussianProposal(["a", "b"], [0.0, 0.0], 0.25 * np.eye(2)), n=64, device=False, evaluate=fine,
                              n_blocks=2, fixed={"epsilon@1": 1.01})
    assert ip.n_problems == 1 and "epsilon@1" in seen[0]


def test_a_joint_fit_without_a_gpu_reaches_the_checks(tmp_path):
    """A JointFit is no longer refused outright: its refusals are those of the other joint loops, before any device call."""
    import victor_amd
    from tests import cases
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import JointFit, per_block
    from victor_amd.utils import InputError
    joint = JointFit([victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(2)])
    params = cases.cobaya_info()["params"]
    names = [n for n, v in params.items() if isinstance(v, dict) and "prior" in v]
    mid = {n: 0.5 * (params[n]["prior"]["min"] + params[n]["prior"]["max"]) for n in names}

    def q_of(ns):
        return victor_amd.GaussianProposal(ns, [mid[n.partition("@")[0]] for n in ns], np.diag([1e-4] * len(ns)))
    with pytest.raises(InputError, match="names block 2 of 2"):
        importance_posterior(joint, params, q_of(names), n=8, fixed={"sigma_v@2": 380.0})
    own = per_block(params, ["epsilon"], 2)
    with pytest.raises(InputError, match="epsilon cannot be sampled per block"):
        importance_posterior(joint, own, q_of([n for n in own if isinstance(own[n], dict) and "prior" in own[n]]), n=8)
    with pytest.raises(InputError, match="beside per-block entries of the same name"):
        importance_posterior(joint, params, q_of(names), n=8, fixed={"sigma_v@0": 380.0})
    with pytest.raises(InputError, match="no column of its own"):
        importance_posterior(joint, dict(params, nonsense={"prior": {"min": 0.0, "max": 1.0}}), q_of(names), n=8)


def test_from_fits_keeps_the_order_of_per_block_names():
    from victor_amd import BestFit, GaussianProposal
    names = ["fsigma8", "sigma_v@0", "sigma_v@1", "sigma_v@2", "epsilon"]
    rng = np.random.default_rng(7)
    scale = np.array([0.02, 10.0, 20.0, 30.0, 0.01])
    centre = np.array([0.45, 350.0, 370.0, 390.0, 1.0])
    x = centre + scale * rng.standard_normal((6, 5))
    status = np.full(6, BestFit.CONVERGED, dtype=np.int32)
    bf = BestFit(names, x, {"beta": np.full(6, 0.4)}, np.zeros(6), np.zeros(6), status, np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.int64))

    class Lap:
        cov = np.repeat(np.diag(scale ** 2)[None], 6, axis=0)
    Lap.names = names
    q = GaussianProposal.from_fits(bf, Lap, inflate=2.0)
    assert q.names == names and np.allclose(q.mean, x.mean(axis=0))
    assert np.allclose(q.cov, 2.0 * (np.cov(x, rowvar=False) + np.diag(scale ** 2)))
    mean, chol = q.ordered("test", names)                         # usable: in the sampled order as it stands
    assert same_bytes(mean, q.mean) and np.allclose(chol @ chol.T, q.cov)
    swapped = ["epsilon", "sigma_v@2", "fsigma8", "sigma_v@0", "sigma_v@1"]
    mean, chol = q.ordered("test", swapped)                       # ... and in any other
    at = [names.index(n) for n in swapped]
    assert same_bytes(mean, q.mean[at]) and np.allclose(chol @ chol.T, q.cov[np.ix_(at, at)])
    # usable: a call whose params block lists the names in another order than the proposal does draws around the right means
    from victor_amd.importance import importance_posterior
    spec = {"fsigma8": (0.2, 0.7), "sigma_v": (200.0, 600.0), "epsilon": (0.8, 1.2)}
    block = {n: {"prior": {"min": spec[n.partition("@")[0]][0], "max": spec[n.partition("@")[0]][1]}} for n in swapped}
    prec = {n: 1.0 / q.cov[j, j] for j, n in enumerate(names)}

    def gauss(batch):
        return -0.5 * sum(prec[n] * (batch[n] - q.mean[j]) ** 2 for j, n in enumerate(names))
    ip = importance_posterior(None, block, q, n=4096, seed=1, device=False, evaluate=gauss, n_blocks=3)
    assert ip.names == swapped and ip.status[0] == ip.OK and ip.ess[0] > 500
    assert np.all(np.abs(ip.mean[0] - q.mean[at]) <= 4 * ip.sigma[0] / np.sqrt(ip.ess[0]))
