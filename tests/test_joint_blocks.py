"""Per-block parameters of a joint fit (``"name@q"``: victor_amd/joint.py) without a GPU: name resolution and the refusals, the
selection rule of victor_amd/csrc/vk_row_select.h compiled on its own under g++ against a NumPy restatement, and the C ABI's
surface."""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.test_joint_cov import boss_joint_cov_file, boss_pair_options, correlated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = cases.cobaya_info()["params"]
NEW = ("vk_joint_eval_blocks_device_async", "vk_joint_cov_eval_blocks_device_async", "vk_joint_cov_eval_realisations_blocks",
       "vk_fit_create_joint_blocks", "vk_chain_create_joint_blocks")


def boom(*a, **k):
    raise AssertionError("the call reached the device before refusing its input")


def no_device(joint):
    for f in joint.fits:
        f._get_engine = boom
    return joint


@pytest.fixture(scope="module")
def joints(tmp_path_factory):
    import victor_amd
    from victor_amd.joint import JointFit
    ds = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(3)]
    boss = [victor_amd.CCFFit(*o) for o in boss_pair_options()]
    grid = boss_joint_cov_file(str(tmp_path_factory.mktemp("blocks") / "joint_cov.npy"))
    return {"diag": no_device(JointFit(ds)), "cov": no_device(JointFit(ds, covariance=correlated([f.covmat for f in ds]))),
            "grid": no_device(JointFit(boss, covariance=grid, likelihood={"form": "gaussian"}))}


# ------------------------------------------------------------------ 1. names
def test_names_resolve_per_block():
    from victor_amd import InputError
    from victor_amd.joint import block_params, has_block_names, per_block, split_name
    assert split_name("sigma_v@2") == ("sigma_v", 2) and split_name("sigma_v") == ("sigma_v", None)
    for bad in ("sigma_v@", "sigma_v@x", "sigma_v@-1", "sigma_v@1.0", "@1", "sigma_v@1@2"):
        with pytest.raises(InputError, match="<name>@<block>"):
            split_name(bad)
    p = {"fsigma8": 0.47, "sigma_v": 380.0, "sigma_v@1": 300.0, "bias@2": 1.9}
    assert has_block_names(p) and not has_block_names({"sigma_v": 1.0}) and not has_block_names(np.zeros((1, 12)))
    assert block_params(p, 0) == {"fsigma8": 0.47, "sigma_v": 380.0}
    assert block_params(p, 1) == {"fsigma8": 0.47, "sigma_v": 300.0}
    assert block_params(p, 2) == {"fsigma8": 0.47, "sigma_v": 380.0, "bias": 1.9}
    out = per_block(PARAMS, ["sigma_v"], 5)
    assert "sigma_v" not in out and [k for k in out if "@" in k] == [f"sigma_v@{q}" for q in range(5)]
    for q in range(5):
        assert out[f"sigma_v@{q}"] == PARAMS["sigma_v"] and out[f"sigma_v@{q}"] is not PARAMS["sigma_v"]
    assert list(out)[list(PARAMS).index("sigma_v")] == "sigma_v@0"                # at the entry's own place in the block
    assert {k: v for k, v in out.items() if "@" not in k} == {k: v for k, v in PARAMS.items() if k != "sigma_v"}
    assert "sigma_v" in PARAMS                                                     # (the input is left alone)
    with pytest.raises(InputError, match="not in the params block"):
        per_block(PARAMS, ["sigma_w"], 3)
    with pytest.raises(InputError, match="alpha"):
        per_block(dict(PARAMS, alpha=1.0), ["alpha"], 3)


def test_refusals_come_before_any_device_call(joints):
    import victor_amd
    from victor_amd import InputError
    pt = {"fsigma8": 0.47, "beta": 0.4, "epsilon": 1.0, "sigma_v": 380.0}
    calls = []
    for name, joint in joints.items():
        calls += [(name, lambda p, j=joint: j.log_likelihood(p)), (name, lambda p, j=joint: j.log_likelihood_batch(p)),
                  (name, lambda p, j=joint: j._sequential(p, {}))]
    for name, call in calls:
        B = len(joints[name].fits)
        with pytest.raises(InputError, match=f"names block {B} of {B}"):
            call(dict(pt, **{f"sigma_v@{B}": 300.0}))
        with pytest.raises(InputError, match="<name>@<block>"):
            call(dict(pt, **{"sigma_v@one": 300.0}))
        with pytest.raises(InputError, match="alpha is one scalar"):
            call(dict(pt, **{"alpha@0": 1.0}))
    for call in (c for n, c in calls if n == "grid"):
        with pytest.raises(InputError, match="shares one beta"):
            call(dict(pt, **{"beta@1": 0.41}))
    # epsilon@q and (without a beta grid) beta@q pass the name checks: the call goes on to the device
    for name in ("diag", "cov"):
        with pytest.raises(AssertionError, match="reached the device"):
            joints[name].log_likelihood(dict(pt, **{"epsilon@1": 1.01, "beta@0": 0.41}))
    with pytest.raises(AssertionError, match="reached the device"):
        joints["grid"].log_likelihood(dict(pt, **{"epsilon@1": 1.01}))
    # best fits and chains: sampled and fixed names, start / step / xtol / proposal / scatter naming an unsampled @ name
    joint = joints["cov"]
    from victor_amd.joint import per_block
    blk = per_block(PARAMS, ["sigma_v"], 3)
    fixed = {"beta": 0.4, "epsilon": 1.0}
    for run in (lambda **kw: joint.best_fit(kw.pop("params", blk), **kw), lambda **kw: joint.sample_chains(kw.pop("params", blk), 5, **kw)):
        with pytest.raises(InputError, match="names block 3 of 3"):
            run(params=per_block(PARAMS, ["sigma_v"], 4), fixed=fixed)
        with pytest.raises(InputError, match="names block 7 of 3"):
            run(fixed=dict(fixed, **{"bias@7": 2.0}))
        with pytest.raises(InputError, match="alpha is one scalar"):
            run(fixed=dict(fixed, **{"alpha@0": 1.0}))
        with pytest.raises(InputError, match="start names parameters that are not"):
            run(fixed=fixed, start={"sigma_v@0": 350.0, "bias@1": 2.0})
        with pytest.raises(InputError, match="start names parameters that are not"):
            run(fixed=dict(fixed, **{"sigma_v@2": 400.0}), start={"sigma_v@2": 350.0})
        with pytest.raises(AssertionError, match="reached the device"):
            run(fixed=fixed, start={"sigma_v@0": 350.0})
    with pytest.raises(InputError, match="step names parameters that are not fitted"):
        joint.best_fit(blk, fixed=fixed, step={"sigma_v": 10.0})
    with pytest.raises(InputError, match="xtol names parameters that are not fitted"):
        joint.best_fit(blk, fixed=fixed, xtol={"Av@0": 10.0})
    with pytest.raises(InputError, match="proposal names parameters that are not sampled"):
        joint.sample_chains(blk, 5, fixed=fixed, proposal={"sigma_v": 10.0})
    with pytest.raises(InputError, match="scatter names parameters that are not sampled"):
        joint.sample_chains(blk, 5, fixed=fixed, start={"sigma_v@1": 300.0}, scatter={"sigma_v@3": 1.0})
    with pytest.raises(InputError, match="shares one beta"):
        joints["grid"].best_fit(per_block(PARAMS, ["beta"], 2))
    with pytest.raises(InputError, match="shares one beta"):
        joints["grid"].sample_chains(PARAMS, 5, fixed={"beta@0": 0.4})
    # a plain sampled name beside an @ entry of the same name, sampled or fixed: the device cannot write "all blocks but q"
    for run in (joint.best_fit, lambda p, **kw: joint.sample_chains(p, 5, **kw)):
        with pytest.raises(InputError, match=r"\['sigma_v'\] cannot be .* beside per-block entries .*\['sigma_v@0'\]"):
            run(PARAMS, fixed=dict(fixed, **{"sigma_v@0": 300.0}))
        with pytest.raises(InputError, match=r"\['sigma_v'\] cannot be .* beside per-block entries"):
            run(dict(PARAMS, **{"sigma_v@2": PARAMS["sigma_v"]}), fixed=fixed)
        with pytest.raises(InputError, match=r"\['sigma_v'\] cannot be .* beside per-block entries"):
            run(dict(PARAMS, **{"sigma_v@1": 310.0}), fixed=fixed)               # (a fixed entry of the cobaya block)
        with pytest.raises(AssertionError, match="reached the device"):         # a fixed plain name beside @ entries is fine
            run(dict(blk, **{"sigma_v@0": 300.0}), fixed=dict(fixed, sigma_v=380.0))
        with pytest.raises(AssertionError, match="reached the device"):
            run({k: v for k, v in blk.items() if k != "sigma_v@0"}, fixed=dict(fixed, **{"sigma_v@0": 300.0}))
    with pytest.raises(InputError, match="no column of its own"):
        joint.best_fit(dict(blk, **{"aperp@0": PARAMS["sigma_v"]}), fixed=fixed)
    # a single fit has no blocks
    fit = victor_amd.CCFFit(*cases.dsplit_options(0))
    fit._get_engine = boom
    for call in (lambda: fit.log_likelihood(dict(pt, **{"sigma_v@0": 300.0})),
                 lambda: fit.log_likelihood_batch({"fsigma8": np.array([0.4, 0.5]), "beta": 0.4, "sigma_v@0": 300.0}),
                 lambda: fit.best_fit(blk, fixed=fixed), lambda: fit.sample_chains(blk, 5, fixed=fixed),
                 lambda: fit.best_fit(PARAMS, fixed=dict(fixed, **{"sigma_v@0": 300.0}))):
        with pytest.raises(InputError, match="need a JointFit"):
            call()


def test_an_eleventh_sampled_value_is_refused_before_any_device_call(joints):
    """kMaxP = 10 sizes the kernels' by-value arguments: three blocks with fsigma8, sigma_v and bias of their own plus beta and
    epsilon are eleven sampled values, and ten of them (epsilon fixed) pass the check and go on to the device."""
    from victor_amd import InputError
    from victor_amd.joint import per_block
    eleven = per_block(dict(PARAMS, bias={"prior": {"min": 1.0, "max": 3.0}, "ref": {"loc": 2.0, "scale": 0.1}, "proposal": 0.05}),
                       ["fsigma8", "sigma_v", "bias"], 3)
    joint = joints["cov"]
    with pytest.raises(InputError, match="at most 10 sampled parameters"):
        joint.sample_chains(eleven, 5)
    with pytest.raises(InputError, match="at most 10 sampled parameters"):
        joint.sample_chains(eleven, 5, move="stretch", walkers=24)
    with pytest.raises(AssertionError, match="reached the device"):
        joint.sample_chains(eleven, 5, fixed={"epsilon": 1.0})


def test_block_rows_are_each_blocks_own_rows(joints):
    """The row of block q is ``fits[q]._fit_rows`` of the dictionary resolved for it - scalars broadcast over a batch."""
    from victor_amd import _native as N
    joint = joints["diag"]
    n = 4
    p = {"fsigma8": np.linspace(0.4, 0.5, n), "beta": 0.4, "epsilon": 1.0, "sigma_v": 380.0, "sigma_v@1": np.linspace(300, 330, n),
         "epsilon@2": 1.02, "bias@0": 1.7}
    rows = joint._block_rows(p, {})
    assert rows.shape == (3, n, N.VK_NPAR) and rows.flags.c_contiguous
    for q, f in enumerate(joint.fits):
        own = {"fsigma8": p["fsigma8"], "beta": 0.4, "epsilon": 1.02 if q == 2 else 1.0, "sigma_v": p["sigma_v@1"] if q == 1 else 380.0}
        if q == 0:
            own["bias"] = 1.7
        assert rows[q].tobytes() == np.ascontiguousarray(f._fit_rows(own, f.model)).tobytes(), q
    assert rows[0, 0, N.P_BIAS] == 1.7 and rows[2, 0, N.P_EPSILON] == 1.02 and rows[1, 3, N.P_SIGMAV] == 330.0
    one = joint._block_rows({"fsigma8": 0.47, "beta": 0.4, "sigma_v@0": 300.0}, {})
    assert one.shape == (3, 1, N.VK_NPAR) and list(one[:, 0, N.P_SIGMAV]) == [300.0, 380.0, 380.0]


# ------------------------------------------------------------------ 2. the selection rule under g++
DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vk_row_select.h"
// stdin: B n d alpha | col[d] | param_block[d] | base [B][n][12] | x [n][d]   stdout: rows [B][n][12] as %a
int main() {
  int B, n, d;
  double alpha;
  if (scanf("%d %d %d %la", &B, &n, &d, &alpha) != 4 || d > vkrow::kMaxP) return 2;
  int col[vkrow::kMaxP] = {};
  vkrow::Blocks b = vkrow::one_set();
  b.n = B;
  b.row_stride = b.base_stride = (long long)n * vkrow::kNpar;
  for (int j = 0; j < d; ++j) if (scanf("%d", &col[j]) != 1) return 2;
  for (int j = 0; j < d; ++j) if (scanf("%d", &b.param_block[j]) != 1) return 2;
  std::vector<double> base((size_t)B * n * vkrow::kNpar), x((size_t)n * d), rows(base.size(), -7.0);
  for (double& v : base) if (scanf("%la", &v) != 1) return 2;
  for (double& v : x) if (scanf("%la", &v) != 1) return 2;
  for (int r = 0; r < n; ++r)
    vkrow::form_rows(b, base.data(), r, rows.data(), r, col, d, alpha, [&](int j) { return x[(size_t)r * d + j]; },
                     [](double e) { return std::pow(e, -2.0 / 3.0); });
  for (double v : rows) printf("%a\n", v);
  return 0;
}
"""


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("row_select")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(base, x, col, block, alpha):
        B, n, _ = base.shape
        text = " ".join([f"{B} {n} {len(col)} {float(alpha).hex()}", *map(str, col), *map(str, block),
                         *(float(v).hex() for v in base.ravel()), *(float(v).hex() for v in x.ravel())])
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split()
        return np.array([float.fromhex(v) for v in out]).reshape(base.shape)
    return run


def restated(base, x, col, block, alpha):
    """The rule in NumPy: block q's row is its base row with value j written where block[j] is -1 or q, in the order of j."""
    from victor_amd import _native as N
    rows = base.copy()
    for q in range(len(base)):
        for j, (c, b) in enumerate(zip(col, block)):
            if b >= 0 and b != q:
                continue
            if c >= 0:
                rows[q, :, c] = x[:, j]
            else:
                aperp, apar = N.epsilon_to_ap(x[:, j], alpha)
                rows[q, :, N.P_APERP], rows[q, :, N.P_APAR], rows[q, :, N.P_EPSILON] = aperp, apar, x[:, j]
    return rows


@pytest.mark.parametrize("eps,alpha", [(None, 1.0), ("shared", 1.0), ("shared", 1.03), ("per_block", 1.0), ("per_block", 0.98)])
def test_selection_rule_against_numpy(select, eps, alpha):
    """B = 3, d = 5: shared and per-block columns mixed; epsilon absent, shared, or one block's own.  Without epsilon the rows
    are the restatement's bytes; with it, the two AP columns agree to 1 ulp (pow here is libm's on both sides, a product may
    differ by a rounding) and every other column stays the same bytes."""
    from victor_amd import _native as N
    rng = np.random.default_rng(8)
    B, n = 3, 7
    base = rng.random((B, n, N.VK_NPAR)) + 0.5
    col = [N.P_FSIGMA8, N.P_SIGMAV, N.P_SIGMAV, N.P_BIAS, N.P_AV]
    block = [-1, 0, 2, 1, -1]
    if eps is not None:
        col[4] = N.VK_WALK_EPSILON
        block[4] = -1 if eps == "shared" else 1
    x = rng.random((n, 5)) + 0.6
    got, want = select(base, x, col, block, alpha), restated(base, x, col, block, alpha)
    ap = [N.P_APERP, N.P_APAR]
    rest = [c for c in range(N.VK_NPAR) if c not in ap]
    assert got[:, :, rest].tobytes() == want[:, :, rest].tobytes()
    if eps is None:
        assert got.tobytes() == want.tobytes()
    else:
        assert np.all(np.abs(got[:, :, ap] - want[:, :, ap]) <= np.spacing(np.abs(want[:, :, ap])))
        touched = [0, 1, 2] if eps == "shared" else [1]
        for q in range(B):
            assert (got[q, :, N.P_EPSILON].tobytes() == x[:, 4].tobytes()) == (q in touched)
            if q not in touched:
                assert got[q][:, ap].tobytes() == base[q][:, ap].tobytes()
    # what each block received: sigma_v of block 0 and 2 their own values, block 1 its base; bias of block 1 alone
    assert got[0, :, N.P_SIGMAV].tobytes() == x[:, 1].tobytes() and got[2, :, N.P_SIGMAV].tobytes() == x[:, 2].tobytes()
    assert got[1, :, N.P_SIGMAV].tobytes() == base[1, :, N.P_SIGMAV].tobytes()
    assert got[1, :, N.P_BIAS].tobytes() == x[:, 3].tobytes() and got[0, :, N.P_BIAS].tobytes() == base[0, :, N.P_BIAS].tobytes()
    for q in range(B):
        assert got[q, :, N.P_FSIGMA8].tobytes() == x[:, 0].tobytes()


def test_one_row_set_is_the_row_of_a_handle_without_blocks(select):
    from victor_amd import _native as N
    rng = np.random.default_rng(9)
    base, x = rng.random((1, 5, N.VK_NPAR)), rng.random((5, 3)) + 0.5
    col = [N.P_FSIGMA8, N.P_SIGMAV, N.P_BETA]
    want = base.copy()
    want[0][:, col] = x
    assert select(base, x, col, [-1, -1, -1], 1.0).tobytes() == want.tobytes()


def test_selection_header_is_free_of_hip():
    text = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_row_select.h")).read()
    assert "hip/" not in text and "#include <" not in text.replace("#include <stddef.h>", "")
    row = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_sampled_row.h")).read()
    assert "vkrow::form_rows" in row and row.count("pow(") == 1


# ------------------------------------------------------------------ 3. the C ABI's surface
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    ctype = {"vk_ctx* const*": C.POINTER(C.c_void_p), "vk_joint_cov*": C.c_void_p, "const vk_eval_opts*": C.POINTER(N.vk_eval_opts),
             "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t, "char*": C.c_char_p,
             "const int32_t*": C.POINTER(C.c_int32)}
    device = {"const double*": C.c_void_p, "double*": C.c_void_p}
    host = {"const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double)}
    for name in NEW:
        decl = re.search(r"(int|vk_fit\*|vk_chain\*) %s\(([^)]*)\);" % name, header)
        assert decl, f"include/victor_hip.h does not declare {name}"
        args = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in decl.group(2).split(",")]
        res, proto = N.SYMBOLS[name]
        assert res is (C.c_int if decl.group(1) == "int" else C.c_void_p)
        table = dict(ctype, **(device if name.endswith("device_async") else host))
        assert proto == [table[t] for t, _ in args], name
        old = name.replace("_blocks", "")
        extra = {"par_stride"} if "eval" in name and "realisations" not in name else {"param_block"} if "create" in name else set()
        old_args = [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in
                    re.search(r"%s\(([^)]*)\);" % old, header).group(1).split(",")]
        assert [a for a in args if a[1] not in extra] == old_args, name       # the sibling's arguments, in its order
        assert {a[1] for a in args} - {a[1] for a in old_args} == extra, name


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    path = N.library_path()
    lib = C.CDLL(path)
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
