"""Accuracy of the shared reciprocals (vk_devmath.h: recip_shared2 / 3 / 4 - one v_rcp_f64 for the 1/sigma_v of a block of velocity
nodes) measured on the hardware itself."""

import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_reciprocals_within_their_rounding_bound(tmp_path):
    """tools/shared_recip_check.hip: 2^20 blocks of 2, 3 and 4 operands, magnitudes log-uniform in [2^-8, 2^8], mixed signs, plus
    1, powers of two and the neighbours of 1, against 1.0 / x in double on the host.  Every result within
    (k + 1) 2^-53 + e_max^3 - k the multiplies on the operand's path (2 for a pair; 4, 4, 3 for a triple; 5 for a quad), e_max the
    worst seed error |1 - P rcp(P)| the same run measures on the same products - and of the operand's sign."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = os.path.join(ROOT, "tools", "shared_recip_check")
    src = os.path.join(ROOT, "tools", "shared_recip_check.hip")
    hdr = os.path.join(ROOT, "victor_amd", "csrc", "vk_devmath.h")
    if not os.path.isfile(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        exe = str(tmp_path / "shared_recip_check")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-I", os.path.join(ROOT, "victor_amd", "csrc"),
                               src, "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.check_output([exe]).decode().strip().splitlines()[-1]
    res = json.loads(out)
    assert res["blocks"] == 1 << 20
    for width in (2, 3, 4):
        r = res[f"w{width}"]
        print(f"width {width}: worst error {r['err']:.3e} of bound {r['bound']:.3e} (margin {r['margin']:.3f}), seed error {r['e_max']:.2e}")
        assert r["signs_ok"] == 1
        assert 1e-9 < r["e_max"] < 1e-6                       # the raw v_rcp_f64 seed, as tests/test_gpu_devmath.py finds it
        assert r["margin"] <= 1.0, r
    assert res["ok"] == 1
