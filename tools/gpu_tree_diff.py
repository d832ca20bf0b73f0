"""Outputs of two CHECKOUTS of this repository (each with its own package and its own built library) on the same inputs, bit for
bit: BOSS and config 3, every RSD model, 4099 wide-box points / 64 / 5 / 1 point (cells, point-major, polling and counter
hand-offs), theory vectors, chi2 and lnL; the joint fits - five density-split blocks block-diagonal and under a fixed joint
covariance, five BOSS-style blocks under a 31-slice beta grid, 4099 / 64 / 1 point - and the realisation paths: Realisations
in cross and pairs mode on the 16-realisation BOSS stack, JointRealisations in both modes on density-split stacks (fixed
covariance) and BOSS stacks (beta grid), the inputs of the GPU tests.  For changes that must not move a bit - a rebuild in
other translation units, a host-side refactoring - across an ABI change, which tools/gpu_lib_diff.py (one package, two
libraries) cannot cross.
Usage: gpu_tree_diff.py <checkout A> <checkout B>"""
import os
import subprocess
import sys
import tempfile

WORKER = r'''
import sys
root = sys.argv[1]
sys.path.insert(0, root)
import numpy as np
import victor_amd
from tests import cases
from tools.gpu_fuzz import params
out = {}
for name, opts, beta in (("boss", cases.boss_options("config"), True), ("config3", cases.synth_options(3), False)):
    fit = victor_amd.CCFFit(*opts)
    for rsd in ("streaming", "dispersion", "kaiser", "euclid_special"):
        for n in (4099, 64, 5, 1):
            rows = fit._fit_rows(params(n, beta, 7, 2.0), fit.model)
            out[f"{name}_{rsd}_{n}_t"] = fit.theory_vector_batch(rows, rsd_model=rsd)
            lnl, chi = fit.log_likelihood_batch(rows, rsd_model=rsd)[:2]
            out[f"{name}_{rsd}_{n}_c"] = chi
            out[f"{name}_{rsd}_{n}_l"] = lnl

import os
import tempfile
from victor_amd.joint import JointFit
from tests.test_joint_cov import boss_joint_cov_file, boss_pair_options, correlated
from tests.test_joint_realisations import boss_stacks, dsplit_stacks
from tests.test_realisations import stack_options
tmp = tempfile.mkdtemp()
dsplit = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(5)]
pair = boss_pair_options()
src = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
np.save(os.path.join(tmp, "cov5.npy"), {"beta": src["beta"], "covmat": np.array([correlated([c] * 5) for c in src["covmat"]])},
        allow_pickle=True)
grid5 = {"dir": tmp, "data_file": "cov5.npy", "cov_key": "covmat", "fixed_beta": False, "beta_key": "beta"}
for name, joint, beta in (("joint_blockdiag", JointFit(dsplit), False),
                          ("joint_fixed", JointFit(dsplit, covariance=correlated([f.covmat for f in dsplit])), False),
                          ("joint_grid", JointFit([victor_amd.CCFFit(*pair[q % 2]) for q in range(5)], covariance=grid5), True)):
    for n in (4099, 64, 1):
        lnl, chi = joint.log_likelihood_batch(params(n, beta, 7, 2.0))
        out[f"{name}_{n}_c"] = chi
        out[f"{name}_{n}_l"] = lnl

hp = cases.halton_params(64, with_beta=True)
rs = victor_amd.CCFFit(*stack_options()).realisations()
out["real_cross_l"], out["real_cross_c"] = rs.log_likelihood(hp)
out["real_pairs_l"], out["real_pairs_c"] = rs.log_likelihood_pairs(hp, (np.arange(64) * 7) % 16)

for name, opts, cov, beta in (("dsplit", dsplit_stacks(tmp, 20), "fixed", False), ("boss", boss_stacks(tmp, 20), "grid", True)):
    fits = [victor_amd.CCFFit(*o) for o in opts]
    if cov == "fixed":
        cov = correlated([f.covmat for f in fits])
    else:
        cov = boss_joint_cov_file(os.path.join(tmp, "cov_boss.npy"))
    jr = JointFit(fits, covariance=cov).realisations()
    p = params(37, beta, 9, 2.0)
    out[f"jreal_{name}_cross_l"], out[f"jreal_{name}_cross_c"] = jr.log_likelihood(p)
    which = np.random.default_rng(5).integers(0, len(jr), 37)
    out[f"jreal_{name}_pairs_l"], out[f"jreal_{name}_pairs_c"] = jr.log_likelihood_pairs(p, which)
np.savez(sys.argv[2], **out)
'''


def main():
    import numpy as np
    res = []
    for root in sys.argv[1:3]:
        f = tempfile.mktemp(suffix=".npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("VICTOR_HIP_")}
        r = subprocess.run([sys.executable, "-c", WORKER, os.path.abspath(root), f], env=env, capture_output=True, text=True, cwd=os.path.abspath(root))
        if r.returncode:
            print(r.stderr[-3000:])
            return 1
        res.append(np.load(f))
    a, b = res
    worst = 0
    for k in a.files:
        same = np.array_equal(a[k], b[k], equal_nan=True)
        if not same:
            worst += 1
            fin = np.isfinite(a[k]) & np.isfinite(b[k])
            print(f"{k}: DIFFERS, max abs {np.max(np.abs(a[k][fin] - b[k][fin])):.3e}")
    print(f"{len(a.files)} arrays compared ({sum(a[k].size for k in a.files)} doubles), {worst} differ" + ("" if worst else ": identical, bit for bit"))
    return 1 if worst else 0


if __name__ == "__main__":
    sys.exit(main())
