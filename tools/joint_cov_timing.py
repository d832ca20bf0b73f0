"""The five density-split blocks (config-3 options, N = 5 x 120) at batch 16384: the joint fit under one full covariance
(vk_joint_cov_eval_device_async) against the block-diagonal path (vk_joint_eval_device_async), fixed and beta-gridded.  Device
buffers are allocated once; each timed call is one enqueue and a synchronisation, medians of STEPS calls after a warm-up, the
two paths alternated.  The gridded case is a 31-slice covariance (slice k = (1 + k / 100) C_joint) entered through the C ABI
with beta drawn over the grid, so the points are sorted into 31 buckets.  Writes joint_cov_timing.txt into the output
directory.  Run under ``rocprofv3 --kernel-trace --stats --output-format csv`` for the theory / chi-square split; ``--trace FILE``
then summarises its kernel_trace.csv into joint_cov_kernels.txt.

    python tools/joint_cov_timing.py OUT_DIR [--commit SHA]
    python tools/joint_cov_timing.py OUT_DIR --trace kernel_trace.csv
"""
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases  # noqa: E402
from victor_amd import _native as N  # noqa: E402

PEAK_FP64 = 78.6e12          # MI355X FP64 vector and matrix peak (AMD specification)
BATCH = 16384
STEPS = 20
N_BETA = 31


def correlated(blocks, rho=0.5):
    import scipy.linalg as sl
    L = sl.block_diag(*[np.linalg.cholesky(c) for c in blocks])
    q = np.arange(len(blocks))
    return L @ np.kron(rho ** np.abs(q[:, None] - q[None, :]), np.eye(blocks[0].shape[0])) @ L.T


def median_ms(fn, sync, steps=STEPS):
    fn()
    sync()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)) * 1e3


def summarise_trace(path, out):
    """Theory launches against the joint chi-square kernel (fixed / 31 slices) and the sort, from rocprofv3's kernel_trace.csv:
    per-dispatch durations, medians; a chi-square dispatch that follows the sort kernels belongs to the gridded covariance."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    prev = ""
    for r in rows:
        name = r["Kernel_Name"]
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3          # us
        if "vk_joint_chi2_kernel" in name:
            g = "joint chi2, 31 slices" if "scatter" in prev else "joint chi2, fixed"
        elif "vk_joint_sum_kernel" in name:
            g = "block-diagonal sum"
        elif "vk_joint_" in name:
            g = "joint sort (3 kernels)"
        elif "vk_theory" in name:
            g = "theory launch (5 overlap)"
        elif "vk_like" in name:
            g = "block chi2 (5 overlap)"
        else:
            continue
        prev = name if "vk_joint" in name else prev
        groups.setdefault(g, []).append(dur)
    lines = ["rocprofv3 --kernel-trace --stats of tools/joint_cov_timing.py (both paths, warm-up included); per-dispatch durations, us"]
    for g, v in groups.items():
        if "sort" in g:                                            # three dispatches per call: their sum per call
            lines.append(f"{g:26s} dispatches {len(v):5d}  per call {3 * float(np.sum(v)) / len(v):10.1f}")
        else:
            lines.append(f"{g:26s} dispatches {len(v):5d}  median {np.median(v):10.1f}  mean {np.mean(v):10.1f}")
    flops = 2.0 * BATCH * 600 * 600
    for g, forms in (("joint chi2, fixed", 1), ("joint chi2, 31 slices", 2)):
        if g in groups:
            t = float(np.median(groups[g])) * 1e-6
            lines.append(f"{g}: {t * 1e3:.3f} ms = {forms * flops / t / 1e12:.2f} TF/s at {forms} form(s) per point "
                         f"({forms} x 2 n NT^2) = {forms * flops / t / PEAK_FP64:.3f} of the {PEAK_FP64 / 1e12:.1f} TF/s FP64 peak")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out, "joint_cov_kernels.txt"), "w") as fh:
        fh.write(text)


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    if "--trace" in sys.argv:
        summarise_trace(sys.argv[sys.argv.index("--trace") + 1], out)
        return
    import victor_amd
    from victor_amd.joint import JointFit
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    fits = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(5)]
    cov = correlated([f.covmat for f in fits])
    full = JointFit(fits, covariance=cov)
    plain = JointFit(fits)
    hp = cases.halton_params(BATCH)
    full.log_likelihood_batch(hp)                                  # engines, handle, buffers
    plain.log_likelihood_batch(hp)
    engines, opts = full._plan_cov({})
    lead = engines[0]
    lib = lead._lib
    ctxs = (C.c_void_p * 5)(*[e._ctx for e in engines])
    rows = fits[0]._fit_rows(hp, fits[0]._merged({}))
    rows[:, N.P_BETA] = 0.2 + 0.4 * cases.halton(BATCH, bases=(11,))[:, 0]
    d_rows = lead.alloc(BATCH * N.VK_NPAR)
    d_out = lead.alloc(2 * BATCH)
    lead.upload(d_rows, rows)
    d_chi = C.c_void_p(d_out + 8 * BATCH)
    ws_plain = lead.alloc(lib.vk_joint_workspace_doubles(ctxs, 5, BATCH))

    # the gridded handle: 31 slices (1 + k / 100) C_joint on beta in [0.15, 0.65]
    beta = np.linspace(0.15, 0.65, N_BETA)
    scale = 1.0 + np.arange(N_BETA) / 100.0
    prec = np.ascontiguousarray(np.linalg.inv(cov)[None] / scale[:, None, None])
    sign, ld = np.linalg.slogdet(cov)
    logdet = ld + cov.shape[0] * np.log(scale)
    eig = np.repeat((scale[-1] / scale)[:, None], cov.shape[0], axis=1)
    bn = np.full(5, 120, dtype=np.int32)
    t = N.vk_joint_cov_tables()
    t.n_blocks, t.block_n, t.n_beta = 5, bn.ctypes.data_as(C.POINTER(C.c_int32)), N_BETA
    t.beta, t.prec, t.logdet, t.eig = N.as_dp(beta), N.as_dp(prec), N.as_dp(logdet), N.as_dp(eig)
    grid = C.c_void_p()
    lead._check(lib.vk_joint_cov_create(lead._ctx, C.byref(t), C.byref(grid)))
    fixed = full._joint_handle(lead)
    ws_cov = lead.alloc(max(lib.vk_joint_cov_workspace_doubles(fixed, BATCH), lib.vk_joint_cov_workspace_doubles(grid, BATCH)))

    def run_plain():
        lead._check(lib.vk_joint_eval_device_async(ctxs, 5, C.byref(opts), d_rows, BATCH, d_out, d_chi, ws_plain))

    def run_cov(h):
        return lambda: lead._check(lib.vk_joint_cov_eval_device_async(h, ctxs, 5, C.byref(opts), d_rows, BATCH, d_out, d_chi,
                                                                       ws_cov))

    res = {"block-diagonal": [], "full, fixed": [], "full, 31 slices": []}
    for _ in range(2):                                             # alternated
        res["block-diagonal"].append(median_ms(run_plain, lead.sync))
        res["full, fixed"].append(median_ms(run_cov(fixed), lead.sync))
        res["full, 31 slices"].append(median_ms(run_cov(grid.value), lead.sync))
    lnl = lead.download(d_out, BATCH)
    assert np.all(np.isfinite(lnl))
    lines = [f"commit {commit}",
             f"density-split, 5 blocks x 120 = 600, {BATCH} points, device buffers; medians of {STEPS} enqueue + sync; ms; two rounds"]
    base = float(np.median(res["block-diagonal"]))
    for name, vals in res.items():
        for v in vals:
            lines.append(f"{name:16s} {v:8.2f} ms  {BATCH / v * 1e-3:6.3f} M evals/s  rate vs block-diagonal {base / v:5.3f}")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(os.path.join(out, "joint_cov_timing.txt"), "w") as fh:
        fh.write(text)
    lib.vk_joint_cov_destroy(grid)
    for p in (d_rows, d_out, ws_plain, ws_cov):
        lead.free(p)


if __name__ == "__main__":
    main()
