"""BOSS at batch 4096 against M simulation realisations (vk_eval_realisations): wall time, the theory / chi-square split of the
library's event timing (vk_timing_*), the matrix-core kernel against its vector-ALU twin (VICTOR_HIP_REAL_VALU, same tiling,
alternated), and the same work as M separate CCFFit objects at M = 64.  Writes realisations_<M>.txt and
realisations_separate_fits.txt into the output directory.

    python tools/realisations_timing.py OUT_DIR [--commit SHA]
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases  # noqa: E402
from victor_amd import _native as N  # noqa: E402

PEAK_FP64 = 78.6e12          # MI355X FP64 vector and matrix peak (AMD specification)
BATCH = 4096


def options(path, m=0):
    model, data = cases.boss_options("config")
    data["redshift_space_ccf"].update(data_file=path, simulation_number=m)
    return model, data


def write_stack(path, n_real):
    s = np.load(os.path.join(cases.GOLDEN, "realisations", "stack.npy"), allow_pickle=True).item()
    scale = (1.0 + (np.arange(n_real) // 16) / 100.0)[:, None, None]
    idx = np.arange(n_real) % 16
    np.save(path, dict(s, monopole=s["monopole"][idx] * scale, quadrupole=s["quadrupole"][idx] * scale), allow_pickle=True)


def timed(rs, hp, reps):
    model = rs.fit._merged({})
    eng = rs.fit._get_engine(rs.fit._engine_key(model), model["simpson_even"])
    rs.log_likelihood(hp)                                       # warm-up (code objects, upload, scratch)
    walls, th, ch = [], [], []
    for _ in range(reps):
        eng.timing(True)
        t0 = time.perf_counter()
        rs.log_likelihood(hp)
        walls.append(time.perf_counter() - t0)
        a, b, _ = eng.read_timing(reset=True)
        eng.timing(False)
        th.append(a)
        ch.append(b)
    return np.median(walls) * 1e3, np.median(th), np.median(ch)


def main():
    import victor_amd
    out = sys.argv[1]
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    os.makedirs(out, exist_ok=True)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "stack1000.npy")
    write_stack(path, 1000)
    hp = cases.halton_params(BATCH, with_beta=True)
    fit = victor_amd.CCFFit(*options(path))
    n = 60
    for m in (64, 1000):
        rs = fit.realisations(list(range(m)))
        lines = [f"commit {commit}", f"BOSS (N = {n}), {BATCH} points x {m} realisations; medians of 5 calls; ms"]
        res = {}
        for rnd in range(2):                                    # alternated A/B: matrix cores, vector ALU
            for name, val in (("mfma", None), ("valu", "1")):
                N.set_knob("VICTOR_HIP_REAL_VALU", val)
                res.setdefault(name, []).append(timed(rs, hp, 5))
        N.set_knob("VICTOR_HIP_REAL_VALU", None)
        flops = 2.0 * n * n * m * BATCH
        flops_pad = 2.0 * 64 * 64 * m * BATCH
        for name, runs in res.items():
            for wall, th, ch in runs:
                lines.append(f"{name:5s} wall {wall:9.2f}  theory {th:8.3f}  chi2 {ch:8.3f}  chi2/theory {ch / th:6.3f}  "
                             f"chi2 rate {flops / (ch * 1e-3) / 1e12:6.2f} TF/s useful ({flops_pad / (ch * 1e-3) / 1e12:6.2f} "
                             f"padded to 64) = {flops / (ch * 1e-3) / PEAK_FP64:6.3f} of the {PEAK_FP64 / 1e12:.1f} TF/s FP64 peak")
        text = "\n".join(lines) + "\n"
        print(text, flush=True)
        with open(os.path.join(out, f"realisations_{m}.txt"), "w") as fh:
            fh.write(text)
    # the same work as 64 separate fits (one context each), one batch of 4096 per fit
    m = 64
    t0 = time.perf_counter()
    fits = [victor_amd.CCFFit(*options(path, i)) for i in range(m)]
    for f in fits:
        f.log_likelihood_batch(cases.point(hp, 0))              # context creation and table upload
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    for f in fits:
        f.log_likelihood_batch(hp)
    t_eval = time.perf_counter() - t0
    rs = fit.realisations(list(range(m)))
    t0 = time.perf_counter()
    rs.log_likelihood(cases.point(hp, 0))
    t_rs_setup = time.perf_counter() - t0
    wall = timed(rs, hp, 5)[0]
    text = (f"commit {commit}\nBOSS, {BATCH} points x {m} realisations\n"
            f"{m} separate CCFFit objects: set-up {t_setup * 1e3:.1f} ms, evaluation {t_eval * 1e3:.1f} ms\n"
            f"one Realisations object:    set-up {t_rs_setup * 1e3:.1f} ms, evaluation {wall:.1f} ms\n"
            f"evaluation speed-up {t_eval * 1e3 / wall:.1f} x\n")
    print(text, flush=True)
    with open(os.path.join(out, "realisations_separate_fits.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
