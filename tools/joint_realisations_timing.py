"""Joint fits under one full covariance against 1000 simulation realisations at 4096 points (JointFit.realisations,
vk_joint_cov_eval_realisations): the five density-split blocks (N = 5 x 120 = 600, fixed correlated covariance) and a two-block
BOSS stack (N = 2 x 60, beta-dependent data, 31 correlated covariance slices), each against a loop of separate JointFits, one per
realisation (five / two CCFFit constructions, a covariance handle and one batch evaluation each), timed over 16 realisations and
extrapolated to 1000.  Host buffers, wall time of whole calls, medians.  The stacks are written into a temporary directory from
the committed goldens (tests/test_joint_realisations.py: write_stacks).  Writes joint_realisations_timing.txt into the output
directory.  Run under ``rocprofv3 --kernel-trace --stats --output-format csv`` for the theory / chi-square split; ``--trace FILE``
then summarises its kernel_trace.csv into joint_realisations_kernels.txt.

    python tools/joint_realisations_timing.py OUT_DIR [--commit SHA]
    python tools/joint_realisations_timing.py OUT_DIR --trace kernel_trace.csv
"""
import csv
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases  # noqa: E402

PEAK_FP64 = 78.6e12          # MI355X FP64 vector and matrix peak (AMD specification)
BATCH = 4096
N_REAL = 1000
LOOP = 16
STEPS = 5


def timed(fn, steps=STEPS):
    fn()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def summarise_trace(path, out):
    """Theory launches, the joint realisation chi-square kernel (dsplit: fixed; BOSS: behind the log-det factor kernel) and the
    per-realisation loop's joint chi-square kernel, from rocprofv3's kernel_trace.csv; per-dispatch durations, medians."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    groups = {}
    prev = ""
    for r in rows:
        name = r["Kernel_Name"]
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3          # us
        if "vk_joint_real_chi2_kernel" in name:
            g = "real chi2, BOSS 31 slices" if "factor" in prev else "real chi2, dsplit fixed"
        elif "vk_joint_real_factor_kernel" in name:
            g = "log-det factor"
        elif "vk_joint_chi2_kernel" in name:
            g = "loop: joint chi2"
        elif "vk_theory" in name:
            g = "theory launch"
        else:
            continue
        prev = name if "vk_joint" in name else prev
        groups.setdefault(g, []).append(dur)
    lines = ["rocprofv3 --kernel-trace --stats of tools/joint_realisations_timing.py (warm-up and loop included); per-dispatch "
             "durations, us"]
    for g, v in groups.items():
        lines.append(f"{g:28s} dispatches {len(v):5d}  median {np.median(v):12.1f}  mean {np.mean(v):12.1f}")
    forms = boss_forms()
    for g, nt, f in (("real chi2, dsplit fixed", 600, 1.0), ("real chi2, BOSS 31 slices", 120, forms)):
        if g in groups:
            t = float(np.median(groups[g])) * 1e-6
            flops = f * 2.0 * nt * nt * BATCH * N_REAL
            lines.append(f"{g}: {t * 1e3:.3f} ms = {flops / t / 1e12:.2f} TF/s at {f:.3f} form(s) per pair ({f:.3f} x 2 NT^2 "
                         f"n M, NT = {nt}) = {flops / t / PEAK_FP64:.3f} of the {PEAK_FP64 / 1e12:.1f} TF/s FP64 peak")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(out, "joint_realisations_kernels.txt"), "w") as fh:
        fh.write(text)


def boss_forms():
    """Quadratic forms per pair of the BOSS case: 1 + the fraction of its points strictly inside the covariance grid and off it
    (those blend slice lo with the last one, ccf_fit.py:213-228)."""
    g = np.asarray(np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()["beta"], dtype=float)
    beta = cases.halton_params(BATCH, with_beta=True)["beta"]
    return 1.0 + float(np.mean((beta > g.min()) & (beta < g.max()) & ~np.isin(beta, g)))


def case(name, opts, covariance_of, params, tmp):
    """(lines, forms per pair): one call over every realisation against the per-realisation loop."""
    import victor_amd
    from victor_amd.joint import JointFit
    from tests.test_joint_realisations import with_number
    fits = [victor_amd.CCFFit(*o) for o in opts]
    cov = covariance_of(fits)
    joint = JointFit(fits, covariance=cov)
    t0 = time.perf_counter()
    jr = joint.realisations()
    t_read = time.perf_counter() - t0
    t_call = timed(lambda: jr.log_likelihood(params))
    lnl, chi2 = jr.log_likelihood(params)
    assert chi2.shape == (BATCH, N_REAL)
    # pairs mode: one realisation per point
    which = np.arange(BATCH) % N_REAL
    t_pairs = timed(lambda: jr.log_likelihood_pairs(params, which))
    # the loop: fresh fits, a joint handle and one evaluation per realisation; evaluation alone on the second call
    total, evals = [], []
    for m in range(LOOP):
        t0 = time.perf_counter()
        fm = [victor_amd.CCFFit(*o) for o in with_number(opts, m)]
        jm = JointFit(fm, covariance=cov)
        l1, c1 = jm.log_likelihood_batch(params)
        total.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        jm.log_likelihood_batch(params)
        evals.append(time.perf_counter() - t0)
        assert np.allclose(c1, chi2[:, m], rtol=1e-9, atol=0)
        jm._release_handle()
        for f in fm:
            f._engine = None
    per, per_eval = float(np.median(total)), float(np.median(evals))
    blended = 0.0
    if not joint.fixed_covmat:
        beta = params["beta"]
        blended = float(np.mean([joint._bracket(b)[1] != 0.0 for b in beta]))
    nt = joint.n_data
    lines = [f"{name}: {len(fits)} blocks, NT = {nt}, {BATCH} points x {N_REAL} realisations, "
             f"{'fixed covariance' if joint.fixed_covmat else f'{len(joint.beta_covmat)} covariance slices, {blended:.3f} of the points blended'}",
             f"  reading the stacks, {N_REAL} realisations x {len(fits)} blocks: {t_read:.2f} s (once)",
             f"  one call, every realisation:       {t_call * 1e3:9.1f} ms   ({BATCH * N_REAL / t_call / 1e6:7.1f} M pairs/s)",
             f"  one call, pairs mode ({BATCH} pairs):  {t_pairs * 1e3:9.1f} ms",
             f"  loop of JointFits, per realisation: {per * 1e3:9.1f} ms (construction + evaluation), {per_eval * 1e3:.1f} ms "
             f"(evaluation only); median of {LOOP}",
             f"  loop extrapolated to {N_REAL}:       {per * N_REAL:9.2f} s  ({per_eval * N_REAL:.2f} s evaluation only)",
             f"  speed-up of one call over the loop: {per * N_REAL / t_call:9.1f} x  ({per_eval * N_REAL / t_call:.1f} x over "
             f"evaluation only)"]
    joint._release_handle()
    return lines, 1.0 + blended


def main():
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    if "--trace" in sys.argv:
        summarise_trace(sys.argv[sys.argv.index("--trace") + 1], out)
        return
    from tests.test_joint_cov import boss_joint_cov_file, boss_pair_options, correlated
    from tests.test_joint_realisations import write_stacks
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    lines = [f"commit {commit}", "wall time of whole calls (host buffers in and out), medians of 5 after a warm-up"]
    with tempfile.TemporaryDirectory() as tmp:
        dsplit = write_stacks(tmp, [cases.dsplit_options(q) for q in range(5)], N_REAL, tag="dsplit")
        text, _ = case("density-split", dsplit, lambda fits: correlated([f.covmat for f in fits]), cases.halton_params(BATCH), tmp)
        lines += text
        print("\n".join(text), flush=True)
        boss = write_stacks(tmp, boss_pair_options(), N_REAL, tag="boss")
        spec = boss_joint_cov_file(os.path.join(tmp, "joint_cov.npy"))
        text, forms = case("BOSS pair", boss, lambda fits: spec, cases.halton_params(BATCH, with_beta=True), tmp)
        lines += text
        print("\n".join(text), flush=True)
    text = "\n".join(lines) + "\n"
    with open(os.path.join(out, "joint_realisations_timing.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
