"""Hessians and Laplace covariances on the GPU (``laplace``, vk_fit_hessian): wall time per call at the best fits of the BOSS stack
(d = 4, M = 33 stencil rows per problem) for R = 1, 16 and 1024 problems (``fit.realisations(np.arange(R) % 16)``); beside each the
same stencil driven from the host through ``log_likelihood_pairs`` - one call per stencil point, and one call per problem (its 33
rows at once) -, the routes a user has without the entry point; and sigma from ``laplace`` beside the square root of the diagonal
of ``sample_chains(...).cov`` for the 16 mocks.  With ``--leg fisher`` the Fisher forecast instead (``fisher``, vk_fit_fisher;
M = 9 rows per problem): its wall time beside the ``2 d + 1`` ``theory_vector_batch`` calls and NumPy a user had before (per
problem and batched) and ``laplace`` in the same process, and sigma(Fisher) / sigma(Laplace) at noise-free truths.  Recorded, not
asserted.

Usage: hessian_timing.py OUT [--commit SHA] [--leg fisher]"""

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases                                   # noqa: E402
from tests.test_realisations import stack_options          # noqa: E402

PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "beta", "sigma_v", "epsilon"]
LO = np.array([PARAMS[n]["prior"]["min"] for n in NAMES], dtype=float)
HI = np.array([PARAMS[n]["prior"]["max"] for n in NAMES], dtype=float)


def timed(fn, reps):
    fn()                                                   # warm: code objects, engines, realisation upload
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()                                         # synchronous: returns after the results have come back
        t.append(time.perf_counter() - t0)
    return out, t


def host_stencil(rs, lap, per):
    """The stencil of ``lap`` through log_likelihood_pairs and the NumPy statement: ``per`` = "point" (one call per stencil
    point) or "problem" (one call per problem, 33 rows)."""
    from victor_amd import laplace as L
    pts = L.stencil_points(lap.x, lap.step, LO, HI)
    R, M, d = pts.shape
    values = np.empty((R, M))
    for p in range(R):
        if per == "problem":
            batch = {n: np.ascontiguousarray(pts[p, :, j]) for j, n in enumerate(NAMES)}
            values[p] = rs.log_likelihood_pairs(batch, np.full(M, p, dtype=np.int32))[0]
        else:
            for m in range(M):
                values[p, m] = rs.log_likelihood_pairs({n: float(pts[p, m, j]) for j, n in enumerate(NAMES)}, [p])[0][0]
    return L.assemble(values, lap.x, lap.step, LO, HI)


def host_fisher(fit, res, batched):
    """The Jacobian stencil of ``res`` through ``theory_vector_batch`` and the NumPy statement, what a user had before:
    ``2 d + 1`` calls per problem (one point each), or - ``batched`` - ``2 d + 1`` calls of R points each."""
    from victor_amd import fisher as F
    pts = F.stencil_points(res.x, res.step, LO, HI)
    R, M, d = pts.shape
    vecs = np.empty((R, M, len(fit.s) * len(fit.poles_s)))
    for m in range(M):
        if batched:
            vecs[:, m] = fit.theory_vector_batch({n: np.ascontiguousarray(pts[:, m, j]) for j, n in enumerate(NAMES)})
        else:
            for p in range(R):
                vecs[p, m] = fit.theory_vector_batch({n: float(pts[p, m, j]) for j, n in enumerate(NAMES)})[0]
    return F.assemble(vecs, res.x, res.step, LO, HI, F.host_blocks(fit, res.params, R), res.scale)


def fisher_leg(out, commit):
    """``--leg fisher``: wall time of ``fisher`` (vk_fit_fisher; d = 4, M = 9 rows per problem) at the best fits of the BOSS stack
    for R = 1 / 16 / 1024, beside the host routes and ``laplace`` in the same process; and sigma(Fisher) / sigma(Laplace) per
    parameter at equal steps for the 16 noise-free mocks of tests/test_gpu_hessian.py's construction."""
    import tempfile

    import victor_amd
    from tests.test_gpu_hessian import NoiseFree
    fit = victor_amd.CCFFit(*stack_options())
    recs = []
    for R, reps, host_reps in ((1, 20, 3), (16, 20, 3), (1024, 5, 1)):
        rs = fit.realisations(np.arange(R) % 16)
        bf = rs.best_fit(PARAMS)
        res, t = timed(lambda: rs.fisher(PARAMS, bf), reps)
        rec = {"label": f"fisher_stack_R{R}", "problems": R, "rows": R * 9, "wall_s_median": float(np.median(t)), "wall_s_all": t,
               "status_counts": {str(k): int(v) for k, v in zip(*np.unique(res.status, return_counts=True))}}
        _, t = timed(lambda: rs.fisher(PARAMS, bf, keep_vectors=True), reps)
        rec["keep_vectors_wall_s_median"] = float(np.median(t))
        _, t = timed(lambda: rs.laplace(PARAMS, bf), reps)
        rec["laplace_wall_s_median"] = float(np.median(t))
        for name, batched in (("batched", True), ("per_problem", False)):
            host, t = timed(lambda: host_fisher(fit, res, batched), host_reps)
            rec[f"host_{name}_wall_s_median"] = float(np.median(t))
            ok = res.ok & (host.status == 0)
            rec[f"host_{name}_max_rel_dsigma"] = (float(np.max(np.abs(
                np.sqrt(np.einsum("rjj->rj", host.cov[ok])) / res.sigma[ok] - 1))) if np.any(ok) else None)
        print(json.dumps({k: v for k, v in rec.items() if k != "wall_s_all"}), flush=True)
        recs.append(rec)
    with tempfile.TemporaryDirectory() as tmp:
        import pathlib
        nf = NoiseFree(pathlib.Path(tmp))
        rs = nf.fit.realisations(list(range(16)))
        at = {n: nf.truth[:16, j] for j, n in enumerate(NAMES)}
        fis, lap = rs.fisher(PARAMS, at), rs.laplace(PARAMS, at)
    both = fis.ok & lap.ok
    quotient = fis.sigma[both] / lap.sigma[both]
    sig = {"names": NAMES, "problems_ok": int(both.sum()), "steps": fis.step[0].tolist(), "steps_equal": bool(np.array_equal(fis.step, lap.step)),
           "fisher_sigma_over_laplace_sigma": quotient.tolist(), "median": np.median(quotient, axis=0).tolist(),
           "min": quotient.min(axis=0).tolist(), "max": quotient.max(axis=0).tolist()}
    print(json.dumps(sig), flush=True)
    with open(out, "w") as fh:
        json.dump({"commit": commit, "d": 4, "stencil_rows_per_problem": 9, "records": recs, "sigma_against_laplace_noise_free_R16": sig},
                  fh, indent=1)


def main():
    import victor_amd
    out = sys.argv[1]
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None
    if "--leg" in sys.argv and sys.argv[sys.argv.index("--leg") + 1] == "fisher":
        return fisher_leg(out, commit)
    fit = victor_amd.CCFFit(*stack_options())
    recs = []
    bf16 = lap16 = None
    for R, reps, host_reps in ((1, 20, 3), (16, 20, 3), (1024, 5, 1)):
        rs = fit.realisations(np.arange(R) % 16)
        bf = rs.best_fit(PARAMS)
        lap, t = timed(lambda: rs.laplace(PARAMS, bf), reps)
        rec = {"label": f"laplace_stack_R{R}", "problems": R, "rows": R * 33, "wall_s_median": float(np.median(t)), "wall_s_all": t,
               "status_counts": {str(k): int(v) for k, v in zip(*np.unique(lap.status, return_counts=True))}}
        _, t = timed(lambda: rs.best_fit(PARAMS, covariance=True), reps)
        rec["best_fit_with_covariance_wall_s_median"] = float(np.median(t))
        _, t = timed(lambda: rs.best_fit(PARAMS), reps)
        rec["best_fit_wall_s_median"] = float(np.median(t))
        for per in ("problem", "point"):
            host, t = timed(lambda: host_stencil(rs, lap, per), host_reps)
            rec[f"host_one_call_per_{per}_wall_s_median"] = float(np.median(t))
            ok = lap.ok & (host.status == 0)
            rec[f"host_one_call_per_{per}_max_rel_dsigma"] = (float(np.max(np.abs(
                np.sqrt(np.einsum("rjj->rj", host.cov[ok])) / lap.sigma[ok] - 1))) if np.any(ok) else None)
        print(json.dumps({k: v for k, v in rec.items() if k != "wall_s_all"}), flush=True)
        recs.append(rec)
        if R == 16:
            bf16, lap16, rs16 = bf, lap, rs
    ch = rs16.sample_chains(PARAMS, 6000, walkers=8, seed=1, start=bf16, burn=1000, keep_chain=False)
    chain_sigma = np.sqrt(np.einsum("rjj->rj", ch.cov))
    def rows(a):                                           # (NaN where a status leaves sigma undefined: null in the file)
        return [[float(v) if np.isfinite(v) else None for v in row] for row in a]
    sig = {"names": NAMES, "x": bf16.x.tolist(), "status": lap16.status.tolist(), "laplace_sigma": rows(lap16.sigma),
           "chain_sigma": rows(chain_sigma), "chain_steps": 6000, "chain_burn": 1000, "chain_walkers": 8,
           "chain_acceptance": ch.acceptance.tolist()}
    print(json.dumps(sig), flush=True)
    with open(out, "w") as fh:
        json.dump({"commit": commit, "d": 4, "stencil_rows_per_problem": 33, "records": recs, "sigma_against_chains_R16": sig}, fh,
                  indent=1)


if __name__ == "__main__":
    main()
