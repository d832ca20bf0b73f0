"""Best fits and Metropolis chains of a joint fit on the GPU (JointRealisations.best_fit / .sample_chains, vk_fit_create_joint /
vk_chain_create_joint): the five-quantile density-split fit under a correlated fixed covariance against stacks of 16 mocks
(beta fixed: the blocks ignore it; d = 3).  best_fit: wall time of a call, iterations and rows per fit.  sample_chains: W = 8 and
64 chains per mock (C = 128, 1024), 512 steps, the device route against the definition route (device=False: the host loop over
log_likelihood_pairs a user could write before), the two alternating in one process, median of the repeats after a warm-up, and
against the ceiling - log_likelihood_pairs alone at batch C, in rows/s.  Then the per-block case beside it in the same run: a
velocity dispersion of each quantile's own (per_block(params, ["sigma_v"], 5): d = 7, a row per block through
vk_fit_create_joint_blocks / vk_chain_create_joint_blocks), the best fits of the 16 mocks and the device route of the chains.

Usage: joint_sampled_timing.py OUT [--commit SHA] [--steps N] [--repeats N] [--profile]
  --profile: just two best-fit calls and one W = 64 device run (the workload of a `rocprofv3 --kernel-trace --stats` run)."""

import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases                                               # noqa: E402
from tests.test_joint_cov import correlated                           # noqa: E402
from tests.test_joint_realisations import dsplit_stacks               # noqa: E402

PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "sigma_v", "epsilon"]
FIXED = {"beta": 0.4}
N_REAL = 16


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def points(x):
    pts = {n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(NAMES)}
    pts["beta"] = np.full(len(x), FIXED["beta"])
    return pts


def warm(jr, seconds=0.5):
    """Keep the GPU busy for ``seconds`` (the allocation stall of a fresh process)."""
    pts = points(np.tile([PARAMS[n]["ref"]["loc"] for n in NAMES], (1024, 1)))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        jr.log_likelihood_pairs(pts, np.arange(1024, dtype=np.int32) % N_REAL)


def main():
    import victor_amd
    from victor_amd.joint import JointFit
    out = sys.argv[1]
    commit = arg("--commit", "")
    steps, repeats = arg("--steps", 512), arg("--repeats", 5)
    tmp = tempfile.mkdtemp(prefix="joint_sampled_")
    fits = [victor_amd.CCFFit(*o) for o in dsplit_stacks(tmp, N_REAL)]
    jr = JointFit(fits, covariance=correlated([f.covmat for f in fits])).realisations()
    tol = dict(xtol={n: 1e-5 * (PARAMS[n]["prior"]["max"] - PARAMS[n]["prior"]["min"]) for n in NAMES}, ftol=1e-6, restarts=1)
    if "--profile" in sys.argv:
        warm(jr)
        for _ in range(2):
            jr.best_fit(PARAMS, fixed=FIXED, **tol)
        jr.sample_chains(PARAMS, steps, walkers=64, seed=0, fixed=FIXED)
        return
    # ---- best fits of the 16 mocks
    jr.best_fit(PARAMS, fixed=FIXED, **tol)                              # code objects, buffers
    warm(jr)
    tb = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        bf = jr.best_fit(PARAMS, fixed=FIXED, **tol)
        tb.append(time.perf_counter() - t0)
    S = max(4, len(NAMES) + 1)
    best = {"problems": N_REAL, "wall_s_median": float(np.median(tb)), "wall_s_all": tb, "n_iter_mean": float(bf.n_iter.mean()),
            "n_iter_max": int(bf.n_iter.max()), "rows_per_fit": float(bf.n_iter.mean()) * S,
            "evaluations_used_per_fit": float(bf.n_evals.mean()), "converged": int((bf.status == bf.CONVERGED).sum())}
    # the host loop a user could write before: scipy's Nelder-Mead over log_likelihood_pairs, one mock after another
    try:
        from scipy.optimize import minimize
        lo = np.array([PARAMS[n]["prior"]["min"] for n in NAMES], dtype=float)
        hi = np.array([PARAMS[n]["prior"]["max"] for n in NAMES], dtype=float)
        x0 = np.array([PARAMS[n]["ref"]["loc"] for n in NAMES], dtype=float)
        step = np.array([PARAMS[n]["proposal"] for n in NAMES], dtype=float)
        sim = (np.array([x0] + [x0 + step[j] * np.eye(len(NAMES))[j] for j in range(len(NAMES))]) - lo) / (hi - lo)
        n_fev = []
        t0 = time.perf_counter()
        for k in range(N_REAL):
            def f(u, k=k):
                x = lo + u * (hi - lo)
                if np.any(x < lo) or np.any(x > hi):
                    return np.inf
                v = -jr.log_likelihood_pairs(points(x[None, :]), [k])[0][0]
                return v if np.isfinite(v) else np.inf
            r = minimize(f, sim[0], method="Nelder-Mead", options=dict(initial_simplex=sim, xatol=1e-5, fatol=1e-6, maxiter=5000))
            n_fev.append(int(r.nfev))
        best["scipy_host_loop_wall_s"] = time.perf_counter() - t0
        best["scipy_evaluations_per_fit"] = float(np.mean(n_fev))
    except ImportError:
        pass
    print(json.dumps({k: v for k, v in best.items() if not k.endswith("_all")}), flush=True)
    # ---- chains
    recs = []
    for W in (8, 64):
        C = N_REAL * W
        jr.sample_chains(PARAMS, 64, walkers=W, seed=0, fixed=FIXED)
        jr.sample_chains(PARAMS, 8, walkers=W, seed=0, fixed=FIXED, device=False)
        warm(jr)
        t = {"device": [], "definition": []}
        acc = {}
        for _ in range(repeats):
            for route, dev in (("device", True), ("definition", False)):
                t0 = time.perf_counter()
                ch = jr.sample_chains(PARAMS, steps, walkers=W, seed=0, fixed=FIXED, device=dev)
                t[route].append(time.perf_counter() - t0)
                acc[route] = float(ch.acceptance.mean())
        pts = points(ch.x.reshape(C, len(NAMES)))
        which = np.repeat(np.arange(N_REAL, dtype=np.int32), W)
        jr.log_likelihood_pairs(pts, which)
        tp = []
        for _ in range(20):
            t0 = time.perf_counter()
            jr.log_likelihood_pairs(pts, which)
            tp.append(time.perf_counter() - t0)
        dev_s, def_s = float(np.median(t["device"])), float(np.median(t["definition"]))
        pairs_rate = C / float(np.median(tp))
        rec = {"walkers": W, "chains": C, "steps": steps, "device_wall_s_median": dev_s, "definition_wall_s_median": def_s,
               "device_wall_s_all": t["device"], "definition_wall_s_all": t["definition"], "definition_over_device": def_s / dev_s,
               "device_us_per_step": 1e6 * dev_s / steps, "device_rows_per_s": C * steps / dev_s,
               "log_likelihood_pairs_rows_per_s_same_batch": pairs_rate, "fraction_of_ceiling": C * steps / dev_s / pairs_rate,
               "acceptance": acc}
        print(json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")}), flush=True)
        recs.append(rec)
    blocks = per_block_case(jr, steps, repeats)
    with open(out, "w") as fh:
        json.dump({"commit": commit or None,
                   "config": "five density-split quantiles, correlated fixed joint covariance, d = 3 (beta fixed), 16-mock stacks",
                   "best_fit": best, "chains": recs, "per_block": blocks}, fh, indent=1)


def per_block_case(jr, steps, repeats):
    """sigma_v per quantile (d = 7 on the five quantiles, 16 mocks): best fits and the chains' device route, timed as above."""
    from victor_amd.joint import per_block
    blk = per_block(PARAMS, ["sigma_v"], 5)
    names = [n for n in blk if n.partition("@")[0] in NAMES]
    width = {n: PARAMS[n.partition("@")[0]]["prior"]["max"] - PARAMS[n.partition("@")[0]]["prior"]["min"] for n in names}
    tol = dict(xtol={n: 1e-5 * w for n, w in width.items()}, ftol=1e-6, restarts=1)
    jr.best_fit(blk, fixed=FIXED, **tol)
    warm(jr)
    tb = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        bf = jr.best_fit(blk, fixed=FIXED, **tol)
        tb.append(time.perf_counter() - t0)
    S = len(names) + 1
    out = {"names": names, "best_fit": {"problems": N_REAL, "wall_s_median": float(np.median(tb)), "wall_s_all": tb,
                                        "n_iter_mean": float(bf.n_iter.mean()), "n_iter_max": int(bf.n_iter.max()),
                                        "rows_per_fit": float(bf.n_iter.mean()) * S,
                                        "converged": int((bf.status == bf.CONVERGED).sum())}, "chains": []}
    print(json.dumps({"per_block_best_fit": {k: v for k, v in out["best_fit"].items() if not k.endswith("_all")}}), flush=True)
    for W in (8, 64):
        C = N_REAL * W
        jr.sample_chains(blk, 64, walkers=W, seed=0, fixed=FIXED)
        warm(jr)
        t = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            ch = jr.sample_chains(blk, steps, walkers=W, seed=0, fixed=FIXED)
            t.append(time.perf_counter() - t0)
        dev_s = float(np.median(t))
        rec = {"walkers": W, "chains": C, "steps": steps, "device_wall_s_median": dev_s, "device_wall_s_all": t,
               "device_us_per_step": 1e6 * dev_s / steps, "device_rows_per_s": C * steps / dev_s,
               "acceptance": float(ch.acceptance.mean())}
        print(json.dumps({"per_block_chains": {k: v for k, v in rec.items() if not k.endswith("_all")}}), flush=True)
        out["chains"].append(rec)
    return out


if __name__ == "__main__":
    main()
