"""Best fits on the GPU (CCFFit.best_fit / Realisations.best_fit, vk_fit_run): wall time per call for the BOSS data (R = 1), the
16-realisation stack and 1024 problems (``fit.realisations(np.arange(1024) % 16)``), with iterations and rows per fit and rows/s
beside log_likelihood_batch's rate at the same batch size; the yardstick is scipy's Nelder-Mead driven from the host through
log_likelihood (R = 1) and log_likelihood_pairs (R = 16, one realisation after another).

Usage: best_fit_timing.py OUT [--commit SHA] [--only-1024]
  --only-1024: just the R = 1024 fit, twice (the workload of a `rocprofv3 --kernel-trace --stats` run: the step kernel's share)."""

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
OPTS = dict(xtol={n: 1e-5 * (h - lo) for n, lo, h in zip(NAMES, LO, HI)}, ftol=1e-6, restarts=1)
S = max(4, len(NAMES) + 1)          # rows per problem and iteration (vk_fit_run)


def timed(fn, reps):
    fn()                                                   # warm: code objects, engines, realisation upload
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()                                         # synchronous: returns after the results have come back
        t.append(time.perf_counter() - t0)
    return out, t


def fit_record(label, call, batch_rate, reps):
    bf, t = timed(call, reps)
    rows = int(np.sum(bf.n_iter)) * S
    wall = float(np.median(t))
    rec = {"label": label, "problems": len(bf), "wall_s_median": wall, "wall_s_all": t,
           "iterations_per_fit_mean": float(np.mean(bf.n_iter)), "iterations_max": int(np.max(bf.n_iter)),
           "rows_per_fit_mean": rows / len(bf), "evals_per_fit_mean": float(np.mean(bf.n_evals)),
           "status_counts": {str(k): int(v) for k, v in zip(*np.unique(bf.status, return_counts=True))},
           "rows_per_s": rows / wall, "log_likelihood_batch_rows_per_s_same_batch": batch_rate(len(bf) * S)}
    print(json.dumps({k: v for k, v in rec.items() if k != "wall_s_all"}), flush=True)
    return rec


def batch_rate(fit):
    def rate(n):
        hp = cases.halton_params(n, with_beta=True)
        hp["epsilon"] = hp.pop("aperp") / hp.pop("apar")
        _, t = timed(lambda: fit.log_likelihood_batch(hp), 20)
        return n / float(np.median(t))
    return rate


def scipy_record(label, neg_lnls, reps=2):
    from scipy.optimize import minimize
    x0 = (np.array([PARAMS[n]["ref"]["loc"] for n in NAMES]) - LO) / (HI - LO)

    def run():
        evals = 0
        for neg in neg_lnls:
            def f(u, neg=neg):
                x = LO + u * (HI - LO)
                if np.any(x < LO) or np.any(x > HI):
                    return np.inf
                return neg({n: float(v) for n, v in zip(NAMES, x)})
            r = minimize(f, x0, method="Nelder-Mead", options=dict(xatol=1e-5, fatol=1e-6, maxiter=20000))
            evals += r.nfev
        return evals
    evals, t = timed(run, reps)
    rec = {"label": label, "problems": len(neg_lnls), "wall_s_median": float(np.median(t)), "wall_s_all": t,
           "evals_per_fit_mean": evals / len(neg_lnls), "evals_per_s": evals / float(np.median(t))}
    print(json.dumps({k: v for k, v in rec.items() if k != "wall_s_all"}), flush=True)
    return rec


def main():
    import victor_amd
    out = sys.argv[1]
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else None
    fit = victor_amd.CCFFit(*stack_options())
    if "--only-1024" in sys.argv:
        rs = fit.realisations(np.arange(1024) % 16)
        for _ in range(2):
            rs.best_fit(PARAMS, **OPTS)
        return
    data = victor_amd.CCFFit(*cases.boss_options("config"))
    rs16 = fit.realisations()
    rs1024 = fit.realisations(np.arange(1024) % 16)
    recs = [
        fit_record("boss_data_R1", lambda: data.best_fit(PARAMS, **OPTS), batch_rate(data), 10),
        fit_record("stack_R16", lambda: rs16.best_fit(PARAMS, **OPTS), batch_rate(fit), 10),
        fit_record("stack_R1024", lambda: rs1024.best_fit(PARAMS, **OPTS), batch_rate(fit), 5),
        scipy_record("scipy_host_boss_data_R1", [lambda p: -data.log_likelihood(p)[0]]),
        scipy_record("scipy_host_stack_R16", [lambda p, k=k: -rs16.log_likelihood_pairs(p, [k])[0][0] for k in range(16)], reps=1),
    ]
    with open(out, "w") as fh:
        json.dump({"commit": commit, "tolerances": {"xtol_over_width": 1e-5, "ftol": 1e-6, "restarts": 1}, "records": recs}, fh,
                  indent=1)


if __name__ == "__main__":
    main()
