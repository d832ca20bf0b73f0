"""Stretch-move ensembles on the GPU (sample_chains(move="stretch"), vk_chain_begin_stretch): time and mixing, BOSS cobaya
configuration (d = 4).  Nothing here asserts anything; DESIGN.md section 7b quotes what it writes.

Time: the 16-realisation stack with W = 10, 64, 1024 walkers per realisation, 512 sweeps after a warm-up, median of five repeats
with the routes alternating in one process:
  device      Realisations.sample_chains(move="stretch"): the sweep loop on the device;
  yardstick   what a user had before: one victor_amd.sampler.EnsembleStretch per realisation over that realisation's
              CCFFit.log_likelihood_batch, in a host loop (16 ensembles one after the other);
  definition  the NumPy loop that defines the device route (device=False: one log_likelihood_pairs call per half-step);
and log_likelihood_pairs alone at batch C / 2 (the rows of a half-step), in rows/s.

Mixing: the data vector (R = 1), 16 walkers, 4096 sweeps / steps after a burn-in of 512, once per move on the device route:
acceptance, and per parameter the integrated autocorrelation time of the ensemble mean (Sokal's window, c = 5) in sweeps / steps.
A sweep and a step both cost W likelihood evaluations, so the effective samples of the ensemble mean per likelihood evaluation are
1 / (W tau).

Cost of ``autocorr=`` (--autocorr parent|this): the 16-realisation stack, stretch, keep_chain=False, W = 10, 64, 1024, wall time
per sweep as the median of five runs (512 sweeps at W = 1024, 2048 below) after a warm-up.  ``parent``: the plain run alone (for the parent commit's
checkout, given with --root, in a process of its own); ``this``: ``autocorr`` off and on (max_lag 128) alternating in one process.

Usage: stretch_timing.py [OUT] [--commit SHA] [--sweeps N] [--repeats N] [--walkers 10,64,1024] [--no-mixing] [--only-device W]
                         [--autocorr parent|this] [--root DIR]
  OUT defaults to profiles/r15/stretch_timing.json.
  --only-device W: just the device route at W walkers per realisation, twice (the workload of a `rocprofv3 --kernel-trace
  --stats` run).
  --root DIR: import the package and the test cases from another checkout (built there) instead of this one."""

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

from tests import cases                                   # noqa: E402
from tests.test_realisations import stack_options          # noqa: E402

PARAMS = cases.cobaya_info()["params"]
NAMES = ["fsigma8", "beta", "sigma_v", "epsilon"]
R = 16


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def warm(rs, seconds=0.5):
    """Keep the GPU busy for ``seconds`` (the allocation stall of a fresh process)."""
    pts = {n: np.full(1024, PARAMS[n]["ref"]["loc"]) for n in NAMES}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        rs.log_likelihood_pairs(pts, np.arange(1024, dtype=np.int32) % R)


def yardstick(fits, specs, fixed, W, sweeps):
    """One EnsembleStretch per realisation over its fit's log_likelihood_batch, one after the other; returns the acceptance."""
    from victor_amd.sampler import EnsembleStretch
    acc = []
    for m, fit in enumerate(fits):
        es = EnsembleStretch(lambda batch, fit=fit: fit.log_likelihood_batch(batch)[0], specs, W, seed=m, fixed=fixed)
        es.run(sweeps)
        acc.append(es.acceptance)
    return float(np.mean(acc))


def time_table(sweeps, repeats, walkers, save):
    import victor_amd
    from victor_amd.sampler import parse_cobaya_params
    specs, fixed = parse_cobaya_params(PARAMS)
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    fits = [victor_amd.CCFFit(*stack_options(simulation_number=m)) for m in range(R)]
    recs = []
    for W in walkers:
        C = R * W
        kw = dict(walkers=W, seed=0, move="stretch")
        rs.sample_chains(PARAMS, 64, **kw)                            # code objects, buffers
        rs.sample_chains(PARAMS, 4, device=False, **kw)
        yardstick(fits, specs, fixed, W, 4)
        warm(rs)
        routes = (("device", lambda: float(rs.sample_chains(PARAMS, sweeps, **kw).acceptance.mean())),
                  ("yardstick", lambda: yardstick(fits, specs, fixed, W, sweeps)),
                  ("definition", lambda: float(rs.sample_chains(PARAMS, sweeps, device=False, **kw).acceptance.mean())))
        t, acc = {k: [] for k, _ in routes}, {}
        for _ in range(repeats):
            for route, run in routes:
                t0 = time.perf_counter()
                acc[route] = run()
                t[route].append(time.perf_counter() - t0)
        # the evaluation alone at the batch of a half-step
        x = rs.sample_chains(PARAMS, 0, **kw).x.reshape(C, len(NAMES))[: C // 2]
        pts = {n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(NAMES)}
        which = np.repeat(np.arange(R, dtype=np.int32), W // 2)
        rs.log_likelihood_pairs(pts, which)
        tp = []
        for _ in range(20):
            t0 = time.perf_counter()
            rs.log_likelihood_pairs(pts, which)
            tp.append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in t.items()}
        pairs_rate = (C // 2) / float(np.median(tp))
        rec = {"walkers": W, "ensemble_walkers_total": C, "sweeps": sweeps, "wall_s_median": med, "wall_s_all": t,
               "yardstick_over_device": med["yardstick"] / med["device"], "definition_over_device": med["definition"] / med["device"],
               "device_us_per_sweep": 1e6 * med["device"] / sweeps, "device_rows_per_s": C * sweeps / med["device"],
               "log_likelihood_pairs_rows_per_s_at_half_batch": pairs_rate,
               "fraction_of_ceiling": C * sweeps / med["device"] / pairs_rate, "acceptance": acc}
        print(json.dumps({k: v for k, v in rec.items() if k != "wall_s_all"}), flush=True)
        recs.append(rec)
        save(recs)                                                    # (what is measured so far survives an interrupted run)
    return recs


def autocorr_cost(which, sweeps, repeats, walkers, save):
    """Wall time per sweep of the keep-nothing stretch run: plain (``parent``), or with ``autocorr`` off and on (``this``)."""
    import victor_amd
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    variants = [("plain", {})] if which == "parent" else [("off", {}), ("on", {"autocorr": {"max_lag": 128}})]
    recs = []
    for W in walkers:
        kw = dict(walkers=W, seed=0, move="stretch", keep_chain=False)
        n = sweeps if W >= 1024 else 4 * sweeps                       # (as the marginals table: 2048 sweeps at W = 10 and 64)
        for _, extra in variants:
            rs.sample_chains(PARAMS, 64, **kw, **extra)               # code objects, buffers
        warm(rs)
        t = {k: [] for k, _ in variants}
        for _ in range(repeats):
            for name, extra in variants:
                t0 = time.perf_counter()
                ch = rs.sample_chains(PARAMS, n, **kw, **extra)
                t[name].append(time.perf_counter() - t0)
        rec = {"walkers": W, "sweeps": n, "wall_s_all": t,
               "us_per_sweep_median": {k: 1e6 * float(np.median(v)) / n for k, v in t.items()},
               "spread_over_median": {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()}}
        if which != "parent":
            med = rec["us_per_sweep_median"]
            rec["on_minus_off_us_per_sweep"] = med["on"] - med["off"]
            ac = ch.autocorr                                          # (of the last run: autocorr on)
            rec["reached_fraction"] = float(ac.reached.mean())
            rec["tau_median_of_reached"] = float(np.nanmedian(ac.tau)) if ac.reached.any() else None
        print(json.dumps({k: v for k, v in rec.items() if k != "wall_s_all"}), flush=True)
        recs.append(rec)
        save(recs)
    return recs


def mixing(sweeps=4096, burn=512, W=16):
    import victor_amd
    from victor_amd.autocorr import sokal_tau
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    out = {}
    for move in ("metropolis", "stretch"):
        t0 = time.perf_counter()
        ch = fit.sample_chains(PARAMS, burn + sweeps, walkers=W, seed=0, burn=burn, move=move)
        wall = time.perf_counter() - t0
        mean = ch.chain[:, 0].mean(axis=1)                           # (kept, d): the ensemble mean
        taus = {n: sokal_tau(mean[:, j]) for j, n in enumerate(ch.names)}
        worst = max(v[0] for v in taus.values())
        out[move] = {"walkers": W, "burn": burn, "kept": int(ch.n_kept), "wall_s": wall, "acceptance": float(ch.acceptance[0]),
                     "tau": {n: v[0] for n, v in taus.items()}, "window": {n: v[1] for n, v in taus.items()},
                     "effective_samples_per_evaluation": {n: 1.0 / (W * v[0]) for n, v in taus.items()},
                     "effective_samples_per_evaluation_worst_parameter": 1.0 / (W * worst),
                     "posterior_mean": dict(zip(ch.names, ch.mean[0].tolist())),
                     "posterior_sd": dict(zip(ch.names, np.sqrt(np.diag(ch.cov[0])).tolist()))}
        print(json.dumps({move: out[move]}), flush=True)
    return out


def main():
    import victor_amd
    out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else os.path.join(ROOT, "profiles", "r15", "stretch_timing.json")
    sweeps, repeats = arg("--sweeps", 512), arg("--repeats", 5)
    if "--only-device" in sys.argv:
        rs = victor_amd.CCFFit(*stack_options()).realisations()
        warm(rs)
        for _ in range(2):
            rs.sample_chains(PARAMS, sweeps, walkers=arg("--only-device", 10), seed=0, move="stretch")
        return
    walkers = [int(w) for w in arg("--walkers", "10,64,1024").split(",")]
    result = {"commit": arg("--commit", "") or None, "config": "BOSS cobaya configuration, d = 4"}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if "--autocorr" in sys.argv:
        which = arg("--autocorr", "this")

        def keep(records):
            result["autocorr_cost"] = {"data": "16-realisation stack, stretch, keep_chain=False", "library": which, "records": records}
            with open(out, "w") as fh:
                json.dump(result, fh, indent=1)
        autocorr_cost(which, sweeps, repeats, walkers, keep)
        return

    def save(records=None):
        if records is not None:
            result["time"] = {"data": "16-realisation stack", "records": records}
        with open(out, "w") as fh:
            json.dump(result, fh, indent=1)
    if "--no-mixing" not in sys.argv:
        result["mixing"] = mixing()
        save()
    time_table(sweeps, repeats, walkers, save)


if __name__ == "__main__":
    main()
