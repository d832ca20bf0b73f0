"""Metropolis chains on the GPU (Realisations.sample_chains, vk_chain_begin): wall time of a call that ends with the results on
the host, BOSS cobaya configuration (d = 4) against the 16-realisation stack with W = 8, 64, 1024 chains per realisation
(C = 128, 1024, 16384), 512 steps.  The device route against the definition route (device=False: the host loop over
log_likelihood_pairs a user could write before), the two alternating in one process, and against the ceiling - log_likelihood_pairs
alone at batch C, in rows/s.

Cost of ``predictive=`` (--predictive parent|this): realisations x 8 walkers with ``keep_chain=False``, R = 16, 128, 1024 mocks
(C = 128, 1024, 8192), both moves, steps/s of the device route: ``parent``: the plain run alone (what the parent commit's built
checkout, given with --root, can run, in a process of its own - the run without ``predictive`` makes the parent's launches, so its
rate against the parent is the check that nothing else moved); ``this``: ``predictive`` off and on alternating in one process.

Usage: chains_timing.py OUT [--commit SHA] [--steps N] [--repeats N] [--only-16384] [--predictive parent|this] [--root DIR]
  --only-16384: just the C = 16384 device run, twice (the workload of a `rocprofv3 --kernel-trace --stats` run).
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


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def warm(rs, seconds=0.5):
    """Keep the GPU busy for ``seconds`` (the allocation stall of a fresh process)."""
    pts = {n: np.full(1024, PARAMS[n]["ref"]["loc"]) for n in NAMES}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        rs.log_likelihood_pairs(pts, np.arange(1024, dtype=np.int32) % 16)


def predictive_cost(fit, which, steps, repeats):
    """Steps/s of the keep-nothing device run of R x 8 chains: plain (``parent``), or with ``predictive`` off and on (``this``)."""
    variants = [("plain", {})] if which == "parent" else [("off", {}), ("on", {"predictive": True})]
    recs = []
    for move, W in (("metropolis", 8), ("stretch", 10)):               # (the stretch move needs W >= 2 (d + 1) = 10)
        for R in (16, 128, 1024):
            rs = fit.realisations([m % 16 for m in range(R)])
            legs = {k: (lambda kw=kw: rs.sample_chains(PARAMS, steps, walkers=W, seed=0, move=move, keep_chain=False, **kw))
                    for k, kw in variants}
            for f in legs.values():                                  # code objects, buffers
                f()
            warm(rs)
            t = {k: [] for k in legs}
            for _ in range(repeats):                                 # the legs alternate
                for k, f in legs.items():
                    t0 = time.perf_counter()
                    f()
                    t[k].append(time.perf_counter() - t0)
            rec = {"move": move, "mocks": R, "walkers": W, "chains": R * W, "steps": steps}
            for k, v in t.items():
                med = float(np.median(v))
                rec.update({k + "_wall_s_all": v, k + "_wall_s_median": med, k + "_steps_per_s": steps / med,
                            k + "_us_per_step": 1e6 * med / steps, k + "_spread": (max(v) - min(v)) / med})
            if which != "parent":
                rec["on_over_off"] = rec["on_wall_s_median"] / rec["off_wall_s_median"]
                rec["on_minus_off_us_per_step"] = rec["on_us_per_step"] - rec["off_us_per_step"]
            print(json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")}), flush=True)
            recs.append(rec)
    return recs


def main():
    import victor_amd
    out = sys.argv[1]
    commit = arg("--commit", "")
    steps, repeats = arg("--steps", 512), arg("--repeats", 5)
    if "--predictive" in sys.argv:
        which = arg("--predictive", "this")
        recs = predictive_cost(victor_amd.CCFFit(*stack_options()), which, steps, repeats)
        with open(out, "w") as fh:
            json.dump({"commit": commit or None, "config": "BOSS cobaya configuration, d = 4, 16-realisation stack, keep_chain=False",
                       "library": which, "records": recs}, fh, indent=1)
        return
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    if "--only-16384" in sys.argv:
        warm(rs)
        for _ in range(2):
            rs.sample_chains(PARAMS, steps, walkers=1024, seed=0)
        return
    recs = []
    for W in (8, 64, 1024):
        C = 16 * W
        rs.sample_chains(PARAMS, 64, walkers=W, seed=0)              # code objects, buffers
        rs.sample_chains(PARAMS, 8, walkers=W, seed=0, device=False)
        warm(rs)
        t = {"device": [], "definition": []}
        acc = {}
        for _ in range(repeats):
            for route, dev in (("device", True), ("definition", False)):
                t0 = time.perf_counter()
                ch = rs.sample_chains(PARAMS, steps, walkers=W, seed=0, device=dev)
                t[route].append(time.perf_counter() - t0)
                acc[route] = float(ch.acceptance.mean())
        # the ceiling: the evaluation alone at batch C
        x = ch.x.reshape(C, len(NAMES))
        pts = {n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(NAMES)}
        which = np.repeat(np.arange(16, dtype=np.int32), W)
        rs.log_likelihood_pairs(pts, which)
        tp = []
        for _ in range(20):
            t0 = time.perf_counter()
            rs.log_likelihood_pairs(pts, which)
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
    with open(out, "w") as fh:
        json.dump({"commit": commit or None, "config": "BOSS cobaya configuration, d = 4, 16-realisation stack", "records": recs}, fh,
                  indent=1)


if __name__ == "__main__":
    main()
