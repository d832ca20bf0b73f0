"""Replica exchange on the GPU (``sample_chains(..., temper=...)``, vk_chain_begin_tempered): what the swaps cost and what they buy,
on the beta-dependent BOSS stack (d = 4 unless beta is fixed).

1. Wall time of a tempered run of R = 1 / 16 / 1024 mocks x 8 rungs x 8 walkers against ``sample_chains`` of the SAME number of
   chains (R x 64) without ``temper``, alternating in one process, ``keep_chain=False``: the difference is the swap kernel and the
   propose launch behind it (every ``swap_every``-th step) and the energy sums.
2. ``--plain-only``: just the untempered leg, which also runs on a tree that knows no ``temper=`` - the parent commit's, in a
   process of its own, alternated with this commit's by the caller (as tools/best_fit_timing.py was used).
3. Mixing: the cold rung's acceptance and integrated autocorrelation time (``autocorr=``) with and without tempering at equal
   cold-chain length (R = 16, W = 8).
4. ``ln_evidence`` by thermodynamic integration against Laplace's (``best_fit(..., covariance=True)``) with beta FIXED, where the
   posterior is close to Gaussian and Laplace can be trusted.

Usage: temper_timing.py OUT [--commit SHA] [--steps N] [--repeats N] [--plain-only] [--skip-1024]"""

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
RUNGS, WALKERS = 8, 8
LADDER = {"rungs": RUNGS, "power": 5, "swap_every": 4}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def warm(rs, seconds=0.5):
    """Keep the GPU busy for ``seconds`` (the allocation stall of a fresh process)."""
    pts = {n: np.full(1024, PARAMS[n]["ref"]["loc"]) for n in NAMES}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        rs.log_likelihood_pairs(pts, np.arange(1024, dtype=np.int32) % len(rs))


def timed(f, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return out


def wall_times(fit, R, steps, repeats, plain_only):
    rs = fit.realisations([m % 16 for m in range(R)])
    legs = {"plain": lambda: rs.sample_chains(PARAMS, steps, walkers=RUNGS * WALKERS, seed=0, keep_chain=False)}
    if not plain_only:
        legs["tempered"] = lambda: rs.sample_chains(PARAMS, steps, walkers=WALKERS, seed=0, keep_chain=False, temper=LADDER)
    for f in legs.values():                                  # code objects, buffers
        f()
    warm(rs)
    t = {k: [] for k in legs}
    for _ in range(repeats):                                 # the legs alternate
        for k, f in legs.items():
            t[k] += timed(f, 1)
    rec = {"mocks": R, "chains": R * RUNGS * WALKERS, "steps": steps}
    for k, v in t.items():
        rec[k + "_wall_s_all"] = v
        rec[k + "_wall_s_median"] = float(np.median(v))
        rec[k + "_us_per_step"] = 1e6 * float(np.median(v)) / steps
        rec[k + "_spread"] = (max(v) - min(v)) / float(np.median(v))
    if not plain_only:
        rec["tempered_over_plain"] = rec["tempered_wall_s_median"] / rec["plain_wall_s_median"]
        rec["tempered_minus_plain_us_per_step"] = rec["tempered_us_per_step"] - rec["plain_us_per_step"]
    return rec


def mixing(fit, steps):
    rs = fit.realisations()
    bf = rs.best_fit(PARAMS)
    kw = dict(walkers=WALKERS, seed=1, start=bf, burn=steps // 4, keep_chain=False, autocorr={"max_lag": 256})
    out = {}
    for name, extra in (("plain", {}), ("tempered", {"temper": LADDER})):
        ch = rs.sample_chains(PARAMS, steps, **kw, **extra)
        out[name] = {"acceptance": ch.acceptance.tolist(), "tau": ch.autocorr.tau.tolist(), "reached": ch.autocorr.reached.tolist(),
                     "ess": ch.autocorr.ess.tolist()}
        if ch.tempering is not None:
            out[name]["swap_acceptance"] = ch.tempering.swap_acceptance.tolist()
            out[name]["acceptance_per_rung"] = ch.tempering.acceptance.tolist()
    return {"mocks": 16, "walkers": WALKERS, "steps": steps, "names": NAMES, **out}


def evidence(fit, steps):
    """beta fixed at the cobaya block's reference: d = 3, no kink; Laplace against thermodynamic integration, mock by mock."""
    rs = fit.realisations()
    fixed = {"beta": float(PARAMS["beta"]["ref"]["loc"])}
    bf = rs.best_fit(PARAMS, fixed=fixed, covariance=True)
    ch = rs.sample_chains(PARAMS, steps, walkers=WALKERS, seed=2, fixed=fixed, start=bf, burn=steps // 8, keep_chain=False,
                          temper={"rungs": 16, "power": 5, "swap_every": 4})
    q = ch.tempering
    return {"mocks": 16, "walkers": WALKERS, "rungs": 16, "steps": steps, "fixed": fixed, "laplace_ln_evidence": bf.laplace.ln_evidence.tolist(),
            "laplace_status": bf.laplace.status.tolist(), "ln_evidence": q.ln_evidence.tolist(), "ln_evidence_trapezoid": q.ln_evidence_trapezoid.tolist(),
            "ln_evidence_error": q.ln_evidence_error.tolist(), "difference": (q.ln_evidence - bf.laplace.ln_evidence).tolist(),
            "swap_acceptance_min": float(np.nanmin(q.swap_acceptance)), "n_not_finite": int(q.n_not_finite.sum())}


def main():
    import victor_amd
    out = sys.argv[1]
    steps, repeats = arg("--steps", 256), arg("--repeats", 5)
    plain_only = "--plain-only" in sys.argv
    fit = victor_amd.CCFFit(*stack_options())
    res = {"commit": arg("--commit", "") or None, "config": "BOSS cobaya configuration, beta-dependent 16-realisation stack",
           "ladder": None if plain_only else LADDER, "records": []}
    def dump():
        with open(out, "w") as fh:
            json.dump(res, fh, indent=1)

    for R in (1, 16) if "--skip-1024" in sys.argv else (1, 16, 1024):
        rec = wall_times(fit, R, steps, repeats, plain_only)
        print(json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")}), flush=True)
        res["records"].append(rec)
        dump()
    if not plain_only:
        res["mixing"] = mixing(fit, arg("--mixing-steps", 4096))
        print(json.dumps({k: (np.round(np.nanmedian(np.array(v["tau"], dtype=float), axis=0), 1).tolist(), float(np.mean(v["acceptance"])))
                          for k, v in res["mixing"].items() if isinstance(v, dict)}), flush=True)
        dump()
        res["evidence"] = evidence(fit, arg("--evidence-steps", 4096))
        print(json.dumps({k: res["evidence"][k] for k in ("difference", "ln_evidence_error", "swap_acceptance_min")}), flush=True)
    dump()


if __name__ == "__main__":
    main()
