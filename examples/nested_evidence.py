"""Nested sampling on the BOSS cobaya configuration, measured (DESIGN.md section 7d quotes the output):

* wall time per iteration of the device route against the definition route (what a user could write before) at the defaults,
  d = 4, for R = 1 (the data vector), 16 (the mock stack) and 1024 (the stack repeated): the two routes alternate in one process
  after a warm-up of each, median of five blocks of 8 iterations;
* beta fixed, d = 3: ``ln_evidence`` against ``grid_posterior(bins=32).ln_evidence`` per mock, in units of ``ln_evidence_error``;
* d = 4, beta sampled: against the thermodynamic integration of ``sample_chains(temper=True)``.

    python examples/nested_evidence.py [--out FILE] [--skip-large]

``--prior`` runs the same two measurements under a Gaussian prior on sigma_v instead (``prior=``): the device route's wall time
per iteration with and without the prior, alternating in one process, for R = 1 and R = 16; and beta fixed, d = 3, ``ln_evidence``
under the prior against ``grid_posterior(bins=32, prior=).ln_evidence`` per mock, seeds 0 - 2.

Needs a GPU and the test fixtures of the repository (tests/golden)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def per_iteration(obj, params, device, blocks=5, **kw):
    """Median seconds per iteration over ``blocks`` blocks of 8 iterations of one run (the start is not timed)."""
    ns = obj.nested_sampling(params, n_iter=0, device=device, **kw)
    ns.extend(8)                                             # warm-up
    out = []
    for _ in range(blocks):
        t = time.perf_counter()
        ns.extend(8)
        out.append((time.perf_counter() - t) / 8)
    return out


def d3_against_the_grid(rs, params, fixed, prior=None):
    """beta fixed, d = 3, every mock: nested sampling against the grid, three seeds (the mocks of a run share their start draw, so
    their errors are correlated within a seed)."""
    kw = {} if prior is None else {"prior": prior}
    out, grid = [], None
    for seed in (0, 1, 2):
        t = time.perf_counter()
        ns = rs.nested_sampling(params, fixed=fixed, seed=seed, **kw)
        t_ns = time.perf_counter() - t
        if grid is None:
            lo = np.maximum(ns._lo, (ns.mean - 6 * ns.sigma).min(axis=0))
            hi = np.minimum(ns._hi, (ns.mean + 6 * ns.sigma).max(axis=0))
            grid = rs.grid_posterior(params, bins=32, fixed=fixed, ranges={n: (float(a), float(b)) for n, a, b in zip(ns.names, lo, hi)}, **kw)
        grid_ln_z = grid.ln_evidence
        if prior is not None:
            # over a sub-range the grid normalises the prior over that sub-range (its own midpoint sum); the nested evidence is
            # normalised over the box: the grid's numerator, brought to the box with the closed-form normalisation
            own = grid.prior_ln_max + np.log(grid.prior_total) + np.sum(np.log(grid._h)) - np.sum(np.log(ns._hi - ns._lo))
            grid_ln_z = grid.ln_evidence + own - ns.ln_prior_norm
        diff = ns.ln_evidence - grid_ln_z
        pull = diff / ns.ln_evidence_error
        out.append({"seed": seed, "names": ns.names, "n_iter": ns.n_iter, "seconds": t_ns, "status": ns.status_names,
                    "nested": ns.ln_evidence.tolist(), "error": ns.ln_evidence_error.tolist(),
                    "grid": np.asarray(grid_ln_z).tolist(), "edge_mass": np.asarray(grid.edge_mass).tolist(),
                    "pull": pull.tolist(), "information": ns.information.tolist(),
                    "acceptance": ns.acceptance.tolist(), "n_stuck": ns.n_stuck.tolist()})
        if prior is not None:
            out[-1].update(prior_norm=ns.prior_norm, ln_prior_norm=ns.ln_prior_norm, ln_prior_norm_error=ns.ln_prior_norm_error)
        print("d = 3 against the grid" + (" under the prior" if prior is not None else "") + ", seed", seed, ": pulls", np.round(pull, 2),
              "mean", pull.mean(), "rms", np.sqrt(np.mean(pull ** 2)), "worst", np.abs(pull).max(), "mean difference", diff.mean(),
              "mean error", ns.ln_evidence_error.mean(), flush=True)
    return out


def under_a_prior(data_fit, rs, params, res):
    """``--prior``: what a Gaussian prior on sigma_v costs per iteration, and the evidence under it against the grid's."""
    from victor_amd.priors import GaussianPrior
    prior = GaussianPrior("sigma_v", 350.0, sigma=30.0)
    res["prior"] = {"names": prior.names, "mean": prior.mean.tolist(), "sigma": prior.sigma.tolist()}
    for name, obj in (("R=1", data_fit), ("R=16", rs)):
        per_iteration(obj, params, True, blocks=1)
        per_iteration(obj, params, True, blocks=1, prior=prior)
        plain, with_prior = [], []
        for _ in range(5):                                   # alternate: one block of each, five times
            plain += per_iteration(obj, params, True, blocks=1)
            with_prior += per_iteration(obj, params, True, blocks=1, prior=prior)
        res["timing"][name] = {"device_s_per_iteration": float(np.median(plain)), "device_prior_s_per_iteration": float(np.median(with_prior)),
                               "device_all": plain, "device_prior_all": with_prior}
        print(name, res["timing"][name], flush=True)
    res["evidence"]["d3_vs_grid_prior"] = d3_against_the_grid(rs, params, {"beta": 0.4}, prior)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-large", action="store_true", help="leave out R = 1024")
    ap.add_argument("--prior", action="store_true", help="the measurements under a Gaussian prior on sigma_v instead")
    args = ap.parse_args()
    import victor_amd
    from tests import cases
    from tests.test_realisations import stack_options
    params = cases.cobaya_info()["params"]
    data_fit = victor_amd.CCFFit(*cases.boss_options("config"))
    stack = victor_amd.CCFFit(*stack_options())
    rs = stack.realisations()
    res = {"defaults": {"n_live": 256, "batch": 32, "steps": 16}, "timing": {}, "evidence": {}}
    if args.prior:
        under_a_prior(data_fit, rs, params, res)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(res, fh, indent=1)
        print(json.dumps(res["timing"]))
        return

    sizes = [("R=1", data_fit), ("R=16", rs)]
    if not args.skip_large:
        sizes.append(("R=1024", stack.realisations(list(np.arange(1024) % 16))))
    for name, obj in sizes:
        dev, ref = [], []
        per_iteration(obj, params, True, blocks=1)
        per_iteration(obj, params, False, blocks=1)
        for _ in range(5):                                   # alternate the routes: one block of each, five times
            dev += per_iteration(obj, params, True, blocks=1)
            ref += per_iteration(obj, params, False, blocks=1)
        res["timing"][name] = {"device_s_per_iteration": float(np.median(dev)), "definition_s_per_iteration": float(np.median(ref)),
                               "device_all": dev, "definition_all": ref}
        print(name, res["timing"][name], flush=True)

    res["evidence"]["d3_vs_grid"] = d3_against_the_grid(rs, params, {"beta": 0.4})

    # d = 4, beta sampled, every mock: against thermodynamic integration
    t = time.perf_counter()
    ns4 = rs.nested_sampling(params, seed=0)
    t_ns4 = time.perf_counter() - t
    t = time.perf_counter()
    ch = rs.sample_chains(params, 4000, walkers=8, seed=0, burn=1000, temper=True, keep_chain=False)
    t_ti = time.perf_counter() - t
    q = ch.tempering
    diff = ns4.ln_evidence - q.ln_evidence
    res["evidence"]["d4_vs_temper"] = {"names": ns4.names, "n_iter": ns4.n_iter, "seconds": t_ns4, "temper_seconds": t_ti,
                                       "status": ns4.status_names, "nested": ns4.ln_evidence.tolist(), "error": ns4.ln_evidence_error.tolist(),
                                       "temper": q.ln_evidence.tolist(), "temper_error": q.ln_evidence_error.tolist(),
                                       "difference": diff.tolist(), "pull": (diff / ns4.ln_evidence_error).tolist()}
    print("d = 4 against temper=: differences", np.round(diff, 3), "mean", diff.mean(), "errors", np.round(ns4.ln_evidence_error, 3), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res["timing"]))


if __name__ == "__main__":
    main()
