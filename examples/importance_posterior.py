"""Importance-sampled posteriors of every mock on the BOSS cobaya configuration (DESIGN.md section 7e quotes the output):

* ``rs.best_fit(covariance=True)``, the shared proposal ``GaussianProposal.from_fits(bf, bf.laplace, inflate=2)`` and the
  posterior of every mock of the stack from one sample: the effective sample size, evidence, mean and width per mock;
* ``--timing``: wall time of ``importance_posterior`` at d = 4, G = 65536 draws, for R = 1 (the data vector), 16 (the mock stack)
  and 1024 (the stack repeated), the device route against the definition route (``device=False``: what a user could write
  before) - the two alternate in one process after a warm-up of each, the median of ``--samples`` runs and their spread;
* ``--evidence``: beta fixed, d = 3: ``ln_evidence`` against ``grid_posterior(bins=32).ln_evidence`` per mock; d = 4: against
  ``nested_sampling``, as pulls in units of the two errors combined;
* ``--joint``: the same three steps for the five-quantile density-split fit under one covariance with a ``sigma_v`` per
  quantile (d = 7): ``JointRealisations.importance_posterior`` for the mock stack (``--stack`` mocks per block), and for
  R = 1 the joint data vector through ``victor_amd.importance.importance_posterior(joint, ...)``.

    python examples/importance_posterior.py [--joint] [--timing] [--evidence] [--sizes 1,16,1024] [--samples 5] [--out FILE]

Needs a GPU and the test fixtures of the repository (tests/golden)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(obj, params, q, device, n):
    t = time.perf_counter()
    ip = obj.importance_posterior(params, q, n=n, seed=0, device=device)
    return time.perf_counter() - t, ip


def joint_main(args):
    """``--joint``: the five-quantile density-split fit under one covariance, a sigma_v per quantile (d = 7: fsigma8, five
    sigma_v@q, epsilon; beta, which these data ignore, fixed), stacks of ``--stack`` mocks written from the goldens."""
    import tempfile
    import victor_amd
    from tests import cases
    from tests.test_joint_cov import correlated
    from tests.test_joint_realisations import dsplit_stacks
    from victor_amd import GaussianProposal
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import JointFit, per_block
    params = per_block(cases.cobaya_info()["params"], ["sigma_v"], 5)
    fixed = {"beta": 0.4}
    fits = [victor_amd.CCFFit(*o) for o in dsplit_stacks(tempfile.mkdtemp(), args.stack)]
    joint = JointFit(fits, covariance=correlated([f.covmat for f in fits]))
    jr = joint.realisations()
    res = {"n": args.n, "stack": args.stack}

    def run(obj, device):
        t = time.perf_counter()
        if obj is joint:       # the joint data vector (R = 1): JointFit has no method of this name, the module function is the way
            ip = importance_posterior(joint, params, q, n=args.n, seed=0, fixed=fixed, device=device)
        else:
            ip = obj.importance_posterior(params, q, n=args.n, seed=0, fixed=fixed, device=device)
        return time.perf_counter() - t, ip

    t = time.perf_counter()
    bf = jr.best_fit(params, fixed=fixed, covariance=True)
    q = GaussianProposal.from_fits(bf, bf.laplace, inflate=2.0)
    t_fit = time.perf_counter() - t
    t_ip, ip = run(jr, True)
    res["mocks"] = {"names": ip.names, "proposal_mean": q.mean.tolist(), "proposal_sigma": np.sqrt(np.diag(q.cov)).tolist(),
                    "best_fit_seconds": t_fit, "seconds": t_ip, "n_drawn": ip.n_drawn, "n_inside": ip.n_inside, "chunk": ip.chunk,
                    "ess": ip.ess.tolist(), "status": ip.status.tolist(), "ln_evidence": ip.ln_evidence.tolist(),
                    "ln_evidence_error": ip.ln_evidence_error.tolist(), "mean": ip.mean.tolist(), "sigma": ip.sigma.tolist()}
    print(f"joint fit, d = {len(ip.names)} {ip.names}: proposal from {int(np.sum(bf.status == bf.CONVERGED))} of {len(bf)} best fits in "
          f"{t_fit:.2f} s; {ip.n_inside} of {ip.n_drawn} draws inside the box, all {len(ip)} joint mocks in {t_ip:.2f} s")
    print("ESS per mock", np.round(ip.ess).astype(int).tolist())
    print("ln_evidence", np.round(ip.ln_evidence, 3).tolist())
    print("error      ", np.round(ip.ln_evidence_error, 4).tolist(), flush=True)

    if args.timing:
        res["timing"] = {}
        for R in (int(v) for v in args.sizes.split(",")):
            obj = joint if R == 1 else jr if R == args.stack else joint.realisations(list(np.arange(R) % args.stack))
            dev, ref = [], []
            run(obj, True)                                       # a warm-up of each route
            run(obj, False)
            for _ in range(args.samples):                        # alternate the routes
                dev.append(run(obj, True)[0])
                ref.append(run(obj, False)[0])
            res["timing"][f"R={R}"] = {"device_s": float(np.median(dev)), "definition_s": float(np.median(ref)),
                                       "ratio": float(np.median(ref) / np.median(dev)), "device_all": dev, "definition_all": ref}
            print(f"R={R}: device {np.median(dev):.3f} s ({min(dev):.3f} .. {max(dev):.3f}), definition {np.median(ref):.3f} s "
                  f"({min(ref):.3f} .. {max(ref):.3f}), ratio {np.median(ref) / np.median(dev):.2f}", flush=True)

    if args.evidence:
        ns = jr.nested_sampling(params, fixed=fixed, seed=0)
        diff = ip.ln_evidence - ns.ln_evidence
        pull = diff / np.hypot(ip.ln_evidence_error, ns.ln_evidence_error)
        res["vs_nested"] = {"importance": ip.ln_evidence.tolist(), "error": ip.ln_evidence_error.tolist(), "nested": ns.ln_evidence.tolist(),
                            "nested_error": ns.ln_evidence_error.tolist(), "pull": pull.tolist()}
        print(f"d = {len(ip.names)} against nested_sampling: pulls", np.round(pull, 2).tolist(), "rms", float(np.sqrt(np.mean(pull ** 2))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--evidence", action="store_true")
    ap.add_argument("--joint", action="store_true", help="the density-split joint fit under one covariance, a sigma_v per quantile")
    ap.add_argument("--stack", type=int, default=16, help="mocks per block of --joint")
    ap.add_argument("--sizes", default="1,16,1024", help="problem counts of --timing")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--n", type=int, default=65536, help="draws")
    args = ap.parse_args()
    if args.joint:
        return joint_main(args)
    import victor_amd
    from tests import cases
    from tests.test_realisations import stack_options
    from victor_amd import GaussianProposal
    params = cases.cobaya_info()["params"]
    data_fit = victor_amd.CCFFit(*cases.boss_options("config"))
    stack = victor_amd.CCFFit(*stack_options())
    rs = stack.realisations()
    res = {"n": args.n}

    # the proposal: pooled over the mocks' best fits and their Laplace covariances
    t = time.perf_counter()
    bf = rs.best_fit(params, covariance=True)
    q = GaussianProposal.from_fits(bf, bf.laplace, inflate=2.0)
    t_fit = time.perf_counter() - t
    t_ip, ip = timed(rs, params, q, True, args.n)
    res["stack"] = {"names": ip.names, "proposal_mean": q.mean.tolist(), "proposal_sigma": np.sqrt(np.diag(q.cov)).tolist(),
                    "best_fit_seconds": t_fit, "seconds": t_ip, "n_drawn": ip.n_drawn, "n_inside": ip.n_inside, "chunk": ip.chunk,
                    "ess": ip.ess.tolist(), "max_weight_share": ip.max_weight_share.tolist(), "status": ip.status.tolist(),
                    "ln_evidence": ip.ln_evidence.tolist(), "ln_evidence_error": ip.ln_evidence_error.tolist(),
                    "mean": ip.mean.tolist(), "sigma": ip.sigma.tolist()}
    print(f"proposal from {int(np.sum(bf.status == bf.CONVERGED))} best fits in {t_fit:.2f} s; {ip.n_inside} of {ip.n_drawn} draws inside the "
          f"box, all {len(ip)} mocks in {t_ip:.2f} s")
    print("ESS per mock", np.round(ip.ess).astype(int).tolist())
    print("ln_evidence", np.round(ip.ln_evidence, 3).tolist())
    print("error      ", np.round(ip.ln_evidence_error, 4).tolist())
    for j, n in enumerate(ip.names):
        lo, hi = ip.interval(n, 0.68)
        print(f"{n:8s} mock 0: mean {ip.mean[0, j]:.4f} sigma {ip.sigma[0, j]:.4f} median {ip.median(n)[0]:.4f} 68% [{lo[0]:.4f}, {hi[0]:.4f}]")

    if args.timing:
        res["timing"] = {}
        for R in (int(v) for v in args.sizes.split(",")):
            obj = data_fit if R == 1 else rs if R == 16 else stack.realisations(list(np.arange(R) % 16))
            dev, ref = [], []
            timed(obj, params, q, True, args.n)                   # a warm-up of each route
            timed(obj, params, q, False, args.n)
            for _ in range(args.samples):                        # alternate the routes
                dev.append(timed(obj, params, q, True, args.n)[0])
                ref.append(timed(obj, params, q, False, args.n)[0])
            res["timing"][f"R={R}"] = {"device_s": float(np.median(dev)), "definition_s": float(np.median(ref)),
                                       "ratio": float(np.median(ref) / np.median(dev)), "device_all": dev, "definition_all": ref}
            print(f"R={R}: device {np.median(dev):.3f} s ({min(dev):.3f} .. {max(dev):.3f}), definition {np.median(ref):.3f} s "
                  f"({min(ref):.3f} .. {max(ref):.3f}), ratio {np.median(ref) / np.median(dev):.2f}", flush=True)

    if args.evidence:
        # beta fixed, d = 3, every mock: against the grid over the proposal's +- 6 sigma
        fixed = {"beta": 0.4}
        bf3 = rs.best_fit(params, fixed=fixed, covariance=True)
        q3 = GaussianProposal.from_fits(bf3, bf3.laplace, inflate=2.0)
        ip3 = rs.importance_posterior(params, q3, n=args.n, fixed=fixed)
        lo = np.maximum(ip3._layout.lo, (ip3.mean - 6 * ip3.sigma).min(axis=0))
        hi = np.minimum(ip3._layout.hi, (ip3.mean + 6 * ip3.sigma).max(axis=0))
        grid = rs.grid_posterior(params, bins=32, fixed=fixed, ranges={n: (float(a), float(b)) for n, a, b in zip(ip3.names, lo, hi)})
        diff = ip3.ln_evidence - grid.ln_evidence
        res["d3_vs_grid"] = {"importance": ip3.ln_evidence.tolist(), "error": ip3.ln_evidence_error.tolist(), "ess": ip3.ess.tolist(),
                             "grid": grid.ln_evidence.tolist(), "difference": diff.tolist(), "pull": (diff / ip3.ln_evidence_error).tolist()}
        print("d = 3 against grid_posterior(bins=32): differences", np.round(diff, 4).tolist(), "errors", np.round(ip3.ln_evidence_error, 4).tolist())
        # d = 4, every mock: against nested sampling
        ip4 = rs.importance_posterior(params, q, n=args.n)
        ns = rs.nested_sampling(params, seed=0)
        diff = ip4.ln_evidence - ns.ln_evidence
        pull = diff / np.hypot(ip4.ln_evidence_error, ns.ln_evidence_error)
        res["d4_vs_nested"] = {"importance": ip4.ln_evidence.tolist(), "error": ip4.ln_evidence_error.tolist(), "ess": ip4.ess.tolist(),
                               "nested": ns.ln_evidence.tolist(), "nested_error": ns.ln_evidence_error.tolist(), "pull": pull.tolist()}
        print("d = 4 against nested_sampling: pulls", np.round(pull, 2).tolist(), "rms", float(np.sqrt(np.mean(pull ** 2))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
