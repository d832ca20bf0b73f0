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
  R = 1 the joint data vector through ``victor_amd.importance.importance_posterior(joint, ...)``;
* ``--predictive``: the same call with ``predictive=True`` - the posterior band of the model multipoles and the DIC of the first
  mocks, from the theory vectors the sample already computed; with ``--timing`` three routes alternate instead of two: the
  device route without and with ``predictive``, and the definition route with it (``device=False, predictive=True``: what a
  user could assemble before from ``theory_vector_batch`` and NumPy) up to ``--definition-max`` problems, beyond it once
  (``--definition-once-max``: beyond that not at all);
* ``--tail``: the same call with ``tail=True`` - per mock the Pareto shape k of its largest weights against the threshold, and
  the raw against the smoothed ``ln_evidence`` in units of ``ln_evidence_error``; with ``--timing`` the same three routes with
  ``tail`` for ``predictive``: the device route without and with it, and the definition route with it;
* ``--own``: the two-pass recipe - the shared sample with ``tail=True``, then the mocks it flags (``LOW_ESS``, ``HIGH_K``; with
  ``--own-all`` every mock) once more from a proposal of their own, ``ProposalSet.from_fits(bf, bf.laplace, inflate=--inflate,
  dof=--dof).take(flagged)`` with ``--own-n`` points per mock, and the two passes side by side.

    python examples/importance_posterior.py [--joint] [--timing] [--evidence] [--predictive] [--tail] [--sizes 1,16,1024]
                                            [--samples 5] [--own] [--own-all] [--own-n 4096] [--inflate 2] [--dof K] [--out FILE]

Needs a GPU and the test fixtures of the repository (tests/golden)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(obj, params, q, device, n, predictive=None, tail=None):
    t = time.perf_counter()
    ip = obj.importance_posterior(params, q, n=n, seed=0, device=device, predictive=predictive, tail=tail)
    return time.perf_counter() - t, ip


def show_tail(ip):
    """Per mock the Pareto shape of the largest weights and the raw against the smoothed evidence."""
    t = ip.tail
    pull = (ip.ln_evidence - t.ln_evidence) / ip.ln_evidence_error
    names = {t.OK: "OK", t.HIGH_K: "HIGH_K", t.SHORT: "SHORT", t.NO_FINITE: "NO_FINITE"}
    print(f"tail of {t.size} weights per mock, k threshold {t.k_threshold:.3f}")
    for r in range(len(ip)):
        print(f"mock {r:3d}: k {t.k[r]:+.3f} {names[int(t.status[r])]:7s} ESS {ip.ess[r]:8.0f} -> {t.ess[r]:8.0f}  ln_evidence {ip.ln_evidence[r]:.4f} -> "
              f"{t.ln_evidence[r]:.4f}  (raw - smoothed) / error {pull[r]:+.3f}")
    return {"size": t.size, "k_threshold": t.k_threshold, "k": t.k.tolist(), "scale": t.scale.tolist(), "status": t.status.tolist(),
            "ess_raw": ip.ess.tolist(), "ess": t.ess.tolist(), "ln_evidence_raw": ip.ln_evidence.tolist(), "ln_evidence": t.ln_evidence.tolist(),
            "ln_evidence_error_raw": ip.ln_evidence_error.tolist(), "ln_evidence_error": t.ln_evidence_error.tolist(),
            "raw_minus_smoothed_over_error": pull.tolist()}


def two_passes(stack, rs, params, bf, first, args):
    """``--own``: the mocks the shared sample ``first`` (``tail=True``) flags, sampled again from their own proposals."""
    from victor_amd import ProposalSet
    t = first.tail
    flagged = np.arange(len(first)) if args.own_all else np.flatnonzero((first.status != first.OK) | (t.status == t.HIGH_K))
    print(f"shared sample: {len(flagged)} of {len(first)} mocks {'taken' if args.own_all else 'flagged (LOW_ESS or HIGH_K)'}: {flagged.tolist()}")
    if not len(flagged):
        return {"flagged": []}
    qs = ProposalSet.from_fits(bf, bf.laplace, inflate=args.inflate, dof=args.dof)
    sub = stack.realisations(rs.numbers[flagged])
    clock = time.perf_counter()
    again = sub.importance_posterior(params, qs.take(flagged), n=args.own_n, seed=0, tail=True)
    seconds = time.perf_counter() - clock
    print(f"second pass: {args.own_n} points per mock from its own proposal (inflate {args.inflate}, dof {args.dof}) in {seconds:.3f} s; "
          f"pooled instead of own: {np.flatnonzero(qs.pooled[flagged]).tolist()}")
    for i, r in enumerate(flagged):
        print(f"mock {r:3d}: ESS {first.ess[r]:8.0f} of {first.n_inside} -> {again.ess[i]:8.0f} of {again.n_inside[i]}  k {t.k[r]:+.3f} -> "
              f"{again.tail.k[i]:+.3f}  ln_evidence {first.ln_evidence[r]:.4f} +- {first.ln_evidence_error[r]:.4f} -> "
              f"{again.ln_evidence[i]:.4f} +- {again.ln_evidence_error[i]:.4f}")
    return {"flagged": flagged.tolist(), "seconds": seconds, "n": args.own_n, "inflate": args.inflate, "dof": args.dof,
            "pooled": qs.pooled[flagged].tolist(), "n_inside": again.n_inside.tolist(), "ess_shared": first.ess[flagged].tolist(),
            "ess_own": again.ess.tolist(), "k_shared": t.k[flagged].tolist(), "k_own": again.tail.k.tolist(),
            "ln_evidence_shared": first.ln_evidence[flagged].tolist(), "ln_evidence_own": again.ln_evidence.tolist(),
            "ln_evidence_error_own": again.ln_evidence_error.tolist(), "status_own": again.status.tolist()}


def show_predictive(ip, first=3):
    """The band of the first multipole's first bins and the DIC of the first mocks."""
    p = ip.predictive
    poles = p.multipoles if p.multipoles is not None else p.multipoles_of(0)
    ell = sorted(poles)[0]
    mean, std = poles[ell]
    for r in range(min(first, len(ip))):
        band = ", ".join(f"{m:+.4f} +- {s:.4f}" for m, s in zip(mean[r, :4], std[r, :4]))
        print(f"mock {r}: ell = {ell} band, first bins: {band}")
        print(f"        <chi2> {p.mean_chi2[r]:.2f}, chi2 at the mean {p.chi2_at_mean[r]:.2f}, p_D {p.p_d[r]:.2f}, p_V {p.p_v[r]:.2f}, "
              f"DIC {p.dic[r]:.2f}")
    return {"mean_chi2": p.mean_chi2.tolist(), "chi2_at_mean": p.chi2_at_mean.tolist(), "p_d": p.p_d.tolist(), "p_v": p.p_v.tolist(),
            "dic": p.dic.tolist()}


def three_routes(run, R, args, what="predictive"):
    """``--timing --predictive`` (or ``--tail``: ``what``): device off / device on / definition on, alternating after a warm-up of
    each; the definition beyond ``--definition-max`` problems runs once, un-warmed (it takes minutes there), and beyond
    ``--definition-once-max`` not at all."""
    many = R <= args.definition_max
    off, on, ref = [], [], []
    run(True, None)
    run(True, True)
    if many:
        run(False, True)
    for i in range(args.samples):
        off.append(run(True, None)[0])
        on.append(run(True, True)[0])
        if many or (i == 0 and R <= args.definition_once_max):
            ref.append(run(False, True)[0])
    med = {k: float(np.median(v)) if v else float("nan") for k, v in (("off", off), ("on", on), ("definition", ref))}
    print(f"R={R}: device {med['off']:.3f} s ({min(off):.3f} .. {max(off):.3f}), with {what} {med['on']:.3f} s ({min(on):.3f} .. "
          f"{max(on):.3f}), added {1e3 * (med['on'] - med['off']):.1f} ms; definition with {what} {med['definition']:.2f} s "
          f"({len(ref)} run{'s' if len(ref) > 1 else ''}), ratio {med['definition'] / med['on']:.1f}", flush=True)
    return {"device_off_s": med["off"], "device_on_s": med["on"], "definition_on_s": med["definition"], "device_off_all": off,
            "device_on_all": on, "definition_on_all": ref}


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

    def run(obj, device, predictive=None):
        t = time.perf_counter()
        if obj is joint:       # the joint data vector (R = 1): JointFit has no method of this name, the module function is the way
            ip = importance_posterior(joint, params, q, n=args.n, seed=0, fixed=fixed, device=device, predictive=predictive)
        else:
            ip = obj.importance_posterior(params, q, n=args.n, seed=0, fixed=fixed, device=device, predictive=predictive)
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
    if args.predictive:
        res["predictive"] = show_predictive(run(jr, True, True)[1])

    if args.timing:
        res["timing"] = {}
        for R in (int(v) for v in args.sizes.split(",")):
            obj = joint if R == 1 else jr if R == args.stack else joint.realisations(list(np.arange(R) % args.stack))
            if args.predictive:
                res["timing"][f"R={R}"] = three_routes(lambda device, predictive, obj=obj: run(obj, device, predictive), R, args)
                continue
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
    ap.add_argument("--predictive", action="store_true", help="the posterior band and the DIC; with --timing its cost")
    ap.add_argument("--tail", action="store_true", help="the Pareto shape of the largest weights and the smoothed evidence; with --timing its cost")
    ap.add_argument("--own", action="store_true", help="the mocks the shared sample flags, once more from a proposal of their own")
    ap.add_argument("--own-all", action="store_true", help="... every mock, flagged or not")
    ap.add_argument("--own-n", type=int, default=4096, help="... points per mock")
    ap.add_argument("--inflate", type=float, default=2.0, help="... the Laplace covariance times this")
    ap.add_argument("--dof", type=float, default=None, help="... a Student-t of this many degrees of freedom")
    ap.add_argument("--definition-max", type=int, default=16, help="problems up to which --timing --predictive repeats the definition route")
    ap.add_argument("--definition-once-max", type=int, default=1024, help="... and up to which it runs it at least once")
    args = ap.parse_args()
    if args.joint:
        if args.tail:
            ap.error("--tail goes with the single fit (the keyword itself works for joint fits: tail=True)")
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
    if args.predictive:
        res["predictive"] = show_predictive(timed(rs, params, q, True, args.n, True)[1])
    if args.tail:
        res["tail"] = show_tail(timed(rs, params, q, True, args.n, tail=True)[1])
    if args.own or args.own_all:
        res["own"] = two_passes(stack, rs, params, bf, timed(rs, params, q, True, args.n, tail=True)[1], args)

    if args.timing:
        res["timing"] = {}
        for R in (int(v) for v in args.sizes.split(",")):
            obj = data_fit if R == 1 else rs if R == 16 else stack.realisations(list(np.arange(R) % 16))
            if args.tail:
                res["timing"][f"R={R}"] = three_routes(lambda device, tail, obj=obj: timed(obj, params, q, device, args.n, tail=tail), R, args, "tail")
                continue
            if args.predictive:
                res["timing"][f"R={R}"] = three_routes(lambda device, predictive, obj=obj: timed(obj, params, q, device, args.n, predictive), R, args)
                continue
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
