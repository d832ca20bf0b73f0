"""The standard scale-cut table on the BOSS cobaya configuration: fsigma8 +- sigma per mock and per s_min, from ONE
``importance_posterior`` call.

``rs.scale_cuts(cuts)`` makes K nested ``s_min`` cuts of the 16-mock stack resident next to the mocks (K x 16 problems); every
point of the shared importance sample costs one theory evaluation, and the kernel forms each cut's chi-square with the inverse of
that cut's own sub-covariance, its log determinant and its count of data points.  The proposal is pooled over the best fits of
the uncut mocks.

    python examples/scale_cuts.py [--drop 0,2,4,7] [--n 16384] [--poles 0,2]

Needs a GPU and the test fixtures of the repository (tests/golden)."""

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drop", default="0,2,4,7", help="innermost s bins dropped, one cut each")
    ap.add_argument("--n", type=int, default=16384, help="draws of the shared sample")
    ap.add_argument("--poles", default=None, help="multipoles kept by every cut (default: all of the fit's)")
    args = ap.parse_args()
    import victor_amd
    from tests import cases
    from tests.test_realisations import stack_options
    from victor_amd import GaussianProposal, ScaleCut
    params = cases.cobaya_info()["params"]
    fit = victor_amd.CCFFit(*stack_options())
    rs = fit.realisations()
    drops = [int(v) for v in args.drop.split(",")]
    poles = None if args.poles is None else [int(v) for v in args.poles.split(",")]
    cuts = [ScaleCut(s_min=None if k == 0 else float(fit.s[k]), poles=poles) for k in drops]
    cr = rs.scale_cuts(cuts)
    K, R = cr.shape
    print(f"{K} cuts x {R} mocks = {len(cr)} problems; entries kept per cut: {[t.n for t in cr.tables]}")

    bf = rs.best_fit(params, covariance=True)
    q = GaussianProposal.from_fits(bf, bf.laplace, inflate=3.0)
    t = time.perf_counter()
    ip = cr.importance_posterior(params, q, n=args.n, seed=0, tail=True)
    seconds = time.perf_counter() - t
    print(f"{ip.n_inside} of {ip.n_drawn} draws inside the box; all {len(cr)} posteriors in {seconds:.2f} s")
    j = ip.names.index("fsigma8")
    mean, sigma, ess = cr.unflatten(ip.mean[:, j]), cr.unflatten(ip.sigma[:, j]), cr.unflatten(ip.ess)
    head = "mock " + "".join(f"  s_min = {fit.s[k]:5.1f} (n = {t.n:2d})" for k, t in zip(drops, cr.tables))
    print("fsigma8 +- sigma")
    print(head)
    for m in range(R):
        print(f"{int(cr.numbers[m]):4d} " + "".join(f"   {mean[k, m]:.4f} +- {sigma[k, m]:.4f}    " for k in range(K)))
    print("mean " + "".join(f"   {mean[k].mean():.4f} +- {sigma[k].mean():.4f}    " for k in range(K)))
    print("smallest effective sample size per cut:", np.round(ess.min(axis=1)).astype(int).tolist())


if __name__ == "__main__":
    main()
