#!/usr/bin/env python3
"""The likelihood calls of the reference's usage notebook (notebooks/victor_usage_demo.ipynb, cells around lines
480-512) run through this package: same configuration file layout, same calls, same printed numbers.

    python examples/usage_demo.py            # needs one MI355X; prints chi2 / lnL for the five model variants
    python examples/usage_demo.py --grid-timing OUT.txt      # instead: times a 32^3 grid posterior (grid_timing below)

The reference prints 65.01 / 284.76 (streaming), 65.03 / 284.76 (dispersion), 103.90 / 266.81 (kaiser),
64.39 / 285.06 (anisotropic real-space ccf; the current reference code with SciPy 1.15 gives 64.40 / 285.05, as does this
package) and 64.80 / 285.30 (beta interpolation of the likelihood).
"""

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import yaml
    from victor import CCFFit

    os.chdir(ROOT)
    with open(os.path.join("config", "boss_config.yaml")) as fh:
        info = yaml.full_load(fh)
    fit = CCFFit(info["model"], info["data"])
    params = {"fsigma8": 0.47, "beta": 0.37, "sigma_v": 380, "epsilon": 1.0}
    variants = [("streaming model", {}),
                ("dispersion model", {"rsd_model": "dispersion"}),
                ("Kaiser model", {"rsd_model": "kaiser"}),
                ("streaming, anisotropic real-space ccf", {"assume_isotropic": False}),
                ("streaming, likelihood interpolated in beta", {"beta_interpolation": "likelihood"})]
    for label, kwargs in variants:
        lnl, chi2 = fit.log_likelihood(dict(params), **kwargs)
        print(f"{label:45s} chi2 = {chi2:7.2f}   lnL = {lnl:7.2f}")
    t0 = time.perf_counter()
    n = 2000
    for _ in range(n):
        fit.log_likelihood(dict(params))
    dt = (time.perf_counter() - t0) / n
    print(f"one log_likelihood call: {dt * 1e6:.0f} us (the reference needs about 75 ms)")
    multipoles = fit.theory_multipoles(fit.s, dict(params), poles=[0, 2])
    print("model monopole at the first / last s bin:", multipoles["0"][0], multipoles["0"][-1])
    # the posterior band of the model through the data: chains on the GPU, the theory vectors summed where they run
    with open(os.path.join("config", "boss_cobaya_config.yaml")) as fh:
        block = yaml.full_load(fh)["params"]
    ch = fit.sample_chains(block, 4000, walkers=8, burn=1000, keep_chain=False, predictive=True)
    mean, std = ch.predictive.multipoles[0]
    print(f"posterior monopole at the first s bin: {mean[0, 0]:.4f} +- {std[0, 0]:.4f}; mean chi2 = {ch.predictive.mean_chi2[0]:.2f}, "
          f"p_D = {ch.predictive.p_d[0]:.2f}, DIC = {ch.predictive.dic[0]:.2f}")


def grid_timing(out):
    """A 32^3 grid of the BOSS cobaya configuration (fsigma8, beta, sigma_v; epsilon fixed) against the data vector and against the
    16 golden realisations, on two routes, alternated: ``grid_posterior(device=True)`` - reduced on the GPU - and what the package
    offered before it, the same chunk through ``log_likelihood_batch`` / ``Realisations.log_likelihood`` with the (G, R) values
    reduced by NumPy on the host (total and 1-D marginals by a log-sum-exp; no profiles, no pairs).  Beside them the plain batch
    rate of the same points: the evaluation alone.  A sample is CALLS calls behind one warm-up; medians over SAMPLES samples, with
    the spread.  Wall clock around synchronous calls.  Written to ``out`` (profiles/)."""
    import numpy as np
    import yaml
    from victor_amd import CCFFit
    from victor_amd.grid import default_chunk

    CALLS, SAMPLES = 5, 7
    os.chdir(ROOT)
    with open(os.path.join("config", "boss_config.yaml")) as fh:
        info = yaml.full_load(fh)
    with open(os.path.join("config", "boss_cobaya_config.yaml")) as fh:
        block = yaml.full_load(fh)["params"]
    fit = CCFFit(info["model"], info["data"])
    info["data"]["redshift_space_ccf"].update(data_file=os.path.join(ROOT, "tests", "golden", "realisations", "stack.npy"), simulation_number=0)
    rs = CCFFit(info["model"], info["data"]).realisations()
    kw = dict(bins=32, fixed={"epsilon": 1.0}, ranges={"fsigma8": (0.3, 0.65), "beta": (0.25, 0.55), "sigma_v": (250.0, 500.0)})
    lines = []
    for label, obj, R in (("data vector", fit, 1), (f"{len(rs)} realisations", rs, len(rs))):
        gp = obj.grid_posterior(block, **kw)                            # (warm-up of the device route; the grid for the host route)
        grid, G = gp._grid, gp._grid.G
        chunk = default_chunk(R, G)
        x = grid.points(np.arange(G))
        batch = dict(kw["fixed"], **{n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(grid.names)})
        evaluate = (lambda b: fit.log_likelihood_batch(b)[0][:, None]) if R == 1 else (lambda b: rs.log_likelihood(b)[0])

        def host():
            top, total, m1 = np.full(R, -np.inf), np.zeros(R), [np.zeros((n, R)) for n in grid.shape]
            for g0 in range(0, G, chunk):
                lnl = evaluate({k: (v[g0:g0 + chunk] if np.ndim(v) else v) for k, v in batch.items()})
                new = np.maximum(top, lnl.max(axis=0))
                scale = np.exp(top - new)
                w = np.exp(lnl - new)
                total = total * scale + w.sum(axis=0)
                k = grid.decode(np.arange(g0, min(g0 + chunk, G)))
                for j in range(grid.d):
                    m1[j] *= scale
                    np.add.at(m1[j], k[:, j], w)
                top = new
            return top + np.log(total)

        routes = {"device": lambda: obj.grid_posterior(block, **kw).ln_evidence, "host": host, "batch": lambda: evaluate(batch)}
        want = gp.ln_max + np.log(gp.raw.total)
        assert np.allclose(host(), want, rtol=0, atol=1e-8), (host(), want)
        times = {name: [] for name in routes}
        for name, run in routes.items():
            run()
        for _ in range(SAMPLES):
            for name, run in routes.items():                            # alternated: the routes share whatever else the host does
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    run()
                times[name].append((time.perf_counter() - t0) / CALLS)
        lines.append(f"{label}: G = {G} points (32^3), R = {R}, chunk = {chunk}, {SAMPLES} samples of {CALLS} calls")
        for name, what in (("device", "grid_posterior(device=True)"), ("host", "same chunks, NumPy reduction on the host"),
                           ("batch", "the evaluation alone (plain batch)")):
            t = np.array(times[name])
            med = float(np.median(t))
            lines.append(f"  {what:45s} {med * 1e3:9.2f} ms (min {t.min() * 1e3:.2f}, max {t.max() * 1e3:.2f})   "
                         f"{G / med / 1e6:7.3f} M points/s   {G * R / med / 1e6:8.3f} M point x mock pairs/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    if "--grid-timing" in sys.argv:
        grid_timing(sys.argv[sys.argv.index("--grid-timing") + 1])
    else:
        main()
