"""Write tests/golden/realisations/ (development container only: the reference is read through oracle/ref_shim.py).

  stack.npy        16 synthetic realisations of the BOSS data file: data.npy plus a correlated draw from cov.npy, the SAME
                   normal draw at every beta (x_b = d_b + L_b z, L_b the Cholesky factor of the covariance slice b), so every
                   realisation is as smooth in beta as the data itself; keys s, beta, monopole / quadrupole [16][n_beta][n_s]
  stack_fixed.npy  its fixed-data twin: the data at one beta plus the same draws through cov_fixed.npy, [16][n_s]
  ref.npz          the reference's (lnL, chi2) for 8 Halton points x every realisation of stack.npy, BOSS configuration, by
                   looping simulation_number (one reference CCFFit per realisation), for the sellentin and gaussian forms

    python tools/make_realisation_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from tests import cases  # noqa: E402

N_REAL = 16
N_POINTS = 8
FIXED_BETA_INDEX = 15
FORMS = ("sellentin", "gaussian")


def main():
    out = os.path.join(cases.GOLDEN, "realisations")
    os.makedirs(out, exist_ok=True)
    d = np.load(os.path.join(cases.GOLDEN, "boss", "data.npy"), allow_pickle=True).item()
    cov = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    cov_fixed = np.load(os.path.join(cases.GOLDEN, "boss", "cov_fixed.npy"), allow_pickle=True).item()["covmat"]
    assert np.array_equal(d["beta"], cov["beta"])
    n_s = len(d["s"])
    z = np.random.default_rng(20261015).standard_normal((N_REAL, 2 * n_s))
    vec = np.concatenate([d["monopole"], d["quadrupole"]], axis=1)                    # (n_beta, N)
    draws = np.stack([vec[b] + z @ np.linalg.cholesky(cov["covmat"][b]).T for b in range(len(d["beta"]))], axis=1)
    stack = {"s": d["s"], "beta": d["beta"], "monopole": draws[:, :, :n_s].copy(), "quadrupole": draws[:, :, n_s:].copy()}
    fixed = vec[FIXED_BETA_INDEX] + z @ np.linalg.cholesky(cov_fixed).T                 # (N_REAL, N)
    stack_fixed = {"s": d["s"], "monopole": fixed[:, :n_s].copy(), "quadrupole": fixed[:, n_s:].copy()}
    np.save(os.path.join(out, "stack.npy"), stack, allow_pickle=True)
    np.save(os.path.join(out, "stack_fixed.npy"), stack_fixed, allow_pickle=True)

    import ref_shim
    if not ref_shim.available():
        sys.exit("the reference is not available: stack.npy / stack_fixed.npy written, ref.npz not")
    ref = ref_shim.load()
    hp = cases.halton_params(N_POINTS, with_beta=True)
    pts = [cases.point(hp, i) for i in range(N_POINTS)]
    res = {}
    for form in FORMS:
        lnl = np.empty((N_POINTS, N_REAL))
        chi2 = np.empty((N_POINTS, N_REAL))
        for m in range(N_REAL):
            model, data = cases.boss_options("config")
            data["redshift_space_ccf"].update(data_file="realisations/stack.npy", simulation_number=m)
            data["likelihood"] = dict(data["likelihood"], form=form)
            fit = ref.CCFFit(model, data)
            for p, q in enumerate(pts):
                lnl[p, m], chi2[p, m] = fit.log_likelihood(dict(q))
        res[f"lnl_{form}"], res[f"chi2_{form}"] = lnl, chi2
    meta = {"points": pts, "n_real": N_REAL, "forms": list(FORMS), "simpson_rule": ref_shim.simpson_rule()}
    np.savez(os.path.join(out, "ref.npz"), meta_json=json.dumps(meta), **res)
    print("wrote", out)


if __name__ == "__main__":
    main()
