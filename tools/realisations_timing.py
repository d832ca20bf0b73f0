"""BOSS at batch 4096 against M simulation realisations (vk_eval_realisations): wall time, the theory / chi-square split of the
library's event timing (vk_timing_*), the matrix-core kernel against its vector-ALU twin (VICTOR_HIP_REAL_VALU, same tiling,
alternated), and the same work as M separate CCFFit objects at M = 64.  Writes realisations_<M>.txt and
realisations_separate_fits.txt into the output directory.  With --paired instead: 65536 rows in pairs mode over 1024 mocks,
realisations(paired_model=True) against the shared model, BOSS and the fixed-table config 3 (paired_main).  With --cuts: scale
cuts in one call against the route without them - 16 mocks, 4096 points, K = 1, 4 and 8 nested s_min cuts:
``CutRealisations.log_likelihood`` (one theory launch, the cuts kernel) against K sliced ``CCFFit`` objects (data stack and
covariance sliced into files, as a user does by hand) evaluated one after another through ``Realisations.log_likelihood``; the
two legs alternate in one process after a warm-up of each, median of --reps timed calls and their spread, and the library's
event split of the one-call leg (cuts_main).

    python tools/realisations_timing.py OUT_DIR [--commit SHA] [--paired | --cuts [--reps 7]]
"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import cases  # noqa: E402
from victor_amd import _native as N  # noqa: E402

PEAK_FP64 = 78.6e12          # MI355X FP64 vector and matrix peak (AMD specification)
BATCH = 4096


def options(path, m=0):
    model, data = cases.boss_options("config")
    data["redshift_space_ccf"].update(data_file=path, simulation_number=m)
    return model, data


def write_stack(path, n_real):
    s = np.load(os.path.join(cases.GOLDEN, "realisations", "stack.npy"), allow_pickle=True).item()
    scale = (1.0 + (np.arange(n_real) // 16) / 100.0)[:, None, None]
    idx = np.arange(n_real) % 16
    np.save(path, dict(s, monopole=s["monopole"][idx] * scale, quadrupole=s["quadrupole"][idx] * scale), allow_pickle=True)


def timed(rs, hp, reps):
    model = rs.fit._merged({})
    eng = rs.fit._get_engine(rs.fit._engine_key(model), model["simpson_even"])
    rs.log_likelihood(hp)                                       # warm-up (code objects, upload, scratch)
    walls, th, ch = [], [], []
    for _ in range(reps):
        eng.timing(True)
        t0 = time.perf_counter()
        rs.log_likelihood(hp)
        walls.append(time.perf_counter() - t0)
        a, b, _ = eng.read_timing(reset=True)
        eng.timing(False)
        th.append(a)
        ch.append(b)
    return np.median(walls) * 1e3, np.median(th), np.median(ch)


def main():
    import victor_amd
    out = sys.argv[1]
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    os.makedirs(out, exist_ok=True)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "stack1000.npy")
    write_stack(path, 1000)
    hp = cases.halton_params(BATCH, with_beta=True)
    fit = victor_amd.CCFFit(*options(path))
    n = 60
    for m in (64, 1000):
        rs = fit.realisations(list(range(m)))
        lines = [f"commit {commit}", f"BOSS (N = {n}), {BATCH} points x {m} realisations; medians of 5 calls; ms"]
        res = {}
        for rnd in range(2):                                    # alternated A/B: matrix cores, vector ALU
            for name, val in (("mfma", None), ("valu", "1")):
                N.set_knob("VICTOR_HIP_REAL_VALU", val)
                res.setdefault(name, []).append(timed(rs, hp, 5))
        N.set_knob("VICTOR_HIP_REAL_VALU", None)
        flops = 2.0 * n * n * m * BATCH
        flops_pad = 2.0 * 64 * 64 * m * BATCH
        for name, runs in res.items():
            for wall, th, ch in runs:
                lines.append(f"{name:5s} wall {wall:9.2f}  theory {th:8.3f}  chi2 {ch:8.3f}  chi2/theory {ch / th:6.3f}  "
                             f"chi2 rate {flops / (ch * 1e-3) / 1e12:6.2f} TF/s useful ({flops_pad / (ch * 1e-3) / 1e12:6.2f} "
                             f"padded to 64) = {flops / (ch * 1e-3) / PEAK_FP64:6.3f} of the {PEAK_FP64 / 1e12:.1f} TF/s FP64 peak")
        text = "\n".join(lines) + "\n"
        print(text, flush=True)
        with open(os.path.join(out, f"realisations_{m}.txt"), "w") as fh:
            fh.write(text)
    # the same work as 64 separate fits (one context each), one batch of 4096 per fit
    m = 64
    t0 = time.perf_counter()
    fits = [victor_amd.CCFFit(*options(path, i)) for i in range(m)]
    for f in fits:
        f.log_likelihood_batch(cases.point(hp, 0))              # context creation and table upload
    t_setup = time.perf_counter() - t0
    t0 = time.perf_counter()
    for f in fits:
        f.log_likelihood_batch(hp)
    t_eval = time.perf_counter() - t0
    rs = fit.realisations(list(range(m)))
    t0 = time.perf_counter()
    rs.log_likelihood(cases.point(hp, 0))
    t_rs_setup = time.perf_counter() - t0
    wall = timed(rs, hp, 5)[0]
    text = (f"commit {commit}\nBOSS, {BATCH} points x {m} realisations\n"
            f"{m} separate CCFFit objects: set-up {t_setup * 1e3:.1f} ms, evaluation {t_eval * 1e3:.1f} ms\n"
            f"one Realisations object:    set-up {t_rs_setup * 1e3:.1f} ms, evaluation {wall:.1f} ms\n"
            f"evaluation speed-up {t_eval * 1e3 / wall:.1f} x\n")
    print(text, flush=True)
    with open(os.path.join(out, "realisations_separate_fits.txt"), "w") as fh:
        fh.write(text)


# ---- --paired: what it costs to give every mock the model of its own real-space CCF (realisations(paired_model=True)) ---------
PAIRED_MOCKS, PAIRED_ROWS = 1024, 65536


def paired_fixtures(tmp):
    """name -> (model, data) of a fit over PAIRED_MOCKS mocks: the BOSS stack tiled by the rule of write_stack (beta-dependent
    tables) and the synthetic config 3 (fixed tables), each against a model file whose real-space multipoles have one
    realisation per mock (base x (1 + 0.03 sin(0.7 m + r / 20)), realisation 0 the base)."""
    m = np.arange(PAIRED_MOCKS)

    def factor(r):
        f = 1.0 + 0.03 * np.sin(0.7 * m[:, None] + np.asarray(r)[None, :] / 20.0)
        f[0] = 1.0
        return f
    out = {}
    base = np.load(os.path.join(cases.GOLDEN, "boss", "model.npy"), allow_pickle=True).item()
    f = factor(base["r"])[:, None, :]
    mpath = os.path.join(tmp, "boss_model_stack.npy")
    np.save(mpath, dict(base, monopole=base["monopole"][None] * f, quadrupole=base["quadrupole"][None] * f), allow_pickle=True)
    dpath = os.path.join(tmp, "boss_data_stack.npy")
    write_stack(dpath, PAIRED_MOCKS)
    model, data = options(dpath)
    model["input_model_data_file"] = mpath
    model["realspace_ccf"]["simulation_number"] = 0
    out["BOSS (n_beta_r = 31)"] = (model, data)
    base = np.load(os.path.join(cases.GOLDEN, "synth", "model.npy"), allow_pickle=True).item()
    f = factor(base["r"])
    keys = ("monopole", "quadrupole", "hexadecapole")
    mpath = os.path.join(tmp, "synth_model_stack.npy")
    np.save(mpath, dict(base, **{k: base[k][None] * f for k in keys}), allow_pickle=True)
    d = np.load(os.path.join(cases.GOLDEN, "synth", "data3.npy"), allow_pickle=True).item()
    scale = (1.0 + (m // 16) / 100.0)[:, None]
    dpath = os.path.join(tmp, "synth_data_stack.npy")
    np.save(dpath, dict(d, **{k: d[k][None] * scale for k in keys}), allow_pickle=True)
    model, data = cases.synth_options(3)
    model["input_model_data_file"] = mpath
    model["realspace_ccf"]["simulation_number"] = 0
    data["redshift_space_ccf"].update(data_file=dpath, simulation_number=0)
    out["config 3 (fixed tables)"] = (model, data)
    return out


def paired_main():
    """PAIRED_ROWS rows in pairs mode over PAIRED_MOCKS mocks, paired_model=True against False: wall time per call, median of
    five and their spread, the two legs alternating in one process after a warm-up of each.  Each leg has a fit - an engine - of
    its own, so the warm-ups carry the uploads and a timed call is the evaluation alone.  Writes paired_realisations.txt."""
    import victor_amd
    from victor_amd import engine
    out = sys.argv[1]
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    os.makedirs(out, exist_ok=True)
    tmp = tempfile.mkdtemp()
    which = ((7 * np.arange(PAIRED_ROWS)) % PAIRED_MOCKS).astype(np.int32)
    lines = [f"commit {commit}", f"{PAIRED_ROWS} rows in pairs mode over {PAIRED_MOCKS} mocks; wall ms per call, median of 5 [min .. max]"]
    for name, (model, data) in paired_fixtures(tmp).items():
        fits = [victor_amd.CCFFit(model, data), victor_amd.CCFFit(model, data)]      # an engine per leg: no re-upload between calls
        hp = cases.halton_params(PAIRED_ROWS, with_beta=not fits[0].fixed_data)
        t0 = time.perf_counter()
        legs = {"shared": fits[0].realisations(), "paired": fits[1].realisations(paired_model=True)}
        sets = legs["paired"].model_sets()
        t_sets = time.perf_counter() - t0
        t, keep = engine.build_tables(fits[0], fits[0])
        n = engine.table_array_lengths(t)
        per_set = 8 * (n["xi.coef"] + n["uni_xi"] + n["uni_xic"])
        del keep
        walls = {k: [] for k in legs}
        values = {}
        for k, rs in legs.items():                                  # warm-up: code objects, uploads, scratch
            t0 = time.perf_counter()
            values[k] = rs.log_likelihood_pairs(hp, which)
            lines.append(f"{name}: first call {k} {1e3 * (time.perf_counter() - t0):.1f} ms")
        for _ in range(5):
            for k, rs in legs.items():
                t0 = time.perf_counter()
                rs.log_likelihood_pairs(hp, which)
                walls[k].append(1e3 * (time.perf_counter() - t0))
        # (mock 0's tables are the fit's own: the same bits there)
        same = np.array_equal(values["paired"][1][which == 0], values["shared"][1][which == 0])
        lines.append(f"{name}: table set {per_set} bytes, {PAIRED_MOCKS} sets {per_set * PAIRED_MOCKS / 1e6:.1f} MB "
                     f"(stacked on the host in {t_sets:.1f} s: {sum(s.nbytes for s in sets if s is not None) / 1e6:.1f} MB); "
                     f"rows of mock 0 equal in both legs: {same}; rows that differ: {int(np.sum(values['paired'][1] != values['shared'][1]))} of {PAIRED_ROWS}")
        for k, w in walls.items():
            lines.append(f"{name}: {k:6s} {np.median(w):9.2f} [{min(w):.2f} .. {max(w):.2f}]")
        lines.append(f"{name}: paired / shared {np.median(walls['paired']) / np.median(walls['shared']):.4f}")
        for f in fits:
            f._engine = None
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(os.path.join(out, "paired_realisations.txt"), "w") as fh:
        fh.write(text)


# ---- --cuts: K scale cuts in one call against K sliced fits --------------------------------------------------------------------
CUT_DROPS = {1: [0], 4: [0, 2, 4, 7], 8: [0, 1, 2, 3, 4, 5, 6, 7]}


def sliced_fit(tmp, first):
    """The fit a user builds for ``s >= s[first]``: sliced data stack and covariance files."""
    import victor_amd
    stack = np.load(os.path.join(cases.GOLDEN, "realisations", "stack.npy"), allow_pickle=True).item()
    cov = np.load(os.path.join(cases.GOLDEN, "boss", "cov.npy"), allow_pickle=True).item()
    keep = np.arange(first, len(stack["s"]))
    idx = np.concatenate([keep, len(stack["s"]) + keep])
    data_path, cov_path = os.path.join(tmp, f"stack_{first}.npy"), os.path.join(tmp, f"cov_{first}.npy")
    np.save(data_path, dict(stack, s=stack["s"][keep], monopole=stack["monopole"][..., keep], quadrupole=stack["quadrupole"][..., keep]),
            allow_pickle=True)
    np.save(cov_path, dict(cov, covmat=np.ascontiguousarray(cov["covmat"][:, idx][:, :, idx])), allow_pickle=True)
    model, data = options(data_path)
    data["covariance_matrix"]["data_file"] = cov_path
    return victor_amd.CCFFit(model, data)


def cuts_main():
    """--cuts (see the module docstring).  Writes scale_cuts.txt."""
    import victor_amd
    from victor_amd import ScaleCut
    out = sys.argv[1]
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else "unknown"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    os.makedirs(out, exist_ok=True)
    tmp = tempfile.mkdtemp()
    hp = cases.halton_params(BATCH, with_beta=True)
    lines = [f"commit {commit}", f"BOSS (N = 60), {BATCH} points x 16 mocks x K nested s_min cuts; wall ms per call, median of {reps} [min .. max]"]
    for K, drops in CUT_DROPS.items():
        fit = victor_amd.CCFFit(*options(os.path.join(cases.GOLDEN, "realisations", "stack.npy")))
        cr = fit.realisations().scale_cuts([ScaleCut(s_min=None if k == 0 else float(fit.s[k])) for k in drops])
        base = [sliced_fit(tmp, k).realisations() for k in drops]
        model = fit._merged({})
        eng = fit._get_engine(fit._engine_key(model), model["simpson_even"])

        def one_call():
            return cr.log_likelihood(hp)

        def one_by_one():
            return [rs.log_likelihood(hp) for rs in base]
        got, want = one_call(), one_by_one()                     # warm-up of each leg
        worst = max(float(np.nanmax(np.abs(got[1][:, k] / w[1] - 1.0))) for k, w in enumerate(want))
        walls = {"one call": [], "K fits": []}
        th, ch = [], []
        for _ in range(reps):                                    # alternated
            eng.timing(True)
            t0 = time.perf_counter()
            one_call()
            walls["one call"].append(1e3 * (time.perf_counter() - t0))
            a, b, _ = eng.read_timing(reset=True)
            eng.timing(False)
            th.append(a)
            ch.append(b)
            t0 = time.perf_counter()
            one_by_one()
            walls["K fits"].append(1e3 * (time.perf_counter() - t0))
        med = {k: float(np.median(v)) for k, v in walls.items()}
        lines.append(f"K = {K} (entries kept {[t.n for t in cr.tables]}): largest |chi2 ratio - 1| between the legs {worst:.1e}")
        for k, v in walls.items():
            lines.append(f"  {k:9s} {med[k]:9.2f} [{min(v):.2f} .. {max(v):.2f}]")
        lines.append(f"  one call, device events: theory launch {np.median(th):.3f} ms, cuts kernel {np.median(ch):.3f} ms")
        lines.append(f"  one call / K fits = {med['one call'] / med['K fits']:.3f}")
        for f in [fit] + [rs.fit for rs in base]:
            f._engine = None
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    with open(os.path.join(out, "scale_cuts.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    cuts_main() if "--cuts" in sys.argv else paired_main() if "--paired" in sys.argv else main()
