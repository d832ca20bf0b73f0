"""Nested sampling (victor_amd/nested.py, vk_nested_begin) without a GPU: the rules of victor_amd/csrc/vk_nested_step.h compiled on
their own under g++ and driven on the analytic functions of tests/test_chains.py, checked iteration by iteration, step by step and
byte for byte against the NumPy loop that defines the runs; cuts and extends; the read-out against a direct float128
restatement; the evidence of Gaussians against quadrature and the closed form; the refusals, raised before any device call; and
the ABI surface.

The evidence caps are conditions, not measurements: every run within 4 of its own ``ln_evidence_error`` of the truth, the mean
over eight fixed seeds within 4 rms(error) / sqrt(8).  The definition alone, at the defaults (n_live 256, batch 32, steps 16),
seeds 0 .. 7: the 2-D Gaussian of tests/test_tempering.py gave a seed mean of -0.026 under a cap of 0.12 and a worst pull of 2.05;
the 4-D Gaussian with widths 0.02, 0.05, 0.1, 0.2 a seed mean of -0.050 under a cap of 0.20 and a worst pull of 1.6."""

import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import DRIVER as CHAIN_DRIVER
from tests.test_chains import LNL, same_bytes
from tests.test_tempering import EXACT_LN_Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf

# the analytic functions of tests/test_chains.py (d = 3), taken from its driver as they stand, and two of any dimension
LNL_OF = CHAIN_DRIVER[CHAIN_DRIVER.index("static double lnl_of"):CHAIN_DRIVER.index("// usage")]


def _quad(x):
    q = 0.0
    for v in x:
        q = q + 8.0 * ((v - 0.1) * (v - 0.1))
    return -q


def _tie(x):
    # plateaus: whole sets of live points share one lnL, and a step inside a plateau never beats L*
    return -float(int((x[0] + 1.0) * 2.0))


FUNCTIONS = dict(LNL, quad=_quad, tie=_tie)

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_nested_step.h"

""" + LNL_OF + r"""
static double lnl_any(const char* fn, int d, const double* x) {
  if (!strcmp(fn, "quad")) {
    double q = 0.0;
    for (int j = 0; j < d; ++j) q = q + 8.0 * ((x[j] - 0.1) * (x[j] - 0.1));
    return -q;
  }
  if (!strcmp(fn, "tie")) return -(double)(int)((x[0] + 1.0) * 2.0);
  return lnl_of(fn, x);
}

// usage: driver fn d R L K S T scale in out  then d values each of lo, hi
// in:  doubles x0[R][L][d], pick[T][R][K], dz[T][S][R][K][d]
// out: doubles, per iteration: dead[R][K], lstar[R], range[R][d], from[R][K], per step (accept[R][K], y[R][K][d], lnl[R][K],
//      chi2[R][K]), then the live x[R][L][d], lnl[R][L], chi2[R][L]; at the end n_accept[R], n_steps[R], n_stuck[R]
// The state is held structure-of-arrays, live points with stride R L and walkers with stride R K, as the device holds it.
int main(int argc, char** argv) {
  const char* fn = argv[1];
  vkchain::Box box{};
  box.d = atoi(argv[2]);
  const int d = box.d, R = atoi(argv[3]), L = atoi(argv[4]), K = atoi(argv[5]), S = atoi(argv[6]), T = atoi(argv[7]);
  const double scale = strtod(argv[8], nullptr);
  int a = 11;
  for (int j = 0; j < d; ++j) box.lo[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < d; ++j) box.hi[j] = strtod(argv[a++], nullptr);
  const size_t RL = (size_t)R * L, RK = (size_t)R * K;
  std::vector<double> in(RL * d + (size_t)T * RK + (size_t)T * S * RK * d);
  FILE* fi = fopen(argv[9], "rb");
  if (!fi || fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const double *x0 = in.data(), *pick = x0 + RL * d, *dz = pick + (size_t)T * RK;
  std::vector<double> lx(RL * d), llnl(RL), lchi(RL), wx(RK * d), wlnl(RK), wchi(RK), range((size_t)R * d), lstar(R);
  std::vector<int64_t> n_accept(RK), n_steps(RK), n_stuck(RK);
  std::vector<int32_t> moved(RK);
  std::vector<int> slot(RK), rank(L);
  auto walker = [&](size_t c) {
    vknest::Walker w{};
    w.stride = RK;
    w.y = wx.data() + c; w.lnl = wlnl.data() + c; w.chi2 = wchi.data() + c;
    w.n_accept = n_accept.data() + c; w.n_steps = n_steps.data() + c; w.n_stuck = n_stuck.data() + c; w.moved = moved.data() + c;
    return w;
  };
  FILE* fo = fopen(argv[10], "wb");
  if (!fo) return 2;
  auto put = [&](double v) { fwrite(&v, sizeof(double), 1, fo); };
  double row[vknest::kMaxP];
  for (size_t i = 0; i < RL; ++i) {
    for (int j = 0; j < d; ++j) lx[j * RL + i] = row[j] = x0[i * d + j];
    const double l = lnl_any(fn, d, row);
    llnl[i] = vkchain::stored(l);
    lchi[i] = -2.0 * l;
  }
  for (int t = 0; t < T; ++t) {
    for (int r = 0; r < R; ++r) {
      const size_t first = (size_t)r * L;
      for (int j = 0; j < d; ++j) range[(size_t)r * d + j] = vknest::range_of(L, [&](int i) { return lx[j * RL + first + i]; });
      for (int i = 0; i < L; ++i) {
        rank[i] = vknest::rank_of(L, i, [&](int m) { return llnl[first + m]; });
        if (rank[i] < K) slot[(size_t)r * K + rank[i]] = i;
      }
      lstar[r] = llnl[first + slot[(size_t)r * K + K - 1]];
      for (int k = 0; k < K; ++k) put((double)slot[(size_t)r * K + k]);
    }
    for (int r = 0; r < R; ++r) put(lstar[r]);
    for (size_t i = 0; i < (size_t)R * d; ++i) put(range[i]);
    for (int r = 0; r < R; ++r) {
      const size_t first = (size_t)r * L;
      for (int i = 0; i < L; ++i) rank[i] = vknest::rank_of(L, i, [&](int m) { return llnl[first + m]; });
      for (int k = 0; k < K; ++k) {
        const size_t c = (size_t)r * K + k;
        const int q = vknest::pick_of(pick[(size_t)t * RK + c], L, K);
        const int from = vknest::survivor_of(L, K, q, [&](int i) { return rank[i]; });
        vknest::Walker w = walker(c);
        vknest::start(d, w, [&](int j) { return lx[j * RL + first + from]; }, llnl[first + from], lchi[first + from]);
        put((double)from);
      }
    }
    for (int s = 0; s < S; ++s) {
      std::vector<double> acc(RK);
      for (int r = 0; r < R; ++r)
        for (int k = 0; k < K; ++k) {
          const size_t c = (size_t)r * K + k;
          vknest::Walker w = walker(c);
          const double* inc = dz + (((size_t)t * S + s) * RK + c) * d;
          auto rg = [&](int j) { return range[(size_t)r * d + j]; };
          const bool in_box = vknest::proposal_inside(box, w, scale, rg, inc);      // the row the launch evaluates
          for (int j = 0; j < d; ++j) row[j] = in_box ? vknest::proposed(w.y[j * w.stride], scale, rg(j), inc[j]) : w.y[j * w.stride];
          const double l = lnl_any(fn, d, row);
          acc[c] = vknest::transition(box, w, scale, rg, inc, lstar[r], l, -2.0 * l) ? 1.0 : 0.0;
        }
      for (size_t c = 0; c < RK; ++c) put(acc[c]);
      for (size_t c = 0; c < RK; ++c)
        for (int j = 0; j < d; ++j) put(wx[j * RK + c]);
      for (size_t c = 0; c < RK; ++c) put(wlnl[c]);
      for (size_t c = 0; c < RK; ++c) put(wchi[c]);
    }
    for (size_t c = 0; c < RK; ++c) {
      const size_t at = (c / K) * L + slot[c];
      vknest::Walker w = walker(c);
      vknest::commit(d, w, lx.data() + at, RL, llnl.data() + at, lchi.data() + at);
    }
    for (size_t i = 0; i < RL; ++i)
      for (int j = 0; j < d; ++j) put(lx[j * RL + i]);
    for (size_t i = 0; i < RL; ++i) put(llnl[i]);
    for (size_t i = 0; i < RL; ++i) put(lchi[i]);
  }
  for (auto* n : {&n_accept, &n_steps, &n_stuck})
    for (int r = 0; r < R; ++r) {
      int64_t sum = 0;
      for (int k = 0; k < K; ++k) sum += (*n)[(size_t)r * K + k];
      put((double)sum);
    }
  fclose(fo);
  return 0;
}
"""


def block_for(d):
    return {f"p{j}": {"prior": {"min": -1.0, "max": 1.0}} for j in range(d)}


def evaluate_of(fn, d):
    f = FUNCTIONS[fn]
    names = [f"p{j}" for j in range(d)]

    def evaluate(batch):
        n = len(batch[names[0]])
        lnl = np.array([f([float(batch[k][i]) for k in names]) for i in range(n)])
        return lnl, -2.0 * lnl
    return evaluate


def host_run(fn, d, n_iter, **kw):
    from victor_amd.nested import run_definition
    return run_definition(block_for(d), evaluate_of(fn, d), n_iter=n_iter, **kw)


def randoms(ns, n_iter):
    """The numbers a run consumed: drawn again by the documented protocol."""
    from victor_amd.nested import BLOCK
    R, L, K, S, d = ns.R, ns.n_live, ns.batch, ns.steps, len(ns.names)
    u = np.random.default_rng([ns.seed, 0]).random((L, d))
    x0 = np.broadcast_to(np.minimum(np.maximum(-1.0 + u * 2.0, -1.0), 1.0), (R, L, d))
    g1, g2 = np.random.default_rng([ns.seed, 1]), np.random.default_rng([ns.seed, 2])
    pick, dz = [], []
    for _ in range((n_iter + BLOCK - 1) // BLOCK):
        pick.append(g1.random((BLOCK, R, K)))
        dz.append(g2.standard_normal((BLOCK, S, R, K, d)))
    return np.ascontiguousarray(x0), np.concatenate(pick)[:n_iter], np.concatenate(dz)[:n_iter]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("nested_driver")
    src, exe = tmp / "driver.cpp", tmp / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(fn, x0, pick, dz, scale):
        T, S, R, K, d = dz.shape
        L = x0.shape[1]
        fin, fout = tmp / "in.bin", tmp / "out.bin"
        np.concatenate([x0.ravel(), pick.ravel(), dz.ravel()]).astype(np.float64).tofile(str(fin))
        args = [str(exe), fn, str(d), str(R), str(L), str(K), str(S), str(T), repr(float(scale)), str(fin), str(fout)]
        args += ["-1.0"] * d + ["1.0"] * d
        subprocess.run(args, check=True)
        out = np.fromfile(str(fout), dtype=np.float64)
        at = 0

        def take(*shape):
            nonlocal at
            n = int(np.prod(shape))
            a = out[at:at + n].reshape(shape)
            at += n
            return a
        its = []
        for _ in range(T):
            it = {"dead": take(R, K).astype(np.int64), "lstar": take(R), "range": take(R, d), "from": take(R, K).astype(np.int64), "steps": []}
            for _ in range(S):
                it["steps"].append((take(R, K) == 1.0, take(R, K, d), take(R, K), take(R, K)))
            it.update(x=take(R, L, d), lnl=take(R, L), chi2=take(R, L))
            its.append(it)
        counts = take(3, R).astype(np.int64)
        assert at == len(out)
        return its, counts
    return run


# ------------------------------------------------------------------ the header against the definition, byte for byte ---------
CASES = {  # fn, d, L, K, S, T, scale
    "gauss": ("gauss", 3, 16, 4, 4, 12, 0.5),              # the mean next to a face: proposals leave the box
    "wide steps": ("gauss", 3, 8, 2, 3, 10, 3.0),          # most proposals outside the box
    "ties": ("tie", 3, 16, 4, 3, 10, 0.2),                 # plateaus of equal lnL: order by index, stuck walkers, duplicates
    "-inf and NaN": ("halfnan", 3, 16, 4, 4, 10, 0.5),
    "no finite point": ("none", 3, 8, 2, 2, 4, 0.5),
    "K = 1": ("gauss", 3, 6, 1, 3, 12, 0.5),
    "K = L / 2": ("gauss", 3, 8, 4, 3, 8, 0.5),
    "d = 1": ("quad", 1, 8, 2, 3, 10, 0.5),
    "d = 10": ("quad", 10, 24, 4, 4, 9, 0.2),
}


@pytest.mark.parametrize("case", list(CASES))
def test_header_against_numpy_bit_for_bit(driver, case):
    fn, d, L, K, S, T, scale = CASES[case]
    ns = host_run(fn, d, 0, n_live=L, batch=K, steps=S, scale=scale, seed=3)
    ns._trace = []
    ns.extend(T)
    x0, pick, dz = randoms(ns, T)
    its, counts = driver(fn, x0, pick, dz, scale)
    assert len(ns._trace) == T == len(its)
    ties = 0
    for t, (want, got) in enumerate(zip(ns._trace, its)):
        for key in ("dead", "from"):
            assert np.array_equal(got[key], want[key]), (case, t, key)                 # the order, the picks
        for key in ("lstar", "range", "x", "lnl", "chi2"):
            assert same_bytes(got[key], want[key]), (case, t, key)
        for s in range(S):
            for i, key in enumerate(("accept", "y", "lnl", "chi2")):
                a, b = got["steps"][s][i], want["steps"][s][i]
                assert np.array_equal(a, b) if i == 0 else same_bytes(a, b), (case, t, s, key)
        assert same_bytes(ns.dead_lnl[t], np.take_along_axis(its[t - 1]["lnl"] if t else _start_lnl(fn, x0), got["dead"], axis=1)), (case, t)
        with np.errstate(invalid="ignore"):
            ties += int((np.diff(np.sort(want["lnl"], axis=1), axis=1) == 0).sum())
    assert np.array_equal(counts, [ns.n_accept, ns.n_steps, ns.n_stuck]), case
    assert np.all(ns.n_steps == T * K * S) and np.all((ns.x >= -1.0) & (ns.x <= 1.0))
    # what each case is there for was reached (conditions on the inputs, not on the code under test)
    outside = sum(int((~st[4]).sum()) for it in ns._trace for st in it["steps"])
    if case in ("gauss", "wide steps"):
        assert outside > (0.5 if case == "wide steps" else 0.0) * T * S * K, outside
    if case == "ties":
        assert ties > 0 and ns.n_stuck[0] > 0
    if case == "-inf and NaN":
        assert np.isneginf(ns.dead_lnl).any() and np.isfinite(ns.lnl).any()
    if case == "no finite point":
        assert ns.status_names == ["NO_FINITE"] and np.isneginf(ns.ln_evidence[0]) and ns.n_accept[0] == 0 and ns.n_stuck[0] == T * K
        assert ns.information[0] == 0.0 and ns.ln_evidence_error[0] == 0.0 and not np.isnan(ns.weights).any()
    else:
        assert ns.n_accept[0] > 0 and np.isfinite(ns.ln_evidence[0])


def _start_lnl(fn, x0):
    f = FUNCTIONS[fn]
    lnl = np.array([[f([float(v) for v in p]) for p in prob] for prob in x0])
    return np.where(np.isnan(lnl), -INF, lnl)


def test_the_order_is_total_and_ties_go_to_the_smaller_index():
    from victor_amd.nested import run_definition
    ns = run_definition(block_for(2), lambda b: np.zeros(len(b["p0"])), n_live=8, batch=2, steps=1, n_iter=0)
    ns._trace = []
    ns.extend(3)
    # every lnL equal: the dead points are the two smallest indices, no step ever beats L*, every walker leaves a duplicate
    for it in ns._trace:
        assert it["dead"].tolist() == [[0, 1]] and not any(a.any() for a, *_ in it["steps"])
    assert ns.n_stuck.tolist() == [6] and ns.n_accept.tolist() == [0]
    assert len({tuple(p) for p in ns.x[0]}) < 8


# ------------------------------------------------------------------ cuts ----------------------------------------------------
ATTRS = ("dead_lnl", "dead_chi2", "dead_x", "x", "lnl", "chi2", "n_accept", "n_steps", "n_stuck", "ln_evidence", "information",
         "ln_evidence_error", "weights", "samples", "mean", "cov", "status")


def test_a_run_does_not_depend_on_how_it_is_cut():
    from victor_amd.nested import run_definition
    kw = dict(n_live=16, batch=4, steps=3, seed=5)
    whole = host_run("gauss", 3, 9, **kw)
    cut = host_run("gauss", 3, 4, **kw).extend(5)
    ones = host_run("gauss", 3, 0, **kw)
    for _ in range(9):
        ones.extend(1)
    short = run_definition(block_for(3), evaluate_of("gauss", 3), n_iter=0, **kw)
    short._cut = 3                                           # another block length: pieces of 3, 3, 2 | 1
    short.extend(9)
    assert whole.n_iter == 9 and whole.dead_lnl.shape == (9, 1, 4) and whole.samples.shape == (1, 36 + 16, 3)
    for other, what in ((cut, "4 + 5"), (ones, "9 x 1"), (short, "pieces of 3")):
        for a in ATTRS:
            assert same_bytes(getattr(whole, a), getattr(other, a)), (what, a)
    # the stop is looked at at multiples of 8 iterations only, so it does not depend on the cut either
    a = host_run("gauss", 3, None, tol=0.5, **kw)
    b = run_definition(block_for(3), evaluate_of("gauss", 3), n_iter=0, tol=0.5, **kw)
    b._cut = 5
    b.run(128 * 4)
    assert a.n_iter == b.n_iter and a.n_iter % 8 == 0 and a.status_names == ["OK"]
    for name in ATTRS:
        assert same_bytes(getattr(a, name), getattr(b, name)), name
    assert host_run("gauss", 3, None, max_iter=8, tol=1e-9, **kw).status_names == ["MAX_ITER"]


# ------------------------------------------------------------------ the read-out -------------------------------------------
def test_read_out_against_a_float128_restatement():
    ns = host_run("gauss", 3, 40, n_live=16, batch=4, steps=3, seed=1)
    ld = np.longdouble
    L, K = 16, 4
    ln_x, terms, lnls = ld(0), [], []
    for t in range(40):
        for k in range(K):
            new = ln_x - 1 / ld(L - k)
            terms.append(np.log(np.exp(ln_x) - np.exp(new)) + ld(ns.dead_lnl[t, 0, k]))
            lnls.append(ld(ns.dead_lnl[t, 0, k]))
            ln_x = new
    for v in ns.lnl[0]:
        terms.append(ln_x - np.log(ld(L)) + ld(v))
        lnls.append(ld(v))
    terms, lnls = np.array(terms, dtype=ld), np.array(lnls, dtype=ld)
    ln_z = np.log(np.exp(terms - terms.max()).sum()) + terms.max()
    p = np.exp(terms - ln_z)
    info = (p * lnls).sum() - ln_z
    assert abs(ns.ln_evidence[0] - float(ln_z)) <= 1e-13 * abs(float(ln_z))
    assert abs(ns.information[0] - float(info)) <= 1e-11 * abs(float(info))
    assert abs(ns.ln_evidence_error[0] - math.sqrt(float(info) / L)) <= 1e-11
    assert np.allclose(ns.weights[0], p.astype(float), rtol=1e-10, atol=0) and abs(ns.weights[0].sum() - 1.0) < 1e-14
    mean = (p[:, None] * ns.samples[0].astype(ld)).sum(axis=0)
    dev = ns.samples[0].astype(ld) - mean
    cov = (p[:, None, None] * dev[:, :, None] * dev[:, None, :]).sum(axis=0)
    assert np.allclose(ns.mean[0], mean.astype(float), rtol=1e-12) and np.allclose(ns.cov[0], cov.astype(float), rtol=1e-10)
    assert same_bytes(ns.sigma[0], np.sqrt(np.diag(ns.cov[0])))
    eq = ns.equal_weight_samples(500, seed=2)
    assert eq.shape == (1, 500, 3) and {tuple(r) for r in eq[0]} <= {tuple(r) for r in ns.samples[0]}
    assert same_bytes(eq, ns.equal_weight_samples(500, seed=2))


def test_resampled_evidences_scatter_about_the_evidence():
    ns = host_run("gauss", 3, None, n_live=64, batch=8, steps=4, seed=2)
    assert ns.status_names == ["OK"]
    z = ns.ln_evidence_samples(200, seed=1)
    assert z.shape == (200, 1) and np.all(np.isfinite(z))
    scatter = z[:, 0].std(ddof=1)
    print("ln_evidence", ns.ln_evidence[0], "resampled mean", z.mean(), "scatter", scatter, "error", ns.ln_evidence_error[0])
    assert abs(z.mean() - ns.ln_evidence[0]) < scatter                     # the mean lies within its own scatter of ln_evidence
    assert 0.5 * ns.ln_evidence_error[0] < scatter < 2.0 * ns.ln_evidence_error[0]      # ... which is what sqrt(H / L) estimates


# ------------------------------------------------------------------ the evidence -------------------------------------------
SEEDS = range(8)


def _within_caps(runs, truth, what):
    diff = np.array([r.ln_evidence[0] - truth for r in runs])
    err = np.array([r.ln_evidence_error[0] for r in runs])
    cap = 4.0 * math.sqrt(float(np.mean(err * err))) / math.sqrt(len(runs))
    print(what, "truth", truth, "differences", np.round(diff, 3), "errors", np.round(err, 3), "pulls", np.round(diff / err, 2),
          "seed mean", diff.mean(), "cap", cap, "iterations", [r.n_iter for r in runs])
    assert all(r.status_names == ["OK"] for r in runs), what
    assert np.all(np.abs(diff) <= 4.0 * err), (what, diff / err)
    assert abs(diff.mean()) <= cap, (what, diff.mean(), cap)


def test_evidence_of_the_gaussian_of_the_tempering_test():
    from victor_amd.nested import run_definition

    def evaluate(batch):
        u, v = batch["a"] - 0.3, batch["b"] - 0.3
        return -0.5 * ((u * u + v * v) / 0.01)
    block = {n: {"prior": {"min": 0.0, "max": 1.0}} for n in ("a", "b")}
    runs = [run_definition(block, evaluate, seed=s) for s in SEEDS]
    assert runs[0].n_live == 256 and runs[0].batch == 32 and runs[0].steps == 16 and runs[0].scale == 0.5 / math.sqrt(2.0)
    _within_caps(runs, EXACT_LN_Z, "2-D Gaussian")


def test_evidence_of_a_gaussian_with_unequal_widths():
    from victor_amd.nested import run_definition
    sig, mu = np.array([0.02, 0.05, 0.1, 0.2]), np.array([0.5, 0.4, 0.6, 0.5])

    def evaluate(batch):
        x = np.stack([batch[f"p{j}"] for j in range(4)], axis=1)
        return -0.5 * (((x - mu) / sig) ** 2).sum(axis=1)
    truth = sum(math.log(s * math.sqrt(2.0 * math.pi) * 0.5 * (math.erf((1.0 - m) / (s * math.sqrt(2.0))) + math.erf(m / (s * math.sqrt(2.0)))))
                for s, m in zip(sig, mu))
    block = {f"p{j}": {"prior": {"min": 0.0, "max": 1.0}} for j in range(4)}
    _within_caps([run_definition(block, evaluate, seed=s) for s in SEEDS], truth, "4-D Gaussian")


# ------------------------------------------------------------------ the refusals -------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the refusal")


def test_refusals_come_before_any_device_call(monkeypatch):
    import victor_amd
    from tests import cases
    from victor_amd import InputError
    monkeypatch.setattr(victor_amd.CCFFit, "_get_engine", lambda self, *a, **k: _NoLibrary())
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    params = cases.cobaya_info()["params"]
    for kw, text in ((dict(prior=object()), "prior= is not accepted"), (dict(beta_interpolation="likelihood"), "beta_interpolation"),
                     (dict(fixed={"epsilon": np.array([1.0, 1.01])}), "must be scalars"), (dict(n_live=256, batch=48), "must divide"),
                     (dict(n_live=64, batch=64), "at most n_live / 2"), (dict(n_live=8192, batch=32), "n_live <= 4096"),
                     (dict(steps=0), "steps must be >= 1"), (dict(scale=0.0), "scale"), (dict(tol=0.0), "tol"),
                     (dict(evaluate=lambda b: 0.0), "definition route only")):
        with pytest.raises(InputError, match=text):
            fit.nested_sampling(params, **kw)
    with pytest.raises(InputError, match="no column of its own"):
        fit.nested_sampling(dict(params, Omega_m={"prior": {"min": 0.2, "max": 0.4}}))
    with pytest.raises(InputError, match="need a JointFit"):
        fit.nested_sampling({**params, "sigma_v@1": {"prior": {"min": 200.0, "max": 500.0}}})
    from victor_amd.nested import run_definition
    with pytest.raises(InputError, match="at most 10"):
        run_definition(block_for(11), evaluate_of("quad", 11), n_iter=0)
    with pytest.raises(InputError, match="every parameter is fixed"):
        run_definition(block_for(1), evaluate_of("quad", 1), fixed={"p0": 0.0})
    for cls in (victor_amd.CCFFit, victor_amd.Realisations, victor_amd.JointFit, victor_amd.JointRealisations):
        assert callable(getattr(cls, "nested_sampling"))


# ------------------------------------------------------------------ the ABI surface ----------------------------------------
NESTED = ("vk_nested_create", "vk_nested_create_joint", "vk_nested_create_joint_blocks", "vk_nested_start", "vk_nested_begin",
          "vk_nested_finish", "vk_nested_state", "vk_nested_last_error", "vk_nested_destroy")


def test_the_abi_declares_exports_and_binds_the_nested_symbols():
    from victor_amd import _native
    from victor_amd.build import build_native
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    declared = set(re.findall(r"\b(vk_nested_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NESTED) and declared <= set(_native.SYMBOLS)
    assert int(re.search(r"#define VK_ABI_VERSION (\d+)", header).group(1)) == _native.VK_ABI_VERSION == 22
    build_native()
    lib = _native.load()
    for name in NESTED:
        assert hasattr(lib, name), name
    assert lib.vk_abi_version() == 22
    from victor_amd import nested
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_nested_step.h")).read()
    assert int(re.search(r"kBlock = (\d+)", src).group(1)) == nested.BLOCK
    assert int(re.search(r"kMaxLive = (\d+)", src).group(1)) == nested.MAX_LIVE
    assert "#include <hip" not in src                       # free of HIP: the driver above is this header under g++
