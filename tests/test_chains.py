"""Metropolis chains (victor_amd/chains.py, vk_chain_begin) without a GPU: the one-chain transition of
victor_amd/csrc/vk_chain_step.h compiled on its own under g++ and driven on analytic functions, checked step by step and bit for
bit against the NumPy loop that defines the chains; its moment sums against exact sums at derived bounds; the host's pooling of
those sums; the definition route against EnsembleMetropolis; the refusals of sample_chains, raised before any device call; and the
bookkeeping of the result.

Bounds (u = 2^-53; they are derived here, not tuned, and the GPU tests import them):

* second-moment sums: S_jk accumulates n terms fl(fl(a) fl(b)), a = x_j - p_j, b = x_k - p_k: three roundings per term (two
  subtractions, one product; a fused multiply-add only removes one) and one per addition, each addition's error at most u times the
  sum of magnitudes so far.  |dS_jk| <= (n + 3) u sum |a b| <= (n + 3) u sqrt(S_jj S_kk) (Cauchy-Schwarz), which
  n 2^-52 sqrt(S_jj S_kk) covers for n >= 3 with the rest of its factor two to spare.  First-moment sums alike: n 2^-52 sum |a|.
* pooled mean and covariance from sums whose errors are |dS2_jk| <= e sqrt(S2_jj S2_kk), |dS1_j| <= e sum |a| <= e sqrt(n_w S2_jj)
  per chain (e = u for exact sums rounded once; e = n 2^-52 for the sums above), formed as pooled_moments forms them (extended
  precision: its own roundings are below u).  With delta_w = p_w - mean and amp = max_wj delta_wj^2 / cov_jj, g = 1 + amp:
  sum_w S2_w,jj = sum (x - p_w)^2 <= 2 [sum (x - mean)^2 + sum_w n_w delta_wj^2] <= 2 n g cov_jj, so
  (n - 1) |dcov_jk| <= e [sqrt(sum S2_jj sum S2_kk) + 2 sqrt(sum S2_jj n amp cov_kk)] <= e n (2 g + 2 sqrt(2) g) sqrt(cov_jj cov_kk)
  (the error of the mean enters at second order: the derivative of the centred sum with respect to the mean vanishes), i.e.
  |dcov_jk| <= 5 g e sqrt(cov_jj cov_kk) n / (n - 1), plus the result's own rounding u |cov_jk|: asserted at
  8 (e + u) g sqrt(cov_jj cov_kk).  The amplification g is the digits a covariance from sums about a pivot loses when the pivot
  lies far from the mean.  The mean: |dmean_j| <= e sum_w sum |a| / n + u (|mean_j| + max_w |p_wj|)
  <= e sqrt(2 g cov_jj) + u (...): asserted at 2 [(e + u) sqrt(2 g cov_jj) + u (|mean_j| + max_w |p_wj|)].
"""

import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import cases
from tests.test_realisations import stack_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
U = 2.0 ** -53

# The analytic functions, as lnL(x), d = 3; the same scalar arithmetic in the same order in C++ (DRIVER) and in Python (LNL).


def _gauss(x):
    # correlated Gaussian whose mean lies next to the face x_0 = 1 of the box [-1, 1]^3: proposals leave the box often
    u, v, w = x[0] - 0.93, x[1] + 0.2, x[2] - 0.1
    q = (9.0 * (u * u) + (2.0 * 3.5) * (u * v)) + 4.0 * (v * v)
    q = q + 25.0 * (w * w)
    return -0.5 * q


def _halfnan(x):
    # -inf on half the box, NaN on a strip, a quadratic elsewhere
    if x[0] < 0.0:
        return -INF
    if x[1] > 0.3 and x[1] < 0.4:
        return math.nan
    return -(2.0 * ((x[0] - 0.3) * (x[0] - 0.3)) + 3.0 * ((x[1] - 0.2) * (x[1] - 0.2)) + (x[2] * x[2]))


LNL = {"gauss": _gauss, "halfnan": _halfnan, "none": lambda x: -INF}

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_chain_step.h"

static double lnl_of(const char* fn, const double* x) {
  if (!strcmp(fn, "gauss")) {
    const double u = x[0] - 0.93, v = x[1] + 0.2, w = x[2] - 0.1;
    double q = (9.0 * (u * u) + (2.0 * 3.5) * (u * v)) + 4.0 * (v * v);
    q = q + 25.0 * (w * w);
    return -0.5 * q;
  }
  if (!strcmp(fn, "halfnan")) {
    if (x[0] < 0.0) return -HUGE_VAL;
    if (x[1] > 0.3 && x[1] < 0.4) return std::nan("");
    return -(2.0 * ((x[0] - 0.3) * (x[0] - 0.3)) + 3.0 * ((x[1] - 0.2) * (x[1] - 0.2)) + (x[2] * x[2]));
  }
  return -HUGE_VAL;
}

// usage: driver fn d C n burn thin in out  then d values each of lo, hi
// in:  doubles x0[C][d], dz[n][C][d], logu[n][C]
// out: doubles, per step: accept[C], x[C][d], lnl[C], chi2[C]; then n_accept[C], n_steps[C], n_kept[C], pivot[C][d], sum1[C][d],
//      sum2[C][d(d+1)/2]
// The state is held structure-of-arrays with stride C, as the device holds it.
int main(int argc, char** argv) {
  const char* fn = argv[1];
  vkchain::Box box{};
  box.d = atoi(argv[2]);
  const int d = box.d, C = atoi(argv[3]), n = atoi(argv[4]);
  const long long burn = atoll(argv[5]), thin = atoll(argv[6]);
  int a = 9;
  for (int j = 0; j < d; ++j) box.lo[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < d; ++j) box.hi[j] = strtod(argv[a++], nullptr);
  std::vector<double> in((size_t)C * d + (size_t)n * C * (d + 1));
  FILE* fi = fopen(argv[7], "rb");
  if (!fi || fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const double *x0 = in.data(), *dz = x0 + (size_t)C * d, *logu = dz + (size_t)n * C * d;
  const int T = vkchain::n_tri(d);
  std::vector<double> x((size_t)d * C), lnl(C), chi2(C), pivot((size_t)d * C), sum1((size_t)d * C), sum2((size_t)T * C);
  std::vector<int64_t> n_accept(C), n_steps(C), n_kept(C);
  auto view = [&](int c) {
    vkchain::View s{};
    s.stride = (size_t)C;
    s.x = x.data() + c; s.lnl = lnl.data() + c; s.chi2 = chi2.data() + c; s.pivot = pivot.data() + c;
    s.sum1 = sum1.data() + c; s.sum2 = sum2.data() + c;
    s.n_accept = n_accept.data() + c; s.n_steps = n_steps.data() + c; s.n_kept = n_kept.data() + c;
    return s;
  };
  auto row_value = [&](const vkchain::View& s, const double* inc, double* l, double* c2) {
    double row[vkchain::kMaxP];                 // what the launch evaluates: the proposal, or outside the box the current position
    const bool move = inc && vkchain::proposal_inside(box, s, inc);
    for (int j = 0; j < d; ++j) row[j] = move ? s.x[j * s.stride] + inc[j] : s.x[j * s.stride];
    *l = lnl_of(fn, row);
    *c2 = -2.0 * *l;
  };
  FILE* fo = fopen(argv[8], "wb");
  if (!fo) return 2;
  auto put = [&](double v) { fwrite(&v, sizeof(double), 1, fo); };
  for (int c = 0; c < C; ++c) {
    vkchain::View s = view(c);
    vkchain::start(box, s, x0 + (size_t)c * d);
    double l, c2;
    row_value(s, nullptr, &l, &c2);
    vkchain::adopt(s, l, c2);
  }
  std::vector<double> acc(C);
  for (int t = 0; t < n; ++t) {
    for (int c = 0; c < C; ++c) {
      vkchain::View s = view(c);
      const double* inc = dz + ((size_t)t * C + c) * d;
      double l, c2;
      row_value(s, inc, &l, &c2);
      acc[c] = vkchain::transition(box, s, inc, logu[(size_t)t * C + c], l, c2, vkchain::is_kept(t, burn, thin)) ? 1.0 : 0.0;
    }
    for (int c = 0; c < C; ++c) put(acc[c]);
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < d; ++j) put(x[(size_t)j * C + c]);
    for (int c = 0; c < C; ++c) put(lnl[c]);
    for (int c = 0; c < C; ++c) put(chi2[c]);
  }
  for (int c = 0; c < C; ++c) put((double)n_accept[c]);
  for (int c = 0; c < C; ++c) put((double)n_steps[c]);
  for (int c = 0; c < C; ++c) put((double)n_kept[c]);
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < d; ++j) put(pivot[(size_t)j * C + c]);
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < d; ++j) put(sum1[(size_t)j * C + c]);
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < T; ++i) put(sum2[(size_t)i * C + c]);
  fclose(fo);
  return 0;
}
"""

NAMES = ["a", "b", "c"]
LO, HI = np.array([-1.0, -1.0, -1.0]), np.array([1.0, 1.0, 1.0])
WIDTH = np.array([0.25, 0.3, 0.15])
REF = {"gauss": (0.8, -0.1, 0.1), "halfnan": (0.4, 0.0, 0.0), "none": (0.0, 0.0, 0.0)}


def block_for(fn):
    return {n: {"prior": {"min": float(LO[j]), "max": float(HI[j])}, "ref": {"loc": REF[fn][j], "scale": 0.1},
                "proposal": float(WIDTH[j])} for j, n in enumerate(NAMES)}


def evaluate_of(fn):
    f = LNL[fn]

    def evaluate(batch):
        n = len(batch[NAMES[0]])
        lnl = np.array([f([float(batch[k][i]) for k in NAMES]) for i in range(n)])
        return lnl, -2.0 * lnl
    return evaluate


def randoms(ch, seed, n_chains, n_steps):
    """The numbers sample_chains consumed for ``ch`` (start from the reference distribution): drawn again by the same protocol."""
    from victor_amd.chains import BLOCK, _draw_start
    specs = ch._specs
    rng = np.random.default_rng(seed)
    loc, scale = np.array([s.ref_loc for s in specs]), np.array([s.ref_scale for s in specs])
    x0 = np.array([_draw_start(rng, loc, scale, LO, HI, "ref") for _ in range(n_chains)])
    dz, logu = [], []
    for _ in range((n_steps + BLOCK - 1) // BLOCK):
        dz.append(WIDTH * rng.standard_normal((BLOCK, n_chains, len(specs))))
        logu.append(np.log(rng.random((BLOCK, n_chains))))
    return x0, np.concatenate(dz)[:n_steps], np.concatenate(logu)[:n_steps]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("chain_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(fn, x0, dz, logu, burn=0, thin=1):
        n, C, dd = dz.shape
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([x0.ravel(), dz.ravel(), logu.ravel()]).astype(np.float64).tofile(str(fin))
        args = [str(exe), fn, str(dd), str(C), str(n), str(burn), str(thin), str(fin), str(fout)]
        args += [repr(float(v)) for v in LO] + [repr(float(v)) for v in HI]
        subprocess.run(args, check=True)
        out = np.fromfile(str(fout), dtype=np.float64)
        per = C * (dd + 3)
        steps = out[: n * per].reshape(n, per)
        tail = out[n * per:]
        T = dd * (dd + 1) // 2
        tri = tail[3 * C + 2 * C * dd:].reshape(C, T)
        sum2 = np.empty((C, dd, dd))
        i = 0
        for j in range(dd):
            for k in range(j, dd):
                sum2[:, j, k] = sum2[:, k, j] = tri[:, i]
                i += 1
        return {"accept": steps[:, :C] == 1.0, "x": steps[:, C:C + C * dd].reshape(n, C, dd), "lnl": steps[:, C + C * dd:2 * C + C * dd],
                "chi2": steps[:, 2 * C + C * dd:], "n_accept": tail[:C].astype(np.int64), "n_steps": tail[C:2 * C].astype(np.int64),
                "n_kept": tail[2 * C:3 * C].astype(np.int64), "pivot": tail[3 * C:3 * C + C * dd].reshape(C, dd),
                "sum1": tail[3 * C + C * dd:3 * C + 2 * C * dd].reshape(C, dd), "sum2": sum2}
    return run


def host_chains(fn, n_steps, walkers=8, seed=3, **kw):
    from victor_amd.chains import sample_chains
    return sample_chains(None, block_for(fn), n_steps, walkers=walkers, seed=seed, device=False, evaluate=evaluate_of(fn), **kw)


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------ the transition, bit for bit ---------------------------
@pytest.mark.parametrize("fn", ["gauss", "halfnan", "none"])
def test_transition_against_numpy_bit_for_bit(driver, fn):
    n, C, seed = 150, 8, 3
    ch = host_chains(fn, n, walkers=C, seed=seed)
    x0, dz, logu = randoms(ch, seed, C, n)
    got = driver(fn, x0, dz, logu)
    assert same_bytes(ch.pivot[0], x0) and same_bytes(got["pivot"], x0)
    assert same_bytes(got["x"], ch.chain[:, 0]), fn                                   # every position
    assert same_bytes(got["lnl"], ch.lnl_chain[:, 0]) and same_bytes(got["chi2"], ch.chi2_chain[:, 0])
    before = np.concatenate([x0[None], ch.chain[:-1, 0]])
    moved = np.any(ch.chain[:, 0] != before, axis=2)                                   # every decision (an accepted dz is never 0)
    assert np.array_equal(got["accept"], moved), fn
    assert np.array_equal(got["n_accept"], ch.n_accept[0]) and np.array_equal(got["n_accept"], moved.sum(axis=0))
    assert np.all(got["n_steps"] == n) and np.all(got["n_kept"] == n) and ch.n_kept == n
    assert np.all((got["x"] >= LO) & (got["x"] <= HI))
    prop = before + dz
    outside = ~((prop >= LO) & (prop <= HI)).all(axis=2)
    assert not np.any(got["accept"] & outside)
    if fn == "gauss":
        assert 0.15 < outside.mean() < 0.85 and 0.05 < moved.mean() < 0.9, (outside.mean(), moved.mean())
    if fn == "halfnan":
        assert not np.any(np.isnan(got["lnl"])) and np.all(got["x"][..., 0] >= 0.0)
        assert np.all((got["x"][..., 1] <= 0.3) | (got["x"][..., 1] >= 0.4))           # never onto the NaN strip
        hit = (prop[..., 0] >= 0) & (prop[..., 1] > 0.3) & (prop[..., 1] < 0.4) & ~outside
        assert hit.any()                                                               # ... which proposals did reach
    if fn == "none":
        assert not moved.any() and np.all(got["lnl"] == -INF) and np.all(got["chi2"] == INF)


@pytest.mark.parametrize("burn,thin", [(0, 1), (10, 3), (37, 7), (149, 1), (200, 2)])
def test_kept_steps_follow_burn_and_thin(driver, burn, thin):
    n, C, seed = 150, 8, 3
    full = host_chains("gauss", n, walkers=C, seed=seed)
    ch = host_chains("gauss", n, walkers=C, seed=seed, burn=burn, thin=thin)
    x0, dz, logu = randoms(ch, seed, C, n)
    got = driver("gauss", x0, dz, logu, burn, thin)
    want = list(range(burn, n, thin))
    assert ch.n_kept == len(want) and np.all(got["n_kept"] == len(want))
    assert same_bytes(ch.chain, full.chain[want]) and same_bytes(ch.lnl_chain, full.lnl_chain[want])
    assert same_bytes(ch.x, full.x) and np.array_equal(ch.n_accept, full.n_accept)
    assert same_bytes(got["x"][-1], ch.x[0]) and np.array_equal(got["n_accept"], ch.n_accept[0])
    # the same steps entered the sums on both sides (to the bounds of test_moment_sums; here: the same count and close values)
    assert np.allclose(got["sum1"], ch.sum1[0], rtol=1e-12, atol=1e-13) and np.allclose(got["sum2"], ch.sum2[0], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("cuts", [(150,), (1, 1, 148), (75, 75), (149, 1)])
def test_a_run_does_not_depend_on_how_it_is_cut(driver, cuts):
    C, seed = 8, 3
    whole = host_chains("gauss", 150, walkers=C, seed=seed, burn=5, thin=2)
    ch = host_chains("gauss", cuts[0], walkers=C, seed=seed, burn=5, thin=2)
    for k in cuts[1:]:
        ch.extend(k)
    for a in ("x", "lnl", "chi2", "chain", "lnl_chain", "chi2_chain", "n_accept", "sum1", "sum2", "mean", "cov", "rhat"):
        assert same_bytes(getattr(ch, a), getattr(whole, a)), (cuts, a)
    assert ch.n_steps == 150 and ch.n_kept == whole.n_kept
    x0, dz, logu = randoms(ch, seed, C, 150)
    got = driver("gauss", x0, dz, logu, 5, 2)
    assert same_bytes(got["x"][5::2], ch.chain[:, 0])


# ------------------------------------------------------------------ moments ---------------------------------------------
def exact_sums(hist, pivot):
    """(S1 (W, d), S2 (W, d, d), A1 (W, d) = sum |x - p|) of hist (n, W, d) about pivot (W, d), exact (rationals), as floats."""
    n, W, d = hist.shape
    s1, s2, a1 = np.empty((W, d)), np.empty((W, d, d)), np.empty((W, d))
    for w in range(W):
        dx = [[Fraction(float(hist[t, w, j])) - Fraction(float(pivot[w, j])) for j in range(d)] for t in range(n)]
        for j in range(d):
            s1[w, j] = float(sum(r[j] for r in dx))
            a1[w, j] = float(sum(abs(r[j]) for r in dx))
            for k in range(d):
                s2[w, j, k] = float(sum(r[j] * r[k] for r in dx))
    return s1, s2, a1


def assert_sums(sum1, sum2, hist, pivot, what=""):
    """Per-chain moment sums accumulated in double, in step order, against the exact sums: the bound of the module docstring."""
    n = hist.shape[0]
    s1, s2, a1 = exact_sums(hist, pivot)
    diag = np.sqrt(np.einsum("wjj->wj", s2))
    b2 = n * 2.0 ** -52 * diag[:, :, None] * diag[:, None, :]
    b1 = n * 2.0 ** -52 * a1
    assert np.all(np.abs(sum2 - s2) <= b2), (what, float(np.max(np.abs(sum2 - s2) / np.where(b2 > 0, b2, 1))))
    assert np.all(np.abs(sum1 - s1) <= b1), (what, float(np.max(np.abs(sum1 - s1) / np.where(b1 > 0, b1, 1))))
    return s1, s2


def assert_pooled(mean, cov, hist, pivot, sum_rel, what=""):
    """Pooled mean (d) / cov (d, d) of one problem against NumPy on its pooled history (n, W, d), in extended precision; sums
    known to ``sum_rel`` (module docstring)."""
    n, W, d = hist.shape
    pooled = hist.reshape(n * W, d).astype(np.longdouble)
    m_ref = pooled.mean(axis=0)
    c_ref = np.atleast_2d(np.cov(pooled, rowvar=False, ddof=1))
    var = np.diag(c_ref).astype(float)
    amp = float(np.max((pivot - m_ref.astype(float)) ** 2 / var))
    g = 1.0 + amp
    e = sum_rel + U
    b_cov = 8 * e * g * np.sqrt(np.outer(var, var))
    b_mean = 2 * (e * np.sqrt(2 * g * var) + U * (np.abs(m_ref.astype(float)) + np.max(np.abs(pivot), axis=0)))
    dc = np.abs((cov.astype(np.longdouble) - c_ref).astype(float))
    dm = np.abs((mean.astype(np.longdouble) - m_ref).astype(float))
    assert np.all(dc <= b_cov), (what, "cov", float(np.max(dc / b_cov)), g)
    assert np.all(dm <= b_mean), (what, "mean", float(np.max(dm / b_mean)), g)
    return g


def test_moment_sums_against_exact_sums(driver):
    n, C, seed = 150, 8, 3
    for burn, thin in ((0, 1), (10, 3)):
        ch = host_chains("gauss", n, walkers=C, seed=seed, burn=burn, thin=thin)
        x0, dz, logu = randoms(ch, seed, C, n)
        got = driver("gauss", x0, dz, logu, burn, thin)
        assert_sums(got["sum1"], got["sum2"], ch.chain[:, 0], got["pivot"], "driver")
        assert_sums(ch.sum1[0], ch.sum2[0], ch.chain[:, 0], ch.pivot[0], "definition route")


def test_pooled_mean_and_covariance_from_exact_sums():
    from victor_amd.chains import pooled_moments
    n, C = 150, 8
    ch = host_chains("gauss", n, walkers=C, seed=3, burn=10)
    hist = ch.chain[:, 0]
    gains = []
    for shift in (0.0, 3.0, 1000.0):                 # pivots at the starts, and far from the mean: the amplification grows
        pivot = ch.pivot[0] + shift
        s1, s2, _ = exact_sums(hist, pivot)
        n_kept = np.full((1, C), len(hist))
        mean, cov = pooled_moments(n_kept, pivot[None], s1[None], s2[None])
        gains.append(assert_pooled(mean[0], cov[0], hist, pivot, U, f"shift {shift}"))
    assert gains[0] < 100 and gains[2] > 1e6
    # and what the object itself reports, from the sums its route accumulated in double
    assert_pooled(ch.mean[0], ch.cov[0], hist, ch.pivot[0], len(hist) * 2.0 ** -52, "Chains.mean / cov")
    assert np.allclose(ch.mean[0], hist.reshape(-1, 3).mean(axis=0), rtol=1e-12)
    assert np.allclose(ch.cov[0], np.cov(hist.reshape(-1, 3), rowvar=False), rtol=1e-10)
    short = host_chains("gauss", 1, walkers=1, seed=3)
    assert np.all(np.isnan(short.cov)) and np.all(np.isfinite(short.mean)) and short.rhat is None


# ------------------------------------------------------------------ the definition route is the existing sampler's chain ---
def test_definition_route_is_the_chain_of_ensemble_metropolis():
    from victor_amd.chains import sample_chains
    from victor_amd.sampler import EnsembleMetropolis, parse_cobaya_params
    block = dict(block_for("gauss"), scale=2.0)

    def f(batch):                                     # elementwise arithmetic only: a row's value does not depend on the batch
        u, v, w = batch["a"] - 0.93, batch["b"] + 0.2, batch["c"] - 0.1
        return -0.5 * batch["scale"] * (9.0 * (u * u) + 7.0 * (u * v) + 4.0 * (v * v) + 25.0 * (w * w))
    specs, fixed = parse_cobaya_params(block)
    for C, seed in ((12, 0), (5, 11)):
        em = EnsembleMetropolis(f, specs, n_walkers=C, seed=seed, fixed=fixed, native=False).initialise()
        start, lnl0 = em.x.copy(), em.lnl.copy()
        chain, lnl = em.run(300)
        ch = sample_chains(None, block, 300, walkers=C, seed=seed, device=False, evaluate=f)
        assert ch.names == em.names and ch.fixed == {"scale": 2.0}
        assert same_bytes(ch.pivot[0], start)
        assert same_bytes(ch.chain[:, 0], chain) and same_bytes(ch.lnl_chain[:, 0], lnl)
        assert same_bytes(ch.chi2_chain, -2.0 * ch.lnl_chain)
        assert int(ch.n_accept.sum()) == em.n_accept and abs(ch.acceptance[0] - em.acceptance) < 1e-15
        assert 0 < em.n_evals < 300 * C + C                                            # proposals did leave the box
        assert np.isfinite(lnl0).all()
        more, more_lnl = em.run(70)
        ch.extend(70)
        assert same_bytes(ch.chain[300:, 0], more) and same_bytes(ch.lnl_chain[300:, 0], more_lnl)


# ------------------------------------------------------------------ refusals (no GPU) ------------------------------------
def _no_device(fit):
    def boom(*a, **k):
        raise AssertionError("sample_chains reached the device before refusing its input")
    fit._get_engine = boom
    return fit


def test_input_errors_are_raised_before_any_device_call():
    import victor_amd
    from victor_amd import InputError
    params = cases.cobaya_info()["params"]
    fit = _no_device(victor_amd.CCFFit(*cases.boss_options("config")))
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    _no_device(rs.fit)
    with pytest.raises(InputError, match="uniform"):
        fit.sample_chains(dict(params, sigma_v={"prior": {"dist": "norm", "loc": 380, "scale": 20}, "proposal": 10}), 10)
    with pytest.raises(InputError, match="no column"):
        fit.sample_chains(dict(params, alpha={"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0}, "proposal": 0.01}), 10)
    with pytest.raises(InputError, match="fixed values must be scalars"):
        rs.sample_chains(params, 10, fixed={"fsigma8": np.linspace(0.3, 0.6, 16)})
    with pytest.raises(InputError, match="beta_interpolation"):
        fit.sample_chains(params, 10, beta_interpolation="likelihood")
    with pytest.raises(InputError, match="beta_interpolation"):
        rs.sample_chains(params, 10, beta_interpolation="likelihood")
    with pytest.raises(InputError, match="alpha"):
        fit.sample_chains(params, 10, fixed={"alpha": np.array([1.0, 1.01])})
    with pytest.raises(InputError, match="start of fsigma8.*outside"):
        fit.sample_chains(params, 10, start={"fsigma8": 1.6})
    with pytest.raises(InputError, match="start of beta.*problem 3.*outside"):
        rs.sample_chains(params, 10, start={"beta": np.where(np.arange(16) == 3, 7.0, 0.4)})
    with pytest.raises(InputError, match="walkers"):
        fit.sample_chains(params, 10, walkers=0)
    with pytest.raises(InputError, match="n_steps"):
        fit.sample_chains(params, -1)
    with pytest.raises(InputError, match="thin"):
        fit.sample_chains(params, 10, thin=0)
    with pytest.raises(InputError, match="burn"):
        fit.sample_chains(params, 10, burn=-1)
    with pytest.raises(InputError, match="65552 chains"):
        rs.sample_chains(params, 10, walkers=4097)
    with pytest.raises(InputError, match="65537 chains"):
        fit.sample_chains(params, 10, walkers=65537)
    with pytest.raises(InputError, match="not sampled"):
        fit.sample_chains(params, 10, proposal={"alpha": 0.1})
    with pytest.raises(InputError, match="proposal width"):
        fit.sample_chains(params, 10, proposal={"beta": 0.0})
    with pytest.raises(InputError, match="one value per problem"):
        rs.sample_chains(params, 10, start={"beta": np.full(5, 0.4)})
    with pytest.raises(InputError, match="device=False"):
        victor_amd.chains.sample_chains(None, params, 10, evaluate=lambda b: b["beta"])
    with pytest.raises(InputError, match="every parameter is fixed"):
        fit.sample_chains(params, 10, fixed={"fsigma8": 0.5, "beta": 0.4, "sigma_v": 380.0, "epsilon": 1.0})


# ------------------------------------------------------------------ the result's bookkeeping -----------------------------
def test_result_bookkeeping():
    from victor_amd.chains import sample_chains
    from victor_amd.sampler import gelman_rubin
    n, W = 130, 6
    ch = host_chains("gauss", n, walkers=W, seed=9, burn=20, thin=5)
    k = len(range(20, n, 5))
    assert ch.names == NAMES and ch.n_steps == n and ch.n_kept == k and (ch.R, ch.W) == (1, W)
    assert ch.x.shape == (1, W, 3) and ch.lnl.shape == ch.chi2.shape == ch.n_accept.shape == (1, W)
    assert ch.chain.shape == (k, 1, W, 3) and ch.lnl_chain.shape == ch.chi2_chain.shape == (k, 1, W)
    assert ch.mean.shape == (1, 3) and ch.cov.shape == (1, 3, 3) and ch.acceptance.shape == (1,) and ch.rhat.shape == (1, 3)
    assert ch.pivot.shape == ch.sum1.shape == (1, W, 3) and ch.sum2.shape == (1, W, 3, 3)
    assert same_bytes(ch.sum2, np.swapaxes(ch.sum2, 2, 3))
    assert same_bytes(ch.rhat[0], gelman_rubin(ch.chain[:, 0]))
    assert ch.acceptance[0] == ch.n_accept[0].sum() / (n * W)
    lean = host_chains("gauss", n, walkers=W, seed=9, burn=20, thin=5, keep_chain=False)
    assert lean.chain is None and lean.lnl_chain is None and lean.chi2_chain is None and lean.rhat is None
    for a in ("x", "lnl", "chi2", "mean", "cov", "n_accept", "sum1", "sum2", "pivot"):
        assert same_bytes(getattr(lean, a), getattr(ch, a)), a
    # a start with a scatter: every chain of the problem around the point; scatter 0: at the point itself
    at = {"a": 0.5, "b": -0.3, "c": 0.2}
    s0 = sample_chains(None, block_for("gauss"), 0, walkers=4, seed=1, device=False, evaluate=evaluate_of("gauss"), start=at, scatter=0)
    assert np.all(s0.x[0] == np.array([0.5, -0.3, 0.2])) and s0.n_steps == 0 and s0.chain.shape == (0, 1, 4, 3)
    s1 = sample_chains(None, block_for("gauss"), 0, walkers=4, seed=1, device=False, evaluate=evaluate_of("gauss"), start=at)
    off = s1.x[0] - np.array([0.5, -0.3, 0.2])
    assert np.all(off != 0) and np.all(np.abs(off) < 6 * WIDTH) and np.all((s1.x >= LO) & (s1.x <= HI))
    # an evaluate that returns lnL alone: chi2 reads -2 lnL
    only = sample_chains(None, block_for("gauss"), 20, walkers=3, seed=1, device=False, evaluate=lambda b: evaluate_of("gauss")(b)[0])
    assert same_bytes(only.chi2, -2.0 * only.lnl)
