"""The tail of an importance sample (rule 7 of victor_amd/importance.py, vk_is_set_tail / vk_is_tail) without a GPU: the selection
of the definition route against ``np.lexsort`` over the whole (G, R) array, for every chunk; the order and the merge positions of
victor_amd/csrc/vk_is_tail.h compiled on their own under g++ and driven the way the kernels drive them (a threshold per chunk,
the slices' candidates in their slots, batches) against the same sort; equal values, the whole sample, failed problems; the
generalised Pareto fit on draws of known shape, its quantile function against scipy's where scipy is installed; the tail index
of a Gaussian target under a Gaussian proposal; the corrected sums against a direct recomputation; the refusals and the C ABI's
surface.

Bounds.  The selection is compared as bytes.  The fit: the Zhang-Stephens estimator's asymptotic standard error is
``(1 + k) / sqrt(n)``; a draw is held to 4 of them.  The corrections: with ONE chunk the raw sums are the plain in-order sums of T
terms of the final weights (the first rescale multiplies zeros), T - 1 additions of 1 u each relative to the sum of the absolute
terms A, a term ``(w y_j) y_k`` or ``w w`` carries up to 2 u of its own, and the corrected sum is rounded to float64 once:
``(T + 4) u`` of A covers them, u = 2^-53."""

import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import tolerances
from tests.test_chains import same_bytes
from tests.test_importance import BLOCK3, EXACT, SUMS, Gaussian, Recorder, failing, host, proposal3, raiser, three

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_is_set_tail", "vk_is_tail")


def sorted_columns(lnpost, K):
    """``(values (R, K), points (R, K), count (R,))`` of the K first entries of every column of ``lnpost`` (G, R) in the total order
    - by ``np.lexsort`` over the whole array -, padded with -inf and -1 behind the finite ones."""
    lnpost = np.where(np.isfinite(lnpost), lnpost, -np.inf)
    G, R = lnpost.shape
    values, points = np.full((R, K), -np.inf), np.full((R, K), -1, dtype=np.int64)
    for r in range(R):
        order = np.lexsort((np.arange(G), -lnpost[:, r]))[:K]
        keep = order[lnpost[order, r] > -np.inf]
        values[r, :len(keep)], points[r, :len(keep)] = lnpost[keep, r], keep
    return values, points, np.count_nonzero(values > -np.inf, axis=1)


def lnpost_of(ip, rec):
    return np.concatenate([c.reshape(len(c), -1) for c in rec.chunks], axis=0) + ip._sample.lno[:, None]


def assert_held(tail, lnpost, what):
    values, points, count = sorted_columns(lnpost, tail.size + 1)
    assert same_bytes(tail.lnpost, values) and same_bytes(tail.index, points) and same_bytes(tail.count, count), what
    assert tail.index.dtype == np.int64 and tail.count.dtype == np.int64 and tail.lnpost.shape == (lnpost.shape[1], tail.size + 1)


# ------------------------------------------------------------------ 1. the selection ---------------------------------------
KW3 = dict(n=300, seed=2, bins=4)


def test_selection_is_the_sort_of_the_whole_sample_for_every_chunk():
    rec = Recorder(three)
    whole = host(rec, BLOCK3, proposal3(), chunk=10 ** 4, tail={"size": 20}, **KW3)
    G = whole.n_inside
    assert whole.n_chunks == 1 and G > 100 and whole.tail.size == 20
    lnpost = lnpost_of(whole, rec)
    assert_held(whole.tail, lnpost, "one chunk")
    assert np.all(whole.tail.count == 21) and np.all(np.diff(whole.tail.lnpost, axis=1) <= 0)
    assert same_bytes(whole.tail.index[:, 0], whole.arg_max) and same_bytes(whole.tail.lnpost[:, 0], whole.ln_max)
    for chunk in (1, 7, 64, G):
        part = host(three, BLOCK3, proposal3(), chunk=chunk, tail={"size": 20}, **KW3)
        for name in ("lnpost", "index", "count", "k", "scale", "status", "n_tail"):
            assert same_bytes(getattr(part.tail, name), getattr(whole.tail, name)), (chunk, name)
    # the keyword changes nothing else, and without it there is no tail
    off = host(three, BLOCK3, proposal3(), chunk=7, **KW3)
    on = host(three, BLOCK3, proposal3(), chunk=7, tail=True, **KW3)
    assert off.tail is None and on.tail.size == min(int(0.2 * G), int(np.ceil(3 * np.sqrt(G))), 4095)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(on.raw, name), getattr(off.raw, name)), name
    for name in ("ln_evidence", "ln_evidence_error", "ess", "max_weight_share", "mean", "cov", "sigma", "status"):
        assert same_bytes(getattr(on, name), getattr(off, name)), name


def test_equal_values_are_held_in_increasing_g():
    from victor_amd import GaussianProposal
    q = proposal3()
    mean, chol = q.ordered("test", ["a", "b", "c"])
    pts = np.repeat(GaussianProposal.draw(mean, chol, None, 60, 7), 3, axis=0)              # every point three times in a row
    lnq = GaussianProposal.ln_density(pts, mean, chol, None)
    rec = Recorder(three)
    ip = host(rec, BLOCK3, sample=pts, ln_proposal=lnq, chunk=7, bins=4, tail={"size": 30})
    assert_held(ip.tail, lnpost_of(ip, rec), "triplicated points")
    t = ip.tail
    assert np.all(t.count == 31)
    for r in range(3):
        same = t.lnpost[r, 1:] == t.lnpost[r, :-1]
        assert same.sum() >= 20 and np.all(t.index[r, 1:][same] == t.index[r, :-1][same] + 1)
    # a cutoff that ties with the entries before it: they are not above it, so they are no part of the tail
    assert np.all(t.n_tail == np.array([np.count_nonzero(t.lnpost[r] > t.lnpost[r, -1]) for r in range(3)])) and np.all(t.n_tail >= 28)


def test_the_whole_sample():
    rec = Recorder(three)
    probe = host(three, BLOCK3, proposal3(), **KW3)
    G = probe.n_inside
    ip = host(rec, BLOCK3, proposal3(), chunk=64, tail={"size": G - 1}, **KW3)
    lnpost = lnpost_of(ip, rec)
    assert_held(ip.tail, lnpost, "size G - 1")
    assert ip.tail.lnpost.shape == (3, G) and np.all(ip.tail.count == G)
    for r in range(3):
        assert sorted(ip.tail.index[r]) == list(range(G))
        assert same_bytes(ip.tail.lnpost[r], lnpost[ip.tail.index[r], r])


@pytest.mark.parametrize("chunk", [7, 200])
def test_failed_and_short_problems(chunk):
    plain = host(failing, BLOCK3, proposal3(), n=200, seed=4, bins=4, chunk=chunk, min_ess=5.0)
    G, nf = plain.n_inside, int(plain.n_finite[1])
    assert 0 < nf < G - 1
    rec = Recorder(failing)
    ip = host(rec, BLOCK3, proposal3(), n=200, seed=4, bins=4, chunk=chunk, min_ess=5.0, tail={"size": nf})
    t = ip.tail
    assert_held(t, lnpost_of(ip, rec), "failing problems")
    assert list(t.count) == [0, nf, nf + 1] and list(t.status[:2]) == [t.NO_FINITE, t.SHORT] and t.status[2] in (t.OK, t.HIGH_K)
    assert np.all(t.index[0] == -1) and np.all(t.lnpost[0] == -np.inf) and t.index[1, nf] == -1 and t.lnpost[1, nf] == -np.inf
    assert np.isnan(t.k[0]) and t.k[1] == np.inf and np.isfinite(t.k[2])
    for name in ("ln_evidence", "ln_evidence_error", "ess", "max_weight_share", "mean", "cov", "sigma"):
        assert same_bytes(getattr(t, name)[:2], getattr(ip, name)[:2]), name                # nothing fitted: the raw figures
        assert not same_bytes(getattr(t, name)[2], getattr(ip, name)[2]), name
    for name in ("total", "sq", "s1", "s2"):
        assert not np.any(np.isnan(t.sums[name])), name
        assert same_bytes(t.sums[name][:2], getattr(ip.raw, name)[:2]), name
    assert same_bytes(ip.status, plain.status)
    # a tail of fewer than five entries is not fitted
    few = host(failing, BLOCK3, proposal3(), n=200, seed=4, bins=4, chunk=chunk, min_ess=5.0, tail={"size": 4}).tail
    assert list(few.count) == [0, 5, 5] and list(few.n_tail[1:]) == [4, 4] and np.all(few.k[1:] == np.inf)
    assert list(few.status) == [few.NO_FINITE, few.HIGH_K, few.HIGH_K]
    for name in ("total", "sq", "s1", "s2"):
        assert same_bytes(few.sums[name], getattr(ip.raw, name)), name


# ------------------------------------------------------------------ 2. vk_is_tail.h under g++ ------------------------------
DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vk_is_tail.h"
// tail K chunk batch pr in out: the values of one problem, point after point, go through a threshold filter per chunk - slice by
// slice, a workgroup of pr problems - and a merge in batches: the steps of vk_kernel_is_tail.h over the rules of the header
// tail geometry n R: the launch shape of a chunk of n rows for R problems as the rules of the header give it - "pr per gy S", the
// gy + 1 block cuts, then "first end step rows" of every slice (tests/test_launch_shapes.py holds its Python twins to this)
static int geometry(int n, int R) {
  const int pr = vkist::problems_per_block(R), per = vkist::slices_per_block(pr), gy = vkist::row_blocks(n, pr), S = gy * per;
  printf("%d %d %d %d\n", pr, per, gy, S);
  for (int y = 0; y <= gy; ++y) printf("%d%c", vkist::block_begin(n, gy, y), y == gy ? '\n' : ' ');
  for (int s = 0; s < S; ++s) {
    const vkist::Slice c = vkist::slice_of(n, pr, gy, s);
    printf("%d %d %d %d\n", c.first, c.end, c.step, vkist::rows_of(c));
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && argv[1][0] == 'g') return geometry(atoi(argv[2]), atoi(argv[3]));
  if (argc != 7) return 2;
  const int K = atoi(argv[1]), chunk = atoi(argv[2]), batch = atoi(argv[3]), pr = atoi(argv[4]);
  FILE* fi = fopen(argv[5], "rb");
  if (!fi) return 3;
  std::vector<double> v;
  double x;
  while (fread(&x, sizeof x, 1, fi) == 1) v.push_back(x);
  fclose(fi);
  const int G = (int)v.size();
  std::vector<double> hv[2] = {std::vector<double>(K), std::vector<double>(K)};
  std::vector<int> hg[2] = {std::vector<int>(K), std::vector<int>(K)};
  int side = 0, h = 0;
  double threshold = vkgrid::neg_inf();
  for (int g0 = 0; g0 < G; g0 += chunk) {
    const int n = std::min(chunk, G - g0);
    // the filter: every slice walks its rows and leaves its candidates in the slots of its first rows
    const int gy = vkist::row_blocks(n, pr), S = gy * vkist::slices_per_block(pr);
    if (S > vkist::kMaxSlices) return 5;
    std::vector<int> slot(n, -1), upto(S), seen(n, 0);
    for (int s = 0; s < S; ++s) {
      const vkist::Slice sc = vkist::slice_of(n, pr, gy, s);
      int at = sc.first, found = 0;
      for (int i = sc.first; i < sc.end; i += sc.step) {
        seen[i] += 1;
        if (vkist::enters(vkgrid::clean(v[g0 + i]), threshold)) {
          if (at < 0 || at >= n || slot[at] != -1) return 6;   // a slot inside the chunk that no other slice wrote
          slot[at] = i, at += sc.step, found += 1;
        }
      }
      if (found > vkist::rows_of(sc)) return 7;
      upto[s] = found + (s ? upto[s - 1] : 0);
    }
    for (int i = 0; i < n; ++i)
      if (seen[i] != 1) return 8;                               // every row belongs to exactly one slice
    // the merge's gather: candidate e lies in the first slice s with upto[s] > e
    const int c = upto[S - 1];
    std::vector<int> cand(c);
    for (int e = 0; e < c; ++e) {
      int lo = 0, hi = S - 1;
      while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (upto[mid] > e) hi = mid;
        else lo = mid + 1;
      }
      const vkist::Slice sc = vkist::slice_of(n, pr, gy, lo);
      cand[e] = slot[sc.first + (e - (lo ? upto[lo - 1] : 0)) * sc.step];
      if (cand[e] < 0) return 9;
    }
    for (int c0 = 0; c0 < c; c0 += batch) {
      const int b = std::min(batch, c - c0);
      std::vector<double> raw_v(b), sv(b);
      std::vector<int> raw_g(b), sg(b);
      for (int k = 0; k < b; ++k) raw_v[k] = vkgrid::clean(v[g0 + cand[c0 + k]]), raw_g[k] = g0 + cand[c0 + k];
      for (int k = 0; k < b; ++k) {
        int rank = 0;
        for (int j = 0; j < b; ++j) rank += vkist::precedes(raw_v[j], raw_g[j], raw_v[k], raw_g[k]) ? 1 : 0;
        sv[rank] = raw_v[k], sg[rank] = raw_g[k];
      }
      const std::vector<double>& fv = hv[side];
      const std::vector<int>& fg = hg[side];
      std::vector<int> hits(K, 0);
      for (int j = 0; j < h; ++j) {
        const int at = j + vkist::preceding(b, fv[j], fg[j], [&](int m, double& vm, int& gm) { vm = sv[m]; gm = sg[m]; });
        if (at < K) hv[side ^ 1][at] = fv[j], hg[side ^ 1][at] = fg[j], hits[at] += 1;
      }
      for (int k = 0; k < b; ++k) {
        const int at = k + vkist::preceding(h, sv[k], sg[k], [&](int m, double& vm, int& gm) { vm = fv[m]; gm = fg[m]; });
        if (at < K) hv[side ^ 1][at] = sv[k], hg[side ^ 1][at] = sg[k], hits[at] += 1;
      }
      h = std::min(K, h + b);
      side ^= 1;
      for (int k = 0; k < K; ++k)
        if (hits[k] != (k < h ? 1 : 0)) return 4;              // every kept position written exactly once
    }
    if (h == K) threshold = hv[side][K - 1];
  }
  FILE* fo = fopen(argv[6], "wb");
  if (!fo) return 3;
  const double count = h;
  fwrite(&count, sizeof count, 1, fo);
  for (int k = 0; k < h; ++k) fwrite(&hv[side][k], sizeof(double), 1, fo);
  for (int k = 0; k < h; ++k) {
    const double g = hg[side][k];
    fwrite(&g, sizeof g, 1, fo);
  }
  fclose(fo);
  return 0;
}
"""


@pytest.fixture(scope="module")
def tail_driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("tail_driver")
    src, exe = d / "tail.cpp", d / "tail"
    src.write_text(DRIVER)
    done = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "victor_amd", "csrc"),
                           str(src), "-o", str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr

    def run(values, K, chunk, batch, pr):
        fin, fout = d / "in.bin", d / "out.bin"
        np.asarray(values, dtype=np.float64).tofile(str(fin))
        done = subprocess.run([str(exe), str(K), str(chunk), str(batch), str(pr), str(fin), str(fout)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        out = np.fromfile(str(fout), dtype=np.float64)
        h = int(out[0])
        return h, out[1:1 + h], out[1 + h:1 + 2 * h].astype(np.int64)

    def geometry(n, R):
        """``((pr, per, gy, S), the block cuts, [(first, end, step, rows) of every slice])`` of a chunk of n rows, R problems."""
        done = subprocess.run([str(exe), "geometry", str(n), str(R)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        lines = [tuple(int(v) for v in line.split()) for line in done.stdout.splitlines()]
        return lines[0], lines[1], lines[2:]
    run.geometry = geometry
    return run


def test_the_header_rules_driven_as_the_kernels_drive_them(tail_driver):
    rng = np.random.default_rng(11)
    G = 1357                                                                                # (a chunk of several blocks of rows at pr = 64)
    v = np.round(rng.normal(size=G), 1)                                                     # many equal values
    v[rng.integers(0, G, 12)] = -np.inf
    v[rng.integers(0, G, 5)] = np.nan
    v[rng.integers(0, G, 3)] = np.inf                                                       # (not finite: never held)
    v[3] = -0.0
    v[90] = 0.0
    n_finite = int(np.isfinite(v).sum())
    for K in (2, 7, 40, n_finite, G):
        want_v, want_g, want_n = sorted_columns(v[:, None], K)
        for chunk, batch, pr in ((1, 4, 1), (7, 3, 4), (64, 5, 64), (64, 1024, 2), (300, 16, 64), (G, 64, 1), (G, 1024, 64)):
            h, got_v, got_g = tail_driver(v, K, chunk, batch, pr)
            assert h == want_n[0] == min(K, n_finite), (K, chunk, batch)
            assert same_bytes(got_g, want_g[0, :h]), (K, chunk, batch)
            assert np.array_equal(got_v, want_v[0, :h]), (K, chunk, batch)                 # (+0.0 and -0.0 tie: whichever point's)
            assert same_bytes(got_v, np.where(np.isfinite(v), v, -np.inf)[got_g]), (K, chunk, batch)


# ------------------------------------------------------------------ 3. the generalised Pareto fit --------------------------
@pytest.mark.parametrize("k", [-0.3, 0.0, 0.3, 0.7, 1.2])
@pytest.mark.parametrize("n", [50, 200, 1000])
def test_gpd_fit_recovers_the_shape(k, n):
    from victor_amd.importance import gpd_fit, gpd_quantile
    for seed in range(4):
        x = np.sort(gpd_quantile(np.random.default_rng([seed, n]).random(n), k, 2.0))
        k_hat, scale = gpd_fit(x)
        print(f"k = {k}, n = {n}, seed {seed}: k_hat = {k_hat:.3f}, scale = {scale:.3f}, bound {4 * (1 + k) / np.sqrt(n):.3f}")
        assert abs(k_hat - k) <= 4.0 * (1.0 + k) / np.sqrt(n), (k, n, seed, k_hat)
        assert scale > 0


def test_gpd_fit_follows_its_formulas_and_its_edges():
    from victor_amd.importance import gpd_fit, gpd_quantile, smooth_tail
    x = np.sort(gpd_quantile(np.random.default_rng(5).random(120), 0.4, 0.5))
    n = len(x)
    m = 30 + int(np.sqrt(n))
    b = 1 / x[-1] + (1 - np.sqrt(m / (np.arange(1, m + 1) - 0.5))) / (3 * x[int(n / 4 + 0.5) - 1])
    k = np.array([np.mean(np.log1p(-bi * x)) for bi in b])
    L = n * (np.log(-b / k) - k - 1)
    w = np.array([1 / np.sum(np.exp(L - Li)) for Li in L])
    keep = w >= 10 * np.finfo(float).eps
    b_post = np.sum(b[keep] * w[keep] / w[keep].sum())
    k_post = np.mean(np.log1p(-b_post * x))
    k_hat, scale = gpd_fit(x)
    assert np.isclose(scale, -k_post / b_post, rtol=1e-12, atol=0) and np.isclose(k_hat, (n * k_post + 5) / (n + 10), rtol=1e-12, atol=0)
    # the limit at k = 0, and continuity about it
    p = np.linspace(0.01, 0.99, 25)
    assert same_bytes(gpd_quantile(p, 0.0, 1.5), -1.5 * np.log1p(-p))
    assert np.allclose(gpd_quantile(p, 1e-9, 1.5), gpd_quantile(p, 0.0, 1.5), rtol=1e-7, atol=0)
    # no fit: too few entries, or excesses that are all zero
    assert smooth_tail(np.array([1.0, 0.9, 0.8, 0.7]), 0.5)[0] == np.inf
    k0, _, same = smooth_tail(np.full(8, 0.5), 0.5)
    assert k0 == np.inf and same_bytes(same, np.full(8, 0.5)) and gpd_fit(np.zeros(8))[0] == np.inf
    # smoothed weights: ascending quantiles handed out in the held (descending) order, capped at 1, all above the cutoff
    w = np.sort(0.2 + gpd_quantile(np.random.default_rng(6).random(40), 0.6, 0.05))[::-1]
    w = w / w[0]
    k1, s1, smoothed = smooth_tail(w, 0.9 * w[-1])
    assert np.isfinite(k1) and np.all(np.diff(smoothed) <= 0) and smoothed.max() <= 1.0 and smoothed.min() > 0.9 * w[-1]


def test_quantile_function_against_scipy():
    genpareto = pytest.importorskip("scipy.stats").genpareto
    from victor_amd.importance import gpd_quantile
    p = np.linspace(0.001, 0.999, 97)
    for k in (-0.4, -1e-3, 0.2, 0.7, 1.3):
        for scale in (0.01, 2.0):
            assert np.allclose(gpd_quantile(p, k, scale), genpareto.ppf(p, k, scale=scale), rtol=64 * tolerances.U, atol=0), (k, scale)
    assert np.allclose(gpd_quantile(p, 0.0, 2.0), genpareto.ppf(p, 0.0, scale=2.0), rtol=64 * tolerances.U, atol=0)


# ------------------------------------------------------------------ 4. a tail index known in closed form -------------------
class Normal1D:
    """lnL = -x^2 / 2 on a box wide enough to cut nothing."""
    block = {"x": {"prior": {"min": -60.0, "max": 60.0}, "ref": {"loc": 0.0, "scale": 1.0}, "proposal": 1.0}}

    def __call__(self, batch):
        return -0.5 * batch["x"] ** 2


def test_tail_index_of_a_gaussian_under_a_gaussian_proposal():
    """A unit Gaussian target under a Gaussian proposal of variance s^2 has weights ~ exp(x^2 (1 / s^2 - 1) / 2): for s^2 < 1 a
    Pareto tail of index 1 - s^2, for s^2 > 1 bounded weights.  Measured (n = 8192, seeds 0 .. 3, the default M = 272):
    s^2 = 0.4: k = 0.503, 0.513, 0.587, 0.485 (index 0.6; below the threshold 0.70, so ``OK``), raw ess 2565 .. 3522, smoothed
    2858 .. 3458; s^2 = 2: k = -1.636, -1.702, -1.837, -1.699, ``OK`` (weights bounded by their value at x = 0, which they
    approach like 1 - x^2 / 4: a density ~ (1 - w)^(-1/2), shape -2).  No fixed k is asserted: the narrow proposal's exceeds
    the wide one's, and the wide one's lies below the threshold."""
    from victor_amd import GaussianProposal
    f = Normal1D()
    for seed in range(4):
        narrow = host(f, f.block, GaussianProposal(["x"], [0.0], [[0.4]]), n=8192, seed=seed, tail=True)
        wide = host(f, f.block, GaussianProposal(["x"], [0.0], [[2.0]]), n=8192, seed=seed, tail=True)
        tn, tw = narrow.tail, wide.tail
        print(f"seed {seed}: s2 = 0.4: k = {tn.k[0]:.3f} (status {tn.status[0]}, ess {narrow.ess[0]:.0f} -> {tn.ess[0]:.0f}); "
              f"s2 = 2: k = {tw.k[0]:.3f} (status {tw.status[0]}); threshold {tw.k_threshold:.3f}, M = {tw.size}")
        assert tn.size == tw.size == 272 and narrow.n_inside == 8192
        assert tw.k_threshold == min(1 - 1 / np.log10(8192), 0.7) == 0.7
        assert tn.k[0] > tw.k[0] and tw.k[0] < tw.k_threshold and tw.status[0] == tw.OK
        assert tn.status[0] == (tn.HIGH_K if tn.k[0] > tn.k_threshold else tn.OK)
        # smoothing a bounded tail changes the evidence by less than its error
        assert abs(tw.ln_evidence[0] - wide.ln_evidence[0]) < wide.ln_evidence_error[0]


# ------------------------------------------------------------------ 5. the corrections -------------------------------------
@pytest.mark.parametrize("prior", [False, True])
def test_corrected_sums_against_a_direct_recomputation(prior):
    from victor_amd.importance import tri
    from victor_amd.priors import GaussianPrior
    ld = np.longdouble
    g = Gaussian(3)
    kw = dict(prior=GaussianPrior(g.names[:2], [0.01, 0.02], sigma=g.sigma[:2])) if prior else {}
    rec = Recorder(g)
    ip = host(rec, g.block, g.proposal(dof=4), n=1500, seed=3, chunk=10 ** 4, tail=True, **kw)
    t, G, d = ip.tail, ip.n_inside, 3
    assert ip.n_chunks == 1 and t.status[0] in (t.OK, t.HIGH_K) and np.isfinite(t.k[0]) and t.n_tail[0] == t.size
    lnpost = lnpost_of(ip, rec)[:, 0]
    w = np.exp(lnpost - ip.ln_max[0])
    n = int(t.n_tail[0])
    assert same_bytes(w[t.index[0, :n]], t.weight[0, :n]) and not same_bytes(t.smoothed_weight[0, :n], t.weight[0, :n])
    assert same_bytes(t.smoothed_weight[0, n:], t.weight[0, n:])                            # the cutoff keeps its weight
    # the smoothed values in the order of the weights they replace
    assert np.all(np.diff(t.smoothed_weight[0, :n]) <= 0) and np.all(t.smoothed_weight[0, :n] >= t.weight[0, n])
    ws = w.copy()
    ws[t.index[0, :n]] = t.smoothed_weight[0, :n]
    y = ip._sample.y.astype(ld)
    want = {"total": (ws.astype(ld), None), "sq": (ws.astype(ld) ** 2, None)}
    for j in range(d):
        want[("s1", j)] = (ws.astype(ld) * y[:, j], None)
        for j2 in range(j, d):
            want[("s2", tri(d, j, j2))] = (ws.astype(ld) * y[:, j] * y[:, j2], None)
    worst = 0.0
    for key, (terms, _) in want.items():
        got = t.sums[key] [0] if isinstance(key, str) else t.sums[key[0]][0, key[1]]
        bound = (G + 4) * tolerances.U * float(np.sum(np.abs(terms)))
        worst = max(worst, abs(float(ld(got) - np.sum(terms))) / bound)
    print(f"corrected sums, prior {prior}: worst |sum - recomputation| / bound = {worst:.3f}")
    assert worst <= 1.0
    # the figures follow rule 5 on the corrected sums, with the same normalisation
    total, sq = t.sums["total"][0], t.sums["sq"][0]
    norm = ip.prior_ln_max + np.log(ip.prior_total) if prior else np.log(float(ip.n_drawn))
    assert same_bytes(t.ln_evidence[0], ip.ln_max[0] + np.log(total) - norm) and same_bytes(t.ess[0], total * total / sq)
    assert same_bytes(t.ln_evidence_error[0], np.sqrt(max(sq / (total * total) - 1.0 / ip.n_drawn, 0.0)))
    assert same_bytes(t.max_weight_share[0], t.smoothed_weight[0, 0] / total)
    assert same_bytes(t.mean[0], ip._sample.centre + t.sums["s1"][0] / total) and np.allclose(t.cov[0], t.cov[0].T)
    assert same_bytes(t.sigma[0], np.sqrt(np.diag(t.cov[0])))
    # what the raw result holds is what it held
    off = host(g, g.block, g.proposal(dof=4), n=1500, seed=3, chunk=10 ** 4, **kw)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(ip.raw, name), getattr(off.raw, name)), name


# ------------------------------------------------------------------ 6. refusals and the surface ----------------------------
def test_refusals_come_before_any_evaluation_and_any_device_call():
    import victor_amd
    from tests import cases
    from victor_amd.importance import default_tail_size, importance_posterior, resolve_tail
    from victor_amd.utils import InputError
    q3 = proposal3()
    G = host(three, BLOCK3, q3, n=80, seed=2, bins=4).n_inside
    for bad in (False, 1, 0, "yes", 20, {"sizes": 3}, {"size": 3, "k": 1}, {}, [3]):
        with pytest.raises(InputError, match="tail must be None, True or"):
            importance_posterior(None, BLOCK3, q3, n=80, seed=2, device=False, evaluate=raiser, tail=bad)
    for bad in (0, -1, G, 2.0, True, "3", None):
        with pytest.raises(InputError, match="tail size must be an integer in 1"):
            importance_posterior(None, BLOCK3, q3, n=80, seed=2, device=False, evaluate=raiser, tail={"size": bad})
    with pytest.raises(InputError, match="tail size"):
        resolve_tail({"size": 4096}, "x", 10 ** 5)
    assert resolve_tail({"size": 4095}, "x", 10 ** 5) == 4095 and resolve_tail({"size": G - 1}, "x", G) == G - 1
    assert resolve_tail(None, "x", 3) is None and resolve_tail(True, "x", 54000) == default_tail_size(54000) == 698
    assert default_tail_size(10 ** 7) == 4095 and default_tail_size(20) == 4 and default_tail_size(5) == 1
    with pytest.raises(InputError, match="at least 5 kept points"):
        resolve_tail(True, "x", 4)
    # with a fit: refused without a context (on a host without a GPU a device call would raise NativeError instead)
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    params = cases.cobaya_info()["params"]
    names = [n for n, v in params.items() if isinstance(v, dict) and "prior" in v]
    q = victor_amd.GaussianProposal(names, [0.5 * (params[n]["prior"]["min"] + params[n]["prior"]["max"]) for n in names],
                                    np.diag([1e-4] * len(names)))
    with pytest.raises(InputError, match="tail must be None, True or"):
        fit.importance_posterior(params, q, n=8, tail="on")
    with pytest.raises(InputError, match="tail size"):
        fit.importance_posterior(params, q, n=8, tail={"size": 8})


def test_the_keyword_reaches_all_four_entry_points():
    import victor_amd
    from victor_amd import importance
    assert inspect.signature(importance.importance_posterior).parameters["tail"].default is None
    for cls in (victor_amd.CCFFit, victor_amd.Realisations, victor_amd.JointRealisations):
        src = inspect.getsource(cls.importance_posterior)
        assert 'kwargs.pop("tail", None)' in src and "tail=tail" in src, cls
        assert 'kwargs.pop("predictive", None)' in src and "predictive=predictive" in src, cls
    t = importance.SampleTail
    assert (t.OK, t.HIGH_K, t.SHORT, t.NO_FINITE) == (0, 1, 2, 3)


def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), f"include/victor_hip.h does not declare {name}"
        assert name in N.SYMBOLS, name
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert N.SYMBOLS["vk_is_set_tail"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert N.SYMBOLS["vk_is_tail"] == (C.c_int, [C.c_void_p, dp, lp, lp])
    csrc = os.path.join(ROOT, "victor_amd", "csrc")
    rules = open(os.path.join(csrc, "vk_is_tail.h")).read()
    assert "hip/hip_runtime.h" not in rules and "asm" not in rules and '#include "vk_grid.h"' in rules
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "vk_kernel_is_tail.h")).read())
    assert "asm" not in code and "IsArgs a" not in code and "struct IsTailArgs" in code
    assert "atomic" not in code and "atomic" not in re.sub(r"//[^\n]*", "", rules)       # slots by position: no atomics of any kind
    # the existing kernels and their argument struct are the parent's: the new kernels live in a header of their own
    parent = open(os.path.join(csrc, "vk_kernel_importance.h")).read()
    assert "IsTailArgs" not in parent and "tail" not in parent.replace("no launch tail", "")
    unit = open(os.path.join(csrc, "vk_sampled.hip")).read()
    assert '#include "vk_kernel_is_tail.h"' in unit
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert len(re.findall(r"obj/\w+\.o", makefile.split("KERNELOBJS :=")[1].split("\n")[0])) == 7       # eight units with victor_hip
    from victor_amd.importance import MAX_TAIL
    assert re.search(r"constexpr int kMaxK = %d;" % (MAX_TAIL + 1), rules)


def test_library_exports_the_new_symbols_and_refuses_null():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.vk_is_set_tail(None, 8) != 0 and lib.vk_is_set_tail(None, 0) != 0
    assert lib.vk_is_tail(None, None, None, None) != 0
