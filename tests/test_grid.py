"""Grid posteriors (victor_amd/grid.py, vk_grid_create / vk_grid_run) without a GPU: the index rules and the step of
victor_amd/csrc/vk_grid.h compiled on their own under g++ against the NumPy statement - every chunk [g0, g1) of five small
shapes -; the definition route on a correlated Gaussian against its analytic evidence, moments and profile, without and with a
Gaussian prior; chunk invariance; failed nodes; the refusals, raised before any evaluation; and the C ABI's surface.

The bound for weight sums.  Two correct evaluations of the same recipe see identical arguments of exp and differ in exp itself
(<= 1 ULP on the host, <= 2.5 ULP on the device: about 7 u together, u = 2^-53) - in the C rescale factors and in every term - and
in the roundings of T positive additions that now see different inputs: a relative bound of (8 (C + 1) + T) u, C the chunks
processed and T the terms of the accumulator (:func:`sum_bound`).  Two runs with DIFFERENT chunks are held to the sum of their
two bounds; their exp arguments differ (another running maximum), and the rounding of an argument, |lnpost - M| u, is not in the
bound: the chunk-invariance test keeps |lnpost - M| below 17, so that per run the argument of a term (17 u), the telescoped
arguments of the rescales (17 u) and exp and the product of each rescale (3 u each) stay inside it.  Maxima, arg max, counts and
statuses are compared as bytes.
"""

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_grid_create", "vk_grid_set_prior", "vk_grid_run", "vk_grid_rows", "vk_grid_result", "vk_grid_last_error", "vk_grid_destroy")
SHAPES = [(5,), (5, 4), (5, 4, 3), (2, 1, 3), (1, 1)]


def sum_bound(n_chunks, n_terms):
    """Relative bound on a weight sum of ``n_terms`` terms accumulated over ``n_chunks`` chunks (module docstring)."""
    return (8.0 * (n_chunks + 1) + n_terms) * tolerances.U


def terms_of(grid):
    """Terms of every accumulator of a grid: (total, per cell of m1, per cell of m2)."""
    t1 = np.concatenate([np.full(n, grid.G // n) for n in grid.shape])
    t2 = np.concatenate([np.full(grid.shape[a] * grid.shape[b], grid.G // (grid.shape[a] * grid.shape[b])) for a, b in grid.pairs] + [[]])
    return grid.G, t1, t2


def assert_sums(got, want, chunks, what, grid):
    """``total``, ``m1``, ``m2`` of two :class:`victor_amd.grid.Accumulators` at the bound; ``chunks``: the chunk count of each
    run (one number: the same recipe; two: each run within its own bound of the exact sum)."""
    T, t1, t2 = terms_of(grid)
    chunks = np.atleast_1d(chunks)
    worst = 0.0
    for name, terms in (("total", T), ("m1", t1), ("m2", t2)):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (what, name)
        bound = sum(sum_bound(c, np.asarray(terms, dtype=float)) for c in chunks) * np.maximum(np.abs(a), np.abs(b))
        diff = np.abs(a - b)
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    tolerances._record(f"grid sums {what}", worst)
    assert worst <= 1.0, (what, worst)


def assert_exact(got, want, what):
    for name in ("ln_max", "arg_max", "n_finite", "p1", "p2"):
        assert same_bytes(getattr(got, name), getattr(want, name)), (what, name)


# ------------------------------------------------------------------ 1. vk_grid.h against the NumPy statement -----------------
DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_grid.h"

static std::vector<double> in;
static FILE* fo;
static void put(double v) { fwrite(&v, sizeof(double), 1, fo); }

// decode d n[d]              out: node[G][d]
// cells  d n[d]              out, for every 0 <= g0 <= g1 <= G: per axis j and node k the count and the visited indices, then
//                            per pair ja < jb and (ka, kb) the same
// run    d n[d] R chunk n_pairs   in: pairs[n_pairs][2], lnpost[G][R]
//                            out per problem: M, arg, n_finite, total, m1[sum n], p1, m2[sum na nb], p2 - the kernels' flow
//                            (vk_kernel_grid.h) on the host: the chunk's Best from three interleaved parts merged out of
//                            order, advance, the weights, then every cell's walk
int main(int argc, char** argv) {
  const char* mode = argv[1];
  FILE* fi = fopen(argv[argc - 2], "rb");
  fo = fopen(argv[argc - 1], "wb");
  if (!fi || !fo) return 2;
  fseek(fi, 0, SEEK_END);
  in.resize((size_t)ftell(fi) / sizeof(double));
  fseek(fi, 0, SEEK_SET);
  if (in.size() && fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const int d = atoi(argv[2]);
  int n[vkgrid::kMaxP] = {};
  for (int j = 0; j < d; ++j) n[j] = atoi(argv[3 + j]);
  const vkgrid::Shape s = vkgrid::make_shape(d, n);
  const long long G = s.G;
  auto ex = [](double x) { return exp(x); };
  if (!strcmp(mode, "decode")) {
    for (long long g = 0; g < G; ++g)
      for (int j = 0; j < d; ++j) put((double)vkgrid::node(s, j, g));
  } else if (!strcmp(mode, "cells")) {
    std::vector<long long> seen;
    auto dump = [&]() {
      put((double)seen.size());
      for (long long g : seen) put((double)g);
      seen.clear();
    };
    for (long long g0 = 0; g0 <= G; ++g0)
      for (long long g1 = g0; g1 <= G; ++g1) {
        for (int j = 0; j < d; ++j)
          for (int k = 0; k < n[j]; ++k) {
            vkgrid::for_axis_cell(s, j, k, g0, g1, [&](long long g) { seen.push_back(g); });
            dump();
          }
        for (int ja = 0; ja < d; ++ja)
          for (int jb = ja + 1; jb < d; ++jb)
            for (int ka = 0; ka < n[ja]; ++ka)
              for (int kb = 0; kb < n[jb]; ++kb) {
                vkgrid::for_pair_cell(s, ja, ka, jb, kb, g0, g1, [&](long long g) { seen.push_back(g); });
                dump();
              }
      }
  } else if (!strcmp(mode, "run")) {
    const int R = atoi(argv[3 + d]), chunk = atoi(argv[4 + d]), np_ = atoi(argv[5 + d]);
    const double* pr = in.data();
    const double* v = pr + 2 * np_;
    int n1 = 0, n2 = 0, aoff[vkgrid::kMaxP], poff[vkgrid::kMaxPairs];
    for (int j = 0; j < d; ++j) aoff[j] = n1, n1 += n[j];
    for (int q = 0; q < np_; ++q) poff[q] = n2, n2 += n[(int)pr[2 * q]] * n[(int)pr[2 * q + 1]];
    for (int r = 0; r < R; ++r) {
      vkgrid::Running run = vkgrid::start();
      double total = 0.0;
      std::vector<double> m1(n1, 0.0), p1(n1, vkgrid::neg_inf()), m2(n2, 0.0), p2(n2, vkgrid::neg_inf()), w(chunk);
      auto post = [&](long long g) { return vkgrid::clean(v[g * R + r]); };
      for (long long g0 = 0; g0 < G; g0 += chunk) {
        const long long g1 = g0 + chunk < G ? g0 + chunk : G;
        vkgrid::Best part[3] = {vkgrid::none(), vkgrid::none(), vkgrid::none()};
        for (long long g = g0; g < g1; ++g) vkgrid::see(part[(g - g0) % 3], post(g), g);
        vkgrid::advance(run, vkgrid::merge(part[2], vkgrid::merge(part[0], part[1])), ex);
        const bool live = run.m > vkgrid::neg_inf();
        for (long long g = g0; g < g1; ++g) w[g - g0] = live ? vkgrid::weight(post(g), run.m, ex) : 0.0;
        vkgrid::rescale(total, run.factor);
        if (live)
          for (long long g = g0; g < g1; ++g) vkgrid::add(total, w[g - g0]);
        for (int j = 0; j < d; ++j)
          for (int k = 0; k < n[j]; ++k) {
            double &acc = m1[aoff[j] + k], &p = p1[aoff[j] + k];
            vkgrid::rescale(acc, run.factor);
            if (live) vkgrid::for_axis_cell(s, j, k, g0, g1, [&](long long g) { vkgrid::add(acc, w[g - g0]); vkgrid::take_max(p, post(g)); });
          }
        for (int q = 0; q < np_; ++q) {
          const int ja = (int)pr[2 * q], jb = (int)pr[2 * q + 1];
          for (int ka = 0; ka < n[ja]; ++ka)
            for (int kb = 0; kb < n[jb]; ++kb) {
              double &acc = m2[poff[q] + ka * n[jb] + kb], &p = p2[poff[q] + ka * n[jb] + kb];
              vkgrid::rescale(acc, run.factor);
              if (live)
                vkgrid::for_pair_cell(s, ja, ka, jb, kb, g0, g1, [&](long long g) { vkgrid::add(acc, w[g - g0]); vkgrid::take_max(p, post(g)); });
            }
        }
      }
      put(run.m), put((double)run.arg), put((double)run.n_finite), put(total);
      for (double x : m1) put(x);
      for (double x : p1) put(x);
      for (double x : m2) put(x);
      for (double x : p2) put(x);
    }
  } else {
    return 3;
  }
  fclose(fo);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("grid_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(mode, shape, args=(), arrays=()):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.zeros(0)] + [np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        subprocess.run([str(exe), mode, str(len(shape))] + [str(n) for n in shape] + [str(a) for a in args] + [str(fin), str(fout)],
                       check=True)
        return np.fromfile(str(fout), dtype=np.float64)
    return run


def grid_of(shape, pairs=()):
    from victor_amd.grid import resolve_grid
    names = [f"p{j}" for j in range(len(shape))]
    return resolve_grid("test", names, np.zeros(len(shape)), np.ones(len(shape)), dict(zip(names, shape)), None,
                        [(names[a], names[b]) for a, b in pairs])


def all_pairs(d):
    return [(a, b) for a in range(d) for b in range(a + 1, d)]


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_and_every_cell_of_every_chunk_against_numpy(driver, shape):
    grid = grid_of(shape)
    G, d = grid.G, len(shape)
    assert G <= 60
    k = grid.decode(np.arange(G))
    assert np.array_equal(driver("decode", shape).astype(np.int64).reshape(G, d), k)
    # the cells NumPy says: the sorted flat indices of every axis node and every pair of nodes
    cells = [np.flatnonzero(k[:, j] == v) for j in range(d) for v in range(shape[j])]
    cells += [np.flatnonzero((k[:, a] == va) & (k[:, b] == vb)) for a, b in all_pairs(d) for va in range(shape[a]) for vb in range(shape[b])]
    out = driver("cells", shape).astype(np.int64)
    at = 0
    for g0 in range(G + 1):
        for g1 in range(g0, G + 1):
            visited = 0
            for c, members in enumerate(cells):
                n = int(out[at])
                got = out[at + 1:at + 1 + n]
                at += 1 + n
                want = members[(members >= g0) & (members < g1)]
                assert np.array_equal(got, want), (shape, g0, g1, c, got, want)     # once each, increasing, in NumPy's cell
                visited += n
            assert visited == (g1 - g0) * (d + len(all_pairs(d)))        # every index of the chunk once per axis and pair
    assert at == len(out)


def values_for(shape, R, seed):
    """lnpost (G, R) with ties of the maximum, -inf and NaN nodes, a problem that fails everywhere and one that starts failing."""
    rng = np.random.default_rng(seed)
    G = int(np.prod(shape))
    v = -30.0 * rng.random((G, R)) ** 2
    v[rng.random((G, R)) < 0.15] = -np.inf
    v[rng.random((G, R)) < 0.05] = np.nan
    if G > 3:
        v[[1, G - 2], 0] = 0.25                                  # the maximum twice: the first index wins
    if R > 1:
        v[:, 1] = -np.inf
    if R > 2:
        v[: G // 2, 2] = -np.inf
    return v


@pytest.mark.parametrize("shape", SHAPES)
def test_rescale_and_add_against_the_definition(driver, shape):
    from victor_amd.grid import Accumulators, step_definition
    R, pairs = 4, all_pairs(len(shape))
    grid = grid_of(shape, pairs)
    G = grid.G
    v = values_for(shape, R, 11 + G)
    for chunk in sorted({1, 2, 7, G, G + 4}):
        want = Accumulators(grid, R)
        for g0 in range(0, G, chunk):
            step_definition(grid, want, g0, v[g0:g0 + chunk])
        out = driver("run", shape, [R, chunk, len(pairs)], [np.array(pairs, dtype=float), v]).reshape(R, -1)
        got = Accumulators(grid, R)
        got.ln_max, got.arg_max, got.n_finite, got.total = out[:, 0], out[:, 1].astype(np.int64), out[:, 2].astype(np.int64), out[:, 3]
        got.m1, got.p1, got.m2, got.p2 = np.split(out[:, 4:], np.cumsum([grid.n1, grid.n1, grid.n2]), axis=1)
        what = f"vk_grid.h {shape} chunk {chunk}"
        assert_exact(got, want, what)
        assert want.ln_max[1] == -np.inf and want.arg_max[1] == -1 and want.n_finite[1] == 0 and want.total[1] == 0
        if G > 3:
            assert want.arg_max[0] == 1 and want.ln_max[0] == 0.25
        assert_sums(got, want, -(-G // chunk), what, grid)


# ------------------------------------------------------------------ 2. a correlated Gaussian, analytically -------------------
MEAN = np.array([0.3, -0.2])
SIG = np.array([1.0, 0.7])
RHO = 0.5
COV = np.array([[SIG[0] ** 2, RHO * SIG[0] * SIG[1]], [RHO * SIG[0] * SIG[1], SIG[1] ** 2]])
PREC = np.linalg.inv(COV)
BLOCK = {n: {"prior": {"min": float(MEAN[j] - 8 * SIG[j]), "max": float(MEAN[j] + 8 * SIG[j])}, "ref": {"loc": float(MEAN[j]), "scale": 0.1},
             "proposal": 0.1} for j, n in enumerate(["x", "y"])}


def gaussian(batch):
    dx, dy = batch["x"] - MEAN[0], batch["y"] - MEAN[1]
    return -0.5 * (PREC[0, 0] * dx * dx + 2.0 * PREC[0, 1] * dx * dy + PREC[1, 1] * dy * dy)


def host_grid(evaluate, block, **kw):
    from victor_amd.grid import grid_posterior
    return grid_posterior(None, block, device=False, evaluate=evaluate, **kw)


def test_gaussian_evidence_moments_and_profile():
    gp = host_grid(gaussian, BLOCK, bins=64, pairs=[("x", "y")])
    assert gp.names == ["x", "y"] and gp.shape == (64, 64) and gp.n_problems == 1 and gp.status[0] == gp.OK
    assert np.allclose(np.diff(gp.axes["x"]), SIG[0] / 4, rtol=1e-12)                  # cell = sigma / 4
    volume = np.prod(16 * SIG)
    assert abs(gp.ln_evidence[0] - np.log(2 * np.pi * np.sqrt(np.linalg.det(COV)) / volume)) < 1e-10
    assert np.max(np.abs(gp.mean[0] - MEAN)) < 1e-10 and np.max(np.abs(gp.sigma[0] - SIG)) < 1e-10
    assert abs(gp.cov_of("x", "y")[0] - COV[0, 1]) < 1e-10 and abs(gp.cov_of("y", "x")[0] - COV[0, 1]) < 1e-10
    # the exact Gaussian at the nodes: its maximum over the other axis' nodes, minus its maximum over all nodes
    X, Y = np.meshgrid(gp.axes["x"], gp.axes["y"], indexing="ij")
    f = gaussian({"x": X, "y": Y})
    assert np.max(np.abs(gp.profile("x")[0] - (f.max(axis=1) - f.max()))) < 1e-10
    assert np.max(np.abs(gp.profile("y")[0] - (f.max(axis=0) - f.max()))) < 1e-10
    assert np.max(np.abs(gp.profile2d("x", "y")[0] - (f - f.max()))) < 1e-10
    assert same_bytes(gp.profile2d("y", "x")[0], gp.profile2d("x", "y")[0].T)
    # ... which the continuous profile -(x - m)^2 / (2 sigma^2) bounds from above, within the curvature over half a cell
    assert np.all(gp.profile("x")[0] + gp.ln_max[0] <= -0.5 * ((gp.axes["x"] - MEAN[0]) / SIG[0]) ** 2 + 1e-12)
    # densities integrate to one; the marginal of x is the normal density to the quadrature's accuracy
    h = 16 * SIG / 64
    assert abs(gp.marginal("x")[0].sum() * h[0] - 1) < 1e-12 and abs(gp.marginal2d("x", "y")[0].sum() * h[0] * h[1] - 1) < 1e-12
    want = np.exp(-0.5 * ((gp.axes["x"] - MEAN[0]) / SIG[0]) ** 2) / (np.sqrt(2 * np.pi) * SIG[0])
    assert np.max(np.abs(gp.marginal("x")[0] - want)) < 1e-10
    assert abs(gp.median("x")[0] - MEAN[0]) < 1e-3 * SIG[0]                             # (linear inside a cell of sigma / 4)
    lo, hi = gp.interval("x", 0.68)
    assert abs(lo[0] - (MEAN[0] - 0.9945 * SIG[0])) < 0.01 * SIG[0] and abs(hi[0] - (MEAN[0] + 0.9945 * SIG[0])) < 0.01 * SIG[0]
    assert gp.edge_mass.shape == (1, 2, 2) and np.all(gp.edge_mass < 1e-13)
    assert gp.best["x"][0] in gp.axes["x"] and abs(gp.best["x"][0] - MEAN[0]) <= SIG[0] / 8 + 1e-12


def test_gaussian_with_a_gaussian_prior():
    from victor_amd.priors import GaussianPrior
    mu_p, sig_p = np.array([0.6, 0.0]), np.array([0.4, 0.3])
    gp = host_grid(gaussian, BLOCK, bins=64, prior=GaussianPrior(["x", "y"], mu_p, sigma=sig_p), pairs=[("x", "y")])
    cov_p = np.diag(sig_p ** 2)
    post = np.linalg.inv(PREC + np.linalg.inv(cov_p))
    mean = post @ (PREC @ MEAN + np.linalg.inv(cov_p) @ mu_p)
    # Z = int L N(mu_p, cov_p) = (2 pi) |COV|^(1/2) N(MEAN; mu_p, COV + cov_p): the prior's normalisation comes from the grid
    s = COV + cov_p
    dm = MEAN - mu_p
    ln_z = np.log(2 * np.pi * np.sqrt(np.linalg.det(COV))) - 0.5 * dm @ np.linalg.inv(s) @ dm - np.log(2 * np.pi * np.sqrt(np.linalg.det(s)))
    assert abs(gp.ln_evidence[0] - ln_z) < 1e-10
    assert np.max(np.abs(gp.mean[0] - mean)) < 1e-10 and np.max(np.abs(gp.sigma[0] - np.sqrt(np.diag(post)))) < 1e-10
    assert abs(gp.cov_of("x", "y")[0] - post[0, 1]) < 1e-10
    assert abs(gp.prior_ln_max + np.log(gp.prior_total) + np.sum(np.log(16 * SIG / 64)) - np.log(2 * np.pi * np.prod(sig_p))) < 1e-10


# ------------------------------------------------------------------ 3. chunks, failures, refusals ----------------------------
NAMES3 = ["a", "b", "c"]
BLOCK3 = {n: {"prior": {"min": -1.0, "max": 1.0 + j}, "ref": {"loc": 0.0, "scale": 0.1}, "proposal": 0.1} for j, n in enumerate(NAMES3)}
BLOCK3["fixed_one"] = 2.5


def three(batch):
    """Three problems on (a, b, c): a Gaussian, the same shifted by 700 in lnL (the sums must not care), a narrower one (q stays
    below 8.5 on the grid: no lnpost lies more than 17 under its maximum, module docstring)."""
    assert np.all(batch["fixed_one"] == 2.5)
    a, b, c = batch["a"], batch["b"], batch["c"]
    q = 3.0 * (a - 0.2) ** 2 + 2.0 * (a - 0.2) * (b - 0.5) + 1.5 * (b - 0.5) ** 2 + 0.7 * (c - 1.0) ** 2
    return np.stack([-0.5 * q, -0.5 * q - 700.0, -2.0 * q], axis=1)


def test_chunk_invariance():
    kw = dict(bins={"a": 5, "b": 4, "c": 3}, pairs=[("a", "c"), ("c", "b")])
    whole = host_grid(three, BLOCK3, chunk=60, **kw)
    G = 60
    assert whole.n_problems == 3 and whole.shape == (5, 4, 3) and whole.n_chunks == 1
    assert np.allclose(whole.raw.total[0], whole.raw.total[1], rtol=1e-11, atol=0) and whole.raw.total[1] > 1      # the offset is gone
    assert abs(whole.ln_evidence[0] - 700.0 - whole.ln_evidence[1]) < 1e-10
    for chunk in (1, 7, G + 4):
        part = host_grid(three, BLOCK3, chunk=chunk, **kw)
        assert_exact(part.raw, whole.raw, f"chunk {chunk} against {G}")
        assert same_bytes(part.status, whole.status)
        assert_sums(part.raw, whole.raw, [part.n_chunks, whole.n_chunks], f"definition route, chunk {chunk} against {G}", whole._grid)
    assert same_bytes(host_grid(three, BLOCK3, chunk=7, **kw).raw.m1, host_grid(three, BLOCK3, chunk=7, **kw).raw.m1)


def failing(batch):
    """Problem 0 fails everywhere, problem 1 on a < 0 (and reads NaN on a strip of b), problem 2 nowhere."""
    good = three(batch)[:, 0]
    part = np.where(batch["a"] < 0, -np.inf, good)
    part = np.where((batch["b"] > 0.4) & (batch["b"] < 0.9), np.nan, part)
    return np.stack([np.full(len(good), -np.inf), part, good], axis=1)


@pytest.mark.parametrize("chunk", [7, 60])
def test_all_failed_and_partly_failed_problems(chunk):
    gp = host_grid(failing, BLOCK3, bins={"a": 5, "b": 4, "c": 3}, pairs=[("a", "b")], chunk=chunk)
    assert list(gp.status) == [gp.NO_FINITE, gp.OK, gp.OK]
    k = gp._grid.points(np.arange(60))
    fails = (k[:, 0] < 0) | ((k[:, 1] > 0.4) & (k[:, 1] < 0.9))
    assert list(gp.n_finite) == [0, 60 - int(fails.sum()), 60] and 0 < fails.sum() < 60
    assert gp.ln_evidence[0] == -np.inf and np.all(np.isfinite(gp.ln_evidence[1:])) and gp.ln_max[0] == -np.inf and gp.arg_max[0] == -1
    assert np.all(gp.marginal("a")[0] == 0) and np.all(gp.marginal2d("a", "b")[0] == 0)
    assert np.all(gp.profile("a")[0] == -np.inf) and np.all(gp.profile2d("a", "b")[0] == -np.inf)
    assert np.all(gp.marginal("a")[1][gp.axes["a"] < 0] == 0) and np.all(gp.profile("a")[1][gp.axes["a"] < 0] == -np.inf)
    assert gp.ln_evidence[1] < gp.ln_evidence[2]
    for name in ("ln_max", "total", "m1", "p1", "m2", "p2"):
        assert not np.any(np.isnan(getattr(gp.raw, name))), name
    for arr in (gp.ln_evidence, gp.mean, gp.sigma, gp.edge_mass, gp.marginal("b"), gp.profile("c"), gp.cov_of("a", "b")):
        assert not np.any(np.isnan(arr))
    assert np.isnan(gp.median("a")[0]) and np.isnan(gp.best["a"][0]) and np.all(np.isfinite(gp.median("a")[1:]))


def raiser(batch):
    raise AssertionError("a refused call reached the evaluator")


class PairedStub:
    paired_model = True

    def __len__(self):
        return 16


def test_every_refusal_comes_before_the_first_evaluation():
    from victor_amd.grid import grid_posterior
    from victor_amd.utils import InputError

    def refused(match, block=BLOCK3, fit=None, device=False, **kw):
        with pytest.raises(InputError, match=match):
            grid_posterior(fit, block, device=device, evaluate=raiser, **kw)
    refused("paired_model", realisations=PairedStub())
    refused("per-block", block=dict(BLOCK3, **{"a@1": BLOCK3["a"]}))
    refused("per-block", fixed={"b@0": 1.0})
    refused("leaves its prior box", ranges={"a": (-1.5, 0.0)})
    refused("leaves its prior box", ranges={"b": (0.0, 2.5)})
    refused("finite a < b", ranges={"a": (0.5, 0.5)})
    refused("not an axis", ranges={"fixed_one": (0.0, 1.0)})
    refused("two different axes", pairs=[("a", "fixed_one")])
    refused("two different axes", pairs=[("a", "a")])
    refused("given twice", pairs=[("a", "b"), ("b", "a")])
    refused("at most 128 bins", bins={"a": 129, "b": 4, "c": 3}, pairs=[("a", "b")])
    refused("1 .. 1024", bins=0)
    refused("1 .. 1024", bins={"a": 1025, "b": 4, "c": 3})
    refused("1 .. 1024", bins=2.5)
    refused("bins names", bins={"a": 4, "b": 4})
    refused("bins names", bins={"a": 4, "b": 4, "c": 4, "zz": 4})
    refused("scalars", fixed={"fixed_one": np.array([1.0, 2.0])})
    refused("chunk", chunk=0)
    refused("chunk", chunk=65537)
    refused("definition route only", device=True)
    eleven = {f"q{j}": BLOCK3["a"] for j in range(11)}
    refused("at most 10 axes", block=eleven, bins=1)
    five = {f"q{j}": BLOCK3["a"] for j in range(5)}
    refused("at most 2\\^40", block=five, bins=1024)                    # 2^50 points, counted in 64 bits and more
    four = {f"q{j}": BLOCK3["a"] for j in range(4)}
    with pytest.raises(AssertionError, match="reached the evaluator"):
        grid_posterior(None, four, bins=1024, device=False, evaluate=raiser)      # 2^40 points exactly: allowed
    with pytest.raises(InputError, match="a fit or an evaluate"):
        grid_posterior(None, BLOCK3)


def test_refusals_that_need_a_fit_come_before_any_device_call():
    """beta_interpolation='likelihood' on beta-dependent data, a column-less name and a joint fit: refused without a context (on a
    host without a GPU a device call would raise NativeError instead)."""
    import victor_amd
    from tests import cases
    from victor_amd.utils import InputError
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    params = cases.cobaya_info()["params"]
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        fit.grid_posterior(params, bins=4, beta_interpolation="likelihood")
    with pytest.raises(InputError, match="per-block"):
        fit.grid_posterior(params, bins=4, fixed={"sigma_v@0": 380.0})
    with pytest.raises(InputError, match="no column of its own"):
        fit.grid_posterior(dict(params, nonsense={"prior": {"min": 0.0, "max": 1.0}}), bins=4)
    assert not hasattr(victor_amd.JointFit, "grid_posterior")


# ------------------------------------------------------------------ 4. the surface ------------------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), f"include/victor_hip.h does not declare {name}"
        assert name in N.SYMBOLS, name
    assert "BIT FOR BIT WITH EPSILON AS AN AXIS" in header
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert N.SYMBOLS["vk_grid_run"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64])
    assert N.SYMBOLS["vk_grid_result"] == (C.c_int, [C.c_void_p, dp, lp, dp, lp, dp, dp, dp, dp, dp, dp])
    assert N.SYMBOLS["vk_grid_create"][1][2:5] == [C.c_int32, ip, ip]
    for h in ("vk_grid.h",):
        src = open(os.path.join(ROOT, "victor_amd", "csrc", h)).read()
        assert "hip/hip_runtime.h" not in src and "asm" not in src and "fp contract(off)" in src


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22


def test_the_two_methods_share_a_signature():
    import victor_amd
    a = inspect.signature(victor_amd.CCFFit.grid_posterior)
    b = inspect.signature(victor_amd.Realisations.grid_posterior)
    assert a == b
    assert list(a.parameters) == ["self", "params", "bins", "ranges", "fixed", "prior", "pairs", "chunk", "device", "kwargs"]
    assert a.parameters["bins"].default == 32 and a.parameters["device"].default is True and a.parameters["chunk"].default is None
    assert victor_amd.GridPosterior.OK == 0 and victor_amd.GridPosterior.NO_FINITE == 1
