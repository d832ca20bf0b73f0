"""Importance-sampled posteriors (victor_amd/importance.py, vk_is_create / vk_is_run) without a GPU: the index rules, the list
walk and the terms of victor_amd/csrc/vk_importance.h compiled on their own under g++ against the NumPy step - every chunk cut
[g0, g1) of nine small samples, once more under AddressSanitizer and UBSan -; the definition route on correlated Gaussians
against their closed-form evidence, without and with a Gaussian prior and under a Student-t proposal; chunk invariance; failed
points and a proposal that misses; the refusals, raised before any evaluation; and the C ABI's surface.

The bound for sums (:func:`sum_bound`), derived as tests/test_grid.py derives the grid's.  Two correct evaluations of the same
recipe see identical arguments of exp and differ in exp itself (<= 1 ULP on the host, <= 2.5 ULP on the device: about 7 u
together, u = 2^-53).  Relative to the sum of the ABSOLUTE terms A of an accumulator with T terms over C chunks:

* a term ``w`` differs by 7 u (8 u with slack, as the grid's), each of the C rescale products by 7 u + 1 u for its own rounding,
  and the T additions now see different inputs, 1 u each: ``(8 (C + 1) + T) u`` for ``total`` and every histogram cell - the
  grid's bound;
* a moment term ``(w y_j) y_k`` carries two more roundings, 2 u per term (relative to the term, so to A once, not T times):
  ``(8 (C + 1) + 2 + T) u`` for ``s1`` and ``s2``;
* a term of ``sq`` is ``w w``, 14 u + 1 u, and ``sq`` is rescaled by the factor twice, 16 u per chunk: ``(16 (C + 1) + T) u``.

The feature's request proposed ``(8 (C + 2) + 3 T) u`` for all of them (the grid's bound "with two more roundings per moment
term").  The derived constants are smaller for ``total``, the histograms and
the moments at every T >= 1, and are the ones used; for ``sq`` the derivation gives the doubled factor term, which exceeds the
proposal when T < 4 C (many short chunks), so ``sq`` is held to its own derived bound.  A is taken from the definition route
itself, run once more with ``|y|`` (:func:`abs_sums`); for the positive sums it is the sum.  Two runs with DIFFERENT chunks
are held to the sum of their two bounds, under the condition tests/test_grid.py states: |lnpost - M| < 17.  Maxima, arg max,
counts and statuses are compared as bytes.
"""

import copy
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
NEW = ("vk_is_create", "vk_is_run", "vk_is_rows", "vk_is_result", "vk_is_last_error", "vk_is_destroy")
EXACT = ("ln_max", "arg_max", "n_finite")
SUMS = ("total", "sq", "s1", "s2", "h1", "h2")


def sum_bound(name, n_chunks, n_terms):
    """Relative bound, against the sum of the absolute terms, on accumulator ``name`` with ``n_terms`` terms accumulated over
    ``n_chunks`` chunks (module docstring)."""
    n_terms = np.asarray(n_terms, dtype=float)
    if name == "sq":
        return (16.0 * (n_chunks + 1) + n_terms) * tolerances.U
    if name in ("s1", "s2"):
        return (8.0 * (n_chunks + 1) + 2.0 + n_terms) * tolerances.U
    return (8.0 * (n_chunks + 1) + n_terms) * tolerances.U


def terms_of(layout, x):
    """Terms of every accumulator: name -> a count, or one per cell."""
    where = layout.cells_of(x)
    G, d = len(x), layout.d
    h = [np.bincount(where[l][where[l] >= 0], minlength=int(layout.cell_off[l + 1] - layout.cell_off[l])) for l in range(layout.n_lists)]
    return {"total": G, "sq": G, "s1": G, "s2": G, "h1": np.concatenate(h[:d]), "h2": np.concatenate(h[d:] + [np.zeros(0, dtype=int)])}


def assert_sums(got, want, absolute, chunks, what, layout, x):
    """The sums of two :class:`victor_amd.importance.Sums` at the bound; ``absolute``: the Sums of the absolute terms;
    ``chunks``: the chunk count of each run (one number: the same recipe; two: each run within its own bound)."""
    terms = terms_of(layout, x)
    chunks = np.atleast_1d(chunks)
    worst = 0.0
    for name in SUMS:
        a, b, s = getattr(got, name), getattr(want, name), np.abs(getattr(absolute, name))
        assert a.shape == b.shape == s.shape and np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (what, name)
        bound = sum(sum_bound(name, c, terms[name]) for c in chunks) * s * (1.0 + 64 * tolerances.U)
        diff = np.abs(a - b)
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    tolerances._record(f"importance sums {what}", worst)
    assert worst <= 1.0, (what, worst)


def assert_exact(got, want, what):
    for name in EXACT:
        assert same_bytes(getattr(got, name), getattr(want, name)), (what, name)


def abs_sums(ip, lnl_chunks):
    """The sums of the absolute terms of a definition-route result ``ip``: the definition once more over the same lnL (one array
    per chunk) with ``|y|`` for ``y``."""
    from victor_amd.importance import run_definition
    s = copy.copy(ip._sample)
    s.y = np.abs(s.y)
    it = iter(lnl_chunks)
    return run_definition(ip._layout, s, ip._lists, ip.n_problems, lambda x: next(it))[0]


class Recorder:
    """An ``evaluate`` callable that keeps what ``inner`` returned, chunk by chunk."""

    def __init__(self, inner):
        self.inner, self.chunks = inner, []

    def __call__(self, batch):
        v = np.asarray(self.inner(batch), dtype=np.float64)
        self.chunks.append(v)
        return v


# ------------------------------------------------------------------ 1. vk_importance.h against the NumPy step ----------------
DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_importance.h"

static std::vector<double> in;
static size_t at = 0;
static double get() { return in[at++]; }
static FILE* fo;
static void put(double v) { fwrite(&v, sizeof(double), 1, fo); }

// run d R G n_lists n_cases    in: cells[n_lists], y[G][d], lnpost[G][R], then per case: n_chunks, and per chunk g0, n and per
//                              list its offsets (cells + 1) and its segment (n entries)
//                              out per case and problem: M, arg, n_finite, then the accumulators in vk_importance.h's order - the
//                              kernels' flow (vk_kernel_importance.h) on the host: the chunk's Best from three interleaved parts
//                              merged out of order, advance, the weights, then every accumulator's walk
// check n cells                in: off[cells + 1], segment[n]      out: the code of check_list and where
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
  auto ex = [](double x) { return exp(x); };
  if (!strcmp(mode, "check")) {
    const int n = atoi(argv[2]), cells = atoi(argv[3]);
    std::vector<int> off(cells + 1), seg(n);
    for (int& v : off) v = (int)get();
    for (int& v : seg) v = (int)get();
    long long where = -1;
    put((double)vkis::check_list(seg.data(), off.data(), cells, n, &where));
    put((double)where);
  } else if (!strcmp(mode, "run")) {
    const int d = atoi(argv[2]), R = atoi(argv[3]), G = atoi(argv[4]), n_lists = atoi(argv[5]), n_cases = atoi(argv[6]);
    std::vector<int> cells(n_lists), cell_off(n_lists + 1, 0);
    for (int l = 0; l < n_lists; ++l) cells[l] = (int)get(), cell_off[l + 1] = cell_off[l] + cells[l];
    const double* y = &in[at];
    at += (size_t)G * d;
    const double* v = &in[at];
    at += (size_t)G * R;
    const int W = vkis::whole(d), A = W + cell_off[n_lists];
    for (int j = 0; j < d; ++j)
      for (int k = j; k < d; ++k) {
        int j2, k2;
        vkis::second_of(d, vkis::second(d, j, k), j2, k2);
        if (j2 != j || k2 != k || vkis::second(d, j, k) >= W || vkis::first(j) >= vkis::second(d, 0, 0)) return 5;
      }
    for (int c = 0; c < n_cases; ++c) {
      std::vector<vkgrid::Running> run(R, vkgrid::start());
      std::vector<double> acc((size_t)R * A, 0.0);
      const int n_chunks = (int)get();
      for (int q = 0; q < n_chunks; ++q) {
        const long long g0 = (long long)get();
        const int n = (int)get();
        std::vector<std::vector<int>> off(n_lists), seg(n_lists);
        for (int l = 0; l < n_lists; ++l) {
          off[l].resize(cells[l] + 1);
          seg[l].resize(n);
          for (int& x : off[l]) x = (int)get();
          for (int& x : seg[l]) x = (int)get();
          long long where;
          if (vkis::check_list(seg[l].data(), off[l].data(), cells[l], n, &where)) return 4;
        }
        std::vector<double> w(n);
        for (int r = 0; r < R; ++r) {
          auto post = [&](long long g) { return vkgrid::clean(v[g * R + r]); };
          vkgrid::Best part[3] = {vkgrid::none(), vkgrid::none(), vkgrid::none()};
          for (long long g = g0; g < g0 + n; ++g) vkgrid::see(part[(g - g0) % 3], post(g), g);
          vkgrid::advance(run[r], vkgrid::merge(part[2], vkgrid::merge(part[0], part[1])), ex);
          const bool live = run[r].m > vkgrid::neg_inf();
          for (int i = 0; i < n; ++i) w[i] = live ? vkgrid::weight(post(g0 + i), run[r].m, ex) : 0.0;
          for (int a = 0; a < A; ++a) {
            double& s = acc[(size_t)r * A + a];
            if (a == vkis::kSq) vkis::rescale_sq(s, run[r].factor);
            else vkgrid::rescale(s, run[r].factor);
            if (!live) continue;
            auto add = [&](double t) { vkgrid::add(s, t); };
            const double* yc = y + g0 * d;
            if (a == vkis::kTotal) {
              vkis::range_ahead<4>(0, n, [&](int i) { return w[i]; }, add);
            } else if (a == vkis::kSq) {
              vkis::range_ahead<3>(0, n, [&](int i) { return vkis::square_term(w[i]); }, add);
            } else if (a < vkis::kFirst + d) {
              const int j = a - vkis::kFirst;
              vkis::range_ahead<4>(0, n, [&](int i) { return vkis::first_term(w[i], yc[i * d + j]); }, add);
            } else if (a < W) {
              int j, k;
              vkis::second_of(d, a, j, k);
              vkis::range_ahead<5>(0, n, [&](int i) { return vkis::second_term(w[i], yc[i * d + j], yc[i * d + k]); }, add);
            } else {
              int l = 0;
              while (l + 1 < n_lists && a - W >= cell_off[l + 1]) ++l;
              const int k = a - W - cell_off[l];
              if (k % 2) vkis::walk(seg[l].data(), off[l][k], off[l][k + 1], g0, [&](long long g) { add(w[g - g0]); });
              else vkis::walk_ahead<4>(seg[l].data(), off[l][k], off[l][k + 1], g0, [&](long long g) { return w[g - g0]; }, add);
            }
          }
        }
      }
      for (int r = 0; r < R; ++r) {
        put(run[r].m), put((double)run[r].arg), put((double)run[r].n_finite);
        for (int a = 0; a < A; ++a) put(acc[(size_t)r * A + a]);
      }
    }
    if (at != in.size()) return 6;
  } else {
    return 3;
  }
  fclose(fo);
  return 0;
}
"""


def build_driver(d, flags=()):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    cmd = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode and flags and re.search(r"cannot find|asan|ubsan|sanitize", done.stderr):
        pytest.skip("the sanitizer runtime is not installed")
    assert done.returncode == 0, done.stderr

    def run(mode, args=(), arrays=()):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.zeros(0)] + [np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        done = subprocess.run([str(exe), mode] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        return np.fromfile(str(fout), dtype=np.float64)
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("importance_driver"))


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("importance_driver_san"), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def layout_of(d):
    """4 bins per axis over [0, 1]^d, axis 0 ranged to [0.2, 0.8]; the pair (0, 1) from d = 2."""
    from victor_amd.importance import resolve_layout
    names = [f"p{j}" for j in range(d)]
    return resolve_layout("test", names, np.zeros(d), np.ones(d), 4, {"p0": (0.2, 0.8)}, [("p1", "p0")] if d > 1 else None)


def small_sample(G, d, R, seed):
    """x (G, d) in the unit box - with, from G = 7, a point on each edge of axis 0's range, one below and one above it, and no
    point in its third bin - and lnpost (G, R) with ties of the maximum, -inf and NaN values, a problem that fails everywhere and
    one that starts failing."""
    rng = np.random.default_rng(seed)
    x = rng.random((G, d))
    third = (x[:, 0] >= 0.5) & (x[:, 0] < 0.65)
    x[third, 0] -= 0.2                                             # bin 2 of [0.2, 0.8] in 4 bins stays empty
    if G >= 7:
        x[[1, 2, 3, 4], 0] = [0.8, 0.2, 0.05, 0.93]
    v = -30.0 * rng.random((G, R)) ** 2
    v[rng.random((G, R)) < 0.15] = -np.inf
    v[rng.random((G, R)) < 0.05] = np.nan
    if G > 3:
        v[[1, G - 2], 0] = 0.25                                    # the maximum twice: the first index wins
        v[0, 0] = -np.inf
    if R > 1:
        v[:, 1] = -np.inf
    if R > 2:
        v[: G // 2, 2] = -np.inf
    return x, v


class CaseLists:
    """The lists of one case's chunks, as :func:`victor_amd.importance.step_definition` asks for them."""

    def __init__(self, layout, x, cuts):
        from victor_amd.importance import Lists
        self.parts = [Lists(layout, x[g0:g1], g1 - g0) for g0, g1 in cuts]

    def members(self, layout, c, l):
        return self.parts[c].members(layout, 0, l)


def cases_of(G):
    """Every chunk cut [g0, g1): the chunks [0, g0), [g0, g1), [g1, G), the empty ones left out."""
    out = []
    for g0 in range(G):
        for g1 in range(g0 + 1, G + 1):
            out.append([(a, b) for a, b in ((0, g0), (g0, g1), (g1, G)) if a < b])
    return out


def run_cases(run, layout, x, y, v, cases):
    """The driver's Sums of every case."""
    from victor_amd.importance import Sums
    G, d = x.shape
    R = v.shape[1]
    arrays = [[int(layout.cell_off[l + 1] - layout.cell_off[l]) for l in range(layout.n_lists)], y, v]
    for cuts in cases:
        lists = CaseLists(layout, x, cuts)
        arrays.append([len(cuts)])
        for c, (g0, g1) in enumerate(cuts):
            arrays.append([g0, g1 - g0])
            for l in range(layout.n_lists):
                entries, off = lists.members(layout, c, l)
                arrays += [off, entries]
    out = run("run", [d, R, G, layout.n_lists, len(cases)], arrays).reshape(len(cases), R, -1)
    W, T = 2 + d + d * (d + 1) // 2, d * (d + 1) // 2
    got = []
    for block in out:
        s = Sums(layout, R)
        s.ln_max, s.arg_max, s.n_finite = block[:, 0].copy(), block[:, 1].astype(np.int64), block[:, 2].astype(np.int64)
        a = block[:, 3:]
        s.total, s.sq, s.s1, s.s2 = a[:, 0].copy(), a[:, 1].copy(), a[:, 2:2 + d].copy(), a[:, 2 + d:2 + d + T].copy()
        s.h1, s.h2 = a[:, W:W + layout.n1].copy(), a[:, W + layout.n1:].copy()
        assert a.shape[1] == W + layout.n1 + layout.n2
        got.append(s)
    return got


def definition_of(layout, x, y, v, cuts):
    from victor_amd.importance import Sums, step_definition
    lists = CaseLists(layout, x, cuts)
    acc = Sums(layout, v.shape[1])
    for c, (g0, g1) in enumerate(cuts):
        step_definition(layout, lists, c, y[g0:g1], acc, g0, v[g0:g1])
    return acc


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("G", [1, 7, 23])
def test_every_chunk_cut_against_the_numpy_step(driver, G, d):
    R = 4
    layout = layout_of(d)
    x, v = small_sample(G, d, R, 100 * G + d)
    y = x - 0.4
    if G >= 7:                                                   # what the sample is for
        s0 = layout.cells_of(x)[0]
        assert s0[1] == 4 and s0[2] == 1 and s0[3] == 0 and s0[4] == 5 and not np.any(s0 == 3) and np.any(v == -np.inf)
    cases = cases_of(G)
    assert len(cases) == G * (G + 1) // 2
    got = run_cases(driver, layout, x, y, v, cases)
    for cuts, g in zip(cases, got):
        want = definition_of(layout, x, y, v, cuts)
        absolute = definition_of(layout, x, np.abs(y), v, cuts)
        what = f"vk_importance.h G {G} d {d} cuts {cuts}"
        assert_exact(g, want, what)
        assert want.ln_max[1] == -np.inf and want.arg_max[1] == -1 and want.n_finite[1] == 0 and want.total[1] == 0
        if G > 3:
            assert want.arg_max[0] == 1 and want.ln_max[0] == 0.25
        assert_sums(g, want, absolute, len(cuts), what, layout, x)


def test_the_driver_under_address_and_undefined_behaviour_sanitizers(driver, sanitized_driver):
    """The same program built with -fsanitize=address,undefined: it runs clean and writes the same bytes."""
    G, d, R = 23, 3, 4
    layout = layout_of(d)
    x, v = small_sample(G, d, R, 7)
    cases = cases_of(G)[::7] + [[(0, G)]]
    plain = run_cases(driver, layout, x, x - 0.4, v, cases)
    checked = run_cases(sanitized_driver, layout, x, x - 0.4, v, cases)
    for a, b in zip(plain, checked):
        for name in EXACT + SUMS:
            assert same_bytes(getattr(a, name), getattr(b, name)), name


def test_check_list_names_what_is_wrong(driver):
    off, seg = [0, 2, 2, 5], [1, 3, 0, 2, 4]
    assert list(driver("check", [5, 3], [off, seg])) == [0, 0]
    assert list(driver("check", [5, 3], [[1, 2, 2, 5], seg])) == [1, 0]            # does not start at 0
    assert list(driver("check", [5, 3], [[0, 3, 2, 5], seg])) == [1, 2]            # decreases
    assert list(driver("check", [4, 3], [off, seg[:4]])) == [1, 3]                 # ends outside the chunk
    assert list(driver("check", [5, 3], [off, [1, 3, 0, 5, 4]])) == [2, 3]         # an entry outside the chunk
    assert list(driver("check", [5, 3], [off, [1, 3, 0, -1, 4]])) == [2, 3]
    assert list(driver("check", [5, 3], [off, [3, 1, 0, 2, 4]])) == [2, 1]         # not increasing inside its cell
    assert list(driver("check", [5, 3], [[0, 2, 2, 4], seg])) == [0, 0]            # (a pair's list may leave points out)


# ------------------------------------------------------------------ 2. correlated Gaussians, analytically --------------------
WIDTHS = np.array([0.02, 0.05, 0.1, 0.2])
SEEDS = range(8)


class Gaussian:
    """lnL = -1/2 x^T C^-1 x on the box [-1, 1]^d: widths 0.02, 0.05, 0.1, 0.2, the first parameter correlated with the rest
    through A = I, A[0, 1:] = 0.5, C = (A sigma)(A sigma)^T.  The proposal: the mean shifted by half a standard deviation per
    parameter, the covariance 2 C."""

    def __init__(self, d):
        self.d, self.names = d, [f"p{j}" for j in range(d)]
        A = np.eye(d)
        A[0, 1:] = 0.5
        As = A * WIDTHS[None, :d]
        self.cov = As @ As.T
        self.prec = np.linalg.inv(self.cov)
        self.sigma = np.sqrt(np.diag(self.cov))
        self.block = {n: {"prior": {"min": -1.0, "max": 1.0}, "ref": {"loc": 0.0, "scale": 0.1}, "proposal": 0.1} for n in self.names}
        self.ln_norm = 0.5 * np.log(np.linalg.det(2 * np.pi * self.cov))
        self.ln_evidence = self.ln_norm - d * np.log(2.0)

    def __call__(self, batch):
        x = np.stack([batch[n] for n in self.names], axis=1)
        return -0.5 * np.einsum("ni,ij,nj->n", x, self.prec, x)

    def proposal(self, dof=None):
        from victor_amd import GaussianProposal
        return GaussianProposal(self.names, 0.5 * self.sigma, 2.0 * self.cov, dof=dof)


def host(evaluate, block, q=None, **kw):
    from victor_amd.importance import importance_posterior
    return importance_posterior(None, block, q, device=False, evaluate=evaluate, **kw)


def assert_caps(runs, truth, what):
    """Cap 1: every run within 4 of its own error; cap 2: the seed mean within 4 rms(error) / sqrt(seeds) of the closed form.
    Under a prior ln_evidence is the difference of two estimates from one sample, ln(sum L prior / q) - ln(sum prior / q), and
    ``ln_evidence_error`` is the first one's alone: each lies within 4 of its own error, so by the triangle inequality the
    difference within 4 of the SUM of ``ln_evidence_error`` and ``prior_error`` - the error the caps then use."""
    ev = np.array([ip.ln_evidence[0] for ip in runs])
    err = np.array([ip.ln_evidence_error[0] + getattr(ip, "prior_error", 0.0) for ip in runs])
    pulls = np.abs(ev - truth) / err
    cap = 4.0 * np.sqrt(np.mean(err ** 2)) / np.sqrt(len(runs))
    print(f"{what}: worst pull {pulls.max():.2f}, seed mean {ev.mean() - truth:+.4f}, cap {cap:.4f}, ESS >= {min(ip.ess[0] for ip in runs):.0f}")
    assert np.all(np.isfinite(ev)) and np.all(err > 0) and np.all(pulls <= 4.0), (what, pulls)
    assert abs(ev.mean() - truth) <= cap, (what, ev.mean() - truth, cap)


@pytest.mark.parametrize("dof", [None, 5])
@pytest.mark.parametrize("d", [2, 4])
def test_gaussian_evidence_and_moments(d, dof):
    g = Gaussian(d)
    runs = [host(g, g.block, g.proposal(dof), n=4096, seed=s, pairs=[("p1", "p0")]) for s in SEEDS]
    assert_caps(runs, g.ln_evidence, f"d = {d}, dof = {dof}")
    for ip in runs:
        assert ip.status[0] == ip.OK and ip.n_drawn == 4096 and 0 < ip.n_inside <= 4096 and ip.n_finite[0] == ip.n_inside
        assert ip.ess[0] > 500 and abs(ip.max_weight_share[0] * ip.raw.total[0] - 1) < 1e-15
        assert np.all(np.abs(ip.mean[0]) <= 4 * ip.sigma[0] / np.sqrt(ip.ess[0])), (ip.mean[0], ip.sigma[0], ip.ess[0])
        assert np.allclose(ip.sigma[0], g.sigma, rtol=0.2) and np.allclose(ip.cov[0], ip.cov[0].T)
        assert np.all(ip.outside_mass == 0)
        assert abs(ip.marginal("p0")[0].sum() * (2.0 / 64) - 1) < 1e-12
        assert abs(ip.marginal2d("p0", "p1")[0].sum() * (2.0 / 64) ** 2 - 1) < 1e-12
        assert same_bytes(ip.marginal2d("p0", "p1")[0], ip.marginal2d("p1", "p0")[0].T)
        lo, hi = ip.interval("p1", 0.68)
        assert abs(ip.median("p1")[0]) < 0.02 and abs(lo[0] + 0.05) < 0.02 and abs(hi[0] - 0.05) < 0.02
        assert ip.best["p0"][0] == ip._sample.x[ip.arg_max[0], 0]


def test_gaussian_with_a_gaussian_prior():
    """Z = int L N(mu_p, cov_p) = |2 pi C|^(1/2) N(0; mu_p, C + cov_p).  The prior is normalised by the sample itself (rule 4), so
    the proposal has to cover the prior as it covers the posterior: the prior's widths are the likelihood's own marginal widths
    (0.032, 0.05), under the proposal's 2 C, and its weights prior / q stay bounded."""
    from victor_amd.priors import GaussianPrior
    g = Gaussian(2)
    mu_p, sig_p = np.array([0.01, 0.02]), g.sigma.copy()
    cov_p = np.diag(sig_p ** 2)
    s = g.cov + cov_p
    truth = g.ln_norm - 0.5 * mu_p @ np.linalg.inv(s) @ mu_p - 0.5 * np.log(np.linalg.det(2 * np.pi * s))
    post = np.linalg.inv(g.prec + np.linalg.inv(cov_p))
    mean = post @ np.linalg.inv(cov_p) @ mu_p
    prior = GaussianPrior(g.names, mu_p, sigma=sig_p)
    runs = [host(g, g.block, g.proposal(), n=4096, seed=s, prior=prior) for s in SEEDS]
    assert_caps(runs, truth, "d = 2 with a Gaussian prior")
    for ip in runs:
        assert np.all(np.abs(ip.mean[0] - mean) <= 4 * ip.sigma[0] / np.sqrt(ip.ess[0]))
        assert np.isfinite(ip.prior_ln_max) and ip.prior_total > 0 and 0 < ip.prior_error < 0.05
    plain = host(g, g.block, g.proposal(), n=4096, seed=0)
    assert not same_bytes(plain.ln_max, runs[0].ln_max)


def test_from_fits_and_a_sample_of_the_callers_own():
    from victor_amd import BestFit, GaussianProposal
    from victor_amd.utils import InputError
    g = Gaussian(2)
    rng = np.random.default_rng(3)
    x = rng.multivariate_normal(np.zeros(2), g.cov, size=6)
    status = np.full(6, BestFit.CONVERGED, dtype=np.int32)
    status[5] = BestFit.MAX_ITER
    bf = BestFit(g.names, x, {}, np.zeros(6), np.zeros(6), status, np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.int64))

    class Lap:
        names, cov = g.names, np.repeat(g.cov[None], 6, axis=0)
    q = GaussianProposal.from_fits(bf, Lap, inflate=2.0)
    assert np.allclose(q.mean, x[:5].mean(axis=0)) and np.allclose(q.cov, 2.0 * (np.cov(x[:5], rowvar=False) + g.cov))
    assert np.allclose(GaussianProposal.from_fits(bf).cov, 2.0 * np.cov(x[:5], rowvar=False))
    one = BestFit(g.names, x[:1], {}, np.zeros(1), np.zeros(1), status[:1], np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64))
    with pytest.raises(InputError, match="nothing gives a covariance"):
        GaussianProposal.from_fits(one)
    ip = host(g, g.block, q, n=2048, seed=1)
    assert abs(ip.ln_evidence[0] - g.ln_evidence) <= 4 * ip.ln_evidence_error[0] and ip.status[0] == ip.OK
    # the same points and density handed over as the caller's own: the same posterior (the centre of y is the caller's mean)
    mean, chol = q.ordered("test", g.names)
    pts = GaussianProposal.draw(mean, chol, None, 2048, 1)
    own = host(g, g.block, sample=pts, ln_proposal=GaussianProposal.ln_density(pts, mean, chol, None))
    assert own.n_drawn == 2048 and own.n_inside == ip.n_inside
    for name in EXACT + ("total", "sq", "h1"):
        assert same_bytes(getattr(own.raw, name), getattr(ip.raw, name)), name
    assert np.allclose(own.mean, ip.mean, rtol=0, atol=1e-12) and np.allclose(own.cov, ip.cov, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ 3. chunks, failures, refusals ----------------------------
NAMES3 = ["a", "b", "c"]
BLOCK3 = {n: {"prior": {"min": -1.0, "max": 1.0 + j}, "ref": {"loc": 0.0, "scale": 0.1}, "proposal": 0.1} for j, n in enumerate(NAMES3)}
BLOCK3["fixed_one"] = 2.5


def proposal3(scale=1.0):
    from victor_amd import GaussianProposal
    return GaussianProposal(["c", "a", "b"], [1.0, 0.2, 0.5], np.diag([0.6, 0.3, 0.4]) ** 2 * scale)     # (not in sampled order)


def three(batch):
    """Three problems on (a, b, c): a Gaussian, the same shifted by 700 in lnL (the sums must not care), a narrower one."""
    assert np.all(batch["fixed_one"] == 2.5)
    a, b, c = batch["a"], batch["b"], batch["c"]
    q = 3.0 * (a - 0.2) ** 2 + 2.0 * (a - 0.2) * (b - 0.5) + 1.5 * (b - 0.5) ** 2 + 0.7 * (c - 1.0) ** 2
    return np.stack([-0.5 * q, -0.5 * q - 700.0, -2.0 * q], axis=1)


def test_chunk_invariance():
    kw = dict(n=80, seed=2, bins={"a": 5, "b": 4, "c": 3}, pairs=[("a", "c"), ("c", "b")], ranges={"b": (0.0, 1.0)})
    rec = Recorder(three)
    whole = host(rec, BLOCK3, proposal3(), chunk=80, **kw)
    G = whole.n_inside
    assert whole.n_problems == 3 and whole.n_chunks == 1 and 40 < G <= 80 and whole.n_drawn == 80
    assert whole._layout.pair_bins == [3, 3] and whole.raw.h2.shape == (3, 18) and whole.raw.h1.shape == (3, 7 + 6 + 5)
    lnpost = rec.chunks[0] + whole._sample.lno[:, None]
    assert np.all(lnpost.max(axis=0) - lnpost.min(axis=0) < 17)                        # the two-run bound's condition
    assert np.allclose(whole.raw.total[0], whole.raw.total[1], rtol=1e-11, atol=0) and whole.raw.total[1] > 1      # the offset is gone
    assert abs(whole.ln_evidence[0] - 700.0 - whole.ln_evidence[1]) < 1e-10
    assert np.any(whole.outside_mass[:, 1] > 0) and np.all(whole.outside_mass[:, [0, 2]] == 0)
    absolute = abs_sums(whole, rec.chunks)
    for chunk in (1, 7, G + 4):
        part = host(three, BLOCK3, proposal3(), chunk=chunk, **kw)
        assert_exact(part.raw, whole.raw, f"chunk {chunk} against {G}")
        assert same_bytes(part.status, whole.status)
        assert_sums(part.raw, whole.raw, absolute, [part.n_chunks, whole.n_chunks], f"definition route, chunk {chunk} against {G}",
                    whole._layout, whole._sample.x)
    a, b = host(three, BLOCK3, proposal3(), chunk=7, **kw), host(three, BLOCK3, proposal3(), chunk=7, **kw)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(a.raw, name), getattr(b.raw, name)), name


def failing(batch):
    """Problem 0 fails everywhere, problem 1 on a < 0 (and reads NaN on a strip of b), problem 2 nowhere."""
    good = three(batch)[:, 0]
    part = np.where(batch["a"] < 0, -np.inf, good)
    part = np.where((batch["b"] > 0.4) & (batch["b"] < 0.9), np.nan, part)
    return np.stack([np.full(len(good), -np.inf), part, good], axis=1)


@pytest.mark.parametrize("chunk", [7, 200])
def test_all_failed_and_partly_failed_problems(chunk):
    ip = host(failing, BLOCK3, proposal3(), n=200, seed=4, bins=4, pairs=[("a", "b")], chunk=chunk, min_ess=5.0)
    assert list(ip.status) == [ip.NO_FINITE, ip.OK, ip.OK]
    x = ip._sample.x
    fails = (x[:, 0] < 0) | ((x[:, 1] > 0.4) & (x[:, 1] < 0.9))
    assert list(ip.n_finite) == [0, ip.n_inside - int(fails.sum()), ip.n_inside] and 0 < fails.sum() < ip.n_inside
    assert ip.ln_evidence[0] == -np.inf and np.all(np.isfinite(ip.ln_evidence[1:])) and ip.ln_max[0] == -np.inf and ip.arg_max[0] == -1
    assert ip.ess[0] == 0 and ip.max_weight_share[0] == 0 and ip.ln_evidence_error[0] == np.inf
    assert np.all(ip.marginal("a")[0] == 0) and np.all(ip.marginal2d("a", "b")[0] == 0) and np.all(ip.outside_mass[0] == 0)
    assert np.all(ip.marginal("a")[1][ip.edges["a"][1:] <= 0] == 0)
    assert ip.ln_evidence[1] < ip.ln_evidence[2]
    for name in EXACT + SUMS:
        assert not np.any(np.isnan(getattr(ip.raw, name))), name
    assert np.all(np.isnan(ip.mean[0])) and np.isnan(ip.best["a"][0]) and np.isnan(ip.median("a")[0])
    for arr in (ip.ln_evidence, ip.ess, ip.mean[1:], ip.cov[1:], ip.sigma[1:], ip.marginal("b"), ip.outside_mass, ip.median("a")[1:]):
        assert not np.any(np.isnan(arr))


def test_a_proposal_that_misses_is_low_ess():
    from victor_amd import GaussianProposal
    g = Gaussian(2)
    far = GaussianProposal(g.names, 6.0 * g.sigma, 0.25 * g.cov)
    ip = host(g, g.block, far, n=4096, seed=0)
    assert ip.status[0] == ip.LOW_ESS and 1 <= ip.ess[0] < 50 and ip.max_weight_share[0] > 0.02
    assert host(g, g.block, far, n=4096, seed=0, min_ess=0.0).status[0] == ip.OK
    assert host(g, g.block, g.proposal(), n=4096, seed=0, min_ess=4000.0).status[0] == ip.LOW_ESS


def raiser(batch):
    raise AssertionError("a refused call reached the evaluator")


class PairedStub:
    paired_model = True

    def __len__(self):
        return 16


def test_every_refusal_comes_before_the_first_evaluation():
    from victor_amd import GaussianProposal
    from victor_amd.importance import importance_posterior
    from victor_amd.utils import InputError
    q3 = proposal3()

    def refused(match, block=BLOCK3, fit=None, device=False, q=q3, **kw):
        with pytest.raises(InputError, match=match):
            importance_posterior(fit, block, q, device=device, evaluate=raiser, **kw)
    refused("paired_model", realisations=PairedStub())
    refused("per-block", block=dict(BLOCK3, **{"a@1": BLOCK3["a"]}))
    refused("per-block", fixed={"b@0": 1.0})
    refused("leaves its prior box", ranges={"a": (-1.5, 0.0)})
    refused("finite a < b", ranges={"a": (0.5, 0.5)})
    refused("not sampled", ranges={"fixed_one": (0.0, 1.0)})
    refused("two different sampled", pairs=[("a", "fixed_one")])
    refused("two different sampled", pairs=[("a", "a")])
    refused("given twice", pairs=[("a", "b"), ("b", "a")])
    refused("1 .. 1024", bins=0)
    refused("1 .. 1024", bins={"a": 1025, "b": 4, "c": 3})
    refused("1 .. 1024", bins=2.5)
    refused("bins names", bins={"a": 4, "b": 4})
    refused("scalars", fixed={"fixed_one": np.array([1.0, 2.0])})
    refused("chunk", chunk=0)
    refused("chunk", chunk=65537)
    refused("n must be", n=0)
    refused("n must be", n=2.5)
    refused("seed", seed=-1)
    refused("min_ess", min_ess=-1.0)
    refused("definition route only", device=True)
    refused("the proposal names", q=GaussianProposal(["a", "b"], [0.0, 0.0], np.eye(2)))
    refused("a GaussianProposal is needed", q=None)
    refused("come together", q=None, sample=np.zeros((4, 3)))
    refused("come together", sample=np.zeros((4, 3)), ln_proposal=np.zeros(4))
    refused("sample must be", q=None, sample=np.zeros((4, 2)), ln_proposal=np.zeros(4))
    refused("must be finite", q=None, sample=np.full((4, 3), np.nan), ln_proposal=np.zeros(4))
    refused("no point of the sample lies inside", q=None, sample=np.full((4, 3), 9.0), ln_proposal=np.zeros(4))
    refused("no point of the sample lies inside", q=GaussianProposal(NAMES3, [50.0, 50.0, 50.0], 1e-4 * np.eye(3)))
    refused("cell offsets", n=4096, chunk=1, bins=1024, pairs=[("a", "b"), ("a", "c"), ("b", "c")])
    eleven = {f"q{j}": BLOCK3["a"] for j in range(11)}
    refused("at most 10", block=eleven, q=GaussianProposal(list(eleven), np.zeros(11), np.eye(11)))
    with pytest.raises(InputError, match="a fit or an evaluate"):
        importance_posterior(None, BLOCK3, q3)
    with pytest.raises(InputError, match="positive definite"):
        GaussianProposal(["a", "b"], [0, 0], [[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(InputError, match="dof"):
        GaussianProposal(["a"], [0], [[1.0]], dof=0)


def test_refusals_that_need_a_fit_come_before_any_device_call():
    """beta_interpolation='likelihood' on beta-dependent data, a column-less name, a per-block name and a joint fit: refused
    without a context (on a host without a GPU a device call would raise NativeError instead)."""
    import victor_amd
    from tests import cases
    from victor_amd.utils import InputError
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    params = cases.cobaya_info()["params"]
    names = [n for n, v in params.items() if isinstance(v, dict) and "prior" in v]
    q = victor_amd.GaussianProposal(names, [params[n]["ref"]["loc"] if isinstance(params[n].get("ref"), dict) else 0.5 * (params[n]["prior"]["min"] + params[n]["prior"]["max"])
                                            for n in names], np.diag([1e-4] * len(names)))
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        fit.importance_posterior(params, q, n=8, beta_interpolation="likelihood")
    with pytest.raises(InputError, match="per-block"):
        fit.importance_posterior(params, q, n=8, fixed={"sigma_v@0": 380.0})
    with pytest.raises(InputError, match="no column of its own"):
        fit.importance_posterior(dict(params, nonsense={"prior": {"min": 0.0, "max": 1.0}}), q, n=8)
    assert not hasattr(victor_amd.JointFit, "importance_posterior")


# ------------------------------------------------------------------ 4. the surface ------------------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), f"include/victor_hip.h does not declare {name}"
        assert name in N.SYMBOLS, name
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert N.SYMBOLS["vk_is_run"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int64])
    assert N.SYMBOLS["vk_is_rows"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, dp])
    assert N.SYMBOLS["vk_is_result"] == (C.c_int, [C.c_void_p, dp, lp, lp, dp, dp, dp, dp, dp, dp, dp, dp])
    assert N.SYMBOLS["vk_is_create"][1][2:5] == [C.c_int32, ip, C.c_int64] and len(N.SYMBOLS["vk_is_create"][1]) == 21
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_importance.h")).read()
    assert "hip/hip_runtime.h" not in src and "asm" not in src and "fp contract(off)" in src and '#include "vk_grid.h"' in src
    kernels = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_kernel_importance.h")).read()
    assert "atomic" not in kernels.replace("no atomics", "") and "__shared__" not in kernels.split("vk_is_accumulate_kernel(IsArgs a)")[1]


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
    a = inspect.signature(victor_amd.CCFFit.importance_posterior)
    b = inspect.signature(victor_amd.Realisations.importance_posterior)
    assert a == b
    assert list(a.parameters) == ["self", "params", "q", "n", "seed", "fixed", "prior", "bins", "ranges", "pairs", "chunk", "min_ess",
                                  "device", "evaluate", "sample", "ln_proposal", "kwargs"]
    assert a.parameters["n"].default == 16384 and a.parameters["bins"].default == 64 and a.parameters["min_ess"].default == 50.0
    assert a.parameters["device"].default is True and a.parameters["chunk"].default is None
    ip = victor_amd.ImportancePosterior
    assert (ip.OK, ip.LOW_ESS, ip.NO_FINITE) == (0, 1, 2)
