"""Posterior-predictive sums of an importance sample (rule 6 of victor_amd/importance.py, vk_is_set_predictive) without a GPU: the
definition against a brute-force ``np.longdouble`` evaluation of the weighted sums; the tile and index rules and the terms of
victor_amd/csrc/vk_is_predict.h compiled on their own under g++ against NumPy, bit for bit; the read-out against closed forms;
the refusals; the C ABI's surface; and ``predictive=None`` leaving every array of a run as it was.

The bounds (:func:`predictive_bound`), derived as tests/test_importance.py derives its own, u = 2^-53, relative to the sum of
the ABSOLUTE terms A of an accumulator with T terms over C chunks.  Two correct evaluations see identical arguments of exp and
differ in exp itself, 7 u together (8 u with slack): a term's weight differs by 8 u, each of the C rescale products by 7 u + 1 u
for its own rounding: ``8 (C + 1) u``, the start of tests/test_importance.py's bound.  What rule 6 adds to a term:

* ``v = T - pivot`` is rounded, 1 u of |v|; ``w v`` is rounded, 1 u: ``+ 2 u`` for ``pt`` and for the first sum of each
  deviance pair;
* ``(w v) v`` holds v twice and one product more: ``+ 4 u`` for ``ptt`` and the second sums.

The additions: a sum of T terms in ANY order errs by at most ``T u`` of A (each term meets at most T - 1 roundings).  Against
an extended-precision reference only the route under test adds in float64: ``(8 (C + 1) + k + T) u``, k = 2 or 4.  Between the
two routes - the definition in increasing g, the device in slices - both add, and a term of the device route meets at most the
additions of its slice, the 3 of the slice combine and one per chunk: ``(8 (C + 1) + k + T + (T + C + 3)) u``.  A is computed
from the reference's own weights (it is a scale: its own rounding is of second order).
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import tolerances
from tests.test_chains import same_bytes
from tests.test_importance import BLOCK3, EXACT, SUMS, Gaussian, PairedStub, layout_of, proposal3, raiser, small_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_is_set_predictive", "vk_is_predictive")
PRED = ("pt", "ptt", "dev")


def predictive_bound(second, n_chunks, n_terms, two_routes=False):
    """Relative bound, against the sum of the absolute terms, on a first (``second=False``) or second sum of rule 6 with
    ``n_terms`` terms over ``n_chunks`` chunks (module docstring)."""
    k = 4.0 if second else 2.0
    adds = n_terms + (n_terms + n_chunks + 3.0 if two_routes else 0.0)
    return (8.0 * (n_chunks + 1) + k + adds) * tolerances.U


def brute_force(lnpost, theory, chi2, lnl):
    """Rule 6 with no chunks, in ``np.longdouble``: ``(pivot_t, pivots, sums, absolute sums)`` with sums ``pt``, ``ptt`` (R, N)
    and ``dev`` (4, R) in units of the weights under the final maximum."""
    ld = np.longdouble
    lnpost = np.where(np.isfinite(lnpost), lnpost, -np.inf)
    M = lnpost.max(axis=0)
    live = M > -np.inf
    with np.errstate(invalid="ignore"):
        w = np.where(live[None, :], np.exp((lnpost - np.where(live, M, 0.0)).astype(ld)), ld(0))       # (G, R)
    clean = lambda v: np.where(np.isfinite(v), v, 0.0)
    pivot_t, pivots = clean(theory[0]), np.stack([clean(chi2[0]), clean(lnl[0])])
    R, N = lnpost.shape[1], theory.shape[1]
    out = {n: np.zeros(s, dtype=ld) for n, s in (("pt", (R, N)), ("ptt", (R, N)), ("dev", (4, R)))}
    absolute = {n: np.zeros_like(v) for n, v in out.items()}
    for g in range(len(lnpost)):
        on = w[g] > 0
        if not np.any(on):
            continue
        v = (theory[g].astype(ld) - pivot_t)[None, :]
        wv = np.where(on[:, None], w[g][:, None] * np.where(np.isfinite(v), v, 0), 0)
        for name, term in (("pt", wv), ("ptt", wv * np.where(np.isfinite(v), v, 0))):
            out[name] += term
            absolute[name] += np.abs(term)
        for j, (values, pivot) in enumerate(((chi2[g], pivots[0]), (lnl[g], pivots[1]))):
            a = np.where(on, values, 0.0).astype(ld) - np.where(on, pivot, 0.0)
            wa = w[g] * a
            for i, term in ((2 * j, wa), (2 * j + 1, wa * a)):
                out["dev"][i] += term
                absolute["dev"][i] += np.abs(term)
    return pivot_t, pivots, out, absolute


def assert_predictive(acc, want, absolute, n_chunks, n_terms, what, two_routes=False, extra=None):
    """``acc`` (a Sums with rule 6's arrays) against the reference sums at the bound; ``extra``: name -> an absolute allowance
    on top (the GPU tests' theory tolerance).  Records and returns the worst margin."""
    worst = 0.0
    for name in PRED:
        got = np.asarray(getattr(acc, name), dtype=np.longdouble)
        assert got.shape == want[name].shape and np.all(np.isfinite(got)), (what, name)
        second = np.zeros(got.shape, dtype=bool)
        if name == "ptt":
            second[...] = True
        if name == "dev":
            second[1::2] = True
        rel = np.where(second, predictive_bound(True, n_chunks, n_terms, two_routes), predictive_bound(False, n_chunks, n_terms, two_routes))
        bound = rel * np.abs(absolute[name]).astype(np.float64) * (1.0 + 64 * tolerances.U)
        if extra is not None:
            bound = bound + extra[name]
        diff = np.abs(got - want[name]).astype(np.float64)
        ratio = np.where(bound > 0, diff / np.where(bound > 0, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
    tolerances._record(f"importance predictive sums {what}", worst)
    assert worst <= 1.0, (what, worst)
    return worst


# ------------------------------------------------------------------ 1. the definition against brute force ------------------
def synthetic(G, R, N, seed):
    """lnL (G, R) of :func:`tests.test_importance.small_sample` (ties, -inf, NaN; problem 1 fails everywhere, problem 2 in the
    first half) with problem 3's maximum rising in every chunk, point 0 failed for every problem with a theory entry that is not
    finite (its pivot reads 0), and point 5 failed with NaN in everything it holds."""
    x, v = small_sample(G, 2, R, seed)
    rng = np.random.default_rng(seed + 100)
    v[:, 3] = -25.0 + 24.0 * np.arange(G) / G + 0.3 * rng.random(G)
    v[0, :] = -np.inf
    v[5, :] = np.nan
    theory = 1.0 + 0.2 * rng.standard_normal((G, N)) + 0.05 * np.arange(N)[None, :]
    theory[0, 2] = np.inf
    theory[5, :] = np.nan
    with np.errstate(invalid="ignore"):
        chi2 = np.where(np.isfinite(v), -2.0 * v + 3.0 * np.arange(R)[None, :], np.inf)
    chi2[5, :] = np.nan
    return x, v, theory, chi2


def run_synthetic(x, v, theory, chi2, chunk, with_theory=True):
    from victor_amd.importance import Lists, Sample, run_definition
    layout = layout_of(2)
    G = len(x)
    rng = np.random.default_rng(7)
    sample = Sample(x, x.mean(axis=0), 0.1 * rng.standard_normal(G), G + 3, np.zeros(2), np.ones(2), None)
    lists = Lists(layout, sample.x, chunk)
    cuts = iter(range(0, G, chunk))
    at = {}

    def values(xc):
        at["g0"] = g0 = next(cuts)
        sl = slice(g0, g0 + len(xc))
        return (v[sl], chi2[sl]) if with_theory else v[sl]

    def vectors(xc):
        return theory[at["g0"]:at["g0"] + len(xc)]
    acc, _ = run_definition(layout, sample, lists, v.shape[1], values, vectors if with_theory else None)
    return acc, sample, lists


@pytest.mark.parametrize("chunk", [1, 4, 7, 23, 64])
def test_definition_against_brute_force(chunk):
    G, R, N = 23, 5, 6
    x, v, theory, chi2 = synthetic(G, R, N, 3)
    acc, sample, lists = run_synthetic(x, v, theory, chi2, chunk)
    assert acc.n_finite[1] == 0 and acc.n_finite[3] == G - 2 and acc.arg_max[3] > G - chunk - 2      # (rises to the last chunk)
    assert not np.any(np.isfinite(v[0])) and (chunk > 10 or v[chunk, 2] == -np.inf)      # chunks that start with -inf, a later one too
    pivot_t, pivots, want, absolute = brute_force(v + sample.lno[:, None], theory, chi2, v)
    assert same_bytes(acc.pivot_t, pivot_t) and same_bytes(acc.pivots, pivots)
    assert acc.pivot_t[2] == 0.0 and np.all(acc.pivots == 0.0) and np.all(acc.pivot_t[[0, 1, 3]] != 0.0)
    assert np.all(acc.pt[1] == 0) and np.all(acc.ptt[1] == 0) and np.all(acc.dev[:, 1] == 0)       # no finite point: zeros, no NaN
    assert_predictive(acc, want, absolute, lists.n_chunks, G, f"definition against brute force, chunk {chunk}")
    # the weighted mean of problem 3 is a number one can check by eye: between the theory's extremes
    m = acc.pivot_t[1] + acc.pt[3, 1] / acc.total[3]
    assert np.nanmin(theory[1:, 1]) < m < np.nanmax(theory[1:, 1])


def test_predictive_none_changes_nothing():
    G, R, N = 23, 5, 6
    x, v, theory, chi2 = synthetic(G, R, N, 3)
    with_sums, _, _ = run_synthetic(x, v, theory, chi2, 7)
    plain, _, _ = run_synthetic(x, v, theory, chi2, 7, with_theory=False)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(with_sums, name), getattr(plain, name)), name
    for name in PRED + ("pivot_t", "pivots"):
        assert hasattr(with_sums, name) and not hasattr(plain, name), name
    g = Gaussian(2)
    from victor_amd.importance import importance_posterior
    ip = importance_posterior(None, g.block, g.proposal(), n=256, device=False, evaluate=g)
    again = importance_posterior(None, g.block, g.proposal(), n=256, device=False, evaluate=g, predictive=None)
    assert ip.predictive is None and again.predictive is None and not hasattr(ip.raw, "pt")
    for name in EXACT + SUMS:
        assert same_bytes(getattr(ip.raw, name), getattr(again.raw, name)), name


# ------------------------------------------------------------------ 2. the shared header under g++ -------------------------
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vk_is_predict.h"

// argv: n R N first in out.  in: w [n][R] | T [n][N] | factor [R] | pivot_t [N] | pt [N][R] | ptt [N][R].
// out: pt [N][R] | ptt [N][R] | pivot_t [N] | visits [N][R] | slices [kSlices + 1] | pr, groups, entry tiles, problem tiles
int main(int argc, char** argv) {
  using namespace vkisp;
  if (argc != 7) return 2;
  const int n = atoi(argv[1]), R = atoi(argv[2]), N = atoi(argv[3]), first = atoi(argv[4]);
  std::vector<double> w((size_t)n * R), T((size_t)n * N), factor(R), pivot_t(N), pt((size_t)N * R), ptt((size_t)N * R), visits((size_t)N * R, 0.0);
  FILE* fi = fopen(argv[5], "rb");
  if (!fi) return 3;
  bool ok = fread(w.data(), 8, w.size(), fi) == w.size() && fread(T.data(), 8, T.size(), fi) == T.size() &&
            fread(factor.data(), 8, R, fi) == (size_t)R && fread(pivot_t.data(), 8, N, fi) == (size_t)N &&
            fread(pt.data(), 8, pt.size(), fi) == pt.size() && fread(ptt.data(), 8, ptt.size(), fi) == ptt.size();
  fclose(fi);
  if (!ok) return 3;
  const int pr = problems_per_wave(R);
  std::vector<double> part((size_t)kSlices * 2 * kTile * kWave);
  const int kPart = 2 * kTile * kWave;
  for (int rtile = 0; rtile < problem_tiles(R, pr); ++rtile)
    for (int etile = 0; etile < entry_tiles(N, pr); ++etile) {
      double piv[kWave][kTile];
      for (int slice = 0; slice < kSlices; ++slice)
        for (int lane = 0; lane < kWave; ++lane) {
          const int r = problem_of(rtile, pr, lane), k0 = first_entry(etile, pr, lane);
          double s1[kTile] = {}, s2[kTile] = {};
          int kk[kTile];
          for (int u = 0; u < kTile; ++u) {
            kk[u] = k0 + u < N ? k0 + u : N - 1;
            piv[lane][u] = first ? pivot_of(T[kk[u]]) : pivot_t[kk[u]];
          }
          if (r < R)
            for (int i = slice_begin(n, slice); i < slice_begin(n, slice + 1); ++i) {
              const double wi = w[(size_t)i * R + r];
              for (int u = 0; u < kTile; ++u) add(s1[u], s2[u], wi > 0.0, wi, T[(size_t)i * N + kk[u]], piv[lane][u]);
            }
          for (int u = 0; u < kTile; ++u) {
            part[(size_t)slice * kPart + u * kWave + lane] = s1[u];
            part[(size_t)slice * kPart + (kTile + u) * kWave + lane] = s2[u];
          }
        }
      for (int lane = 0; lane < kWave; ++lane) {
        const int r = problem_of(rtile, pr, lane), k0 = first_entry(etile, pr, lane);
        for (int u = 0; u < kTile; ++u) {
          if (r >= R || k0 + u >= N) continue;
          const size_t at = (size_t)(k0 + u) * R + r;
          pt[at] = combine(first ? 0.0 : pt[at], factor[r], part.data() + u * kWave + lane, kPart);
          ptt[at] = combine(first ? 0.0 : ptt[at], factor[r], part.data() + (kTile + u) * kWave + lane, kPart);
          visits[at] += 1.0;
          if (first && r == 0) pivot_t[k0 + u] = piv[lane][u];
        }
      }
    }
  FILE* fo = fopen(argv[6], "wb");
  if (!fo) return 3;
  fwrite(pt.data(), 8, pt.size(), fo);
  fwrite(ptt.data(), 8, ptt.size(), fo);
  fwrite(pivot_t.data(), 8, N, fo);
  fwrite(visits.data(), 8, visits.size(), fo);
  for (int s = 0; s <= kSlices; ++s) {
    const double b = slice_begin(n, s);
    fwrite(&b, 8, 1, fo);
  }
  const double shape[4] = {(double)pr, (double)groups(pr), (double)entry_tiles(N, pr), (double)problem_tiles(R, pr)};
  fwrite(shape, 8, 4, fo);
  fclose(fo);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("is_predict_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    done = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "victor_amd", "csrc"),
                           str(src), "-o", str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr

    def run(n, R, N, first, arrays):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        done = subprocess.run([str(exe), str(n), str(R), str(N), str(int(first)), str(fin), str(fout)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        return np.fromfile(str(fout), dtype=np.float64)
    return run


def numpy_mapping(w, T, factor, pivot_t, pt, ptt, first):
    """The header's order in NumPy: per slice the terms one at a time from zero, the slices in order, then ``acc f + p``."""
    n, R = w.shape
    N = T.shape[1]
    cuts = [n * s // 4 for s in range(5)]
    if first:
        pivot_t = np.where(np.isfinite(T[0]), T[0], 0.0)
        pt, ptt = np.zeros_like(pt), np.zeros_like(ptt)
    out1, out2 = np.empty((N, R)), np.empty((N, R))
    for k in range(N):
        for r in range(R):
            parts = []
            for s in range(4):
                s1 = s2 = np.float64(0.0)
                for i in range(cuts[s], cuts[s + 1]):
                    if w[i, r] > 0:
                        v = T[i, k] - pivot_t[k]
                        wv = w[i, r] * v
                        s1, s2 = s1 + wv, s2 + wv * v
                parts.append((s1, s2))
            for out, j, acc in ((out1, 0, pt), (out2, 1, ptt)):
                p = ((parts[0][j] + parts[1][j]) + parts[2][j]) + parts[3][j]
                out[k, r] = acc[k, r] * factor[r] + p
    return out1, out2, pivot_t, cuts


@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("n,N", [(1, 1), (7, 13), (10, 8), (67, 80)])
def test_header_against_numpy_term_by_term(driver, n, N, R):
    """n not a multiple of the slice count, N not a multiple of the entry tile, R below, between and past the powers of two: every
    (entry, problem) is combined exactly once, and the sums are NumPy's bit for bit, in a first chunk and in a later one."""
    rng = np.random.default_rng(1000 * n + 10 * N + R)
    w = np.exp(-8.0 * rng.random((n, R)))
    w[rng.random((n, R)) < 0.25] = 0.0
    T = 1.0 + 0.3 * rng.standard_normal((n, N))
    dead = np.flatnonzero(~np.any(w > 0, axis=1))
    T[dead] = np.nan                                              # a point nobody weighs may hold anything
    if n > 1:
        w[0, :] = 0.0
        T[0, N // 2] = np.inf                                     # (a pivot entry that is not finite reads 0)
    factor = np.where(rng.random(R) < 0.5, 1.0, np.exp(-rng.random(R)))
    pivot_t, pt, ptt = 1.0 + rng.standard_normal(N), rng.standard_normal((N, R)), 5.0 + rng.random((N, R))
    for first in (True, False):
        out = driver(n, R, N, first, [w, T, factor, pivot_t, pt, ptt])
        NR = N * R
        got1, got2, got_piv = out[:NR].reshape(N, R), out[NR:2 * NR].reshape(N, R), out[2 * NR:2 * NR + N]
        visits, tail = out[2 * NR + N:3 * NR + N], out[3 * NR + N:]
        want1, want2, want_piv, cuts = numpy_mapping(w, T, factor, pivot_t, pt, ptt, first)
        assert np.all(visits == 1.0), (n, N, R)
        assert same_bytes(got1, want1) and same_bytes(got2, want2) and same_bytes(got_piv, want_piv), (n, N, R, first)
        assert np.all(np.isfinite(got1)) and np.all(np.isfinite(got2))
        assert list(tail[:5]) == cuts and cuts[0] == 0 and cuts[4] == n
        pr = int(tail[5])
        assert pr == min(64, 1 << (R - 1).bit_length()) and tail[6] == 64 // pr
        assert tail[7] == -(-N // (4 * (64 // pr))) and tail[8] == -(-R // pr)


# ------------------------------------------------------------------ 3. the read-out ----------------------------------------
@pytest.mark.parametrize("d", [2, 4])
def test_gaussian_read_out_against_closed_forms(d):
    """lnL = -chi2 / 2 with chi2 = x^T C^-1 x and a theory vector linear in x: the band is ``b`` with scatter ``sqrt(diag(A C
    A^T))``, mean chi2 = d, var chi2 = 2 d, so p_d = d and p_v = d - each within 4 of its Monte Carlo error from ``ess``."""
    from victor_amd.importance import ImportancePosterior, SamplePredictive, importance_posterior, run_definition
    g = Gaussian(d)
    rng = np.random.default_rng(d)
    N = 7
    A, b = rng.standard_normal((N, d)), 1.0 + rng.random(N)
    ip0 = importance_posterior(None, g.block, g.proposal(), n=8192, seed=1, device=False, evaluate=g, chunk=1000)

    def values(x):
        lnl = g({n: x[:, j] for j, n in enumerate(g.names)})
        return lnl, -2.0 * lnl
    acc, pacc = run_definition(ip0._layout, ip0._sample, ip0._lists, 1, values, lambda x: b[None, :] + x @ A.T)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(acc, name), getattr(ip0.raw, name)), name
    ip = ImportancePosterior(ip0._layout, ip0._sample, ip0._lists, acc, pacc, 50.0)
    lnl_at = g({n: ip.mean[:, j] for j, n in enumerate(g.names)})
    p = SamplePredictive(acc, ip._ok, [slice(0, N)], [([0], N)], -2.0 * lnl_at, lnl_at)
    ess = ip.ess[0]
    assert ess > 1000
    scatter = np.sqrt(np.einsum("ki,ij,kj->k", A, g.cov, A))
    assert p.mean.shape == p.std.shape == (1, N)
    assert np.all(np.abs(p.mean[0] - b) <= 4 * scatter / np.sqrt(ess)), (p.mean[0] - b, scatter / np.sqrt(ess))
    # the variance of a variance estimate of a Gaussian: 2 sigma^4 / ess
    assert np.all(np.abs(p.std[0] ** 2 - scatter ** 2) <= 4 * np.sqrt(2.0 / ess) * scatter ** 2)
    # the moments of chi2 ~ chi-square with d degrees of freedom: mean d (variance 2 d), variance 2 d (whose own variance
    # is mu_4 - mu_2^2 = 48 d + 12 d^2 - 4 d^2 = 48 d + 8 d^2)
    err_mean, err_var = np.sqrt(2.0 * d / ess), np.sqrt((48.0 * d + 8.0 * d * d) / ess)
    assert abs(p.mean_chi2[0] - d) <= 4 * err_mean and abs(p.var_chi2[0] - 2 * d) <= 4 * err_var
    assert abs(p.mean_lnl[0] + 0.5 * p.mean_chi2[0]) < 1e-12 and abs(p.var_lnl[0] - 0.25 * p.var_chi2[0]) < 1e-12
    # D(mean position) = chi2 at a point within sigma / sqrt(ess) of 0: of order d / ess
    assert 0 <= p.chi2_at_mean[0] <= 16.0 * d / ess
    assert abs(p.p_d[0] - d) <= 4 * err_mean + 16.0 * d / ess, (p.p_d[0], d, err_mean)
    assert abs(p.p_v[0] - d) <= 4 * err_var / 2
    assert same_bytes(p.dic, -2.0 * p.mean_lnl + p.p_d) and same_bytes(p.p_v, 2.0 * p.var_lnl)
    assert set(p.multipoles) == {0} and same_bytes(p.multipoles[0][0], p.mean) and p.blocks == [slice(0, N)]
    assert set(p.state) == {"pivot_t", "sum_t", "sum_tt", "pivots", "deviance", "total"} and p.state["sum_t"].shape == (1, N)
    # the weighted variance is the one ip.cov uses: the band of a vector that is x itself reads ip.mean and ip.cov
    acc2, _ = run_definition(ip0._layout, ip0._sample, ip0._lists, 1, values, lambda x: x)
    p2 = SamplePredictive(acc2, ip._ok, [slice(0, d)], [([0], d)])
    assert np.allclose(p2.mean[0], ip.mean[0], rtol=0, atol=1e-13) and np.allclose(p2.std[0], ip.sigma[0], rtol=1e-9)
    assert np.all(np.isnan(p2.p_d)) and np.all(np.isnan(p2.dic))               # (no likelihood at the mean was given)


def test_a_problem_without_a_finite_point_reads_nan_and_blocks_are_sliced():
    from victor_amd.importance import SamplePredictive
    G, R, N = 23, 5, 6
    x, v, theory, chi2 = synthetic(G, R, N, 3)
    acc, _, _ = run_synthetic(x, v, theory, chi2, 7)
    ok = acc.n_finite > 0
    p = SamplePredictive(acc, ok, [slice(0, 4), slice(4, 6)], [([0, 2], 2), ([0], 2)], np.ones(R), -0.5 * np.ones(R))
    assert not ok[1] and ok[0] and p.multipoles is None
    for name in ("mean", "std", "mean_chi2", "var_chi2", "mean_lnl", "var_lnl", "chi2_at_mean", "lnl_at_mean", "p_d", "p_v", "dic"):
        a = getattr(p, name)
        assert np.all(np.isnan(a[1])) and np.all(np.isfinite(a[[0, 2, 3, 4]])), name
    first, second = p.multipoles_of(0), p.multipoles_of(1)
    assert set(first) == {0, 2} and set(second) == {0}
    assert same_bytes(first[2][0], p.mean[:, 2:4]) and same_bytes(second[0][1], p.std[:, 4:6])
    from victor_amd.utils import InputError
    with pytest.raises(InputError, match="outside 0 .. 1"):
        p.multipoles_of(2)


# ------------------------------------------------------------------ 4. refusals and the surface ----------------------------
def test_refusals_come_before_any_evaluation_and_any_device_call():
    import victor_amd
    from tests import cases
    from victor_amd.importance import importance_posterior
    from victor_amd.predictive import PredictiveError, resolve_predictive, resolve_sample_predictive
    from victor_amd.utils import InputError
    assert issubclass(PredictiveError, InputError) and issubclass(PredictiveError, ValueError)
    q3 = proposal3()
    for bad in (False, 1, "yes", 0):
        with pytest.raises(PredictiveError, match="must be None or True"):
            importance_posterior(None, BLOCK3, q3, device=False, evaluate=raiser, predictive=bad)
    with pytest.raises(PredictiveError, match="needs a fit"):
        importance_posterior(None, BLOCK3, q3, device=False, evaluate=raiser, predictive=True)
    assert resolve_sample_predictive(None, "x") is False and resolve_sample_predictive(True, "x") is True
    with pytest.raises(PredictiveError, match="joint fits"):       # the chains' resolver is what it was
        resolve_predictive(True, "sample_chains", joint=True)
    # with a fit: every refusal of the call itself still comes first, and none reaches a context (a host without a GPU would
    # raise NativeError from a device call)
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    params = cases.cobaya_info()["params"]
    names = [n for n, v in params.items() if isinstance(v, dict) and "prior" in v]
    q = victor_amd.GaussianProposal(names, [0.5 * (params[n]["prior"]["min"] + params[n]["prior"]["max"]) for n in names],
                                    np.diag([1e-4] * len(names)))
    with pytest.raises(PredictiveError, match="must be None or True"):
        fit.importance_posterior(params, q, n=8, predictive="on")
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        fit.importance_posterior(params, q, n=8, predictive=True, beta_interpolation="likelihood")
    with pytest.raises(InputError, match="per-block"):
        fit.importance_posterior(params, q, n=8, predictive=True, fixed={"sigma_v@0": 380.0})
    with pytest.raises(PredictiveError, match="paired_model"):
        importance_posterior(fit, params, q, n=8, predictive=True, realisations=PairedStub())
    assert not hasattr(victor_amd.JointFit, "importance_posterior")


def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), f"include/victor_hip.h does not declare {name}"
        assert name in N.SYMBOLS, name
    dp = C.POINTER(C.c_double)
    assert N.SYMBOLS["vk_is_set_predictive"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert N.SYMBOLS["vk_is_predictive"] == (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp])
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_is_predict.h")).read()
    assert "hip/hip_runtime.h" not in src and "asm" not in src and "fp contract(off)" in src and '#include "vk_grid.h"' in src
    kernel = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_kernel_is_predict.h")).read()
    code = re.sub(r"//[^\n]*", "", kernel)
    assert "atomic" not in code and "asm" not in code and "IsArgs a" not in code and "struct IsPredictArgs" in code
    # the existing kernels and their argument struct are the parent's: the new kernel lives in a header of its own
    assert "IsPredictArgs" not in open(os.path.join(ROOT, "victor_amd", "csrc", "vk_kernel_importance.h")).read()
    makefile = open(os.path.join(ROOT, "victor_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"obj/\w+\.o", makefile.split("KERNELOBJS :=")[1].split("\n")[0])) == 7       # eight units with victor_hip


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.vk_is_set_predictive(None, 1) != 0 and lib.vk_is_predictive(None, None, None, None, None, None) != 0


def test_the_keyword_reaches_all_four_entry_points():
    import inspect

    import victor_amd
    from victor_amd import importance
    assert inspect.signature(importance.importance_posterior).parameters["predictive"].default is None
    for cls in (victor_amd.CCFFit, victor_amd.Realisations, victor_amd.JointRealisations):
        src = inspect.getsource(cls.importance_posterior)
        assert 'kwargs.pop("predictive", None)' in src and "predictive=predictive" in src, cls
