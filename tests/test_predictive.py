"""Posterior-predictive sums of the chains (victor_amd/predictive.py, vk_chain_set_predictive / vk_chain_predictive) without a
GPU: the rules of victor_amd/csrc/vk_predictive.h compiled on their own under g++ and driven with synthetic theory vectors,
accept counters and kept flags, against a NumPy ``longdouble`` restatement in this file and against ``PredictiveState`` - the hold
on a changed counter only, the rows of a stretch half-step, the pivot rule, the skip rule, cuts -; the read-out ``Predictive`` on
hand-made sums against NumPy on the samples; the refusals of the option; and the C ABI's surface.

Sums are held to the rounding bound of an n-term sum of their terms (the products may be contracted), not bit for bit:
``|d sum_t| <= (n + 1) u sum |v|`` (n - 1 additions and the rounding of v = t - pivot itself) and ``|d sum_tt| <= (n + 3) u sum
v^2`` (the rounding of v twice, of the product, and n - 1 additions), first order, u = 2^-53.  What is copied - ``held``, ``seen``,
the pivots, the counters - is compared exactly.
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_chain_set_predictive", "vk_chain_predictive")
U = 2.0 ** -53
LD = np.longdouble

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vk_predictive.h"

// run R W N resume    in: [state, if resume] then th0[C][N] chi2[C] lnl[C] (if not resume), then events until the input ends:
//                         half side M kept | th[M][N] | n_accept[C] | chi2[C] | lnl[C]
//                     out: the state  pivot_t sum_t sum_tt [R][N] | held [C][N] | dev [R][6] | n n_skipped [R] | seen [C]  (as doubles)
int main(int argc, char** argv) {
  if (argc != 7) return 3;
  const int R = atoi(argv[1]), W = atoi(argv[2]), N = atoi(argv[3]), resume = atoi(argv[4]);
  const size_t C = (size_t)R * W;
  FILE* fi = fopen(argv[5], "rb");
  FILE* fo = fopen(argv[6], "wb");
  if (!fi || !fo) return 2;
  fseek(fi, 0, SEEK_END);
  std::vector<double> in((size_t)ftell(fi) / sizeof(double));
  fseek(fi, 0, SEEK_SET);
  if (fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const size_t nd = vkpred::state_doubles(C, R, N), nc = vkpred::state_counters(C, R);
  if (nd != (C + 3 * (size_t)R) * N + 6 * (size_t)R || nc != C + 2 * (size_t)R) return 5;
  std::vector<double> d(nd, 0.0);
  std::vector<long long> k(nc, 0), acc(C, 0);
  vkpred::Predictive p{};
  p.on = 1, p.group = W, p.N = N;
  p.pivot_t = d.data(), p.sum_t = p.pivot_t + (size_t)R * N, p.sum_tt = p.sum_t + (size_t)R * N, p.held = p.sum_tt + (size_t)R * N;
  p.dev = p.held + C * N;
  p.n = k.data(), p.n_skipped = p.n + R, p.seen = p.n_skipped + R;
  const double* q = in.data();
  const double* end = q + in.size();
  if (resume) {
    for (size_t i = 0; i < nd; ++i) d[i] = *q++;
    for (size_t i = 0; i < nc; ++i) k[i] = (long long)*q++;
  } else {
    vkpred::hold(p, q, acc.data(), (int)C, 0, 0, true);
    q += C * N;
    vkpred::pivots(p, q, q + C, R);
    q += 2 * C;
  }
  while (q < end) {
    const int half = (int)q[0], side = (int)q[1], M = (int)q[2], kept = (int)q[3];
    q += 4;
    const double* th = q;
    q += (size_t)M * N;
    for (size_t c = 0; c < C; ++c) acc[c] = (long long)*q++;
    vkpred::hold(p, th, acc.data(), M, half, side, false);
    if (kept) vkpred::accumulate(p, q, q + C, R);
    q += 2 * C;
  }
  fwrite(d.data(), sizeof(double), nd, fo);
  for (size_t i = 0; i < nc; ++i) {
    const double v = (double)k[i];
    fwrite(&v, sizeof(double), 1, fo);
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
    d = tmp_path_factory.mktemp("predictive_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(R, W, N, arrays, resume=False):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        subprocess.run([str(exe), str(R), str(W), str(N), str(int(resume)), str(fin), str(fout)], check=True)
        return np.fromfile(str(fout), dtype=np.float64)
    return run


def unpack(raw, R, W, N):
    C_ = R * W
    out, at = {}, 0
    for name, shape in (("pivot_t", (R, N)), ("sum_t", (R, N)), ("sum_tt", (R, N)), ("held", (C_, N)), ("deviance", (R, 6)),
                        ("n", (R,)), ("n_skipped", (R,)), ("seen", (C_,))):
        size = int(np.prod(shape))
        out[name] = raw[at:at + size].reshape(shape)
        at += size
    assert at == len(raw)
    return out


class Script:
    """A synthetic run of R problems of W chains with theory vectors of N entries: a start and a list of events (half, side, rows'
    chains, kept, th (M, N), n_accept (C,), chi2 (C,), lnl (C,)) - what the hold and the accumulate see, launch after launch."""

    def __init__(self, R, W, N, start, events):
        self.R, self.W, self.N, self.start, self.events = R, W, N, start, events

    def packed(self, events=None, start=True):
        out = list(self.start) if start else []
        for half, side, chains, kept, th, acc, chi2, lnl in (self.events if events is None else events):
            out += [np.array([half, side, len(chains), kept], dtype=float), th, acc.astype(float), chi2, lnl]
        return out


def rows_of(C_, half, side):
    if half == 0:
        return np.arange(C_)
    i = np.arange(C_ // 2)
    return (2 * (i // half) + side) * half + i % half


def make_script(seed, R, W, N, steps, stretch, bad_start=False, inf_chain=None):
    """Accepts with probability 0.4 per moving chain; kept from step 3 on every second step; theory vectors about 1 +- 0.1 with a
    slope over the entries; chi2 about 60, lnl about -30.  ``bad_start``: entries of the first chain of problem 1 that are not
    finite at the start, and its chi2.  ``inf_chain``: a chain whose chi2 reads +inf on steps 4 .. 9."""
    rng = np.random.default_rng(seed)
    C_ = R * W
    th0 = 1.0 + 0.1 * rng.standard_normal((C_, N)) + np.linspace(0.0, 2.0, N)
    chi0, lnl0 = 60.0 + 5.0 * rng.standard_normal(C_), -30.0 + 2.5 * rng.standard_normal(C_)
    if bad_start:
        th0[W, 0], th0[W, N - 1], th0[W, N // 2] = np.nan, np.inf, -np.inf
        chi0[W] = np.inf
    acc, chi2, lnl = np.zeros(C_, dtype=np.int64), chi0.copy(), lnl0.copy()
    events = []
    for t in range(steps):
        kept = int(t >= 3 and (t - 3) % 2 == 0)
        for side in ((0, 1) if stretch else (0,)):
            chains = rows_of(C_, W // 2 if stretch else 0, side)
            th = 1.0 + 0.1 * rng.standard_normal((len(chains), N)) + np.linspace(0.0, 2.0, N)
            won = chains[rng.random(len(chains)) < 0.4]
            acc[won] += 1
            chi2[won] = 60.0 + 5.0 * rng.standard_normal(len(won))
            lnl[won] = -30.0 + 2.5 * rng.standard_normal(len(won))
            c2 = chi2.copy()
            if inf_chain is not None and 4 <= t <= 9:
                c2[inf_chain] = np.inf
            last = side == 1 or not stretch
            events.append((W // 2 if stretch else 0, side, chains, kept if last else 0, th, acc.copy(), c2, lnl.copy()))
    return Script(R, W, N, (th0, chi0, lnl0), events)


def restated(sc):
    """The rules in this file's own words, every sum in ``longdouble``: the state, and the sums of the terms' magnitudes the
    bounds are formed from."""
    R, W, N = sc.R, sc.W, sc.N
    C_ = R * W
    th0, chi0, lnl0 = sc.start
    held, seen = th0.copy(), np.zeros(C_, dtype=np.int64)
    first = np.arange(R) * W
    piv = lambda v: np.where(np.isfinite(v), v, 0.0)          # noqa: E731
    pivot_t, pc, pl = piv(held[first]), piv(chi0[first]), piv(lnl0[first])
    s1, s2, a1, a2 = (np.zeros((R, N), dtype=LD) for _ in range(4))
    dev, adev = np.zeros((R, 4), dtype=LD), np.zeros((R, 4), dtype=LD)
    n, skipped = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    for half, side, chains, kept, th, acc, chi2, lnl in sc.events:
        for i, c in enumerate(chains):
            if acc[c] != seen[c]:
                held[c], seen[c] = th[i], acc[c]
        if not kept:
            continue
        for r in range(R):
            for w in range(W):
                c = r * W + w
                if not (np.isfinite(chi2[c]) and np.isfinite(lnl[c])):
                    skipped[r] += 1
                    continue
                v = held[c].astype(LD) - pivot_t[r].astype(LD)
                s1[r] += v
                s2[r] += v * v
                a1[r] += np.abs(v)
                a2[r] += v * v
                a, b = LD(chi2[c]) - LD(pc[r]), LD(lnl[c]) - LD(pl[r])
                dev[r] += [a, a * a, b, b * b]
                adev[r] += [abs(a), a * a, abs(b), b * b]
                n[r] += 1
    return dict(pivot_t=pivot_t, pivot_chi2=pc, pivot_lnl=pl, sum_t=s1, sum_tt=s2, abs_t=a1, abs_tt=a2, dev=dev, abs_dev=adev, n=n,
                n_skipped=skipped, held=held, seen=seen)


def assert_state(got, want, what):
    """``got`` (a dict in the layout of ``unpack`` / ``PredictiveState.arrays``) against ``restated``."""
    for k in ("pivot_t", "held"):
        assert same_bytes(np.asarray(got[k], dtype=float), want[k]), (what, k)
    assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["n_skipped"], want["n_skipped"]), what
    if "seen" in got:
        assert np.array_equal(got["seen"], want["seen"]), what
    dev = np.asarray(got["deviance"], dtype=float)
    assert same_bytes(dev[:, 0], want["pivot_chi2"]) and same_bytes(dev[:, 1], want["pivot_lnl"]), what
    n = want["n"].astype(float)[:, None]
    for name, ref, mag, extra in (("sum_t", want["sum_t"], want["abs_t"], 1), ("sum_tt", want["sum_tt"], want["abs_tt"], 3)):
        diff = np.abs(np.asarray(got[name], dtype=LD) - ref).astype(float)
        bound = (n + extra) * U * mag.astype(float)
        assert np.all(diff <= bound), (what, name, float(np.max(diff / np.where(bound > 0, bound, 1.0))))
    extra = np.array([1, 3, 1, 3], dtype=float)
    diff = np.abs(dev[:, 2:].astype(LD) - want["dev"]).astype(float)
    bound = (n + extra) * U * want["abs_dev"].astype(float)
    assert np.all(diff <= bound), (what, "deviance", diff, bound)


def python_state(sc, events=None, state=None):
    """The same script through ``victor_amd.predictive.PredictiveState``."""
    from victor_amd.predictive import PredictiveState
    q = state
    if q is None:
        q = PredictiveState(sc.R, sc.W, sc.N)
        q.start(sc.start[0], np.zeros(sc.R * sc.W, dtype=np.int64), sc.start[1], sc.start[2])
    for half, side, chains, kept, th, acc, chi2, lnl in (sc.events if events is None else events):
        take = q.changed(chains, acc)
        q.hold(chains[take], th[take], acc)
        if kept:
            q.add(chi2, lnl)
    return q


# ------------------------------------------------------------------ 1. the header against the restatement --------------------
@pytest.mark.parametrize("stretch", [False, True], ids=["metropolis", "stretch"])
@pytest.mark.parametrize("R,W,N", [(3, 8, 5), (2, 6, 70), (1, 2, 1)])
def test_header_and_numpy_state_follow_the_rules(driver, stretch, R, W, N):
    """N = 70 is more than a wave of entries; W = 6 gives halves of 3; (1, 2, 1) is the smallest shape there is."""
    sc = make_script(R * 100 + N, R, W, N, 30, stretch)
    want = restated(sc)
    assert 0 < want["seen"].sum() < 30 * R * W and np.all(want["n"] == 14 * W) and not want["n_skipped"].any()
    got = unpack(driver(R, W, N, sc.packed()), R, W, N)
    assert_state(got, want, "g++")
    py = python_state(sc)
    assert_state(dict(py.arrays(), seen=py.seen), want, "PredictiveState")
    # without contraction (x86-64 at -O2 has no fma to contract into) the two are the same bytes
    for k in ("sum_t", "sum_tt", "deviance"):
        assert np.allclose(got[k], getattr(py, k), rtol=1e-13, atol=0.0), k


def test_hold_only_on_a_changed_counter(driver):
    """Every event offers every chain a fresh row; only the chains whose counter moved may take it - and a counter that moves by
    two, or down, is a change like any other."""
    R, W, N = 2, 4, 3
    sc = make_script(7, R, W, N, 12, False)
    half, side, chains, kept, th, acc, chi2, lnl = sc.events[5]
    acc = acc.copy()
    acc[2] += 2
    acc[5] -= 1
    sc.events[5] = (half, side, chains, kept, th, acc, chi2, lnl)
    for i in range(6, 12):                                     # (later counters follow on from the edited ones)
        e = list(sc.events[i])
        e[5] = e[5].copy()
        e[5][2] += 2
        e[5][5] -= 1
        sc.events[i] = tuple(e)
    want = restated(sc)
    got = unpack(driver(R, W, N, sc.packed()), R, W, N)
    assert same_bytes(got["held"], want["held"]) and np.array_equal(got["seen"], want["seen"])
    # stated directly: held[c] is the row of the LAST event at which c's counter differed from the one before
    for c in range(R * W):
        last, before = None, 0
        for e in sc.events:
            if e[5][c] != before:
                last, before = e[4][c], e[5][c]
        assert same_bytes(got["held"][c], sc.start[0][c] if last is None else last), c


def test_rows_of_a_stretch_half_go_to_the_moving_walkers(driver):
    """Half-step ``side`` of ensembles of W = 6: row i serves walker (2 (i // 3) + side) 3 + i % 3.  Every row carries its own
    index in its entries and every moving walker accepts, so ``held`` names the row each walker took."""
    from victor_amd.predictive import stretch_chains
    R, W, N = 3, 6, 2
    C_, M = R * W, R * W // 2
    start = (np.full((C_, N), -1.0), np.full(C_, 60.0), np.full(C_, -30.0))
    acc = np.zeros(C_, dtype=np.int64)
    events = []
    for side in (0, 1):
        chains = stretch_chains(M, W // 2, side)
        assert np.array_equal(chains, rows_of(C_, W // 2, side))
        acc = acc.copy()
        acc[chains] += 1
        th = np.repeat(np.arange(M, dtype=float) + 100.0 * side, N).reshape(M, N)
        events.append((W // 2, side, chains, 0, th, acc, start[1], start[2]))
    sc = Script(R, W, N, start, events)
    got = unpack(driver(R, W, N, sc.packed()), R, W, N)
    want = np.empty(C_)
    for r in range(R):
        for w in range(W):
            want[r * W + w] = r * 3 + w % 3 + (100.0 if w >= 3 else 0.0)
    assert np.array_equal(got["held"][:, 0], want) and np.array_equal(got["held"][:, 1], want)
    assert np.array_equal(got["seen"], np.ones(C_))


def test_pivot_rule_with_a_start_that_is_not_finite(driver):
    R, W, N = 3, 4, 9
    sc = make_script(11, R, W, N, 20, False, bad_start=True)
    want = restated(sc)
    got = unpack(driver(R, W, N, sc.packed()), R, W, N)
    assert got["pivot_t"][1, 0] == 0.0 and got["pivot_t"][1, N - 1] == 0.0 and got["pivot_t"][1, N // 2] == 0.0
    assert got["deviance"][1, 0] == 0.0 and got["deviance"][1, 1] == sc.start[2][W]          # chi2 was +inf, lnl finite
    assert same_bytes(got["pivot_t"][0], sc.start[0][0]) and same_bytes(got["pivot_t"][2], sc.start[0][2 * W])
    assert_state(got, want, "pivots")
    assert_state(dict(python_state(sc).arrays()), want, "PredictiveState")
    assert np.all(np.isfinite(got["sum_t"][0])) and np.all(np.isfinite(got["sum_t"][2]))


def test_a_chain_that_is_not_finite_is_skipped_and_sums_nothing(driver):
    R, W, N = 2, 4, 6
    sc = make_script(13, R, W, N, 20, False, inf_chain=5)
    clean = make_script(13, R, W, N, 20, False)
    want = restated(sc)
    assert want["n_skipped"].tolist() == [0, 3] and want["n"].tolist() == [9 * W, 9 * W - 3]      # kept steps 5, 7, 9 of 3, 5, .. 19
    got = unpack(driver(R, W, N, sc.packed()), R, W, N)
    assert_state(got, want, "skip")
    assert_state(dict(python_state(sc).arrays()), want, "PredictiveState")
    assert np.all(np.isfinite(got["sum_t"])) and np.all(np.isfinite(got["sum_tt"])) and np.all(np.isfinite(got["deviance"]))
    # problem 0 never saw it: the same bytes as the run without the infinity
    ref = unpack(driver(R, W, N, clean.packed()), R, W, N)
    for k in ("sum_t", "sum_tt", "deviance"):
        assert same_bytes(got[k][0], ref[k][0]), k
        assert not same_bytes(got[k][1], ref[k][1]), k


@pytest.mark.parametrize("stretch", [False, True], ids=["metropolis", "stretch"])
def test_a_cut_run_gives_the_same_bytes(driver, stretch):
    """70 steps against 40 + 30, the second piece resumed from the state the first left."""
    R, W, N = 2, 4, 7
    sc = make_script(17, R, W, N, 70, stretch)
    per = 2 if stretch else 1
    whole = driver(R, W, N, sc.packed())
    first = driver(R, W, N, sc.packed(sc.events[:40 * per]))
    second = driver(R, W, N, [first] + sc.packed(sc.events[40 * per:], start=False), resume=True)
    assert same_bytes(second, whole) and not same_bytes(first, whole)
    q = python_state(sc, sc.events[:40 * per])
    part = q.arrays()
    q = python_state(sc, sc.events[40 * per:], q)
    full = python_state(sc).arrays()
    assert all(same_bytes(q.arrays()[k], full[k]) for k in full) and not same_bytes(part["sum_t"], full["sum_t"])


# ------------------------------------------------------------------ 2. the read-out ------------------------------------------
def sums_of(t, chi2, lnl):
    """The state (as ``PredictiveState.arrays``) of samples t (n, R, N), chi2, lnl (n, R), pivots at the first sample, every sum
    in longdouble and rounded once."""
    n, R, N = t.shape
    v = (t - t[0]).astype(LD)
    a, b = (chi2 - chi2[0]).astype(LD), (lnl - lnl[0]).astype(LD)
    dev = np.stack([chi2[0], lnl[0], a.sum(axis=0).astype(float), (a * a).sum(axis=0).astype(float), b.sum(axis=0).astype(float),
                    (b * b).sum(axis=0).astype(float)], axis=1)
    return dict(pivot_t=t[0].copy(), sum_t=v.sum(axis=0).astype(float), sum_tt=(v * v).sum(axis=0).astype(float), deviance=dev,
                n=np.full(R, n, dtype=np.int64), n_skipped=np.zeros(R, dtype=np.int64), held=np.zeros((R, N)))


def test_read_out_against_numpy_on_the_samples():
    from victor_amd.predictive import Predictive
    rng = np.random.default_rng(3)
    n, R, n_s = 500, 3, 7
    N = 3 * n_s
    t = 5.0 + 0.01 * rng.standard_normal((n, R, N)) * np.linspace(1.0, 3.0, N)          # a pivot far from zero, a small scatter
    chi2 = 60.0 + 5.0 * rng.standard_normal((n, R))
    lnl = -1000.0 - 0.5 * chi2
    at = -1000.0 - 0.5 * np.array([55.0, 56.0, 57.0])
    p = Predictive(sums_of(t, chi2, lnl), [0, 2, 4], n_s, chi2_at_mean=[55.0, 56.0, 57.0], lnl_at_mean=at)
    assert p.mean.shape == (R, N) and p.std.shape == (R, N) and p.n.tolist() == [n] * R
    tl = t.astype(LD)
    assert np.allclose(p.mean, tl.mean(axis=0).astype(float), rtol=1e-14, atol=0.0)
    assert np.allclose(p.std, tl.std(axis=0, ddof=1).astype(float), rtol=1e-10, atol=0.0)
    assert sorted(p.multipoles) == [0, 2, 4]
    for i, ell in enumerate((0, 2, 4)):
        m, s = p.multipoles[ell]
        assert m.shape == (R, n_s) and np.array_equal(m, p.mean[:, i * n_s:(i + 1) * n_s]) and np.array_equal(s, p.std[:, i * n_s:(i + 1) * n_s])
    assert np.allclose(p.mean_chi2, chi2.mean(axis=0), rtol=1e-13) and np.allclose(p.var_chi2, chi2.var(axis=0, ddof=1), rtol=1e-11)
    assert np.allclose(p.mean_lnl, lnl.mean(axis=0), rtol=1e-13) and np.allclose(p.var_lnl, lnl.var(axis=0, ddof=1), rtol=1e-11)
    D = -2.0 * lnl
    p_d = D.mean(axis=0) - (-2.0 * at)
    assert np.allclose(p.p_d, p_d, rtol=1e-10) and np.allclose(p.p_v, D.var(axis=0, ddof=1) / 2.0, rtol=1e-11)
    assert np.allclose(p.dic, D.mean(axis=0) + p_d, rtol=1e-12)
    assert np.allclose(p.p_d, chi2.mean(axis=0) - np.array([55.0, 56.0, 57.0]), rtol=1e-9)      # lnL = const - chi2 / 2
    assert np.array_equal(p.chi2_at_mean, [55.0, 56.0, 57.0]) and set(p.state) == {"pivot_t", "sum_t", "sum_tt", "deviance", "n", "n_skipped", "held"}


def test_read_out_is_nan_below_one_and_two_samples():
    from victor_amd.predictive import Predictive
    rng = np.random.default_rng(4)
    t, chi2 = rng.standard_normal((3, 3, 4)), rng.standard_normal((3, 3)) + 50.0
    q = sums_of(t, chi2, -0.5 * chi2)
    one = sums_of(t[:1], chi2[:1], -0.5 * chi2[:1])
    for k in ("sum_t", "sum_tt", "deviance"):
        q[k][1], q[k][2] = one[k][1], 0.0
    q["pivot_t"][2] = 0.0
    q["n"][:] = [3, 1, 0]
    p = Predictive(q, [0], 4)
    assert np.all(np.isfinite(p.mean[0])) and np.all(np.isfinite(p.std[0])) and np.isfinite(p.var_chi2[0]) and np.isfinite(p.p_v[0])
    assert same_bytes(p.mean[1], t[0, 1]) and np.all(np.isnan(p.std[1])) and p.mean_chi2[1] == chi2[0, 1]
    assert np.isnan(p.var_chi2[1]) and np.isnan(p.var_lnl[1]) and np.isnan(p.p_v[1])
    assert np.all(np.isnan(p.mean[2])) and np.all(np.isnan(p.std[2])) and np.isnan(p.mean_chi2[2]) and np.isnan(p.mean_lnl[2])
    assert np.all(np.isnan(p.dic)) and np.all(np.isnan(p.chi2_at_mean))                  # (no evaluation at the mean was handed over)
    assert np.all(np.isnan(p.multipoles[0][0][2])) and np.all(np.isnan(p.multipoles[0][1][1]))


# ------------------------------------------------------------------ 3. the option ---------------------------------------------
def boom(*a, **k):
    raise AssertionError("the call reached an evaluation before refusing its input")


def test_refusals_name_their_reason_and_come_before_any_evaluation(tmp_path):
    import victor_amd
    from tests import cases
    from tests.test_joint_realisations import write_stacks
    from tests.test_realisations import stack_options
    from victor_amd.chains import sample_chains
    from victor_amd.joint import JointFit
    params = cases.cobaya_info()["params"]
    opts = write_stacks(tmp_path, [cases.dsplit_options(q) for q in range(2)], 3, tag="dsplit")
    fits = [victor_amd.CCFFit(*o) for o in opts]
    single = victor_amd.CCFFit(*stack_options())
    for f in fits + [single]:
        f._get_engine = boom
    joint = JointFit(fits)
    for target in (joint, joint.realisations()):
        with pytest.raises(ValueError, match="joint fits"):
            target.sample_chains(params, 10, predictive=True)
        with pytest.raises(victor_amd.InputError, match="joint fits"):
            target.sample_chains(params, 10, predictive=True, device=False)
    for target in (single, single.realisations([0, 1])):
        for device in (True, False):
            with pytest.raises(ValueError, match="temper="):
                target.sample_chains(params, 10, predictive=True, temper=True, device=device)
            with pytest.raises(ValueError, match="None or True"):
                target.sample_chains(params, 10, predictive={"bins": 3}, device=device)
        with pytest.raises(AssertionError, match="reached an evaluation"):               # a good option goes on
            target.sample_chains(params, 10, predictive=True, device=False)
    with pytest.raises(ValueError, match="needs a fit"):
        sample_chains(None, params, 5, device=False, evaluate=boom, predictive=True)
    with pytest.raises(ValueError, match="None or True"):                                # (False is not "off": None is)
        sample_chains(None, params, 5, device=False, evaluate=boom, predictive=False)
    with pytest.raises(AssertionError, match="reached an evaluation"):
        sample_chains(None, params, 5, device=False, evaluate=boom, predictive=None)


def test_the_keyword_is_on_every_public_path():
    import inspect

    import victor_amd
    from victor_amd.chains import sample_chains
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for fn in (victor_amd.CCFFit.sample_chains, Realisations.sample_chains, JointFit.sample_chains, JointRealisations.sample_chains, sample_chains):
        sig = inspect.signature(fn).parameters
        assert "predictive" in sig and sig["predictive"].default is None, fn


# ------------------------------------------------------------------ 4. the surface ------------------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    want = {"vk_chain_set_predictive": ["vk_chain* f", "int32_t group"],
            "vk_chain_predictive": ["vk_chain* f", "double* pivot_t", "double* sum_t", "double* sum_tt", "double* deviance", "int64_t* n",
                                    "int64_t* n_skipped", "double* held"]}
    for name in NEW:
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, f"include/victor_hip.h does not declare {name}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")] == want[name]
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert N.SYMBOLS["vk_chain_set_predictive"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert N.SYMBOLS["vk_chain_predictive"] == (C.c_int, [C.c_void_p, dp, dp, dp, dp, lp, lp, dp])
    csrc = os.path.join(ROOT, "victor_amd", "csrc")
    src = open(os.path.join(csrc, "vk_predictive.h")).read()
    assert "hip/hip_runtime.h" not in src and "asm" not in src
    kernel = open(os.path.join(csrc, "vk_kernel_predictive.h")).read().split("#pragma once")[1]
    assert "vk_chain_hold_kernel" in kernel and "vk_chain_predict_kernel" in kernel and "__syncthreads()" in kernel
    assert "atomic" not in kernel and "__shared__" not in kernel
    assert '#include "vk_kernel_predictive.h"' in open(os.path.join(csrc, "vk_sampled.hip")).read()
    # the step kernels and their arguments know nothing of it: the accept counter is the hand-off
    for name in ("vk_kernel_chain.h", "vk_kernel_stretch.h", "vk_chain_step.h", "vk_stretch_step.h"):
        assert "pred" not in open(os.path.join(csrc, name)).read().lower(), name


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
