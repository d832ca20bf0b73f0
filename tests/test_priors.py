"""Gaussian priors (victor_amd/priors.py, vk_fit_set_prior / vk_chain_set_prior) without a GPU: ln prior of
victor_amd/csrc/vk_prior.h compiled on its own under g++ against the NumPy statement, bit for bit; the Metropolis and stretch
decisions under a prior (vkchain::transition_prior, stretch_transition_prior) driven on analytic functions against the NumPy
loops that define the chains, bit for bit; the Nelder-Mead search of vk_fit_simplex.h on a quadratic lnL plus the prior against
the closed-form maximum; the refusals of ``GaussianPrior`` and ``prior=``, raised before any device call; the packing; and the
C ABI's surface.

The analytic functions are those of tests/test_chains.py ("gauss": a correlated Gaussian whose mean lies next to a face of the
box, so proposals leave the box often; "halfnan": -inf on half the box and NaN on a strip), restated in the driver below with the
same scalar arithmetic in the same order.
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.test_chains import HI, LO, NAMES, evaluate_of, same_bytes
from tests.test_chains import block_for as metropolis_block
from tests.test_chains import randoms as metropolis_randoms
from tests.test_stretch import block_for as stretch_block
from tests.test_stretch import randoms as stretch_randoms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_fit_set_prior", "vk_chain_set_prior")

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_stretch_step.h"
#include "vk_fit_simplex.h"
#include "vk_prior.h"

static double lnl_of(const char* fn, const double* x) {
  if (!strcmp(fn, "gauss")) {
    const double u = x[0] - 0.93, v = x[1] + 0.2, w = x[2] - 0.1;
    double q = (9.0 * (u * u) + (2.0 * 3.5) * (u * v)) + 4.0 * (v * v);
    q = q + 25.0 * (w * w);
    return -0.5 * q;
  }
  if (x[0] < 0.0) return -HUGE_VAL;
  if (x[1] > 0.3 && x[1] < 0.4) return std::nan("");
  return -(2.0 * ((x[0] - 0.3) * (x[0] - 0.3)) + 3.0 * ((x[1] - 0.2) * (x[1] - 0.2)) + (x[2] * x[2]));
}

static std::vector<double> in;
static FILE* fo;
static void put(double v) { fwrite(&v, sizeof(double), 1, fo); }

static vkprior::Prior prior_at(const double* p, int on, int d) {
  vkprior::Prior pr{};
  pr.on = on;
  for (int j = 0; j < d; ++j) pr.mu[j] = p[j];
  for (int i = 0; i < d * (d + 1) / 2; ++i) pr.pp[i] = p[d + i];
  return pr;
}

struct Chains {
  int C, d;
  std::vector<double> x, lnl, chi2, pivot, sum1, sum2;
  std::vector<int64_t> n_accept, n_steps, n_kept;
  Chains(int C_, int d_) : C(C_), d(d_), x((size_t)d_ * C_), lnl(C_), chi2(C_), pivot((size_t)d_ * C_), sum1((size_t)d_ * C_),
                           sum2((size_t)vkchain::n_tri(d_) * C_), n_accept(C_), n_steps(C_), n_kept(C_) {}
  vkchain::View view(int c) {
    vkchain::View s{};
    s.stride = (size_t)C;
    s.x = x.data() + c; s.lnl = lnl.data() + c; s.chi2 = chi2.data() + c; s.pivot = pivot.data() + c;
    s.sum1 = sum1.data() + c; s.sum2 = sum2.data() + c;
    s.n_accept = n_accept.data() + c; s.n_steps = n_steps.data() + c; s.n_kept = n_kept.data() + c;
    return s;
  }
  void begin(const vkchain::Box& box, const char* fn, const double* x0) {
    for (int c = 0; c < C; ++c) {
      vkchain::View s = view(c);
      vkchain::start(box, s, x0 + (size_t)c * d);
      const double l = lnl_of(fn, x0 + (size_t)c * d);
      vkchain::adopt(s, l, -2.0 * l);
    }
  }
  void step_out(const std::vector<double>& acc) {
    for (int c = 0; c < C; ++c) put(acc[c]);
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < d; ++j) put(x[(size_t)j * C + c]);
    for (int c = 0; c < C; ++c) put(lnl[c]);
    for (int c = 0; c < C; ++c) put(chi2[c]);
  }
  void tail_out() {
    for (int c = 0; c < C; ++c) put((double)n_accept[c]);
    for (int c = 0; c < C; ++c) put((double)n_steps[c]);
    for (int c = 0; c < C; ++c) put((double)n_kept[c]);
  }
};

// lnp d n           in: mu[d], pp[T], x[n][d]                                  out: lnprior[n], then tri mismatches (one double)
// metro fn d C n on old burn thin   in: lo[d], hi[d], mu[d], pp[T], x0[C][d], dz[n][C][d], logu[n][C]
// stretch fn d W n on old burn thin in: lo[d], hi[d], mu[d], pp[T], x0[W][d], z, lz, logu, partner [n][2][W/2]
//    out (both): per step accept[C], x[C][d], lnl[C], chi2[C]; then n_accept[C], n_steps[C], n_kept[C]
//    old = 1: the decision functions without a prior argument (vkchain::transition / stretch_transition)
// simplex d max_iter restarts ftol   in: lo[d], hi[d], step[d], xtol[d], x0[d], a[d], A[d][d], mu[d], pp[T]
//    lnL = -1/2 (x - a)^T A (x - a);  out: status, iterations, x[d], f[0]
int main(int argc, char** argv) {
  const char* mode = argv[1];
  FILE* fi = fopen(argv[argc - 2], "rb");
  fo = fopen(argv[argc - 1], "wb");
  if (!fi || !fo) return 2;
  fseek(fi, 0, SEEK_END);
  in.resize((size_t)ftell(fi) / sizeof(double));
  fseek(fi, 0, SEEK_SET);
  if (fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const double* p = in.data();
  if (!strcmp(mode, "lnp")) {
    const int d = atoi(argv[2]), n = atoi(argv[3]), T = d * (d + 1) / 2;
    const vkprior::Prior pr = prior_at(p, 1, d);
    const double* x = p + d + T;
    for (int i = 0; i < n; ++i) put(vkprior::lnprior(pr, d, [&](int j) { return x[(size_t)i * d + j]; }));
    int bad = vkprior::kMaxTri != vkchain::n_tri(vkchain::kMaxP);
    for (int dd = 1; dd <= vkprior::kMaxP; ++dd)
      for (int j = 0; j < dd; ++j)
        for (int k = j; k < dd; ++k) bad += vkprior::tri(dd, j, k) != vkchain::tri(dd, j, k);
    put((double)bad);
  } else if (!strcmp(mode, "metro") || !strcmp(mode, "stretch")) {
    const char* fn = argv[2];
    vkchain::Box box{};
    box.d = atoi(argv[3]);
    const int d = box.d, Cn = atoi(argv[4]), n = atoi(argv[5]), on = atoi(argv[6]), old = atoi(argv[7]), T = d * (d + 1) / 2;
    const long long burn = atoll(argv[8]), thin = atoll(argv[9]);
    for (int j = 0; j < d; ++j) box.lo[j] = p[j], box.hi[j] = p[d + j];
    const vkprior::Prior pr = prior_at(p + 2 * d, on, d);
    const double* x0 = p + 3 * d + T;
    Chains ch(Cn, d);
    ch.begin(box, fn, x0);
    std::vector<double> acc(Cn);
    if (!strcmp(mode, "metro")) {
      const double *dz = x0 + (size_t)Cn * d, *logu = dz + (size_t)n * Cn * d;
      for (int t = 0; t < n; ++t) {
        for (int c = 0; c < Cn; ++c) {
          vkchain::View s = ch.view(c);
          const double* inc = dz + ((size_t)t * Cn + c) * d;
          double row[vkchain::kMaxP];             // what the launch evaluates: the proposal, or outside the box the current position
          const bool move = vkchain::proposal_inside(box, s, inc);
          for (int j = 0; j < d; ++j) row[j] = move ? s.x[j * s.stride] + inc[j] : s.x[j * s.stride];
          const double l = lnl_of(fn, row), lu = logu[(size_t)t * Cn + c];
          const bool kept = vkchain::is_kept(t, burn, thin);
          acc[c] = (old ? vkchain::transition(box, s, inc, lu, l, -2.0 * l, kept)
                        : vkchain::transition_prior(box, pr, s, inc, lu, l, -2.0 * l, kept)) ? 1.0 : 0.0;
        }
        ch.step_out(acc);
      }
    } else {
      const int half = Cn / 2;
      const size_t per = (size_t)n * 2 * half;
      const double *z = x0 + (size_t)Cn * d, *lz = z + per, *logu = lz + per, *partner = logu + per;
      std::vector<double> prop((size_t)d * half), res_l(half);
      for (int t = 0; t < n; ++t) {
        const bool kept = vkchain::is_kept(t, burn, thin);
        for (int side = 0; side < 2; ++side) {
          const size_t at = ((size_t)t * 2 + side) * half;
          for (int i = 0; i < half; ++i) {        // the proposals of the whole half first, as the propose kernel does
            const int c = side * half + i, pa = (1 - side) * half + (int)partner[at + i];
            const vkchain::View s = ch.view(c);
            const bool inb = vkchain::propose(box, s, ch.x.data() + pa, z[at + i], prop.data() + i, (size_t)half);
            double row[vkchain::kMaxP];
            for (int j = 0; j < d; ++j) row[j] = inb ? prop[(size_t)j * half + i] : s.x[j * s.stride];
            res_l[i] = lnl_of(fn, row);
          }
          for (int i = 0; i < half; ++i) {
            const int c = side * half + i;
            vkchain::View s = ch.view(c);
            const double l = res_l[i];
            acc[c] = (old ? vkchain::stretch_transition(box, s, prop.data() + i, (size_t)half, lz[at + i], logu[at + i], l, -2.0 * l, kept)
                          : vkchain::stretch_transition_prior(box, pr, s, prop.data() + i, (size_t)half, lz[at + i], logu[at + i], l,
                                                              -2.0 * l, kept)) ? 1.0 : 0.0;
          }
        }
        ch.step_out(acc);
      }
    }
    ch.tail_out();
  } else if (!strcmp(mode, "simplex")) {
    vkfit::Params q{};
    q.d = atoi(argv[2]);
    const int d = q.d;
    q.S = vkfit::slots(d);
    q.max_iter = atoi(argv[3]);
    q.restarts = atoi(argv[4]);
    q.ftol = strtod(argv[5], nullptr);
    for (int j = 0; j < d; ++j) q.lo[j] = p[j], q.hi[j] = p[d + j], q.step[j] = p[2 * d + j], q.xtol[j] = p[3 * d + j];
    const double *x0 = p + 4 * d, *a = x0 + d, *A = a + d;
    const vkprior::Prior pr = prior_at(A + d * d, 1, d);
    static vkfit::State s;
    vkfit::start(s, q, x0);
    double lnl[vkfit::kMaxS], chi[vkfit::kMaxS];
    while (s.phase != vkfit::kDone) {
      for (int slot = 0; slot < q.S; ++slot) {
        const double* x = s.pt[slot];
        double quad = 0.0;
        for (int j = 0; j < d; ++j)
          for (int k = 0; k < d; ++k) quad += (x[j] - a[j]) * A[j * d + k] * (x[k] - a[k]);
        const double l = -0.5 * quad;
        chi[slot] = quad;
        // the value of a live slot, as vk_fit_step_kernel forms it: lnL + ln prior at the slot's point
        lnl[slot] = s.live[slot] ? l + vkprior::lnprior(pr, d, [&](int j) { return s.pt[slot][j]; }) : l;
      }
      vkfit::transition(s, q, lnl, chi);
    }
    put((double)s.status);
    put((double)s.iter);
    for (int j = 0; j < d; ++j) put(s.v[0][j]);
    put(s.f[0]);
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
    d = tmp_path_factory.mktemp("prior_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(args, arrays):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        subprocess.run([str(exe)] + [str(a) for a in args] + [str(fin), str(fout)], check=True)
        return np.fromfile(str(fout), dtype=np.float64)
    return run


def resolved(names, priors):
    from victor_amd.priors import resolve_prior
    d = len(names)
    return resolve_prior(priors, "test", names, np.full(d, -10.0), np.full(d, 10.0))


# ------------------------------------------------------------------ 1. ln prior, bit for bit --------------------------------
def priors_of(d, kind, rng):
    """(names, priors): ``diag`` - independent priors on every second parameter (zero rows between them); ``corr`` - a correlated
    pair that is NOT adjacent in sampled order (first and last parameter), with a diagonal prior in between when there is room."""
    from victor_amd.priors import GaussianPrior
    names = [f"p{j}" for j in range(d)]
    if kind == "diag" or d == 1:
        pick = list(range(0, d, 2))
        return names, GaussianPrior([names[j] for j in pick], rng.uniform(-1, 1, len(pick)), sigma=rng.uniform(0.05, 2.0, len(pick)))
    a = rng.standard_normal((2, 2))
    cov = a @ a.T + 0.1 * np.eye(2)
    out = [GaussianPrior([names[d - 1], names[0]], rng.uniform(-1, 1, 2), cov=cov)]         # (named in reverse order)
    if d > 3:
        out.append(GaussianPrior([names[2]], [0.3], sigma=[0.7]))
    return names, out


@pytest.mark.parametrize("d", [1, 4, 7, 10])
@pytest.mark.parametrize("kind", ["diag", "corr"])
def test_lnprior_against_numpy_bit_for_bit(driver, d, kind):
    rng = np.random.default_rng(100 * d + len(kind))
    names, priors = priors_of(d, kind, rng)
    r = resolved(names, priors)
    assert r.pp.shape == (d * (d + 1) // 2,) and r.mu.shape == (d,)
    zero_rows = [j for j in range(d) if not np.any(r.precision[j])]
    assert bool(zero_rows) == (d > 1), zero_rows            # every case beyond d = 1 has parameters without a prior
    x = rng.uniform(-3, 3, (257, d))
    x[0] = r.mu                                             # at the mean
    x[1] = r.mu + 1e-300                                    # (next to it: the difference rounds to zero or a denormal)
    x[2] = np.nextafter(r.mu, np.inf)
    x[3] = r.mu + 1e6                                       # far beyond it
    x[4] = -x[3]
    out = driver(["lnp", d, len(x)], [r.mu, r.pp, x])
    assert out[-1] == 0.0, "vkprior::tri is not vkchain::tri"
    want = r.lnprior(x)
    assert same_bytes(out[:-1], want), (d, kind)
    assert want[0] == 0.0 and np.all(want <= 0.0) and np.all(np.isfinite(want))
    # ... and the statement is the quadratic form (to rounding): the packing, the doubling and the zero rows are right
    dx = x - r.mu
    ref = -0.5 * np.einsum("ij,jk,ik->i", dx, r.precision, dx)
    assert np.allclose(want, ref, rtol=1e-12, atol=1e-300)
    if zero_rows:                                           # a parameter without a prior does not enter
        y = x.copy()
        y[:, zero_rows] += 1.0
        assert same_bytes(r.lnprior(y), want)


def test_packing_does_not_depend_on_the_order_of_the_names():
    from victor_amd.priors import GaussianPrior
    names = ["a", "b", "c", "d", "e"]
    rng = np.random.default_rng(7)
    a = rng.standard_normal((3, 3))
    cov = a @ a.T + 0.2 * np.eye(3)
    mean = np.array([0.1, -0.2, 0.3])
    first = resolved(names, GaussianPrior(["e", "a", "c"], mean, cov=cov))
    for perm in ([1, 2, 0], [2, 1, 0], [0, 2, 1]):
        again = resolved(names, GaussianPrior([["e", "a", "c"][i] for i in perm], mean[perm], cov=cov[np.ix_(perm, perm)]))
        assert same_bytes(again.pp, first.pp) and same_bytes(again.mu, first.mu), perm
    assert first.mu.tolist() == [-0.2, 0.0, 0.3, 0.0, 0.1]
    inv = np.linalg.inv(cov[np.ix_([1, 2, 0], [1, 2, 0])])
    assert np.allclose(first.precision[np.ix_([0, 2, 4], [0, 2, 4])], inv, rtol=1e-12)
    from victor_amd.priors import tri
    assert first.pp[tri(5, 0, 4)] == 2.0 * first.precision[0, 4] and first.pp[tri(5, 2, 2)] == first.precision[2, 2]
    assert not np.any(first.precision[1]) and not np.any(first.precision[3])
    # several priors with disjoint names: one block each; sigma gives 1 / sigma^2 on the diagonal
    two = resolved(names, [GaussianPrior(["e", "a", "c"], mean, cov=cov), GaussianPrior(["d"], [0.5], sigma=[0.25])])
    assert two.precision[3, 3] == 16.0 and two.mu[3] == 0.5 and same_bytes(two.precision[[0, 2, 4]][:, [0, 2, 4]],
                                                                              first.precision[[0, 2, 4]][:, [0, 2, 4]])


# ------------------------------------------------------------------ 2. the decisions, bit for bit ---------------------------
def chain_prior():
    """Correlated on (a, c) - not adjacent in sampled order - and diagonal on b, inside the box [-1, 1]^3."""
    from victor_amd.priors import GaussianPrior
    return [GaussianPrior(["c", "a"], [0.05, 0.6], cov=[[0.04, 0.018], [0.018, 0.09]]), GaussianPrior(["b"], [0.1], sigma=[0.3])]


def unpack(out, n, Cn, d):
    per = Cn * (d + 3)
    steps, tail = out[:n * per].reshape(n, per), out[n * per:]
    return {"accept": steps[:, :Cn] == 1.0, "x": steps[:, Cn:Cn + Cn * d].reshape(n, Cn, d),
            "lnl": steps[:, Cn + Cn * d:2 * Cn + Cn * d], "chi2": steps[:, 2 * Cn + Cn * d:],
            "n_accept": tail[:Cn].astype(np.int64), "n_steps": tail[Cn:2 * Cn].astype(np.int64), "n_kept": tail[2 * Cn:].astype(np.int64)}


def check_walk(got, ch, x0, n, fn):
    assert same_bytes(ch.pivot[0], x0)
    assert same_bytes(got["x"], ch.chain[:, 0]), fn                                   # every position
    assert same_bytes(got["lnl"], ch.lnl_chain[:, 0]) and same_bytes(got["chi2"], ch.chi2_chain[:, 0])
    before = np.concatenate([x0[None], ch.chain[:-1, 0]])
    moved = np.any(ch.chain[:, 0] != before, axis=2)
    assert np.array_equal(got["accept"], moved), fn                                   # every decision
    assert np.array_equal(got["n_accept"], ch.n_accept[0]) and np.array_equal(got["n_accept"], moved.sum(axis=0))
    assert np.all(got["n_steps"] == n) and np.all(got["n_kept"] == ch.n_kept)
    assert ch.n_outside.sum() > 0, "no proposal left the box: the test does not reach that rule"
    assert 0.03 < moved.mean() < 0.97, moved.mean()
    assert same_bytes(ch.lnprior_chain, ch._prior.lnprior(ch.chain)) if ch._prior is not None else np.all(ch.lnprior_chain == 0)
    if fn == "halfnan":
        assert not np.any(np.isnan(got["lnl"]))
        assert np.all((got["x"][..., 1] <= 0.3) | (got["x"][..., 1] >= 0.4))           # never onto the NaN strip
    return moved


@pytest.mark.parametrize("fn", ["gauss", "halfnan"])
def test_metropolis_under_a_prior_against_numpy_bit_for_bit(driver, fn):
    from victor_amd.chains import sample_chains
    n, Cn, seed = 200, 8, 3
    kw = dict(walkers=Cn, seed=seed, device=False, evaluate=evaluate_of(fn))
    ch = sample_chains(None, metropolis_block(fn), n, prior=chain_prior(), **kw)
    free = sample_chains(None, metropolis_block(fn), n, **kw)
    r = ch._prior
    x0, dz, logu = metropolis_randoms(ch, seed, Cn, n)
    got = unpack(driver(["metro", fn, 3, Cn, n, 1, 0, 0, 1], [LO, HI, r.mu, r.pp, x0, dz, logu]), n, Cn, 3)
    check_walk(got, ch, x0, n, fn)
    assert not same_bytes(ch.chain, free.chain), "the prior changed no decision: the test does not reach it"
    if fn == "halfnan":                                    # proposals reached the -inf half and the NaN strip
        before = np.concatenate([x0[None], ch.chain[:-1, 0]])
        prop = before + dz
        inside = ((prop >= LO) & (prop <= HI)).all(axis=2)
        assert np.any(inside & (prop[..., 0] < 0)) and np.any(inside & (prop[..., 0] >= 0) & (prop[..., 1] > 0.3) & (prop[..., 1] < 0.4))
    # burn and thin: the kept steps are those of the full history
    thinned = sample_chains(None, metropolis_block(fn), n, prior=chain_prior(), burn=7, thin=3, **kw)
    assert same_bytes(thinned.chain, ch.chain[7::3]) and same_bytes(thinned.lnprior_chain, ch.lnprior_chain[7::3])
    got = unpack(driver(["metro", fn, 3, Cn, n, 1, 0, 7, 3], [LO, HI, r.mu, r.pp, x0, dz, logu]), n, Cn, 3)
    assert np.all(got["n_kept"] == thinned.n_kept) and same_bytes(got["x"][7::3], thinned.chain[:, 0])


@pytest.mark.parametrize("fn", ["gauss", "halfnan"])
def test_stretch_under_a_prior_against_numpy_bit_for_bit(driver, fn):
    from victor_amd.chains import sample_chains
    n, Wn, seed = 200, 8, 3
    kw = dict(walkers=Wn, seed=seed, move="stretch", device=False, evaluate=evaluate_of(fn))
    ch = sample_chains(None, stretch_block(fn), n, prior=chain_prior(), **kw)
    free = sample_chains(None, stretch_block(fn), n, **kw)
    r = ch._prior
    x0, z, k, logu = stretch_randoms(fn, seed, n)
    lz = 2 * np.log(z)
    got = unpack(driver(["stretch", fn, 3, Wn, n, 1, 0, 0, 1], [LO, HI, r.mu, r.pp, x0, z, lz, logu, k.astype(np.float64)]), n, Wn, 3)
    check_walk(got, ch, x0, n, fn)
    assert not same_bytes(ch.chain, free.chain), "the prior changed no decision: the test does not reach it"
    # cut with extend(): the prior stays
    cut = sample_chains(None, stretch_block(fn), 70, prior=chain_prior(), **kw).extend(130)
    for a in ("chain", "lnl_chain", "lnprior_chain", "x", "n_accept"):
        assert same_bytes(getattr(cut, a), getattr(ch, a)), a


@pytest.mark.parametrize("fn", ["gauss", "halfnan"])
def test_without_a_prior_the_new_decisions_are_the_old_ones(driver, fn):
    """prior.on == 0 (mu and pp hold numbers that must not be read): transition_prior and stretch_transition_prior return what
    transition and stretch_transition return on the same inputs - which is the NumPy loop without a prior."""
    from victor_amd.chains import sample_chains
    n, Cn, seed = 200, 8, 3
    r = resolved(NAMES, chain_prior())
    ch = sample_chains(None, metropolis_block(fn), n, walkers=Cn, seed=seed, device=False, evaluate=evaluate_of(fn))
    x0, dz, logu = metropolis_randoms(ch, seed, Cn, n)
    arrays = [LO, HI, r.mu, r.pp, x0, dz, logu]
    new, old = driver(["metro", fn, 3, Cn, n, 0, 0, 0, 1], arrays), driver(["metro", fn, 3, Cn, n, 0, 1, 0, 1], arrays)
    assert same_bytes(new, old) and same_bytes(unpack(new, n, Cn, 3)["x"], ch.chain[:, 0])
    assert not same_bytes(driver(["metro", fn, 3, Cn, n, 1, 0, 0, 1], arrays), old)
    sx0, z, k, slogu = stretch_randoms(fn, seed, n)
    arrays = [LO, HI, r.mu, r.pp, sx0, z, 2 * np.log(z), slogu, k.astype(np.float64)]
    new, old = driver(["stretch", fn, 3, Cn, n, 0, 0, 0, 1], arrays), driver(["stretch", fn, 3, Cn, n, 0, 1, 0, 1], arrays)
    assert same_bytes(new, old)
    assert not same_bytes(driver(["stretch", fn, 3, Cn, n, 1, 0, 0, 1], arrays), old)
    # the NumPy loop: prior=None and no keyword are the same call
    again = sample_chains(None, metropolis_block(fn), n, walkers=Cn, seed=seed, device=False, evaluate=evaluate_of(fn), prior=None)
    for a in ("chain", "lnl_chain", "x", "n_accept", "sum1", "sum2"):
        assert same_bytes(getattr(again, a), getattr(ch, a)), a
    assert again.decision_margin == ch.decision_margin and np.all(ch.lnprior_chain == 0.0)


# ------------------------------------------------------------------ 3. Nelder-Mead on lnL + ln prior ------------------------
def test_the_search_ends_at_the_precision_weighted_mean(driver):
    """lnL = -1/2 (x - a)^T A (x - a) and the prior -1/2 (x - mu)^T P (x - mu): the posterior's maximum is the
    precision-weighted mean (A + P)^-1 (A a + P mu), the closed form.  xtol: the search stops when its simplex spans less than
    xtol and its values less than ftol; f = O(1e-1) is resolved to u f = 1e-17, which a curvature of order 10 turns into
    sqrt(2 x 1e-17 / 10) = 1.5e-9 in position - xtol = 1e-6 of a box of width 2 leaves that three orders of room, so the end
    point must lie within xtol of the closed form in every coordinate."""
    from victor_amd.priors import GaussianPrior
    d = 4
    names = ["w", "x", "y", "z"]
    a = np.array([0.30, -0.20, 0.10, 0.45])
    A = np.array([[9.0, 1.5, 0.0, 0.5], [1.5, 6.0, 1.0, 0.0], [0.0, 1.0, 12.0, 2.0], [0.5, 0.0, 2.0, 8.0]])
    r = resolved(names, [GaussianPrior(["y", "w"], [-0.15, 0.05], cov=[[0.05, 0.02], [0.02, 0.08]]), GaussianPrior(["x"], [0.2], sigma=[0.25])])
    assert not np.any(r.precision[3])                      # z carries no prior
    want = np.linalg.solve(A + r.precision, A @ a + r.precision @ r.mu)
    assert np.all(np.abs(want - a) > 1e-3), "the prior does not move the maximum: the test would pass without it"
    xtol = np.full(d, 1e-6)
    out = driver(["simplex", d, 5000, 3, 1e-15], [np.full(d, -1.0), np.full(d, 1.0), np.full(d, 0.1), xtol, np.zeros(d), a, A, r.mu, r.pp])
    status, n_iter, x, f0 = int(out[0]), int(out[1]), out[2:2 + d], out[2 + d]
    print("status", status, "iterations", n_iter, "x - closed form", x - want)
    assert status == 0, status
    assert np.all(np.abs(x - want) <= xtol), (x, want)
    dx = x - a
    assert abs(-f0 - (-0.5 * dx @ A @ dx + r.lnprior(x))) <= 1e-14


# ------------------------------------------------------------------ 4. refusals ---------------------------------------------
def boom(*a, **k):
    raise AssertionError("the call reached the device before refusing its input")


def test_refusals_come_before_any_device_call():
    import victor_amd
    from victor_amd import GaussianPrior, InputError
    from victor_amd.joint import JointFit, per_block
    params = cases.cobaya_info()["params"]
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    fit._get_engine = boom
    ds = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(3)]
    for f in ds:
        f._get_engine = boom
    joint = JointFit(ds)
    blk = per_block(params, ["sigma_v"], 3)
    # the object's own checks
    with pytest.raises(InputError, match="exactly one of cov and sigma"):
        GaussianPrior(["sigma_v"], [380.0], cov=[[400.0]], sigma=[20.0])
    with pytest.raises(InputError, match="exactly one of cov and sigma"):
        GaussianPrior(["sigma_v"], [380.0])
    with pytest.raises(InputError, match="not symmetric"):
        GaussianPrior(["fsigma8", "sigma_v"], [0.47, 380.0], cov=[[0.01, 0.1], [0.2, 400.0]])
    with pytest.raises(InputError, match="not positive definite"):
        GaussianPrior(["fsigma8", "sigma_v"], [0.47, 380.0], cov=[[0.01, 3.0], [3.0, 400.0]])
    with pytest.raises(InputError, match="named twice"):
        GaussianPrior(["sigma_v", "sigma_v"], [380.0, 380.0], sigma=[20.0, 20.0])
    with pytest.raises(InputError, match="sigma"):
        GaussianPrior(["sigma_v"], [380.0], sigma=[0.0])
    ok = GaussianPrior(["sigma_v"], [380.0], sigma=[20.0])
    calls = [lambda **kw: fit.best_fit(params, **kw), lambda **kw: fit.sample_chains(params, 5, **kw),
             lambda **kw: fit.sample_chains(params, 5, walkers=10, move="stretch", **kw)]
    for call in calls:
        with pytest.raises(InputError, match="not sampled .it is not in the params block"):
            call(prior=GaussianPrior(["sigma_w"], [380.0], sigma=[20.0]))
        with pytest.raises(InputError, match="not sampled .it is fixed"):
            call(prior=ok, fixed={"sigma_v": 380.0})
        with pytest.raises(InputError, match="named by two priors"):
            call(prior=[ok, GaussianPrior(["beta", "sigma_v"], [0.4, 370.0], sigma=[0.1, 20.0])])
        with pytest.raises(InputError, match="outside its box"):
            call(prior=GaussianPrior(["sigma_v"], [5000.0], sigma=[20.0]))
        with pytest.raises(InputError, match="needs a JointFit"):
            call(prior=GaussianPrior(["sigma_v@1"], [380.0], sigma=[20.0]))
        with pytest.raises(InputError, match="GaussianPrior or a list"):
            call(prior={"sigma_v": (380.0, 20.0)})
        with pytest.raises(AssertionError, match="reached the device"):                # a good prior goes on to the device
            call(prior=ok)
    # a joint fit: "name@q" is a sampled parameter; the plain name is not (every block has an entry of its own)
    fixed = {"beta": 0.4, "epsilon": 1.0}
    for call in (lambda **kw: joint.best_fit(blk, fixed=fixed, **kw), lambda **kw: joint.sample_chains(blk, 5, fixed=fixed, **kw)):
        with pytest.raises(InputError, match="not sampled"):
            call(prior=ok)
        with pytest.raises(InputError, match="not sampled"):
            call(prior=GaussianPrior(["sigma_v@3"], [380.0], sigma=[20.0]))
        with pytest.raises(AssertionError, match="reached the device"):
            call(prior=GaussianPrior(["sigma_v@2", "sigma_v@0"], [380.0, 370.0], cov=[[400.0, 100.0], [100.0, 900.0]]))
    # the block's own dist: norm stays refused, with its present message
    with pytest.raises(InputError, match="uniform"):
        fit.best_fit(dict(params, sigma_v={"prior": {"dist": "norm", "loc": 380, "scale": 20}, "proposal": 10}), prior=ok)


def test_the_keyword_is_on_all_eight_methods():
    import inspect

    import victor_amd
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for cls in (victor_amd.CCFFit, Realisations, JointFit, JointRealisations):
        for method in (cls.best_fit, cls.sample_chains):
            sig = inspect.signature(method).parameters
            assert "prior" in sig and sig["prior"].default is None, (cls, method)
    assert victor_amd.GaussianPrior is victor_amd.priors.GaussianPrior


def test_best_fit_result_without_a_prior():
    from victor_amd.fitting import BestFit
    x, lnl = np.zeros((2, 1)), np.array([-3.0, -4.0])
    bf = BestFit(["a"], x, {}, lnl, -2 * lnl, np.zeros(2, np.int32), np.ones(2, np.int32), np.ones(2, np.int64))
    assert same_bytes(bf.lnpost, bf.lnl) and same_bytes(bf.lnl, lnl) and np.all(bf.lnprior == 0.0)
    lp = np.array([-0.5, -0.25])
    bf = BestFit(["a"], x, {}, lnl, -2 * lnl, np.zeros(2, np.int32), np.ones(2, np.int32), np.ones(2, np.int64), lp)
    assert same_bytes(bf.lnpost, lnl) and same_bytes(bf.lnprior, lp) and same_bytes(bf.lnl, lnl - lp)


# ------------------------------------------------------------------ 5. the C ABI's surface ----------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    dp = C.POINTER(C.c_double)
    for name, handle in zip(NEW, ("vk_fit", "vk_chain")):
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, f"include/victor_hip.h does not declare {name}"
        args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
        assert args == [f"{handle}* f", "const double* mu", "const double* pp_packed"]
        assert N.SYMBOLS[name] == (C.c_int, [C.c_void_p, dp, dp])
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_prior.h")).read()
    assert "hip/hip_runtime.h" not in src and "#pragma clang fp contract(off)" in src


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
