"""Replica exchange on the chains (victor_amd/tempering.py, victor_amd/csrc/vk_temper_step.h) - no GPU needed.

* vk_temper_step.h compiled on its own under g++ and driven on the analytic functions of tests/test_chains.py, step by step and
  bit for bit against the NumPy definition (``sample_chains(..., device=False, evaluate=..., temper=...)``): every decision, every
  position, the swap counters and the energy sums; at beta = 1 against vkchain::transition / transition_prior.
* ``temper={"betas": [1.0]}`` is the plain chains bit for bit.
* A run does not depend on how it is cut, with swap events inside and across the blocks of 64 steps.
* The evidence of a 2-D Gaussian likelihood in the unit box against quadrature.  The bounds are the issue's: a stand-alone NumPy
  restatement of the scheme, 12 seeds on the CPU, gave ``ln_evidence - exact`` with rms 0.0075 and maximum 0.016, walker-scatter
  errors of 0.007-0.013, swap acceptance 0.91, and by quadrature a ladder bias of 7e-4 for the corrected rule (-0.039 for the plain
  trapezoid); asserted: within 0.05 (six times the rms), an error estimate in (0, 0.05), every swap acceptance above 0.5.
* Refusals.
"""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import HI, LO, NAMES, block_for, evaluate_of, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_temper_step.h"

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

// usage: driver fn d R K W n burn thin swap_every prior plain in out
// in:  doubles lo[d], hi[d], betas[K], mu[d], pp[d(d+1)/2], x0[C][d], dz[n][C][d], logu[n][C], logs[n][C]
// out: doubles, per step: accept[C], x[C][d], lnl[C], chi2[C] (after the step's swap event, if any), n_swap_acc[C] so far; then
//      n_accept[C], n_swap_try[C], n_swap_acc[C], pivot_e[C], e1[C], e2[C], n_e[C]
// plain != 0: every chain steps with vkchain::transition_prior instead (no beta, no swap).  State: structure-of-arrays, stride C.
int main(int argc, char** argv) {
  const char* fn = argv[1];
  vkchain::Box box{};
  box.d = atoi(argv[2]);
  const int d = box.d, R = atoi(argv[3]), K = atoi(argv[4]), W = atoi(argv[5]), n = atoi(argv[6]);
  const long long burn = atoll(argv[7]), thin = atoll(argv[8]), swap_every = atoll(argv[9]);
  const int with_prior = atoi(argv[10]), plain = atoi(argv[11]);
  const int C = R * K * W, T = vkchain::n_tri(d);
  std::vector<double> in((size_t)2 * d + K + d + T + (size_t)C * d + (size_t)n * C * (d + 2));
  FILE* fi = fopen(argv[12], "rb");
  if (!fi || fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const double* p = in.data();
  for (int j = 0; j < d; ++j) box.lo[j] = *p++;
  for (int j = 0; j < d; ++j) box.hi[j] = *p++;
  const double* betas = p;
  p += K;
  vkprior::Prior pr{};
  pr.on = with_prior;
  for (int j = 0; j < d; ++j) pr.mu[j] = *p++;
  for (int i = 0; i < T; ++i) pr.pp[i] = *p++;
  const double *x0 = p, *dz = x0 + (size_t)C * d, *logu = dz + (size_t)n * C * d, *logs = logu + (size_t)n * C;
  std::vector<double> x((size_t)d * C), lnl(C), chi2(C), pivot((size_t)d * C), sum1((size_t)d * C), sum2((size_t)T * C);
  std::vector<double> pivot_e(C), e1(C), e2(C);
  std::vector<int64_t> n_accept(C), n_steps(C), n_kept(C), n_e(C), n_try(C), n_acc(C);
  auto view = [&](int c) {
    vkchain::View s{};
    s.stride = (size_t)C;
    s.x = x.data() + c; s.lnl = lnl.data() + c; s.chi2 = chi2.data() + c; s.pivot = pivot.data() + c;
    s.sum1 = sum1.data() + c; s.sum2 = sum2.data() + c;
    s.n_accept = n_accept.data() + c; s.n_steps = n_steps.data() + c; s.n_kept = n_kept.data() + c;
    return s;
  };
  auto row_value = [&](const vkchain::View& s, const double* inc, double* l, double* c2) {
    double row[vkchain::kMaxP];
    const bool move = inc && vkchain::proposal_inside(box, s, inc);
    for (int j = 0; j < d; ++j) row[j] = move ? s.x[j * s.stride] + inc[j] : s.x[j * s.stride];
    *l = lnl_of(fn, row);
    *c2 = -2.0 * *l;
  };
  FILE* fo = fopen(argv[13], "wb");
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
    const bool kept = vkchain::is_kept(t, burn, thin);
    for (int c = 0; c < C; ++c) {
      vkchain::View s = view(c);
      const double* inc = dz + ((size_t)t * C + c) * d;
      double l, c2;
      row_value(s, inc, &l, &c2);
      const double u = logu[(size_t)t * C + c];
      if (plain) {
        acc[c] = vkchain::transition_prior(box, pr, s, inc, u, l, c2, kept) ? 1.0 : 0.0;
        continue;
      }
      acc[c] = vktemper::transition(box, pr, s, betas[vktemper::rung_of(c, K, W)], inc, u, l, c2, kept) ? 1.0 : 0.0;
      if (kept) {
        vktemper::Energy e{pivot_e.data() + c, e1.data() + c, e2.data() + c, n_e.data() + c};
        vktemper::energy_add(e, *s.lnl);
      }
    }
    if (!plain && vktemper::is_swap(t, swap_every)) {
      const int parity = vktemper::swap_parity(t, swap_every), pairs = vktemper::pairs_of(K, parity);
      for (int i = 0; i < R * pairs * W; ++i) {              // the swap kernel's thread i
        const int w = i % W, q = (i / W) % pairs, r = i / (W * pairs), k = parity + 2 * q;
        const int lo = (r * K + k) * W + w, hi = lo + W;
        vkchain::View a = view(lo), b = view(hi);
        vktemper::swap_pair(d, a, b, betas[k], betas[k + 1], logs[(size_t)t * C + lo], n_try.data() + lo, n_acc.data() + lo);
      }
    }
    for (int c = 0; c < C; ++c) put(acc[c]);
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < d; ++j) put(x[(size_t)j * C + c]);
    for (int c = 0; c < C; ++c) put(lnl[c]);
    for (int c = 0; c < C; ++c) put(chi2[c]);
    for (int c = 0; c < C; ++c) put((double)n_acc[c]);
  }
  for (int c = 0; c < C; ++c) put((double)n_accept[c]);
  for (int c = 0; c < C; ++c) put((double)n_try[c]);
  for (int c = 0; c < C; ++c) put((double)n_acc[c]);
  for (int c = 0; c < C; ++c) put(pivot_e[c]);
  for (int c = 0; c < C; ++c) put(e1[c]);
  for (int c = 0; c < C; ++c) put(e2[c]);
  for (int c = 0; c < C; ++c) put((double)n_e[c]);
  fclose(fo);
  return 0;
}
"""


def prior_for(fn):
    from victor_amd.priors import GaussianPrior
    if fn == "gauss":
        return GaussianPrior(["a", "c"], [0.7, 0.0], cov=[[0.04, 0.01], [0.01, 0.09]])
    return GaussianPrior(["b"], [0.1], sigma=[0.3])


def tempered(fn, n_steps, temper, walkers=4, seed=3, prior=None, **kw):
    from victor_amd.chains import sample_chains
    return sample_chains(None, block_for(fn), n_steps, walkers=walkers, seed=seed, device=False, evaluate=evaluate_of(fn), prior=prior,
                         temper=temper, **kw)


def randoms(ch, seed, n_steps):
    """The numbers sample_chains consumed for ``ch`` (start from the reference distribution): drawn again by the protocol."""
    from victor_amd.chains import BLOCK, _draw_start
    specs, C = ch._specs, ch._RK * ch.W
    rng, rng_s = np.random.default_rng(seed), np.random.default_rng([seed, 1])
    loc, scale = np.array([s.ref_loc for s in specs]), np.array([s.ref_scale for s in specs])
    x0 = np.array([_draw_start(rng, loc, scale, LO, HI, "ref") for _ in range(C)])
    dz, logu, logs = [], [], []
    for _ in range((n_steps + BLOCK - 1) // BLOCK):
        dz.append(ch._width * rng.standard_normal((BLOCK, C, len(specs))))
        logu.append(np.log(rng.random((BLOCK, C))))
        logs.append(np.log(rng_s.random((BLOCK, C))))
    return x0, np.concatenate(dz)[:n_steps], np.concatenate(logu)[:n_steps], np.concatenate(logs)[:n_steps]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("temper_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(fn, K, W, betas, x0, dz, logu, logs, swap_every, prior=None, burn=0, thin=1, plain=False):
        n, C, dd = dz.shape
        T = dd * (dd + 1) // 2
        mu, pp = (prior.mu, prior.pp) if prior is not None else (np.zeros(dd), np.zeros(T))
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([LO, HI, betas, mu, pp, x0.ravel(), dz.ravel(), logu.ravel(), logs.ravel()]).astype(np.float64).tofile(str(fin))
        subprocess.run([str(exe), fn, str(dd), str(C // (K * W)), str(K), str(W), str(n), str(burn), str(thin), str(swap_every),
                        "1" if prior is not None else "0", "1" if plain else "0", str(fin), str(fout)], check=True)
        out = np.fromfile(str(fout), dtype=np.float64)
        per = C * (dd + 4)
        steps, tail = out[: n * per].reshape(n, per), out[n * per:].reshape(7, C)
        at = np.cumsum([0, C, C * dd, C, C, C])
        return {"accept": steps[:, :C] == 1.0, "x": steps[:, at[1]:at[2]].reshape(n, C, dd), "lnl": steps[:, at[2]:at[3]],
                "chi2": steps[:, at[3]:at[4]], "swapped": steps[:, at[4]:at[5]].astype(np.int64),
                "n_accept": tail[0].astype(np.int64), "n_swap_try": tail[1].astype(np.int64), "n_swap_acc": tail[2].astype(np.int64),
                "pivot_e": tail[3], "e1": tail[4], "e2": tail[5], "n_e": tail[6].astype(np.int64)}
    return run


LADDERS = {1: [1.0], 3: [1.0, 0.25, 0.0], 4: [1.0, 0.5, 0.1, 0.0]}


# ------------------------------------------------------------------ the header against the definition ---------------------
@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("fn,K", [("gauss", 1), ("gauss", 3), ("gauss", 4), ("halfnan", 3), ("halfnan", 4), ("none", 3)])
def test_header_against_numpy_bit_for_bit(driver, fn, K, with_prior):
    """Step by step: the definition is advanced one step at a time (``extend(1)``), so that its state after every swap event and
    its counters after every step are seen, and compared with what the C++ loop over vk_temper_step.h leaves."""
    n, W, seed, swap_every = 70, 4, 3, 3
    prior = prior_for(fn) if with_prior else None
    temper = {"betas": LADDERS[K], "swap_every": swap_every}
    ch = tempered(fn, 0, temper, walkers=W, seed=seed, prior=prior, burn=4, thin=2)
    C = K * W
    xs, lnls, chi2s, acc, swapped = [], [], [], [], []
    for _ in range(n):
        ch.extend(1)
        q = ch.tempering
        xs.append(q.x.reshape(C, -1))
        lnls.append(q.lnl.ravel())
        chi2s.append(q.chi2.ravel())
        acc.append(ch._n_accept.copy())
        swapped.append(q.n_swap_acc.ravel())
    x0, dz, logu, logs = randoms(ch, seed, n)
    got = driver(fn, K, W, np.array(LADDERS[K]), x0, dz, logu, logs, swap_every, ch._prior, burn=4, thin=2)
    assert same_bytes(got["x"], np.array(xs)), (fn, K)                                  # every position, after every swap event
    assert same_bytes(got["lnl"], np.array(lnls)) and same_bytes(got["chi2"], np.array(chi2s))
    decisions = np.diff(np.concatenate([np.zeros((1, C), dtype=np.int64), np.array(acc)]), axis=0) == 1
    assert np.array_equal(got["accept"], decisions), (fn, K)                             # every decision of a step
    assert np.array_equal(got["swapped"], np.array(swapped)), (fn, K)                    # ... and of a swap, event by event
    q = ch.tempering
    assert np.array_equal(got["n_accept"], ch._n_accept)
    assert np.array_equal(got["n_swap_try"], q.n_swap_try.ravel()) and np.array_equal(got["n_swap_acc"], q.n_swap_acc.ravel())
    for name in ("pivot_e", "e1", "e2"):
        assert same_bytes(got[name], getattr(q, name).ravel()), (fn, K, name)
    assert np.array_equal(got["n_e"], q.n_e.ravel())
    # what the cases are for
    events = sum(1 for s in range(n) if (s + 1) % swap_every == 0)
    tries = q.n_swap_try.reshape(K, W)
    for k in range(K - 1):                                   # rung k is the lower rung of the events of parity k % 2
        assert np.all(tries[k] == sum(1 for e in range(events) if e % 2 == k % 2))
    assert np.all(tries[K - 1] == 0) and np.all(q.n_swap_acc <= q.n_swap_try)
    prop_outside = ~((np.concatenate([x0[None], got["x"][:-1]]) + dz >= LO) & (np.concatenate([x0[None], got["x"][:-1]]) + dz <= HI)).all(axis=2)
    assert prop_outside.any() and not np.any(got["accept"] & prop_outside)              # proposals left the box; none was taken
    if fn == "gauss" and K > 1:
        assert q.n_swap_acc.sum() > 0 and got["accept"].any()
        if not with_prior:                                   # beta = 0 without a prior: every proposal inside the box is accepted
            hot = np.arange(C).reshape(K, W)[-1]
            assert np.array_equal(got["accept"][:, hot], ~prop_outside[:, hot])
        assert np.all(q.n_e == ch.n_kept) and np.all(q.n_not_finite == 0)
    if fn == "halfnan":
        assert not np.any(np.isnan(got["lnl"])) and np.all(np.isfinite(got["lnl"]))      # never onto a failed row, at any beta
        assert np.all(got["x"][..., 0] >= 0.0) and np.all((got["x"][..., 1] <= 0.3) | (got["x"][..., 1] >= 0.4))
    if fn == "none":                                         # the dead end: a stored -inf never moves, by a step or by a swap
        assert not got["accept"].any() and q.n_swap_acc.sum() == 0 and np.all(q.n_e == 0) and np.all(got["lnl"] == -math.inf)
        assert np.all(q.n_not_finite == ch.n_kept * W) and np.all(np.isnan(q.mean_lnl)) and np.all(q.e2 == 0)


@pytest.mark.parametrize("with_prior", [False, True])
@pytest.mark.parametrize("fn", ["gauss", "halfnan"])
def test_beta_one_is_the_plain_transition_bit_for_bit(driver, fn, with_prior):
    """vktemper::transition at beta = 1 against vkchain::transition / transition_prior on the same numbers."""
    n, W, seed = 150, 8, 3
    prior = prior_for(fn) if with_prior else None
    ch = tempered(fn, n, {"betas": [1.0]}, walkers=W, seed=seed, prior=prior)
    x0, dz, logu, logs = randoms(ch, seed, n)
    a = driver(fn, 1, W, np.array([1.0]), x0, dz, logu, logs, 4, ch._prior)
    b = driver(fn, 1, W, np.array([1.0]), x0, dz, logu, logs, 4, ch._prior, plain=True)
    for name in ("accept", "x", "lnl", "chi2", "n_accept"):
        assert same_bytes(a[name], b[name]), (fn, name)
    assert a["accept"].any() and not a["accept"].all()
    assert same_bytes(a["x"], ch.chain[:, 0]) and same_bytes(a["lnl"], ch.lnl_chain[:, 0])
    assert a["n_swap_try"].sum() == 0


# ------------------------------------------------------------------ the plain chains ---------------------------------------
@pytest.mark.parametrize("with_prior", [False, True])
def test_a_ladder_of_one_rung_is_the_plain_chains(with_prior):
    from victor_amd.chains import sample_chains
    prior = prior_for("gauss") if with_prior else None
    kw = dict(walkers=8, seed=11, device=False, evaluate=evaluate_of("gauss"), burn=7, thin=3, prior=prior, marginals=True, autocorr={"max_lag": 16})
    plain = sample_chains(None, block_for("gauss"), 150, **kw)
    one = sample_chains(None, block_for("gauss"), 150, temper={"betas": [1.0]}, **kw)
    for a in ("x", "lnl", "chi2", "chain", "lnl_chain", "chi2_chain", "lnprior_chain", "n_accept", "acceptance", "pivot", "sum1", "sum2",
              "mean", "cov", "rhat", "n_outside"):
        assert same_bytes(getattr(one, a), getattr(plain, a)), a
    assert one.decision_margin == plain.decision_margin and one.n_kept == plain.n_kept
    for n in NAMES:
        assert np.array_equal(one.marginals.counts[n], plain.marginals.counts[n])
    assert same_bytes(one.autocorr.tau, plain.autocorr.tau)
    assert plain.tempering is None and one.tempering.swap_acceptance.shape == (1, 0) and np.isnan(one.tempering.ln_evidence[0])
    assert same_bytes(one.tempering.x[:, 0], plain.x) and same_bytes(one.tempering.acceptance[:, 0], plain.acceptance)


# ------------------------------------------------------------------ determinism and cuts -----------------------------------
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("swap_every", [1, 3, 64, 100])
def test_a_tempered_run_does_not_depend_on_how_it_is_cut(swap_every, K):
    temper = {"rungs": K, "power": 3, "swap_every": swap_every}
    kw = dict(walkers=4, seed=2, burn=10, thin=2, marginals=True, autocorr={"max_lag": 8})
    whole = tempered("gauss", 130, temper, **kw)
    again = tempered("gauss", 130, temper, **kw)
    cut = tempered("gauss", 50, temper, **kw).extend(80)
    for ch in (again, cut):
        for a in ("x", "lnl", "chi2", "chain", "lnl_chain", "n_accept", "sum1", "sum2", "mean", "cov", "rhat"):
            assert same_bytes(getattr(ch, a), getattr(whole, a)), (swap_every, K, a)
        for a in ("x", "lnl", "chain", "lnl_chain", "pivot_e", "e1", "e2", "n_e", "n_swap_try", "n_swap_acc", "mean_lnl", "var_lnl",
                  "acceptance", "swap_acceptance", "ln_evidence", "ln_evidence_trapezoid", "ln_evidence_error"):
            assert same_bytes(getattr(ch.tempering, a), getattr(whole.tempering, a)), (swap_every, K, a)
        assert same_bytes(ch.autocorr.acf, whole.autocorr.acf)
        assert all(np.array_equal(ch.marginals.counts[n], whole.marginals.counts[n]) for n in NAMES)
    q = whole.tempering
    events = 130 // swap_every
    assert q.n_swap_try[0, 0, 0] == (events + 1) // 2 and q.n_swap_try[0, 1, 0] == events // 2
    assert q.chain.shape == (60, 1, K, 4, 3) and same_bytes(q.chain[:, :, 0], whole.chain) and whole.chain.shape == (60, 1, 4, 3)
    assert q.betas[0] == 1.0 and q.betas[-1] == 0.0 and np.all(np.diff(q.betas) < 0)
    assert np.all(whole.marginals.n == 60 * 4) and whole.autocorr.n == 60


def test_the_power_ladder_and_the_default_scales():
    from victor_amd.tempering import default_scales, power_ladder, resolve_temper
    b = power_ladder(16, 5)
    assert b[0] == 1.0 and b[-1] == 0.0 and np.all(np.diff(b) < 0) and b[8] == (7 / 15) ** 5.0
    lad = resolve_temper(True, "t", np.array([0.1, 0.05]), np.zeros(2), np.ones(2))
    assert lad.K == 16 and lad.swap_every == 4 and same_bytes(lad.betas, b)
    s = default_scales(b, np.array([0.1, 0.05]), np.zeros(2), np.ones(2))
    assert s[0] == 1.0 and s[-1] == 5.0 and np.all(np.diff(s) >= 0) and s[5] == 1.0 / np.sqrt(b[5])
    assert resolve_temper(None, "t", None, None, None) is None and resolve_temper(False, "t", None, None, None) is None
    lad = resolve_temper({"betas": [1, 0.5], "scales": [1, 3], "swap_every": 0}, "t", np.array([0.1]), np.zeros(1), np.ones(1))
    assert lad.scales.tolist() == [1.0, 3.0] and lad.swap_every == 0


# ------------------------------------------------------------------ the evidence -------------------------------------------
EXACT_LN_Z = -2.76999                     # ln of the integral of the likelihood below over the unit box, by quadrature


def test_evidence_of_a_gaussian_in_the_unit_box():
    from victor_amd.chains import sample_chains
    # the constant of the quadrature: the integral over the box of exp(-r^2 / (2 sigma^2)), a product of two error functions
    one = 0.1 * math.sqrt(math.pi / 2.0) * (math.erf(0.7 / (0.1 * math.sqrt(2.0))) + math.erf(0.3 / (0.1 * math.sqrt(2.0))))
    assert abs(2.0 * math.log(one) - EXACT_LN_Z) < 1e-5

    def evaluate(batch):
        u, v = batch["a"] - 0.3, batch["b"] - 0.3
        return -0.5 * ((u * u + v * v) / 0.01)

    block = {n: {"prior": {"min": 0.0, "max": 1.0}, "ref": {"loc": 0.3, "scale": 0.05}, "proposal": 0.1} for n in ("a", "b")}
    ch = sample_chains(None, block, 4000, walkers=8, seed=5, device=False, evaluate=evaluate, burn=500,
                       temper={"rungs": 16, "power": 5, "swap_every": 4})
    q = ch.tempering
    print("ln_evidence", q.ln_evidence[0], "trapezoid", q.ln_evidence_trapezoid[0], "error", q.ln_evidence_error[0], "exact", EXACT_LN_Z,
          "swap acceptance", q.swap_acceptance.min(), q.swap_acceptance.mean())
    assert q.betas.shape == (16,) and q.mean_lnl.shape == (1, 16) and q.swap_acceptance.shape == (1, 15)
    assert abs(q.ln_evidence[0] - EXACT_LN_Z) <= 0.05
    assert 0.0 < q.ln_evidence_error[0] < 0.05
    assert np.all(q.swap_acceptance > 0.5)
    # the pieces: <lnL> falls from the posterior's -1 (d / 2 = 1 below the peak) towards the prior's mean; the variance at
    # beta = 1 is that of a chi-square with two degrees of freedom over two: 1
    assert q.mean_lnl[0, -1] < q.mean_lnl[0, 8] < q.mean_lnl[0, 0] and abs(q.mean_lnl[0, 0] + 1.0) < 0.1 and abs(q.var_lnl[0, 0] - 1.0) < 0.25
    assert ch.x.shape == (1, 8, 2) and ch.rhat is not None and np.all(ch.rhat < 1.05)


def test_energy_moments_pool_the_walkers():
    from victor_amd.tempering import energy_moments, trapezoid_weights
    rng = np.random.default_rng(1)
    v = rng.normal(-40.0, 3.0, (2, 3, 4, 50))                # (R, K, W, n)
    pivot = v[..., 0]
    a = v - pivot[..., None]
    mean, var, walker = energy_moments(np.full((2, 3, 4), 50), pivot, a.sum(axis=-1), (a * a).sum(axis=-1))
    assert np.allclose(mean, v.reshape(2, 3, -1).mean(axis=2), rtol=1e-13) and np.allclose(var, v.reshape(2, 3, -1).var(axis=2, ddof=1), rtol=1e-11)
    assert np.allclose(walker, v.mean(axis=-1), rtol=1e-13)
    b = np.array([1.0, 0.4, 0.1, 0.0])
    assert np.isclose(trapezoid_weights(b) @ (3.0 * b + 1.0), 2.5)       # exact for a straight line


# ------------------------------------------------------------------ refusals -----------------------------------------------
@pytest.mark.parametrize("temper,text", [
    ({"betas": [0.9, 0.5]}, "betas\\[0\\] must be 1"), ({"betas": [1.0, 0.5, 0.5]}, "decrease strictly"),
    ({"betas": [1.0, 0.5, 0.7]}, "decrease strictly"), ({"betas": [1.0, -0.1]}, "finite and >= 0"),
    ({"betas": [1.0, math.nan]}, "finite and >= 0"), ({"betas": []}, "at least one"), ({"rungs": 0}, "rungs >= 1"),
    ({"rungs": 4, "betas": [1.0, 0.0]}, "not both"), ({"rungs": 4, "power": 0}, "power > 0"), ({"swap_every": -1}, "swap_every >= 0"),
    ({"rungs": 3, "scales": [1.0, 2.0]}, "one finite factor"), ({"rungs": 3, "scales": [1.0, 0.0, 2.0]}, "one finite factor"),
    ({"ladder": 3}, "no option"), ("yes", "None, True or a dict")])
def test_a_bad_ladder_is_refused(temper, text):
    from victor_amd.utils import InputError
    with pytest.raises(InputError, match=text):
        tempered("gauss", 10, temper)


def test_stretch_and_too_many_chains_are_refused():
    from victor_amd.chains import sample_chains
    from victor_amd.utils import InputError
    called = []

    def evaluate(batch):
        called.append(1)
        return np.zeros(len(batch["a"]))
    with pytest.raises(InputError, match="Metropolis move only"):
        sample_chains(None, block_for("gauss"), 10, walkers=8, device=False, evaluate=evaluate, move="stretch", temper=True)
    with pytest.raises(InputError, match="1 problems x 16 rungs x 4097 walkers = 65552 chains: at most 65536"):
        sample_chains(None, block_for("gauss"), 10, walkers=4097, device=False, evaluate=evaluate, temper=True)
    assert not called
    ch = sample_chains(None, block_for("gauss"), 0, walkers=2, device=False, evaluate=evaluate, temper={"rungs": 2})
    assert ch.tempering.x.shape == (1, 2, 2, 3) and ch.x.shape == (1, 2, 3)


def test_the_abi_declares_the_tempering_symbols():
    import re
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    for name in ("vk_chain_set_tempering", "vk_chain_begin_tempered", "vk_chain_tempering"):
        assert re.search(r"\bint %s\(vk_chain\* f" % name, header) and name in N.SYMBOLS
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22          # the symbols are additive
    sampled = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_sampled.hip")).read()
    assert '#include "vk_kernel_temper.h"' in sampled
