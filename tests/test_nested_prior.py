"""Nested sampling under a Gaussian prior (victor_amd/nested.py, ``prior=``; vk_nprior_set) without a GPU: the prior forms of
victor_amd/csrc/vk_nested_step.h with vk_prior.h compiled on their own under g++ and held, byte for byte, to the NumPy loop that
defines the run; the evidence against closed forms; the closed-form normalisation; the read-out identities; and the surface - the
two C symbols, the four method signatures and the refusals, raised before the library is entered.

The evidence caps are those of tests/test_nested.py, conditions and not measurements: every run within 4 of its own
``ln_evidence_error`` of the truth, the mean over seeds 0 .. 7 within 4 rms(error) / sqrt(8).  The truths are closed forms (A) and
a 2000 x 2000 midpoint quadrature (B), computed here and held to the figures the cases were specified with."""

import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import same_bytes
from tests.test_nested import LNL_OF, NESTED, SEEDS, _NoLibrary, block_for, evaluate_of, randoms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_nested_step.h"
#include "vk_prior.h"

""" + LNL_OF + r"""
// usage: driver fn d R L K S T scale in out
// in:  doubles x0[R][L][d], pick[T][R][K], dz[T][S][R][K][d], mu[d], pp[d (d + 1) / 2]; the box is [-1, 1]^d
// out: doubles, per iteration: the dead record lnl[R][K], lnprior[R][K], x[R][K][d]; at the end the live x[R][L][d], lnl[R][L],
//      chi2[R][L], lnprior[R][L] and n_accept[R], n_steps[R], n_stuck[R]
// The state is held structure-of-arrays, live points with stride R L and walkers with stride R K, as the device holds it.
int main(int argc, char** argv) {
  const char* fn = argv[1];
  vkchain::Box box{};
  box.d = atoi(argv[2]);
  const int d = box.d, R = atoi(argv[3]), L = atoi(argv[4]), K = atoi(argv[5]), S = atoi(argv[6]), T = atoi(argv[7]);
  const double scale = strtod(argv[8], nullptr);
  for (int j = 0; j < d; ++j) {
    box.lo[j] = -1.0;
    box.hi[j] = 1.0;
  }
  const size_t RL = (size_t)R * L, RK = (size_t)R * K, tri = (size_t)d * (d + 1) / 2;
  std::vector<double> in(RL * d + (size_t)T * RK + (size_t)T * S * RK * d + d + tri);
  FILE* fi = fopen(argv[9], "rb");
  if (!fi || fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const double *x0 = in.data(), *pick = x0 + RL * d, *dz = pick + (size_t)T * RK, *mu = dz + (size_t)T * S * RK * d, *pp = mu + d;
  vkprior::Prior prior{};
  prior.on = 1;
  for (int j = 0; j < d; ++j) prior.mu[j] = mu[j];
  for (size_t i = 0; i < tri; ++i) prior.pp[i] = pp[i];
  std::vector<double> lx(RL * d), llnl(RL), lchi(RL), llp(RL), lpost(RL), wx(RK * d), wlnl(RK), wchi(RK), wlp(RK), range((size_t)R * d),
      lstar(R);
  std::vector<int64_t> n_accept(RK), n_steps(RK), n_stuck(RK);
  std::vector<int32_t> moved(RK);
  std::vector<int> slot(RK), rank(L);
  auto walker = [&](size_t c) {
    vknest::Walker w{};
    w.stride = RK;
    w.y = wx.data() + c; w.lnl = wlnl.data() + c; w.chi2 = wchi.data() + c; w.lnprior = wlp.data() + c;
    w.n_accept = n_accept.data() + c; w.n_steps = n_steps.data() + c; w.n_stuck = n_stuck.data() + c; w.moved = moved.data() + c;
    return w;
  };
  FILE* fo = fopen(argv[10], "wb");
  if (!fo) return 2;
  auto put = [&](double v) { fwrite(&v, sizeof(double), 1, fo); };
  double row[vknest::kMaxP];
  for (size_t i = 0; i < RL; ++i) {
    for (int j = 0; j < d; ++j) lx[j * RL + i] = row[j] = x0[i * d + j];
    const double l = lnl_of(fn, row);
    llnl[i] = vkchain::stored(l);
    lchi[i] = -2.0 * l;
    llp[i] = vkprior::lnprior(prior, d, [&](int j) { return lx[j * RL + i]; });
  }
  for (int t = 0; t < T; ++t) {
    for (size_t i = 0; i < RL; ++i) lpost[i] = llnl[i] + llp[i];
    for (int r = 0; r < R; ++r) {
      const size_t first = (size_t)r * L;
      for (int j = 0; j < d; ++j) range[(size_t)r * d + j] = vknest::range_of(L, [&](int i) { return lx[j * RL + first + i]; });
      for (int i = 0; i < L; ++i) {
        rank[i] = vknest::rank_of(L, i, [&](int m) { return lpost[first + m]; });
        if (rank[i] < K) slot[(size_t)r * K + rank[i]] = i;
      }
      lstar[r] = lpost[first + slot[(size_t)r * K + K - 1]];
      for (int k = 0; k < K; ++k) put(llnl[first + slot[(size_t)r * K + k]]);
    }
    for (int r = 0; r < R; ++r)
      for (int k = 0; k < K; ++k) put(llp[(size_t)r * L + slot[(size_t)r * K + k]]);
    for (int r = 0; r < R; ++r)
      for (int k = 0; k < K; ++k)
        for (int j = 0; j < d; ++j) put(lx[j * RL + (size_t)r * L + slot[(size_t)r * K + k]]);
    for (int r = 0; r < R; ++r) {
      const size_t first = (size_t)r * L;
      for (int i = 0; i < L; ++i) rank[i] = vknest::rank_of(L, i, [&](int m) { return lpost[first + m]; });
      for (int k = 0; k < K; ++k) {
        const size_t c = (size_t)r * K + k;
        const int q = vknest::pick_of(pick[(size_t)t * RK + c], L, K);
        const int from = vknest::survivor_of(L, K, q, [&](int i) { return rank[i]; });
        vknest::Walker w = walker(c);
        vknest::start(d, w, [&](int j) { return lx[j * RL + first + from]; }, llnl[first + from], lchi[first + from]);
        *w.lnprior = llp[first + from];
      }
    }
    for (int s = 0; s < S; ++s)
      for (int r = 0; r < R; ++r)
        for (int k = 0; k < K; ++k) {
          const size_t c = (size_t)r * K + k;
          vknest::Walker w = walker(c);
          const double* inc = dz + (((size_t)t * S + s) * RK + c) * d;
          auto rg = [&](int j) { return range[(size_t)r * d + j]; };
          const bool in_box = vknest::proposal_inside(box, w, scale, rg, inc);      // the row the launch evaluates
          for (int j = 0; j < d; ++j) row[j] = in_box ? vknest::proposed(w.y[j * w.stride], scale, rg(j), inc[j]) : w.y[j * w.stride];
          const double l = lnl_of(fn, row);
          vknest::transition(box, prior, w, scale, rg, inc, lstar[r], l, -2.0 * l);
        }
    for (size_t c = 0; c < RK; ++c) {
      const size_t at = (c / K) * L + slot[c];
      vknest::Walker w = walker(c);
      vknest::commit(d, w, lx.data() + at, RL, llnl.data() + at, lchi.data() + at, llp.data() + at);
    }
  }
  for (size_t i = 0; i < RL; ++i)
    for (int j = 0; j < d; ++j) put(lx[j * RL + i]);
  for (size_t i = 0; i < RL; ++i) put(llnl[i]);
  for (size_t i = 0; i < RL; ++i) put(lchi[i]);
  for (size_t i = 0; i < RL; ++i) put(llp[i]);
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


def lowest_differ(ns):
    """Iterations of a run (its record kept) in which the K points lowest in lnpost were NOT the K lowest in lnL: the dead
    record's largest lnL exceeds the smallest lnL that stayed alive.  Needs the trace of the definition route."""
    n = 0
    for t, it in enumerate(ns._trace):
        before = ns._trace[t - 1]["lnl"] if t else None
        if before is None:
            continue
        for r in range(ns.R):
            alive = np.delete(before[r], it["dead"][r])
            n += bool(before[r][it["dead"][r]].max() > alive.min())
    return n


# ------------------------------------------------------------------ 1. three compilers, one decision -------------------------
def test_header_under_a_prior_against_numpy_byte_for_byte(tmp_path):
    from victor_amd.nested import NestedSampling
    from victor_amd.priors import GaussianPrior, resolve_prior
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    R, L, K, S, d, T, scale = 2, 8, 2, 3, 3, 16, 0.5
    prior = GaussianPrior(["p2", "p0"], [0.4, -0.3], cov=[[0.16, 0.1], [0.1, 0.25]])       # correlated, on two of the three
    names, lo, hi = [f"p{j}" for j in range(d)], -np.ones(d), np.ones(d)
    function = evaluate_of("gauss", d)

    def evaluator(x, rows_which=None):
        return function({n: x[:, j] for j, n in enumerate(names)})
    # two problems against the same function from the same start: they part at the first pick
    ns = NestedSampling(names, lo, hi, {}, R, L, K, S, scale, 3, 1e-3, True, evaluator, None, None,
                        prior=resolve_prior(prior, "test", names, lo, hi))
    ns.ln_prior_norm = ns.ln_prior_norm_error = 0.0
    x0 = ns.start_points()
    ns._start_host(x0)
    ns._trace = []
    ns.extend(T)
    _, pick, dz = randoms(ns, T)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([x0.ravel(), pick.ravel(), dz.ravel(), ns.prior.mu, ns.prior.pp]).astype(np.float64).tofile(str(fin))
    subprocess.run([str(exe), "gauss", str(d), str(R), str(L), str(K), str(S), str(T), repr(scale), str(fin), str(fout)], check=True)
    out = np.fromfile(str(fout), dtype=np.float64)
    at = 0

    def take(*shape):
        nonlocal at
        n = int(np.prod(shape))
        a = out[at:at + n].reshape(shape)
        at += n
        return a
    for t in range(T):
        for key, shape in (("dead_lnl", (R, K)), ("dead_lnprior", (R, K)), ("dead_x", (R, K, d))):
            assert same_bytes(take(*shape), getattr(ns, key)[t]), (t, key)
    for key, shape in (("x", (R, L, d)), ("lnl", (R, L)), ("chi2", (R, L)), ("lnprior", (R, L))):
        assert same_bytes(take(*shape), getattr(ns, key)), key
    assert np.array_equal(take(3, R).astype(np.int64), [ns.n_accept, ns.n_steps, ns.n_stuck]) and at == len(out)
    # conditions on the inputs, not on the code under test: the two orders differ somewhere, both outcomes of a step occurred
    assert lowest_differ(ns) > 0
    assert np.all((0 < ns.n_accept) & (ns.n_accept < ns.n_steps)) and not same_bytes(ns.dead_lnl[:, 0], ns.dead_lnl[:, 1])
    assert same_bytes(ns.dead_lnprior, ns.prior.lnprior(ns.dead_x)) and same_bytes(ns.lnprior, ns.prior.lnprior(ns.x))


# ------------------------------------------------------------------ 2. the evidence against closed forms ---------------------
def _half_erf(a, b, m, s):
    """integral over [a, b] of exp(-(x - m)^2 / (2 s^2))"""
    return s * math.sqrt(math.pi / 2.0) * (math.erf((b - m) / (s * math.sqrt(2.0))) - math.erf((a - m) / (s * math.sqrt(2.0))))


def _within_caps(runs, truth, what, attr="ln_evidence", errors=None):
    diff = np.array([getattr(r, attr)[0] for r in runs]) - truth
    err = np.array([r.ln_evidence_error[0] for r in runs]) if errors is None else errors
    cap = 4.0 * math.sqrt(float(np.mean(err * err))) / math.sqrt(len(runs))
    print(what, attr, "truth", truth, "differences", np.round(diff, 3), "errors", np.round(err, 3), "pulls", np.round(diff / err, 2),
          "seed mean", diff.mean(), "cap", cap, "iterations", [r.n_iter for r in runs])
    assert all(r.status_names == ["OK"] for r in runs), what
    assert np.all(np.abs(diff) <= 4.0 * err), (what, attr, diff / err)
    assert abs(diff.mean()) <= cap, (what, attr, diff.mean(), cap)


CENTRE, WIDTH = np.array([0.1, -0.2, 0.3]), np.array([0.05, 0.1, 0.2])


def _gauss3(batch):
    x = np.stack([batch[f"p{j}"] for j in range(3)], axis=1)
    return -0.5 * (((x - CENTRE) / WIDTH) ** 2).sum(axis=1)


def _truth_a():
    ln_unnorm, ln_norm = 0.0, 0.0
    for c, s, pr in zip(CENTRE, WIDTH, ((0.2, 0.1), None, (0.0, 0.3))):
        if pr is None:
            ln_unnorm += math.log(_half_erf(-1.0, 1.0, c, s) / 2.0)
            continue
        mu, sg = pr
        v = s * s * sg * sg / (s * s + sg * sg)
        m = (c * sg * sg + mu * s * s) / (s * s + sg * sg)
        ln_unnorm += -0.5 * (c - mu) ** 2 / (s * s + sg * sg) + math.log(_half_erf(-1.0, 1.0, m, math.sqrt(v)) / 2.0)
        ln_norm += math.log(_half_erf(-1.0, 1.0, mu, sg) / 2.0)
    return ln_unnorm, ln_norm


@pytest.fixture(scope="module")
def runs_a():
    from victor_amd.nested import run_definition
    from victor_amd.priors import GaussianPrior
    prior = [GaussianPrior("p0", 0.2, sigma=0.1), GaussianPrior("p2", 0.0, sigma=0.3)]
    return prior, [run_definition(block_for(3), _gauss3, seed=s, prior=prior) for s in SEEDS]


def test_evidence_under_independent_priors(runs_a):
    prior, runs = runs_a
    ln_unnorm, ln_norm = _truth_a()
    assert abs(ln_unnorm + 7.27197) < 1e-5 and abs(ln_norm + 3.05583) < 1e-5 and abs(ln_unnorm - ln_norm + 4.21614) < 2e-5
    assert runs[0].n_live == 256 and runs[0].batch == 32 and runs[0].steps == 16 and runs[0].prior_norm == "exact"
    shrink = np.array([math.sqrt(r.information[0] / r.n_live) for r in runs])
    _within_caps(runs, ln_unnorm, "(A)", "ln_evidence_unnormalised", shrink)
    _within_caps(runs, ln_unnorm - ln_norm, "(A) exact")
    for r in runs:
        assert r.ln_prior_norm_error == 0.0 and abs(r.ln_prior_norm - ln_norm) < 1e-14 and same_bytes(r.ln_evidence_error, np.sqrt(r.information / r.n_live + 0.0))
        assert same_bytes(r.ln_evidence, r.ln_evidence_unnormalised - r.ln_prior_norm)


def test_evidence_under_independent_priors_normalised_by_its_own_run(runs_a):
    from victor_amd.nested import run_definition
    prior, exact = runs_a
    ln_unnorm, ln_norm = _truth_a()
    runs = [run_definition(block_for(3), _gauss3, seed=s, prior=prior, prior_norm="nested") for s in SEEDS]
    for r, e in zip(runs, exact):
        assert r.prior_norm == "nested" and r.ln_prior_norm_error > 0.0
        assert same_bytes(r.ln_evidence_unnormalised, e.ln_evidence_unnormalised) and same_bytes(r.dead_lnl, e.dead_lnl)
        assert same_bytes(r.ln_evidence_error, np.sqrt(r.information / r.n_live + r.ln_prior_norm_error ** 2))
    norms = np.array([r.ln_prior_norm for r in runs])
    errs = np.array([r.ln_prior_norm_error for r in runs])
    print("(A) normalisation runs [seed, 3 .. 5]: pulls", np.round((norms - ln_norm) / errs, 2), "seed mean", (norms - ln_norm).mean())
    _within_caps(runs, ln_unnorm - ln_norm, "(A) nested")


def test_normalisation_of_a_correlated_prior():
    """(B): the prior alone (lnL = 0), as the main run with the streams [seed, 0 .. 2] and as the product's normalisation run with
    [seed, 3 .. 5]."""
    from victor_amd.nested import nested_prior_norm, run_definition
    from victor_amd.priors import GaussianPrior
    mu, cov = np.array([0.3, -0.1]), np.array([[0.09, 0.036], [0.036, 0.04]])
    n = 2000
    g = -1.0 + (np.arange(n) + 0.5) * (2.0 / n)
    P = np.linalg.inv(cov)
    u, v = g[:, None] - mu[0], g[None, :] - mu[1]
    truth = math.log(np.exp(-0.5 * (P[0, 0] * u * u + 2.0 * P[0, 1] * u * v + P[1, 1] * v * v)).mean())
    assert abs(truth + 2.59485) < 1e-5
    prior = GaussianPrior(["p0", "p1"], mu, cov=cov)
    runs = [run_definition(block_for(2), lambda b: np.zeros(len(b["p0"])), seed=s, prior=prior) for s in SEEDS]
    shrink = np.array([math.sqrt(r.information[0] / r.n_live) for r in runs])
    _within_caps(runs, truth, "(B) main streams", "ln_evidence_unnormalised", shrink)
    # the same problem as the product normalises it: auto chose the prior's own run
    assert all(r.prior_norm == "nested" for r in runs)
    norms = np.array([r.ln_prior_norm for r in runs]) - truth
    errs = np.array([r.ln_prior_norm_error for r in runs])
    cap = 4.0 * math.sqrt(float(np.mean(errs * errs))) / math.sqrt(len(runs))
    print("(B) normalisation streams: differences", np.round(norms, 3), "pulls", np.round(norms / errs, 2), "seed mean", norms.mean(), "cap", cap)
    assert np.all(np.abs(norms) <= 4.0 * errs) and abs(norms.mean()) <= cap
    r = runs[0]
    value, error = nested_prior_norm(r.prior, r.names, r._lo, r._hi, r.n_live, r.batch, r.steps, r.scale, 0, r.tol, 128 * 8)
    assert value == r.ln_prior_norm and error == r.ln_prior_norm_error
    # lnL = 0 and the evidence normalised by a run of the same problem: ln Z scatters about 0
    _within_caps(runs, 0.0, "(B) ln Z of lnL = 0")


# ------------------------------------------------------------------ 3. the closed-form normalisation -------------------------
def test_closed_form_normalisation_and_its_refusal():
    from victor_amd import InputError
    from victor_amd.nested import exact_prior_norm, run_definition
    from victor_amd.priors import GaussianPrior, resolve_prior
    names, lo, hi = ["a", "b", "c"], np.array([0.0, -2.0, 100.0]), np.array([1.0, 3.0, 500.0])
    want = sum(math.log(s * math.sqrt(math.pi / 2.0) * (math.erf((h - m) / (s * math.sqrt(2.0))) - math.erf((l - m) / (s * math.sqrt(2.0)))) / (h - l))
               for m, s, l, h in ((380.0, 25.0, 100.0, 500.0), (0.9, 0.4, 0.0, 1.0)))
    for prior in ([GaussianPrior(["c", "a"], [380.0, 0.9], sigma=[25.0, 0.4])],
                  [GaussianPrior("c", 380.0, sigma=25.0), GaussianPrior("a", 0.9, cov=[[0.4 * 0.4]])],
                  GaussianPrior(["a", "c"], [0.9, 380.0], cov=np.diag([0.4 * 0.4, 25.0 * 25.0]))):
        got = exact_prior_norm(resolve_prior(prior, "t", names, lo, hi), lo, hi)
        assert abs(got - want) <= 1e-14, (got, want)
    corr = GaussianPrior(["a", "b"], [0.5, 0.0], cov=[[0.04, 0.01], [0.01, 0.09]])
    assert exact_prior_norm(resolve_prior(corr, "t", names, lo, hi), lo, hi) is None
    with pytest.raises(InputError, match="prior_norm='exact' needs independent priors"):
        run_definition({n: {"prior": {"min": l, "max": h}} for n, l, h in zip(names, lo, hi)}, lambda b: np.zeros(len(b["a"])),
                       prior=corr, prior_norm="exact", n_iter=0)


# ------------------------------------------------------------------ 4. the read-out ------------------------------------------
def test_read_out_identities():
    from victor_amd.nested import read_out, run_definition
    from victor_amd.priors import GaussianPrior
    ns = run_definition(block_for(3), evaluate_of("gauss", 3), n_live=16, batch=4, steps=4, n_iter=12, seed=1)
    plain = read_out(ns.dead_lnl, ns.lnl, 16, 4)
    # ln prior = 0: not a bit moves
    zero = read_out(ns.dead_lnl, ns.lnl, 16, 4, dead_lnprior=np.zeros_like(ns.dead_lnl), live_lnprior=np.zeros_like(ns.lnl))
    assert same_bytes(zero["ln_evidence"], plain["ln_evidence"]) and same_bytes(np.exp(zero["log_weights"]).astype(float), ns.weights)
    # ln prior = c: the evidence moves by c and the weights stay, up to the one rounded addition lnL + c (relative 2^-53 of values
    # below 64 in size: 1e-14 absolute in a log weight, so 1e-12 covers the sums)
    c = -1.75
    const = read_out(ns.dead_lnl, ns.lnl, 16, 4, dead_lnprior=np.full_like(ns.dead_lnl, c), live_lnprior=np.full_like(ns.lnl, c))
    assert np.all(np.abs(ns.dead_lnl) < 64.0) and np.all(np.abs(ns.lnl) < 64.0)
    assert abs((const["ln_evidence"][0] - c) - plain["ln_evidence"][0]) <= 1e-12
    assert abs(const["information"][0] - plain["information"][0]) <= 1e-12
    assert np.allclose(np.exp(const["log_weights"]).astype(float), ns.weights, rtol=1e-12, atol=0.0)
    # a run under a prior: the weights sum to 1, and every published number is the read-out of lnL + ln prior
    pr = run_definition(block_for(3), evaluate_of("gauss", 3), n_live=16, batch=4, steps=4, n_iter=12, seed=1,
                        prior=GaussianPrior("p0", 0.2, sigma=0.3))
    assert abs(pr.weights.sum() - 1.0) <= 1e-12 and pr.weights.shape == (1, 12 * 4 + 16)
    direct = read_out(pr.dead_lnl + pr.dead_lnprior, pr.lnl + pr.lnprior, 16, 4)
    assert same_bytes(direct["ln_evidence"], pr.ln_evidence_unnormalised) and same_bytes(direct["information"], pr.information)
    assert same_bytes(pr.ln_evidence, pr.ln_evidence_unnormalised - pr.ln_prior_norm) and pr.prior_norm == "exact"
    post = (pr.dead_lnl + pr.dead_lnprior).transpose(1, 0, 2).reshape(1, -1)
    assert np.all(np.diff(post, axis=1) >= 0) and not np.all(np.diff(pr.dead_lnl.transpose(1, 0, 2).reshape(1, -1), axis=1) >= 0)
    # without a prior: the new attributes are None and the unnormalised evidence is the evidence
    assert ns.prior is None and ns.dead_lnprior is None and ns.lnprior is None and ns.ln_prior_norm is None
    assert ns.ln_prior_norm_error is None and ns.prior_norm is None and ns.ln_evidence_unnormalised is ns.ln_evidence
    # the start is the same bytes with and without a prior, and extend() goes on under it
    assert same_bytes(pr.start_points(), ns.start_points())
    longer = run_definition(block_for(3), evaluate_of("gauss", 3), n_live=16, batch=4, steps=4, n_iter=7, seed=1,
                            prior=GaussianPrior("p0", 0.2, sigma=0.3)).extend(5)
    assert same_bytes(longer.dead_lnprior, pr.dead_lnprior) and same_bytes(longer.ln_evidence, pr.ln_evidence)


# ------------------------------------------------------------------ 5. the surface -------------------------------------------
NPRIOR = ("vk_nprior_set", "vk_nprior_record")


def test_the_abi_declares_exports_and_binds_the_prior_symbols():
    from victor_amd import _native
    from victor_amd.build import build_native
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert set(re.findall(r"\b(vk_nprior_[a-z0-9_]+)\s*\(", header)) == set(NPRIOR) <= set(_native.SYMBOLS)
    assert set(re.findall(r"\b(vk_nested_[a-z0-9_]+)\s*\(", header)) == set(NESTED)
    assert int(re.search(r"#define VK_ABI_VERSION (\d+)", header).group(1)) == _native.VK_ABI_VERSION == 22
    build_native()
    lib = _native.load()
    for name in NPRIOR:
        assert hasattr(lib, name), name
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_nested_step.h")).read()
    assert "#include <hip" not in src and '#include "vk_prior.h"' in src


def test_the_four_methods_have_one_signature():
    import victor_amd
    sigs = [inspect.signature(getattr(cls, "nested_sampling")) for cls in
            (victor_amd.CCFFit, victor_amd.Realisations, victor_amd.JointFit, victor_amd.JointRealisations)]
    assert all(s == sigs[0] for s in sigs)
    names = list(sigs[0].parameters)
    assert names[-3:] == ["prior", "prior_norm", "kwargs"] and sigs[0].parameters["prior"].default is None
    assert sigs[0].parameters["prior_norm"].default == "auto"


def test_prior_refusals_come_before_the_library(monkeypatch):
    import victor_amd
    from tests import cases
    from victor_amd import InputError
    from victor_amd.priors import GaussianPrior
    monkeypatch.setattr(victor_amd.CCFFit, "_get_engine", lambda self, *a, **k: _NoLibrary())
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    params = cases.cobaya_info()["params"]
    ok = GaussianPrior("sigma_v", 380.0, sigma=30.0)
    corr = GaussianPrior(["fsigma8", "sigma_v"], [0.5, 380.0], cov=[[0.01, 0.5], [0.5, 900.0]])
    for kw, text in ((dict(prior=object()), r"nested_sampling: prior= is not accepted: it must be a GaussianPrior or a list of them"),
                     (dict(prior=[]), "prior= is not accepted"), (dict(prior=[ok, 3]), "prior= is not accepted"),
                     (dict(prior=ok, prior_norm="grid"), "prior_norm must be"),
                     (dict(prior=corr, prior_norm="exact"), "needs independent priors"),
                     (dict(prior=GaussianPrior("Omega_m", 0.3, sigma=0.1)), "which is not sampled"),
                     (dict(prior=ok, fixed={"sigma_v": 380.0}), "it is fixed"),
                     (dict(prior=GaussianPrior("sigma_v", 600.0, sigma=30.0)), "outside its box"),
                     (dict(prior=GaussianPrior("sigma_v@1", 380.0, sigma=30.0)), "needs a JointFit"),
                     (dict(prior=[ok, GaussianPrior("sigma_v", 300.0, sigma=30.0)]), "named by two priors")):
        with pytest.raises(InputError, match=text):
            fit.nested_sampling(params, **kw)
    from victor_amd.nested import run_definition
    with pytest.raises(InputError, match="which is not sampled"):
        run_definition(block_for(2), evaluate_of("quad", 2), n_iter=0, prior=GaussianPrior("sigma_v", 380.0, sigma=30.0))
