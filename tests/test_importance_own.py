"""Importance-sampled posteriors with a proposal per problem (victor_amd/importance.py rule 8, vk_is_create_own) without a GPU:
the layouts and index rules of victor_amd/csrc/vk_importance.h compiled on their own under g++ against the NumPy definition;
the definition route on eight Gaussian problems scattered over their box, against the closed-form evidence and against the
pooled proposal; identical proposals against the shared route; ``ProposalSet``; the refusals; the C ABI's surface.

How the header is held to the definition: as tests/test_importance.py holds it.  The driver's exp is libm's and the definition's
is NumPy's, which may differ in the last place, so maxima, arg max, counts and statuses are compared as bytes and the sums at
that module's derived bound (:func:`tests.test_importance.sum_bound`), per problem over the points it holds inside the box; a
second sample whose lnpost takes the values 0 and -inf alone (weights 0 and 1, exact under any exp) is compared as bytes
throughout.

Identical proposals against the shared route: with ``sample=`` / ``ln_proposal=`` the shared route centres ``y`` on the mean of
the kept points (rule 1), rule 8 on the proposal's mean, so ``s1`` and ``s2`` cannot agree as bytes with that call; they are
compared as bytes with the shared route given the same ``GaussianProposal`` and seed (the same points, by the common random
numbers), and every field that does not hold ``y`` with both."""

import copy
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import same_bytes
from tests.test_importance import EXACT, SUMS, assert_exact, assert_sums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------ 1. vk_importance.h's own-mode rules against the definition --
DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vk_importance.h"

static std::vector<double> in;
static size_t at = 0;
static double get() { return in[at++]; }

// own d R G chunk n_lists prior    in: cells[n_lists], y[G][R][d], lnl[G][R], lno[G][R], lists[R][n_lists][G],
//                                  offsets[n_chunks][R][cells + n_lists]
// out per problem r < Rp (Rp = 2 R with a prior, problem R + r the prior problem of r): M, arg, n_finite, the accumulators
int main(int argc, char** argv) {
  FILE* fi = fopen(argv[argc - 2], "rb");
  FILE* fo = fopen(argv[argc - 1], "wb");
  if (!fi || !fo) return 2;
  fseek(fi, 0, SEEK_END);
  in.resize((size_t)ftell(fi) / sizeof(double));
  fseek(fi, 0, SEEK_SET);
  if (in.size() && fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  auto ex = [](double x) { return exp(x); };
  const int d = atoi(argv[1]), R = atoi(argv[2]), G = atoi(argv[3]), chunk = atoi(argv[4]), n_lists = atoi(argv[5]);
  const bool prior = atoi(argv[6]) != 0;
  const int Rp = prior ? 2 * R : R;
  std::vector<int> cells(n_lists), cell_off(n_lists + 1, 0);
  for (int l = 0; l < n_lists; ++l) cells[l] = (int)get(), cell_off[l + 1] = cell_off[l] + cells[l];
  const long long per = cell_off[n_lists] + n_lists;
  const int n_chunks = (G + chunk - 1) / chunk;
  const double* y = &in[at];
  at += (size_t)G * R * d;
  const double* lnl = &in[at];
  at += (size_t)G * R;
  const double* lno = &in[at];
  at += (size_t)G * R;
  std::vector<int> lists((size_t)R * n_lists * G), offsets((size_t)n_chunks * R * per);
  for (int& v : lists) v = (int)get();
  for (int& v : offsets) v = (int)get();
  if (at != in.size()) return 6;
  const int W = vkis::whole(d), A = W + cell_off[n_lists];
  std::vector<vkgrid::Running> run(Rp, vkgrid::start());
  std::vector<double> acc((size_t)Rp * A, 0.0), w(chunk);
  for (long long c = 0; c < n_chunks; ++c) {
    const long long g0 = c * chunk;
    const int n = (int)(G - g0 < chunk ? G - g0 : chunk);
    for (int r = 0; r < Rp; ++r) {
      const int p = vkis::prior_of(r, R);
      if (vkis::prior_of(p, R) != p || (r >= R) != (p != r)) return 5;
      auto post = [&](long long i) {
        const long long v = vkis::value_at(g0 + i, p, R);
        if (v != vkis::own_row(g0 + i, p, R)) return (double)NAN;          // ([G][R] values and rows share their index)
        if (r >= R) return vkgrid::clean(lno[v]);
        double s = lnl[v];
        s = s + lno[v];
        return vkgrid::clean(s);
      };
      vkgrid::Best part[2] = {vkgrid::none(), vkgrid::none()};
      for (int i = 0; i < n; ++i) vkgrid::see(part[i % 2], post(i), g0 + i);
      vkgrid::advance(run[r], vkgrid::merge(part[1], part[0]), ex);
      const bool live = run[r].m > vkgrid::neg_inf();
      for (int i = 0; i < n; ++i) w[i] = live ? vkgrid::weight(post(i), run[r].m, ex) : 0.0;
      for (int a = 0; a < A; ++a) {
        if (r >= R && a != vkis::kTotal) continue;
        double& s = acc[(size_t)r * A + a];
        if (a == vkis::kSq) vkis::rescale_sq(s, run[r].factor);
        else vkgrid::rescale(s, run[r].factor);
        if (!live) continue;
        auto add = [&](double t) { vkgrid::add(s, t); };
        const double* yc = y + vkis::value_at(g0, p, R) * d;               // y of (g0 + i, p) at yc[i R d + j]
        const size_t step = (size_t)R * d;
        if (a == vkis::kTotal) {
          vkis::range_ahead<4>(0, n, [&](int i) { return w[i]; }, add);
        } else if (a == vkis::kSq) {
          vkis::range_ahead<3>(0, n, [&](int i) { return vkis::square_term(w[i]); }, add);
        } else if (a < vkis::kFirst + d) {
          const int j = a - vkis::kFirst;
          vkis::range_ahead<4>(0, n, [&](int i) { return vkis::first_term(w[i], yc[i * step + j]); }, add);
        } else if (a < W) {
          int j, k;
          vkis::second_of(d, a, j, k);
          vkis::range_ahead<5>(0, n, [&](int i) { return vkis::second_term(w[i], yc[i * step + j], yc[i * step + k]); }, add);
        } else {
          int l = 0;
          while (l + 1 < n_lists && a - W >= cell_off[l + 1]) ++l;
          const int k = a - W - cell_off[l];
          const int* seg = lists.data() + vkis::own_list(p, l, n_lists, G) + g0;
          const int* off = offsets.data() + vkis::own_offsets(c, p, R, per) + cell_off[l] + l;
          long long where;
          if (vkis::check_list(seg, off, cells[l], n, &where)) return 4;
          vkis::walk_ahead<4>(seg, off[k], off[k + 1], g0, [&](long long g) { return w[g - g0]; }, add);
        }
      }
    }
  }
  for (int r = 0; r < Rp; ++r) {
    const double head[3] = {run[r].m, (double)run[r].arg, (double)run[r].n_finite};
    fwrite(head, sizeof(double), 3, fo);
    fwrite(&acc[(size_t)r * A], sizeof(double), A, fo);
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
    d = tmp_path_factory.mktemp("importance_own_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    cmd = [gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr

    def run(args, arrays):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        done = subprocess.run([str(exe)] + [str(a) for a in args] + [str(fin), str(fout)], capture_output=True, text=True)
        assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
        return np.fromfile(str(fout), dtype=np.float64)
    return run


class FlatPrior:
    """ln prior = -8 |x - 0.5|^2: what OwnSample asks of a resolved prior."""

    @staticmethod
    def lnprior(x):
        return -8.0 * np.sum((np.asarray(x) - 0.5) ** 2, axis=-1)


def small_own(prior, exact_weights=False, seed=11):
    """R = 3, d = 2, n = 11 on the unit box with 3 bins per axis (axis 0 ranged to [0.2, 0.8]) and the pair: problem 1 has two
    points outside the box, every point of problem 2 is outside; lnL with -inf and NaN entries and a tie of the maximum."""
    from victor_amd.importance import OwnSample, resolve_layout
    n, R, d = 11, 3, 2
    rng = np.random.default_rng(seed)
    layout = resolve_layout("test", ["p0", "p1"], np.zeros(d), np.ones(d), 3, {"p0": (0.2, 0.8)}, [("p1", "p0")])
    x = rng.random((n, R, d))
    middle = (x[:, :, 0] >= 0.4) & (x[:, :, 0] < 0.6)
    x[:, :, 0][middle] -= 0.2                                     # the middle bin of axis 0 stays empty
    x[[2, 7], 1, 0] = [1.25, -0.5]
    x[:, 2, 1] += 1.0
    centre = np.array([[0.5, 0.5], [0.45, 0.55], [0.5, 0.6]])
    lnq = np.zeros((n, R)) if exact_weights else rng.normal(size=(n, R))
    smp = OwnSample(x, centre, lnq, np.zeros(d), np.ones(d), (FlatPrior if prior and not exact_weights else None))
    if prior and exact_weights:
        smp.lnop = smp.lno
    lnl = np.zeros((n, R)) if exact_weights else -20.0 * rng.random((n, R)) ** 2
    lnl[rng.random((n, R)) < 0.15] = -np.inf
    if not exact_weights:
        lnl[3, 0] = np.nan
        lnl[[1, 9], 0] = 5.0 - smp.lno[[1, 9], 0]                 # the maximum twice: the first index wins
    assert list(smp.n_inside) == [n, n - 2, 0] and np.all(smp.x[[2, 7], 1] == centre[1]) and np.all(smp.y[:, 2] == 0)
    assert np.all(smp.lno[[2, 7], 1] == -np.inf) and np.all(smp.lno[:, 2] == -np.inf)
    return layout, smp, lnl


def definition(layout, smp, lnl, chunk, tail=None):
    from victor_amd.importance import OwnLists, run_definition_own
    lists = OwnLists(layout, smp, chunk)
    cuts = iter(range(0, smp.G, chunk))

    def values(x, which):
        g0 = next(cuts)
        part = lnl[g0:g0 + chunk]
        assert same_bytes(x, smp.x[g0:g0 + chunk].reshape(-1, layout.d)) and list(which) == list(range(smp.R)) * len(part)
        return part.ravel()
    return lists, run_definition_own(layout, smp, lists, values, tail)


def one_problem(acc, r):
    from victor_amd.importance import Sums
    out = object.__new__(Sums)
    for name in EXACT + SUMS:
        setattr(out, name, getattr(acc, name)[r:r + 1])
    return out


def driver_sums(run, layout, smp, lnl, lists, prior):
    from victor_amd.importance import Sums
    d, R = layout.d, smp.R
    cells = [int(layout.cell_off[l + 1] - layout.cell_off[l]) for l in range(layout.n_lists)]
    Rp = 2 * R if prior else R
    out = run([d, R, smp.G, lists.chunk, layout.n_lists, int(prior)], [cells, smp.y, lnl, smp.lno, lists.entries, lists.offsets]).reshape(Rp, -1)
    W, T = 2 + d + d * (d + 1) // 2, d * (d + 1) // 2
    got = []
    for block in (out[:R], out[R:]):
        if not len(block):
            got.append(None)
            continue
        s = Sums(layout, R)
        s.ln_max, s.arg_max, s.n_finite = block[:, 0].copy(), block[:, 1].astype(np.int64), block[:, 2].astype(np.int64)
        a = block[:, 3:]
        s.total, s.sq, s.s1, s.s2 = a[:, 0].copy(), a[:, 1].copy(), a[:, 2:2 + d].copy(), a[:, 2 + d:2 + d + T].copy()
        s.h1, s.h2 = a[:, W:W + layout.n1].copy(), a[:, W + layout.n1:].copy()
        got.append(s)
    return got


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("chunk", [4, 11, 16])
def test_the_header_rules_against_the_numpy_definition(driver, chunk, prior):
    from victor_amd.importance import ImportancePosterior, OwnLists
    layout, smp, lnl = small_own(prior)
    lists, (want, pwant) = definition(layout, smp, lnl, chunk)
    got, pgot = driver_sums(driver, layout, smp, lnl, lists, prior)
    assert lists.n_chunks == -(-11 // chunk) and lists.entries.shape == (3, 3, 11) and lists.offsets.shape == (lists.n_chunks, 3, 5 + 5 + 9 + 3)
    assert_exact(got, want, f"own header, chunk {chunk}")
    assert want.arg_max[0] == 1 and want.n_finite[2] == 0 and want.ln_max[2] == -np.inf and want.total[2] == 0 and want.arg_max[2] == -1
    assert 0 < want.n_finite[1] <= 9
    empty = np.flatnonzero(np.all(np.diff(lists.offsets[:, 0, :6], axis=1) == 0, axis=0))
    assert len(empty) >= 1 and np.all(want.h1[0, empty] == 0)     # empty cells
    assert np.all(lists.offsets[:, 2] == 0)                       # every point of problem 2 is outside: it is in no list
    absolute_y = copy.copy(smp)
    absolute_y.y = np.abs(smp.y)
    _, (absolute, _) = definition(layout, absolute_y, lnl, chunk)
    for r in range(3):
        inside = smp.x[smp.inside[:, r], r]
        assert_sums(one_problem(got, r), one_problem(want, r), one_problem(absolute, r), lists.n_chunks, f"own header, chunk {chunk}, problem {r}",
                    layout, inside)
    if prior:
        assert same_bytes(pgot.ln_max, pwant.ln_max) and same_bytes(pgot.arg_max, pwant.arg_max) and same_bytes(pgot.n_finite, pwant.n_finite)
        assert np.allclose(pgot.total, pwant.total, rtol=1e-14, atol=0) and pwant.total[2] == 0
    ip = ImportancePosterior(layout, smp, lists, got, pgot, 1.0)
    assert list(ip.status) == [ip.OK, ip.OK, ip.NO_FINITE] and ip.ln_evidence[2] == -np.inf and list(ip.n_inside) == [11, 9, 0]
    assert isinstance(lists, OwnLists) and np.all(np.isnan(ip.mean[2])) and np.all(np.isfinite(ip.mean[:2]))
    if prior:
        assert ip.prior_ln_max.shape == ip.prior_total.shape == ip.prior_error.shape == (3,)


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("chunk", [4, 11, 16])
def test_the_header_rules_bit_for_bit_with_exact_weights(driver, chunk, prior):
    """lnpost takes the values 0 and -inf alone: every weight is 0 or 1 under any exp, and every field agrees as bytes."""
    layout, smp, lnl = small_own(prior, exact_weights=True)
    smp.lno[np.isfinite(smp.lno)] = 0.0
    lists, (want, pwant) = definition(layout, smp, lnl, chunk)
    got, pgot = driver_sums(driver, layout, smp, lnl, lists, prior)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(got, name), getattr(want, name)), name
    assert want.total[0] == want.n_finite[0] > 0 and np.any(want.s1[:2] != 0) and np.any(want.h2[:2] != 0)
    if prior:
        for name in EXACT + ("total",):
            assert same_bytes(getattr(pgot, name), getattr(pwant, name)), name
        assert list(pwant.total) == [11.0, 9.0, 0.0]


def test_lists_are_those_of_one_problem_at_a_time():
    """OwnLists, built over all problems at once, against Lists of every problem's inside points alone."""
    from victor_amd.importance import Lists, OwnLists
    layout, smp, _ = small_own(False)
    for chunk in (4, 11):
        own = OwnLists(layout, smp, chunk)
        for r in range(2):
            x = smp.x[:, r].copy()
            x[~smp.inside[:, r]] = 7.0                            # outside every pair range; the axis slots are taken out below
            ref = Lists(layout, x, chunk)
            for c in range(own.n_chunks):
                for l in range(layout.n_lists):
                    e, off = own.of(r).members(layout, c, l)
                    e0, off0 = ref.members(layout, c, l)
                    g0 = c * chunk
                    for k in range(len(off) - 1):
                        mine = [g for g in e0[off0[k]:off0[k + 1]] if smp.inside[g0 + g, r]]
                        assert list(e[off[k]:off[k + 1]]) == mine, (chunk, r, c, l, k)


# ------------------------------------------------------------------ 2. eight Gaussian problems, analytically -----------------
NAMES = ["a", "b", "c"]
BLOCK = {n: {"prior": {"min": 0.0, "max": 1.0}, "ref": {"loc": 0.5, "scale": 0.1}, "proposal": 0.1} for n in NAMES}
SIGMA = np.array([0.02, 0.05, 0.01])


class Eight:
    """Eight Gaussian likelihoods of one covariance (sigma 0.02, 0.05, 0.01, correlation 0.5 between the first two) on the box
    [0, 1]^3, their means scattered +-4 sigma about the middle: exact ln Z = 1/2 ln |2 pi C| under the uniform prior."""

    def __init__(self):
        corr = np.eye(3)
        corr[0, 1] = corr[1, 0] = 0.5
        self.cov = corr * np.outer(SIGMA, SIGMA)
        self.prec = np.linalg.inv(self.cov)
        self.means = 0.5 + (np.random.default_rng(3).random((8, 3)) - 0.5) * 8.0 * SIGMA
        self.ln_evidence = 0.5 * np.log(np.linalg.det(2 * np.pi * self.cov))

    def pairs(self, batch, which):
        dx = np.stack([batch[n] for n in NAMES], axis=1) - self.means[which]
        return -0.5 * np.einsum("ni,ij,nj->n", dx, self.prec, dx)

    def cross(self, batch):
        dx = np.stack([batch[n] for n in NAMES], axis=1)[:, None, :] - self.means[None]
        return -0.5 * np.einsum("nri,ij,nrj->nr", dx, self.prec, dx)

    def fits(self):
        """The best fit and Laplace stand-ins every problem would give: its mean, its covariance."""
        from victor_amd import BestFit
        status = np.full(8, BestFit.CONVERGED, dtype=np.int32)
        bf = BestFit(NAMES, self.means, {}, np.zeros(8), np.zeros(8), status, np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64))
        lap = type("Lap", (), {"names": NAMES, "cov": np.repeat(self.cov[None], 8, axis=0)})
        return bf, lap


def host(evaluate, q, **kw):
    from victor_amd.importance import importance_posterior
    return importance_posterior(None, BLOCK, q, device=False, evaluate=evaluate, **kw)


def test_eight_gaussians_each_from_its_own_proposal():
    from victor_amd import GaussianProposal, ProposalSet
    g = Eight()
    bf, lap = g.fits()
    qs = ProposalSet.from_fits(bf, lap, inflate=2.0)
    pooled = GaussianProposal.from_fits(bf, lap, inflate=2.0)
    assert len(qs) == 8 and not np.any(qs.pooled) and np.allclose(qs.cov, 2.0 * g.cov) and same_bytes(qs.mean, g.means)
    n = 4096
    for seed in range(4):
        ip = host(g.pairs, qs, n=n, seed=seed, tail=True)
        shared = host(g.cross, pooled, n=n, seed=seed)
        pulls = (ip.ln_evidence - g.ln_evidence) / ip.ln_evidence_error
        print(f"seed {seed}: pulls {pulls.min():+.2f} .. {pulls.max():+.2f}, ESS {ip.ess.min():.0f} (closed form {0.6495 * n:.0f}), "
              f"pooled ESS {shared.ess.min():.0f} .. {shared.ess.max():.0f}, k {ip.tail.k.max():.2f} <= {ip.tail.k_threshold:.2f}")
        assert ip.n_problems == 8 and ip.n_drawn == n and np.all(ip.n_inside == n) and ip.proposals is qs
        assert np.all(ip.status == ip.OK)
        assert np.all(np.abs(ip.ln_evidence - g.ln_evidence) <= 4.0 * ip.ln_evidence_error)
        assert np.all(ip.ess >= 0.5 * n)
        assert np.all(ip.ess >= 5.0 * shared.ess)
        assert np.all(ip.tail.k <= ip.tail.k_threshold) and np.all(ip.tail.status == ip.tail.OK)
        assert np.all(np.abs(ip.mean - g.means) <= 4.0 * ip.sigma / np.sqrt(ip.ess)[:, None])
        assert np.allclose(ip.sigma, SIGMA[None, :], rtol=0.1)
        lo, hi = ip.interval("b", 0.68)
        assert np.all(np.abs(ip.median("b") - g.means[:, 1]) < 0.01) and np.all(hi - lo > 0.05) and np.all(hi - lo < 0.15)
        assert ip.marginal("a").shape == (8, 64) and np.all(np.isfinite(ip.quantile("c", 0.9)))
        for j, name in enumerate(NAMES):
            assert same_bytes(ip.best[name], ip._sample.x[ip.arg_max, np.arange(8), j])


def test_a_gaussian_prior_is_normalised_per_problem():
    """Under a prior every problem normalises the prior by its own sample: Z = int L N(mu_p, S_p) over a box that holds both."""
    from victor_amd import ProposalSet
    from victor_amd.priors import GaussianPrior
    g = Eight()
    mu_p, sig_p = np.array([0.5, 0.5, 0.5]), 4.0 * SIGMA
    prior = GaussianPrior(NAMES, mu_p, sigma=sig_p)
    s = g.cov + np.diag(sig_p ** 2)
    dm = g.means - mu_p
    truth = g.ln_evidence - 0.5 * np.einsum("ri,ij,rj->r", dm, np.linalg.inv(s), dm) - 0.5 * np.log(np.linalg.det(2 * np.pi * s))
    # the proposal has to cover the prior as well as the posterior: the prior's own covariance about every problem's mean
    qs = ProposalSet(NAMES, g.means, np.repeat((2.0 * np.diag(sig_p ** 2))[None], 8, axis=0))
    ip = host(g.pairs, qs, n=8192, seed=1, prior=prior, min_ess=20.0)
    assert ip.prior_ln_max.shape == ip.prior_total.shape == ip.prior_error.shape == (8,) and np.all(ip.prior_total > 0)
    assert len(set(ip.prior_total)) == 8                          # every problem's own
    assert np.all(ip.status == ip.OK)
    assert np.all(np.abs(ip.ln_evidence - truth) <= 4.0 * (ip.ln_evidence_error + ip.prior_error)), (ip.ln_evidence - truth, ip.ln_evidence_error)


def test_identical_proposals_equal_the_shared_route():
    from victor_amd import GaussianProposal, ProposalSet
    g = Eight()
    mean, cov = np.array([0.5, 0.5, 0.5]), 4.0 * g.cov                # five of its sigmas to the box: no point leaves it
    q = GaussianProposal(NAMES, mean, cov)
    qs = ProposalSet(NAMES, np.repeat(mean[None], 8, axis=0), np.repeat(cov[None], 8, axis=0))
    kw = dict(n=500, seed=9, chunk=64, bins={"a": 7, "b": 5, "c": 6}, pairs=[("a", "b")], tail={"size": 20})
    own = host(g.pairs, qs, **kw)
    shared = host(g.cross, q, **kw)
    assert np.all(own.n_inside == 500) and shared.n_inside == 500 and own.n_chunks == shared.n_chunks == 8
    for name in EXACT + SUMS:
        assert same_bytes(getattr(own.raw, name), getattr(shared.raw, name)), name
    for name in ("lnpost", "index", "count"):
        assert same_bytes(getattr(own.tail, name), getattr(shared.tail, name)), name
    for name in ("ln_evidence", "ess", "mean", "cov", "status"):
        assert same_bytes(getattr(own, name), getattr(shared, name)), name
    assert same_bytes(own.tail.k, shared.tail.k) and same_bytes(own.tail.ess, shared.tail.ess)
    # the same points handed to the shared route as the caller's own: y is centred on their mean there, so s1 and s2 differ
    pts = GaussianProposal.draw(*q.ordered("test", NAMES), None, 500, 9)
    assert same_bytes(pts, own._sample.x[:, 3])
    given = host(g.cross, None, sample=pts, ln_proposal=GaussianProposal.ln_density(pts, *q.ordered("test", NAMES), None),
                 **{k: v for k, v in kw.items() if k not in ("n", "seed")})
    for name in EXACT + ("total", "sq", "h1", "h2"):
        assert same_bytes(getattr(own.raw, name), getattr(given.raw, name)), name
    assert np.allclose(own.mean, given.mean, rtol=0, atol=1e-12) and np.allclose(own.cov, given.cov, rtol=0, atol=1e-12)


# ------------------------------------------------------------------ 3. ProposalSet ------------------------------------------
def test_proposal_set_take_and_from_fits():
    from victor_amd import BestFit, GaussianProposal, ProposalSet
    from victor_amd.utils import InputError
    g = Eight()
    bf, lap = g.fits()
    status = np.array(bf.status)
    status[5] = BestFit.MAX_ITER
    cov = np.array(lap.cov)
    cov[2, 0, 0] = np.nan
    bf = BestFit(NAMES, g.means, {}, np.zeros(8), np.zeros(8), status, np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64))
    lap = type("Lap", (), {"names": NAMES, "cov": cov})
    qs = ProposalSet.from_fits(bf, lap, inflate=3.0, dof=4)
    pool = GaussianProposal.from_fits(bf, lap, inflate=3.0, dof=4)
    assert list(np.flatnonzero(qs.pooled)) == [2, 5] and qs.dof == 4.0 and len(qs) == 8
    for r in range(8):
        if r in (2, 5):
            assert same_bytes(qs.mean[r], pool.mean) and same_bytes(qs.cov[r], pool.cov)
        else:
            assert same_bytes(qs.mean[r], g.means[r]) and np.allclose(qs.cov[r], 3.0 * g.cov, rtol=1e-15)
    sub = qs.take([5, 0, 3])
    assert len(sub) == 3 and list(sub.pooled) == [True, False, False] and same_bytes(sub.mean, qs.mean[[5, 0, 3]]) and sub.dof == 4.0
    assert same_bytes(sub.cov, qs.cov[[5, 0, 3]]) and sub.names == NAMES
    mask = np.zeros(8, dtype=bool)
    mask[[1, 6]] = True
    assert same_bytes(qs.take(mask).mean, qs.mean[[1, 6]])
    # the subset runs with the matching problems
    ip = host(lambda batch, which: g.pairs(batch, np.array([5, 0, 3])[which]), sub, n=512, seed=0)
    # (a Gaussian of covariance 3 C against C has ESS n ((2 - 1/3) / 3)^(3/2) = 0.41 n; the pooled proposal of problem 5 far less)
    assert ip.n_problems == 3 and ip.ess[1] > 0.3 * 512 and ip.ess[0] < 0.5 * ip.ess[1]
    none = BestFit(NAMES, g.means, {}, np.zeros(8), np.zeros(8), np.full(8, BestFit.MAX_ITER, dtype=np.int32), np.zeros(8, dtype=np.int32),
                   np.zeros(8, dtype=np.int64))
    with pytest.raises(InputError, match="no problem of the best fit converged"):
        ProposalSet.from_fits(none, lap)
    for bad, text in ((8, "0 .. 7"), ([], "non-empty"), (np.zeros(3, dtype=bool), "one entry per problem"), ([0.5], "non-empty")):
        with pytest.raises(InputError, match=text):
            qs.take(bad)
    ok = np.repeat(np.eye(2)[None], 3, axis=0)
    for r, spoil, text in ((1, np.nan, "covariance of problem 1 is not finite"), (2, 5.0, "covariance of problem 2 is not positive definite")):
        c = ok.copy()
        c[r, 0, 1] = c[r, 1, 0] = spoil
        with pytest.raises(InputError, match=text):
            ProposalSet(["a", "b"], np.zeros((3, 2)), c)
    c = ok.copy()
    c[0, 0, 1] = 0.1
    c[1, 0, 1] = 0.2
    with pytest.raises(InputError, match="covariance of problem 0 is not symmetric"):
        ProposalSet(["a", "b"], np.zeros((3, 2)), c)
    with pytest.raises(InputError, match=r"cov must be \(3, 2, 2\)"):
        ProposalSet(["a", "b"], np.zeros((3, 2)), np.eye(2))
    with pytest.raises(InputError, match="mean must be"):
        ProposalSet(["a", "b"], np.zeros(2), ok)
    with pytest.raises(InputError, match="dof"):
        ProposalSet(["a", "b"], np.zeros((3, 2)), ok, dof=-1)


# ------------------------------------------------------------------ 4. the refusals ------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the refusal")


def raiser(batch, which=None):
    raise AssertionError("a refused call reached the evaluator")


class Stub:
    def __init__(self, n, paired):
        self.n, self.paired_model = n, paired

    def __len__(self):
        return self.n


def test_every_refusal_comes_before_the_first_evaluation():
    from victor_amd import GaussianProposal, JointFit, ProposalSet
    from victor_amd.importance import importance_posterior
    from victor_amd.predictive import PredictiveError
    from victor_amd.utils import InputError
    g = Eight()
    qs = ProposalSet(NAMES, g.means, np.repeat(g.cov[None], 8, axis=0))

    def refused(match, q=qs, fit=None, error=InputError, **kw):
        with pytest.raises(error, match=match):
            importance_posterior(fit, BLOCK, q, device=False, evaluate=raiser, **kw)
    refused("predictive needs a fit", error=PredictiveError, predictive=True)       # (with a fit: the test below)
    refused("not beside a ProposalSet", sample=np.zeros((4, 3)), ln_proposal=np.zeros(4))
    refused("not beside a ProposalSet", sample=np.zeros((4, 3)))
    refused("not supported for joint fits", fit=object.__new__(JointFit))
    refused("not supported for joint fits", n_blocks=2)
    refused("holds 8 proposals, there are 16 realisations", realisations=Stub(16, False))
    refused("the proposals name", q=ProposalSet(["a", "b"], g.means[:, :2], np.repeat(g.cov[None, :2, :2], 8, axis=0)))
    far = g.means.copy()
    far[6, 1] = 1.5
    refused("proposal of problem 6 has its mean", q=ProposalSet(NAMES, far, qs.cov))
    refused("more than 2\\^24 points", n=1 << 22)
    refused("rows of one launch", chunk=8193)
    refused("chunk must be", chunk=0)
    refused("n must be", n=0)
    refused("seed", seed=-1)
    refused("tail", tail={"size": 4096}, n=64)
    refused("cell offsets", n=4096, chunk=1, bins=1024, pairs=[("a", "b"), ("a", "c"), ("b", "c")])
    with pytest.raises(InputError, match="needs realisations"):
        importance_posterior(object(), BLOCK, qs, device=False)
    # a GaussianProposal keeps today's refusal of paired-model realisations, a ProposalSet goes through them
    with pytest.raises(InputError, match="have no cross mode"):
        importance_posterior(None, BLOCK, GaussianProposal(NAMES, g.means[0], g.cov), device=False, evaluate=raiser, realisations=Stub(8, True))
    ip = importance_posterior(None, BLOCK, qs, device=False, evaluate=g.pairs, realisations=Stub(8, True), n=64)
    assert ip.n_problems == 8


def test_refusals_with_a_fit_come_before_any_device_call(monkeypatch):
    import victor_amd
    from tests import cases
    from tests.test_realisations import stack_options
    from victor_amd.predictive import PredictiveError
    from victor_amd.utils import InputError
    monkeypatch.setattr(victor_amd.CCFFit, "_get_engine", lambda self, *a, **k: _NoLibrary())
    fit = victor_amd.CCFFit(*stack_options())
    rs = fit.realisations()
    params = cases.cobaya_info()["params"]
    names = [n for n, v in params.items() if isinstance(v, dict) and "prior" in v]
    mid = np.array([0.5 * (params[n]["prior"]["min"] + params[n]["prior"]["max"]) for n in names])
    width = np.array([params[n]["prior"]["max"] - params[n]["prior"]["min"] for n in names])
    cov = np.diag((0.01 * width) ** 2)
    qs = victor_amd.ProposalSet(names, np.repeat(mid[None], 16, axis=0), np.repeat(cov[None], 16, axis=0))
    assert len(rs) == 16
    for kw, text, error in ((dict(predictive=True), "points of its own", PredictiveError),
                            (dict(sample=np.zeros((4, len(names))), ln_proposal=np.zeros(4)), "not beside a ProposalSet", InputError),
                            (dict(n=1 << 21), "more than 2\\^24", InputError),
                            (dict(chunk=4097), "rows of one launch", InputError),
                            (dict(beta_interpolation="likelihood"), "beta_interpolation 'likelihood'", InputError),
                            (dict(tail=3), "tail must be", InputError)):
        with pytest.raises(error, match=text):
            rs.importance_posterior(params, qs, **kw)
    with pytest.raises(InputError, match="holds 3 proposals, there are 16"):
        rs.importance_posterior(params, qs.take([0, 1, 2]))
    out = qs.mean.copy()
    out[9, 0] = params[names[0]]["prior"]["max"] + 1.0
    with pytest.raises(InputError, match="proposal of problem 9"):
        rs.importance_posterior(params, victor_amd.ProposalSet(names, out, qs.cov))
    with pytest.raises(InputError, match="needs realisations"):
        fit.importance_posterior(params, qs)
    with pytest.raises(AssertionError, match="the library was reached"):      # an accepted call goes on to the device
        rs.importance_posterior(params, qs, n=8)


# ------------------------------------------------------------------ 5. the surface ------------------------------------------
def test_abi_surface():
    import victor_amd
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    assert re.search(r"\bvk_is\* vk_is_create_own\(vk_ctx\* ctx, const vk_eval_opts\* opts, int32_t n_axes, const int32_t\* columns, "
                     r"int64_t n_points,\s+int32_t n_problems, const int32_t\* which,", header)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    res, args = N.SYMBOLS["vk_is_create_own"]
    assert res == C.c_void_p and len(args) == 22
    assert args[0] == C.c_void_p and args[1] == N.SYMBOLS["vk_is_create"][1][1] and args[2:7] == [C.c_int32, ip, C.c_int64, C.c_int32, ip]
    assert args[7:12] == [dp] * 5 and args[-4:] == [C.c_double, C.c_int32, C.c_char_p, C.c_size_t]
    assert len(N.SYMBOLS["vk_is_create"][1]) == 21
    rules = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_importance.h")).read()
    for name in ("value_at", "own_row", "own_list", "own_offsets", "prior_of"):
        assert re.search(r"VK_GRID_HD inline \w[\w ]* %s\(" % name, rules), name
    assert "hip/hip_runtime.h" not in rules
    kernels = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_kernel_is_own.h")).read()
    assert set(re.findall(r"\b(vk_\w+_kernel)\(", kernels)) == {"vk_is_own_rows_kernel", "vk_is_own_accumulate_kernel"}
    assert "atomic" not in kernels.replace("no atomics", "") and "__shared__" not in kernels
    for shared in ("vk_kernel_importance.h", "vk_kernel_is_tail.h"):
        assert "vkis::value_at(" in open(os.path.join(ROOT, "victor_amd", "csrc", shared)).read(), shared
    assert victor_amd.ProposalSet is victor_amd.importance.ProposalSet and "ProposalSet" in victor_amd.__all__


def test_library_exports_the_new_symbol():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    assert hasattr(lib, "vk_is_create_own")
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
