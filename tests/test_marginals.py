"""Marginal histograms of the chains (victor_amd/marginals.py, vk_chain_set_marginals / vk_chain_marginals) without a GPU: the
binning rule of victor_amd/csrc/vk_marginals.h compiled on its own under g++ against the NumPy statement, slot for slot; the
definition route of ``sample_chains(..., marginals=...)`` against the rule applied to its own history; quantiles and intervals on
hand-built counts and against the sample quantile; the refusals, raised before any evaluation; and the C ABI's surface.

The analytic function is the correlated Gaussian of tests/test_chains.py ("gauss": its mean lies next to a face of the box).
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.test_chains import block_for as metropolis_block
from tests.test_chains import evaluate_of
from tests.test_stretch import block_for as stretch_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_chain_set_marginals", "vk_chain_marginals")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_marginals.h"

static std::vector<double> in;
static FILE* fo;
static void put(double v) { fwrite(&v, sizeof(double), 1, fo); }

// slot n m          in: a, b, v[m]                              out: slot[m]
// cell n m          in: aj, bj, ak, bk, vj[m], vk[m]            out: cell[m] (-1: outside either range)
// count d C group n_bins n_bins2 n_pairs m
//                   in: a[d], b[d], pairs[n_pairs][2], x[m][C][d]   out: h1[C / group][d][n_bins + 2], h2[C / group][n_pairs][n_bins2][n_bins2]
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
  if (!strcmp(mode, "slot")) {
    const int n = atoi(argv[2]), m = atoi(argv[3]);
    const double a = p[0], b = p[1], inv = vkmarg::inverse_width(n, a, b);
    for (int i = 0; i < m; ++i) put((double)vkmarg::slot(p[2 + i], a, b, inv, n));
  } else if (!strcmp(mode, "cell")) {
    const int n = atoi(argv[2]), m = atoi(argv[3]);
    const double aj = p[0], bj = p[1], ak = p[2], bk = p[3];
    const double invj = vkmarg::inverse_width(n, aj, bj), invk = vkmarg::inverse_width(n, ak, bk);
    const double *vj = p + 4, *vk = vj + m;
    for (int i = 0; i < m; ++i) put((double)vkmarg::cell(vj[i], aj, bj, invj, vk[i], ak, bk, invk, n));
  } else if (!strcmp(mode, "count")) {
    const int d = atoi(argv[2]), Cn = atoi(argv[3]), m = atoi(argv[8]);
    vkmarg::Marginals q{};
    q.on = 1;
    q.group = atoi(argv[4]);
    q.n_bins = atoi(argv[5]);
    q.n_bins2 = atoi(argv[6]);
    q.n_pairs = atoi(argv[7]);
    for (int j = 0; j < d; ++j) {
      q.a[j] = p[j], q.b[j] = p[d + j];
      q.inv[j] = vkmarg::inverse_width(q.n_bins, q.a[j], q.b[j]);
      q.inv2[j] = vkmarg::inverse_width(q.n_bins2, q.a[j], q.b[j]);
    }
    const double* pr = p + 2 * d;
    for (int i = 0; i < q.n_pairs; ++i) q.pair[i][0] = (int)pr[2 * i], q.pair[i][1] = (int)pr[2 * i + 1];
    const double* x = pr + 2 * q.n_pairs;
    const size_t R = (size_t)(Cn / q.group);
    std::vector<unsigned long long> h1(R * d * (q.n_bins + 2)), h2(R * q.n_pairs * q.n_bins2 * q.n_bins2 + 1);
    q.h1 = h1.data();
    q.h2 = h2.data();
    for (int t = 0; t < m; ++t)
      for (int c = 0; c < Cn; ++c) {
        const double* xc = x + ((size_t)t * Cn + c) * d;
        vkmarg::count(q, d, (size_t)(c / q.group), [&](int j) { return xc[j]; }, [](unsigned long long* at) { *at += 1; });
      }
    for (size_t i = 0; i < h1.size(); ++i) put((double)h1[i]);
    for (size_t i = 0; i + 1 < h2.size(); ++i) put((double)h2[i]);
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
    d = tmp_path_factory.mktemp("marginals_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(args, arrays):
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in arrays]).tofile(str(fin))
        subprocess.run([str(exe)] + [str(a) for a in args] + [str(fin), str(fout)], check=True)
        return np.fromfile(str(fout), dtype=np.float64).astype(np.int64)
    return run


# ------------------------------------------------------------------ 1. the header against NumPy, slot for slot --------------
START = {0.3: 0.1, 1e-3: -0.37, 400.0: -123.456}       # b = a + width: sums that round


def adversarial(a, b, n):
    """a, b, their neighbours, every interior edge (as a + k (b - a) / n rounds) and both of its neighbours."""
    edges = a + np.arange(1, n) * (b - a) / n
    pts = np.concatenate([[a, b], edges])
    return np.concatenate([pts, np.nextafter(pts, -np.inf), np.nextafter(pts, np.inf)])


@pytest.mark.parametrize("n", [7, 128, 1024])
@pytest.mark.parametrize("width", [0.3, 1e-3, 400.0])
def test_slots_against_numpy(driver, width, n):
    from victor_amd.marginals import slots
    a = START[width]
    b = a + width
    rng = np.random.default_rng(n + int(1000 * width))
    v = np.concatenate([rng.uniform(a - 0.2 * width, b + 0.2 * width, 10000), adversarial(a, b, n), [-np.inf, np.inf, -1e300, 1e300]])
    got = driver(["slot", n, len(v)], [[a, b], v])
    want = slots(v, a, b, n)
    assert np.array_equal(got, want), (width, n, v[got != want][:5])
    # what the rule says, whoever computes it: the ends, the outside, and order
    assert np.all(got[v < a] == 0) and np.all(got[v > b] == n + 1) and np.all((got[(v >= a) & (v <= b)] >= 1) & (got[(v >= a) & (v <= b)] <= n))
    assert got[v == a][0] == 1 and got[v == b][0] == n and got[v == np.nextafter(a, -np.inf)][0] == 0 and got[v == np.nextafter(b, np.inf)][0] == n + 1
    order = np.argsort(v, kind="stable")
    assert np.all(np.diff(got[order]) >= 0)
    assert set(np.unique(got)) == set(range(n + 2)), "a slot was never reached"
    # the true bin of a value is within one of its slot: the rule's two roundings move a value at most across one edge
    inner = (v >= a) & (v <= b)
    exact = np.floor((v[inner].astype(np.longdouble) - np.longdouble(a)) / (np.longdouble(b) - np.longdouble(a)) * n).astype(np.int64)
    assert np.all(np.abs(got[inner] - 1 - np.minimum(exact, n - 1)) <= 1)


@pytest.mark.parametrize("n", [1, 8, 32, 128])
def test_cells_against_numpy(driver, n):
    from victor_amd.marginals import cells, slots
    aj, bj, ak, bk = 0.1, 0.1 + 0.3, -123.456, -123.456 + 400.0
    rng = np.random.default_rng(n)
    ej, ek = adversarial(aj, bj, n), adversarial(ak, bk, n)
    vj = np.concatenate([rng.uniform(aj - 0.06, bj + 0.06, 10000), ej, rng.uniform(aj, bj, len(ek)), np.repeat(ej[:6], 6)])
    vk = np.concatenate([rng.uniform(ak - 80.0, bk + 80.0, 10000), rng.uniform(ak, bk, len(ej)), ek, np.tile(ek[:6], 6)])
    got = driver(["cell", n, len(vj)], [[aj, bj, ak, bk], vj, vk])
    want = cells(vj, aj, bj, vk, ak, bk, n)
    assert np.array_equal(got, want), n
    # inside both, or not counted; the cell is the pair of 1-D bins
    sj, sk = slots(vj, aj, bj, n), slots(vk, ak, bk, n)
    inside = (sj >= 1) & (sj <= n) & (sk >= 1) & (sk <= n)
    assert np.array_equal(got >= 0, inside) and np.any(~inside) and np.any((sj >= 1) & (sj <= n) & ~inside) and np.any((sk >= 1) & (sk <= n) & ~inside)
    assert np.array_equal(got[inside], (sj[inside] - 1) * n + (sk[inside] - 1))


def test_count_fills_the_pooled_layout(driver):
    """vkmarg::count with a plain += 1 against ``Binning.add``: problems, parameters and pairs land where the layout says."""
    from victor_amd.marginals import resolve_marginals
    names = ["p", "q", "r", "s"]
    lo, hi = np.array([-1.0, 0.0, 10.0, -5.0]), np.array([1.0, 0.3, 410.0, 5.0])
    q = resolve_marginals({"bins": 7, "bins2d": 5, "range": {"p": (-0.5, 0.25)}, "pairs": [("s", "p"), ("q", "r"), ("p", "q")]}, "test", names, lo, hi)
    assert q.pairs.tolist() == [[0, 3], [1, 2], [0, 1]] and q.pair_names == [("s", "p"), ("q", "r"), ("p", "q")]
    Cn, W, m = 6, 2, 50
    x = np.random.default_rng(5).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (m, Cn, 4))
    h1, h2 = q.zeros(Cn // W)
    for t in range(m):
        q.add(h1, h2, x[t], W)
    got = driver(["count", 4, Cn, W, 7, 5, 3, m], [q.a, q.b, q.pairs, x])
    assert np.array_equal(got[:h1.size].reshape(h1.shape), h1) and np.array_equal(got[h1.size:].reshape(h2.shape), h2)
    assert np.all(h1.sum(axis=2) == m * W) and h1[:, :, 0].min() > 0 and h1[:, :, -1].min() > 0
    assert np.all(h2.sum(axis=(2, 3)) < m * W) and np.all(h2.sum(axis=(2, 3)) > 0)


# ------------------------------------------------------------------ 2. the definition route ---------------------------------
# The stretch move refuses fewer than 2 (d + 1) = 8 walkers, so its ensemble has 8 where the Metropolis run has 4 chains.
RUNS = {"metropolis": (4, metropolis_block), "stretch": (8, stretch_block)}
NARROW = {"a": (0.3, 0.9), "b": (-0.3, 0.1), "c": (-0.05, 0.25)}          # narrower than the chains' excursion in all three
OPTION = {"bins": 16, "range": NARROW, "pairs": [("a", "c"), ("c", "b")], "bins2d": 6}


def host(move, n, marginals, **kw):
    from victor_amd.chains import sample_chains
    W, block = RUNS[move]
    return sample_chains(None, block("gauss"), n, walkers=W, seed=3, burn=5, thin=2, device=False, evaluate=evaluate_of("gauss"),
                         move=move, marginals=marginals, **kw)


def restated(chain, option, names, lo, hi):
    """(counts, below, above, counts2d) of a history (n_kept, R, W, d): the binning rule applied to it, problem by problem."""
    from victor_amd.marginals import cells, slots
    n, n2 = option.get("bins", 128), option.get("bins2d", 32)
    rng = {m: option.get("range", {}).get(m, (lo[j], hi[j])) for j, m in enumerate(names)}
    R = chain.shape[1]
    counts, below, above, counts2d = {}, {}, {}, {}
    for j, m in enumerate(names):
        h = np.stack([np.bincount(slots(chain[:, r, :, j].ravel(), *rng[m], n), minlength=n + 2) for r in range(R)])
        counts[m], below[m], above[m] = h[:, 1:-1], h[:, 0], h[:, -1]
    pairs = option.get("pairs", [])
    if isinstance(pairs, str):
        pairs = [(names[j], names[k]) for j in range(len(names)) for k in range(j + 1, len(names))]
    for n1, n2_ in pairs:
        j, k = names.index(n1), names.index(n2_)
        out = []
        for r in range(R):
            at = cells(chain[:, r, :, j].ravel(), *rng[n1], chain[:, r, :, k].ravel(), *rng[n2_], n2)
            out.append(np.bincount(at[at >= 0], minlength=n2 * n2).reshape(n2, n2))
        counts2d[(n1, n2_)] = np.stack(out)
    return counts, below, above, counts2d


def assert_marginals(m, want, what=""):
    counts, below, above, counts2d = want
    assert list(m.counts) == list(counts) and list(m.counts2d) == list(counts2d), what
    for k in counts:
        assert m.counts[k].dtype == np.int64 and np.array_equal(m.counts[k], counts[k]), (what, k)
        assert np.array_equal(m.below[k], below[k]) and np.array_equal(m.above[k], above[k]), (what, k)
    for k in counts2d:
        assert m.counts2d[k].shape == counts2d[k].shape and np.array_equal(m.counts2d[k], counts2d[k]), (what, k)


def same_marginals(a, b, what=""):
    assert a.names == b.names and np.array_equal(a.n, b.n), what
    assert_marginals(a, (b.counts, b.below, b.above, b.counts2d), what)
    for k in a.edges:
        assert np.array_equal(a.edges[k], b.edges[k]), (what, k)


@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_definition_route_counts_its_own_history(move):
    W = RUNS[move][0]
    ch = host(move, 70, OPTION)
    m = ch.marginals
    assert ch.chain.shape == (33, 1, W, 3) and m.names == ["a", "b", "c"] and m.n.tolist() == [33 * W]
    assert_marginals(m, restated(ch.chain, OPTION, ch.names, ch._lo, ch._hi), move)
    for k in m.names:
        assert m.counts[k].shape == (1, 16) and m.edges[k].shape == (17,)
        assert m.edges[k][0] == NARROW[k][0] and m.edges[k][-1] == NARROW[k][1]
        assert m.counts[k].sum() + m.below[k][0] + m.above[k][0] == ch.n_kept * W
        assert m.below[k][0] > 0 and m.above[k][0] > 0, "the range is not narrower than the excursion: the test does not reach the outside slots"
    assert m.counts2d[("a", "c")].shape == (1, 6, 6) and 0 < m.counts2d[("c", "b")].sum() < 33 * W
    # a pair named against sampled order is the transpose of the pair named along it
    other = host(move, 70, dict(OPTION, pairs=[("b", "c")])).marginals
    assert np.array_equal(other.counts2d[("b", "c")], np.swapaxes(m.counts2d[("c", "b")], 1, 2))
    # nothing else changes, and off is off
    plain = host(move, 70, None)
    assert plain.marginals is None
    for a in ("chain", "lnl_chain", "x", "n_accept", "sum1", "sum2"):
        assert getattr(plain, a).tobytes() == getattr(ch, a).tobytes(), a
    # a cut run keeps counting; without a history the counts are the same
    same_marginals(host(move, 40, OPTION).extend(30).marginals, m, "40 + 30")
    bare = host(move, 70, OPTION, keep_chain=False)
    assert bare.chain is None
    same_marginals(bare.marginals, m, "keep_chain=False")


def test_true_means_every_parameter_over_its_box():
    ch = host("metropolis", 70, True)
    m = ch.marginals
    assert all(m.counts[k].shape == (1, 128) for k in "abc") and m.counts2d == {}
    assert all(m.edges[k][0] == -1.0 and m.edges[k][-1] == 1.0 for k in "abc")
    assert all(m.below[k][0] == 0 and m.above[k][0] == 0 and m.counts[k].sum() == 132 for k in "abc")    # the chains never leave the box
    assert_marginals(m, restated(ch.chain, {}, ch.names, ch._lo, ch._hi))
    every = host("metropolis", 70, {"pairs": "all"}).marginals
    assert list(every.counts2d) == [("a", "b"), ("a", "c"), ("b", "c")] and every.counts2d[("a", "b")].shape == (1, 32, 32)


# ------------------------------------------------------------------ 3. quantiles and intervals ------------------------------
def built(counts, below, above, a=0.0, b=4.0):
    from victor_amd.marginals import Binning, Marginals
    counts = np.atleast_2d(np.asarray(counts, dtype=np.int64))
    below, above = np.atleast_1d(below).astype(np.int64), np.atleast_1d(above).astype(np.int64)
    h1 = np.concatenate([below[:, None], counts, above[:, None]], axis=1)[:, None, :]
    q = Binning(["p"], counts.shape[1], [a], [b], [], [], 1)
    return Marginals(q, h1, q.zeros(len(counts))[1], h1.sum(axis=(1, 2)))


def test_quantiles_of_hand_built_counts():
    m = built([1, 0, 2, 1], 0, 0)                            # n = 4, cum = 0 1 1 3 4
    assert m.n.tolist() == [4] and m.edges["p"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert m.quantile("p", 0.5)[0] == 2.5                    # t = 2: bin 2 (the empty bin 1 is passed over), (2 - 1) / 2 into it
    assert m.quantile("p", 0.25)[0] == 1.0 and m.quantile("p", 1.0)[0] == 4.0 and m.quantile("p", 0.0)[0] == 0.0
    assert m.quantile("p", 0.375)[0] == 2.25 and m.median("p")[0] == 2.5
    lo, hi = m.interval("p", 0.5)                            # the quantiles at 0.25 and 0.75
    assert lo[0] == 1.0 and hi[0] == 3.0
    assert np.array_equal(m.density("p"), [[0.25, 0.0, 0.5, 0.25]])
    # mass outside the range: n = 7, below 2, above 1, cum = 2 3 3 5 6
    m = built([1, 0, 2, 1], 2, 1)
    assert m.quantile("p", 0.5)[0] == 2.25                   # t = 3.5
    assert np.isnan(m.quantile("p", 0.2)[0])                 # t = 1.4 lies in the mass below
    assert np.isnan(m.quantile("p", 0.9)[0])                 # t = 6.3 lies in the mass above
    lo, hi = m.interval("p", 0.9)
    assert np.isnan(lo[0]) and np.isnan(hi[0])
    assert np.array_equal(m.density("p"), [[0.25, 0.0, 0.5, 0.25]])      # unit integral over the range
    # several problems: nothing kept, everything below, everything in one bin
    m = built([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 6, 0], [1, 0, 2, 1]], [0, 5, 0, 0], [0, 0, 0, 0])
    q = m.quantile("p", 0.5)
    assert q.shape == (4,) and np.isnan(q[0]) and np.isnan(q[1]) and q[2] == 2.5 and q[3] == 2.5
    assert np.all(np.isnan(m.density("p")[:2])) and m.density("p")[2].tolist() == [0.0, 0.0, 1.0, 0.0]
    from victor_amd import InputError
    with pytest.raises(InputError, match="no histogram"):
        m.quantile("r", 0.5)
    with pytest.raises(InputError, match="q must lie"):
        m.quantile("p", 1.5)
    with pytest.raises(InputError, match="level"):
        m.interval("p", 1.0)


@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_quantiles_against_the_sample_quantile(move):
    """Within one bin width of ``np.quantile(..., method="inverted_cdf")``: with t = q n, the sample quantile is the ceil(t)-th
    smallest sample, which lies in the bin where the cumulative count first reaches t - the bin the histogram's answer lies in."""
    ch = host(move, 70, {"bins": 32})
    m = ch.marginals
    for j, k in enumerate(m.names):
        samples = ch.chain[:, 0, :, j].ravel()
        width = 2.0 / 32
        for q in (0.05, 0.16, 0.5, 0.84, 0.95):
            want = np.quantile(samples, q, method="inverted_cdf")
            got = m.quantile(k, q)[0]
            assert abs(got - want) <= width, (move, k, q, got, want)
        lo, hi = m.interval(k)
        assert lo[0] == m.quantile(k, (1.0 - 0.68) / 2.0)[0] and hi[0] == m.quantile(k, (1.0 + 0.68) / 2.0)[0] and lo[0] < m.median(k)[0] < hi[0]
        assert abs(np.sum(m.density(k)[0] * np.diff(m.edges[k])) - 1.0) < 1e-12


# ------------------------------------------------------------------ 4. refusals and the ABI's surface ------------------------
def boom(*a, **k):
    raise AssertionError("the call reached an evaluation before refusing its input")


REFUSED = [({"range": {"d": (0.0, 1.0)}}, "range names parameters that are not sampled"),
           ({"pairs": [("a", "d")]}, "pairs names parameters that are not sampled"),
           ({"range": {"a": (0.5, 0.5)}}, "finite with a < b"),
           ({"range": {"a": (0.5, 0.1)}}, "finite with a < b"),
           ({"range": {"a": (0.0, np.inf)}}, "finite with a < b"),
           ({"range": {"a": (np.nan, 1.0)}}, "finite with a < b"),
           ({"range": {"a": (-1e308, 1e308)}}, "finite with a < b"),
           ({"range": {"a": 0.5}}, "must be a pair"),
           ({"bins": 0}, "bins must be an integer in 1..1024"),
           ({"bins": 1025}, "bins must be an integer in 1..1024"),
           ({"bins": 12.5}, "bins must be an integer in 1..1024"),
           ({"bins2d": 0}, "bins2d must be an integer in 1..128"),
           ({"bins2d": 129}, "bins2d must be an integer in 1..128"),
           ({"pairs": [("a", "a")]}, "names one parameter twice"),
           ({"pairs": [("a", "b"), ("b", "a")]}, "given twice"),
           ({"pairs": "some"}, "or 'all'"),
           ({"pairs": ["ab", "c"]}, "list of .name, name."),
           ({"binz": 3}, "unknown keys"),
           ("all", "None, True or a dict"),
           (5, "None, True or a dict")]


def test_refusals_come_before_any_evaluation():
    import victor_amd
    from victor_amd import InputError
    from victor_amd.chains import sample_chains
    from victor_amd.joint import JointFit, per_block
    for option, text in REFUSED:
        for move, (W, block) in RUNS.items():
            with pytest.raises(InputError, match=text):
                sample_chains(None, block("gauss"), 5, walkers=W, device=False, evaluate=boom, move=move, marginals=option)
    with pytest.raises(AssertionError, match="reached an evaluation"):                     # a good option goes on
        sample_chains(None, metropolis_block("gauss"), 5, walkers=4, device=False, evaluate=boom, marginals=OPTION)
    # the fits: a fixed parameter is not sampled; "name@q" needs a joint fit, where it is a sampled parameter
    params = cases.cobaya_info()["params"]
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    fit._get_engine = boom
    ds = [victor_amd.CCFFit(*cases.dsplit_options(q)) for q in range(3)]
    for f in ds:
        f._get_engine = boom
    joint = JointFit(ds)
    blk = per_block(params, ["sigma_v"], 3)
    for device in (True, False):
        with pytest.raises(InputError, match="not sampled"):
            fit.sample_chains(params, 5, device=device, fixed={"sigma_v": 380.0}, marginals={"range": {"sigma_v": (300.0, 400.0)}})
        with pytest.raises(InputError, match="not sampled"):
            fit.sample_chains(params, 5, device=device, marginals={"pairs": [("sigma_v@1", "beta")]})
        with pytest.raises(InputError, match="bins must be"):
            fit.sample_chains(params, 5, device=device, marginals={"bins": 4096})
        with pytest.raises(AssertionError, match="reached an evaluation"):
            fit.sample_chains(params, 5, device=device, marginals={"pairs": [("fsigma8", "sigma_v")]})
        fixed = {"beta": 0.4, "epsilon": 1.0}
        with pytest.raises(InputError, match="not sampled"):
            joint.sample_chains(blk, 5, device=device, fixed=fixed, marginals={"range": {"sigma_v": (300.0, 400.0)}})
        with pytest.raises(InputError, match="not sampled"):
            joint.sample_chains(blk, 5, device=device, fixed=fixed, marginals={"pairs": [("sigma_v@1", "sigma_v@3")]})
        with pytest.raises(AssertionError, match="reached an evaluation"):
            joint.sample_chains(blk, 5, device=device, fixed=fixed, marginals={"pairs": [("sigma_v@2", "sigma_v@0")], "range": {"sigma_v@1": (300.0, 400.0)}})


def test_the_keyword_is_on_every_public_path():
    import inspect

    import victor_amd
    from victor_amd.chains import sample_chains
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for fn in (victor_amd.CCFFit.sample_chains, Realisations.sample_chains, JointFit.sample_chains, JointRealisations.sample_chains, sample_chains):
        sig = inspect.signature(fn).parameters
        assert "marginals" in sig and sig["marginals"].default is None, fn


def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    want = {"vk_chain_set_marginals": ["vk_chain* f", "int32_t group", "int32_t n_bins", "const double* lo", "const double* hi", "int32_t n_pairs",
                                       "const int32_t* pairs", "int32_t n_bins2"],
            "vk_chain_marginals": ["vk_chain* f", "int64_t* h1", "int64_t* h2"]}
    for name in NEW:
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, f"include/victor_hip.h does not declare {name}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")] == want[name]
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert N.SYMBOLS["vk_chain_set_marginals"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, dp, dp, C.c_int32, ip, C.c_int32])
    assert N.SYMBOLS["vk_chain_marginals"] == (C.c_int, [C.c_void_p, lp, lp])
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_marginals.h")).read()
    assert "hip/hip_runtime.h" not in src and "asm" not in src


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
