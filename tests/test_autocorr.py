"""Autocorrelation times and effective sample sizes of the chains (victor_amd/autocorr.py, vk_chain_set_autocorr /
vk_chain_autocorr) without a GPU: the update of victor_amd/csrc/vk_autocorr.h compiled on its own under g++ against the NumPy
statement, bit for bit; the read-out of the state against the centred autocorrelation summed directly from the same series in
extended precision, at a derived bound, and against ``sokal_tau`` of the history; the definition route of
``sample_chains(..., autocorr=...)`` against the state rebuilt from its own history; the refusals; and the C ABI's surface.

The analytic function is the correlated Gaussian of tests/test_chains.py ("gauss"), run as tests/test_marginals.py runs it.
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import block_for as metropolis_block
from tests.test_chains import evaluate_of, same_bytes
from tests.test_stretch import block_for as stretch_block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_chain_set_autocorr", "vk_chain_autocorr")
FIELDS = ("pivot", "total", "head", "ring", "acc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_autocorr.h"

static std::vector<double> in;
static FILE* fo;
static void put(const double* v, size_t n) { fwrite(v, sizeof(double), n, fo); }

// the series value of W chains, element w at x[w * stride]: the lanes' partial sums and the butterfly
static double series(const double* x, size_t stride, int W) {
  double v[vkac::kLanes];
  for (int l = 0; l < vkac::kLanes; ++l) v[l] = vkac::lane_partial(W, l, [&](int w) { return x[(size_t)w * stride]; });
  vkac::combine(v);
  for (int l = 1; l < vkac::kLanes; ++l)
    if (memcmp(&v[l], &v[0], sizeof(double))) exit(4);       // every lane ends with the same bits
  return v[0];
}

// combine W m        in: x[m][W]                 out: s[m]
// state R d W L m    in: x[m][R W][d]            out: pivot[R d], total[R d], head[R d][L], ring[R d][L], acc[R d][L]
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
  if (!strcmp(mode, "combine")) {
    const int W = atoi(argv[2]), m = atoi(argv[3]);
    for (int i = 0; i < m; ++i) {
      const double s = series(p + (size_t)i * W, 1, W);
      put(&s, 1);
    }
  } else if (!strcmp(mode, "state")) {
    const int R = atoi(argv[2]), d = atoi(argv[3]), W = atoi(argv[4]), L = atoi(argv[5]), m = atoi(argv[6]);
    const size_t S = (size_t)R * d;
    if (vkac::state_doubles(S, L) != S * (3 * (size_t)L + 2)) return 5;
    std::vector<double> pivot(S), total(S), head(S * L), ring(S * L), acc(S * L);
    for (int t = 0; t < m; ++t)
      for (int r = 0; r < R; ++r)
        for (int j = 0; j < d; ++j) {
          const size_t q = (size_t)r * d + j;
          const double s = series(p + ((size_t)t * R * W + (size_t)r * W) * d + j, (size_t)d, W);
          vkac::step(&pivot[q], &total[q], &head[q * L], &ring[q * L], &acc[q * L], s, t, L);
        }
    put(pivot.data(), S), put(total.data(), S), put(head.data(), S * L), put(ring.data(), S * L), put(acc.data(), S * L);
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
    d = tmp_path_factory.mktemp("autocorr_driver")
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


def ar1(rng, phi, n, shape=()):
    """AR(1) series of unit variance along axis 0, (n,) + shape."""
    e = rng.standard_normal((n,) + tuple(shape))
    y = np.empty_like(e)
    y[0] = e[0]
    for t in range(1, n):
        y[t] = phi * y[t - 1] + np.sqrt(1.0 - phi * phi) * e[t]
    return y


def walkers_of(rng, phi, n, R, W, d):
    """Positions (n, R W, d) whose per-problem sums are AR(1) series about 380 +- 20, each walker with noise of its own."""
    centre = 380.0 + 20.0 * ar1(rng, phi, n, (R, 1, d))
    return (centre / W + 0.3 * rng.standard_normal((n, R, W, d))).reshape(n, R * W, d)


# ------------------------------------------------------------------ 1. the header against NumPy, bit for bit ----------------
@pytest.mark.parametrize("W", [1, 8, 63, 64, 65, 100, 200])
def test_combine_against_numpy(driver, W):
    from victor_amd.autocorr import series_sum
    rng = np.random.default_rng(W)
    m = 200
    x = 380.0 + 20.0 * rng.standard_normal((m, W))
    x[:5] *= 1e-300                                                # sums that lose bits differently in another order
    x[5:10, ::2] = -0.0
    got = driver(["combine", W, m], [x])
    want = series_sum(x.reshape(m * W, 1), m, W)[:, 0]
    assert same_bytes(got, want), W
    # the order is part of the rule: a plain left-to-right sum gives other bits somewhere (W > 2), the same value to rounding
    if W > 2:
        plain = np.array([sum(row.tolist()) for row in x])
        assert not same_bytes(plain, want)
        assert np.allclose(plain, want, rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("L", [7, 64, 100])
@pytest.mark.parametrize("W", [8, 64, 100])
@pytest.mark.parametrize("length", ["short", "wrapped"])
def test_state_against_numpy(driver, W, L, length):
    """W = 8: partial lanes; 64: every lane once; 100: a second, partial row.  L = 100 is no multiple of 64.  n < L leaves the
    head unfilled; n = 3 L + 5 wraps the ring three times."""
    from victor_amd.autocorr import SeriesState
    R, d = 2, 3
    n = L - 2 if length == "short" else 3 * L + 5
    x = walkers_of(np.random.default_rng(1000 * W + L), 0.8, n, R, W, d)
    st = SeriesState(R, d, W, L)
    for t in range(n):
        st.add(x[t])
    assert st.n == n
    got = driver(["state", R, d, W, L, n], [x])
    S = R * d
    parts = np.split(got, np.cumsum([S, S, S * L, S * L]))
    for name, g in zip(FIELDS, parts):
        assert same_bytes(g, getattr(st, name)), (name, W, L, length)
    # what the state says, whoever computes it
    from victor_amd.autocorr import series_sum
    s = np.stack([series_sum(x[t], R, W) for t in range(n)])               # (n, R, d)
    a = s - s[0]
    assert same_bytes(st.pivot, s[0]) and np.all(a[0] == 0.0)
    m = min(n, L)
    assert same_bytes(st.head[:, :, :m], np.moveaxis(a[:m], 0, 2)) and not st.head[:, :, m:].any()
    for u in range(max(0, n - L), n):
        assert same_bytes(st.ring[:, :, u % L], a[u]), u
    if length == "short":
        assert not st.acc[:, :, n:].any() and not st.ring[:, :, n:].any()
    k = min(3, m - 1)
    direct = np.zeros((R, d))
    for t in range(k, n):
        direct = direct + a[t] * a[t - k]
    assert same_bytes(st.acc[:, :, k], direct)


# ------------------------------------------------------------------ 2. the read-out against the history ---------------------
def direct_acf(a, L):
    """rho_k, k < L, and the sums N_k = sum_t (a_t - mu)(a_{t-k} - mu), A_k = sum_t |a_t a_{t-k}| of a series, in extended precision."""
    a = np.asarray(a, dtype=np.longdouble)
    n = len(a)
    c = a - a.sum() / n
    N = np.array([np.sum(c[k:] * c[:n - k]) for k in range(L)], dtype=np.longdouble)
    A = np.array([np.sum(np.abs(a[k:] * a[:n - k])) for k in range(L)], dtype=np.longdouble)
    return N / N[0], N, A


def rho_bound(a, N, A, rho):
    """How far rho_k read from the state may lie from the exact rho_k of the same values a_t (n of them, mean mu).

    The state: acc[k] is a running double sum of n - k rounded products; each product carries u |a_t a_{t-k}| (u = 2^-53), each
    addition u times a partial sum of magnitude at most A_k = sum |a_t a_{t-k}|, so |d acc[k]| <= (n + 1) u A_k <= 2^-52 n A_k.
    total is a running sum of the a_t: |d total| <= n u sum |a_t|, so |d mu| <= u sum |a_t|.  head and ring hold the a_t themselves.
    The read-out N_k = acc[k] - mu (2 total - H_k - Z_k) + (n - k) mu^2 has |dN_k / d mu| <= |2 total - H_k - Z_k| + 2 (n - k) |mu|
    <= 4 sum |a_t| (and dN_k / d total = -2 mu, covered by the same product), and (sum |a_t|)^2 <= n A_0 (Cauchy-Schwarz), so
        |d N_k| <= 2^-52 n A_k + 4 u n A_0 = 2^-52 n (A_k + 2 A_0),
    plus 2^-60 A_0 for evaluating the formula and the reference in extended precision (2^-64 on a handful of terms of size A_0).
    rho_k = N_k / N_0:  |d rho_k| <= (|d N_k| + |rho_k| |d N_0|) / (N_0 - |d N_0|), and the stored acf is rounded to double once
    more (u |rho_k|).  A_0 / N_0 = 1 + n mu^2 / N_0 is the amplification of the centring: it is what a pivot far from the series
    would cost, and why the series is kept about its first value."""
    n = len(a)
    e = np.longdouble(2.0) ** -52
    dN = e * n * (A + 2 * A[0]) + np.longdouble(2.0) ** -60 * A[0]
    return ((dN + np.abs(rho) * dN[0]) / (N[0] - dN[0]) + e * np.abs(rho)).astype(float)


CASES = [(0.5, 64, 4096), (0.9, 128, 8192)]


@pytest.mark.parametrize("phi,L,n", CASES)
def test_read_out_against_the_history(phi, L, n):
    from victor_amd.autocorr import Autocorr, SeriesState, series_sum, sokal_tau, sokal_window
    R, W, c = 3, 2, 5.0                                            # three seeds side by side
    x = np.concatenate([walkers_of(np.random.default_rng(seed), phi, n, 1, W, 1) for seed in (11, 12, 13)], axis=1)
    st = SeriesState(R, 1, W, L)
    for t in range(n):
        st.add(x[t])
    ac = Autocorr(["p"], W, st.n, c, st.arrays())
    assert ac.n == n and ac.max_lag == L and ac.c == c and ac.acf.shape == (R, 1, L) and ac.tau.shape == (R, 1)
    s = np.stack([series_sum(x[t], R, W) for t in range(n)])[:, :, 0]       # (n, R): the series the state was given
    assert np.all(np.abs(s - 380.0) < 120.0) and np.all(s.std(axis=0) > 10.0)
    for r in range(R):
        a = s[:, r] - s[0, r]
        rho, N, A = direct_acf(a, L)
        bound = rho_bound(a, N, A, rho)
        err = np.abs(ac.acf[r, 0].astype(np.longdouble) - rho).astype(float)
        amp = float(A[0] / N[0])
        print(f"phi {phi} seed {r}: max |d rho| {err.max():.3e}, bound {bound.max():.3e}, amplification {amp:.2f}")
        assert np.all(err <= bound), (r, np.argmax(err / bound))
        assert bound.max() < 1e-9 and amp < 20.0                   # (about the pivot: a few; about zero it would be ~ 380^2 / 20^2)
        # Sokal's window on the exact rho_k; the decision must lie outside what the bound can move
        taus = 2 * np.cumsum(rho) - 1
        dtau = 2 * np.cumsum(bound)
        tau_ref, window_ref, reached = sokal_window(rho, c)
        assert reached and 0 < window_ref < L - 1
        gap = np.abs(np.arange(L) - c * taus)[:window_ref + 1].astype(float)
        assert np.all(gap > c * dtau[:window_ref + 1]), "the window decision lies within the bound: choose another seed"
        assert ac.reached[r, 0] and ac.window[r, 0] == window_ref
        assert abs(ac.tau[r, 0] - tau_ref) <= dtau[window_ref] + 2.0 ** -52 * abs(tau_ref)
        assert ac.ess[r, 0] == W * n / ac.tau[r, 0]
        # ... and the history-based estimate: the same estimator through an FFT of length N = 2 n in double precision, whose
        # autocorrelations carry the transforms' rounding - for three radix-2 transforms and the squaring in between, at most
        # 16 u log2(N) of rho_0 = 1 per lag (the Cooley-Tukey bound, u log2 N in the 2-norm per transform, with room)
        fft = 16 * 2.0 ** -53 * np.log2(2 * n)
        assert np.all(gap > c * (dtau[:window_ref + 1] + 2 * fft * np.arange(1, window_ref + 2)))
        tau_h, window_h = sokal_tau(s[:, r], c)
        print(f"    tau {ac.tau[r, 0]:.12f}, from the history {tau_h:.12f}, window {window_ref}")
        assert window_h == window_ref
        assert abs(ac.tau[r, 0] - tau_h) <= dtau[window_ref] + 2 * fft * (window_ref + 1) + 2.0 ** -51 * abs(tau_ref)
        # the expected time of an AR(1) series, (1 + phi) / (1 - phi), to the noise of n samples
        assert 0.6 < ac.tau[r, 0] * (1 - phi) / (1 + phi) < 1.6


def test_a_window_that_is_not_reached():
    from victor_amd.autocorr import Autocorr, SeriesState
    n, L = 4096, 16
    x = walkers_of(np.random.default_rng(5), 0.99, n, 1, 2, 1)
    st = SeriesState(1, 1, 2, L)
    for t in range(n):
        st.add(x[t])
    ac = Autocorr(["p"], 2, st.n, 5.0, st.arrays())
    assert np.isnan(ac.tau[0, 0]) and not ac.reached[0, 0] and ac.window[0, 0] == -1 and np.isnan(ac.ess[0, 0])
    assert np.all(np.isfinite(ac.acf)) and np.all(ac.acf[0, 0, :8] > 0.8)
    # fewer steps than lags: the lags no step has reached are NaN, and nothing kept is all NaN
    few = SeriesState(1, 1, 2, L)
    for t in range(5):
        few.add(x[t])
    ac = Autocorr(["p"], 2, few.n, 5.0, few.arrays())
    assert np.all(np.isfinite(ac.acf[0, 0, :5])) and np.all(np.isnan(ac.acf[0, 0, 5:])) and ac.acf[0, 0, 0] == 1.0
    none = Autocorr(["p"], 2, 0, 5.0, SeriesState(1, 1, 2, L).arrays())
    assert np.all(np.isnan(none.acf)) and np.isnan(none.tau[0, 0]) and not none.reached[0, 0]


# ------------------------------------------------------------------ 3. the definition route ---------------------------------
# The stretch move refuses fewer than 2 (d + 1) = 8 walkers, so its ensemble has 8 where the Metropolis run has 4 chains.
RUNS = {"metropolis": (4, metropolis_block), "stretch": (8, stretch_block)}
OPTION = {"max_lag": 16, "c": 4.0}                                 # 33 kept steps: the ring wraps twice


def host(move, n, autocorr, **kw):
    from victor_amd.chains import sample_chains
    W, block = RUNS[move]
    return sample_chains(None, block("gauss"), n, walkers=W, seed=3, burn=5, thin=2, device=False, evaluate=evaluate_of("gauss"),
                         move=move, autocorr=autocorr, **kw)


def rebuilt(chain, L):
    """The state of a history (n_kept, R, W, d), rebuilt step by step."""
    from victor_amd.autocorr import SeriesState
    n, R, W, d = chain.shape
    st = SeriesState(R, d, W, L)
    for t in range(n):
        st.add(chain[t].reshape(R * W, d))
    return st


def same_state(ac, want, what=""):
    state = want.state if hasattr(want, "state") else {k: getattr(want, k) for k in FIELDS}
    assert ac.n == want.n, what
    for k in FIELDS:
        assert ac.state[k].dtype == np.float64 and same_bytes(ac.state[k], state[k]), (what, k)


@pytest.mark.parametrize("move", ["metropolis", "stretch"])
def test_definition_route_keeps_the_series_of_its_own_history(move):
    from victor_amd import GaussianPrior
    W = RUNS[move][0]
    ch = host(move, 70, OPTION)
    ac = ch.autocorr
    assert ch.chain.shape == (33, 1, W, 3) and ac.names == ["a", "b", "c"] and ac.n == 33 and ac.max_lag == 16 and ac.c == 4.0
    assert ac.tau.shape == ac.window.shape == ac.ess.shape == ac.reached.shape == (1, 3) and ac.acf.shape == (1, 3, 16)
    assert set(ac.state) == set(FIELDS) and ac.state["acc"].shape == (1, 3, 16) and ac.state["pivot"].shape == (1, 3)
    same_state(ac, rebuilt(ch.chain, 16), move)
    assert np.all(ac.acf[:, :, 0] == 1.0) and np.all(ac.state["acc"][:, :, 0] > 0.0)
    ok = ac.reached
    assert np.all(np.isnan(ac.tau[~ok])) and np.all(ac.ess[ok] == W * 33 / ac.tau[ok]) and np.all(ac.window[~ok] == -1)
    # nothing else changes, and off is off
    plain = host(move, 70, None)
    assert plain.autocorr is None and host(move, 70, False).autocorr is None
    for a in ("chain", "lnl_chain", "x", "n_accept", "sum1", "sum2"):
        assert getattr(plain, a).tobytes() == getattr(ch, a).tobytes(), a
    # True: the defaults
    default = host(move, 70, True).autocorr
    assert default.max_lag == 128 and default.c == 5.0 and np.all(np.isnan(default.acf[:, :, 33:]))
    assert same_bytes(default.state["acc"][:, :, :16], ac.state["acc"])
    # a cut run keeps accumulating (rebuilt after every extend); without a history the state is the same
    cut = host(move, 40, OPTION)
    part = cut.autocorr
    cut.extend(30)
    assert 0 < part.n < 33 and cut.autocorr is not part
    same_state(cut.autocorr, ac, "40 + 30")
    bare = host(move, 70, OPTION, keep_chain=False)
    assert bare.chain is None
    same_state(bare.autocorr, ac, "keep_chain=False")
    # under a prior and with histograms on: the state of that run's own history, and the run is the run without autocorr=
    kw = dict(prior=GaussianPrior(["a", "c"], [0.5, 0.1], cov=[[0.04, 0.01], [0.01, 0.02]]), marginals={"bins": 16})
    both, without = host(move, 70, OPTION, **kw), host(move, 70, None, **kw)
    same_state(both.autocorr, rebuilt(both.chain, 16), "prior and marginals")
    assert not same_bytes(both.chain, ch.chain), "the prior changed no decision"
    for a in ("chain", "lnl_chain", "lnprior_chain", "x", "n_accept", "sum1", "sum2", "mean", "cov"):
        assert same_bytes(getattr(both, a), getattr(without, a)), a
    assert all(np.array_equal(both.marginals.counts[k], without.marginals.counts[k]) for k in "abc")


def boom(*a, **k):
    raise AssertionError("the call reached an evaluation before refusing its input")


REFUSED = [({"max_lag": 0}, "max_lag must be an integer in 1..1024"),
           ({"max_lag": 1025}, "max_lag must be an integer in 1..1024"),
           ({"max_lag": 12.5}, "max_lag must be an integer in 1..1024"),
           ({"c": 0.0}, "c must be a finite number > 0"),
           ({"c": -5.0}, "c must be a finite number > 0"),
           ({"c": np.inf}, "c must be a finite number > 0"),
           ({"lag": 16}, "unknown keys"),
           ("yes", "None, True or a dict"),
           (128, "None, True or a dict")]


def test_refusals_come_before_any_evaluation():
    from victor_amd import InputError
    from victor_amd.chains import sample_chains
    for option, text in REFUSED:
        for move, (W, block) in RUNS.items():
            with pytest.raises(InputError, match=text):
                sample_chains(None, block("gauss"), 5, walkers=W, device=False, evaluate=boom, move=move, autocorr=option)
    with pytest.raises(AssertionError, match="reached an evaluation"):                     # a good option goes on
        sample_chains(None, metropolis_block("gauss"), 5, walkers=4, device=False, evaluate=boom, autocorr=OPTION)


# ------------------------------------------------------------------ 4. the surface ------------------------------------------
def test_the_keyword_is_on_every_public_path():
    import inspect

    import victor_amd
    from victor_amd.chains import sample_chains
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for fn in (victor_amd.CCFFit.sample_chains, Realisations.sample_chains, JointFit.sample_chains, JointRealisations.sample_chains, sample_chains):
        sig = inspect.signature(fn).parameters
        assert "autocorr" in sig and sig["autocorr"].default is None, fn


def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    want = {"vk_chain_set_autocorr": ["vk_chain* f", "int32_t group", "int32_t max_lag"],
            "vk_chain_autocorr": ["vk_chain* f", "double* pivot", "double* total", "double* head", "double* ring", "double* acc", "int64_t* n"]}
    for name in NEW:
        decl = re.search(r"int %s\(([^)]*)\);" % name, header)
        assert decl, f"include/victor_hip.h does not declare {name}"
        assert [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")] == want[name]
    dp = C.POINTER(C.c_double)
    assert N.SYMBOLS["vk_chain_set_autocorr"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32])
    assert N.SYMBOLS["vk_chain_autocorr"] == (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp, C.POINTER(C.c_int64)])
    csrc = os.path.join(ROOT, "victor_amd", "csrc")
    src = open(os.path.join(csrc, "vk_autocorr.h")).read()
    assert "hip/hip_runtime.h" not in src and "asm" not in src and "fp contract(off)" in src
    kernel = open(os.path.join(csrc, "vk_kernel_autocorr.h")).read()
    assert "vk_chain_series_kernel" in kernel and "atomic" not in kernel.split("#pragma once")[1] and "__shared__" not in kernel
    assert '#include "vk_kernel_autocorr.h"' in open(os.path.join(csrc, "vk_sampled.hip")).read()
    # one estimator in the tree: the timing tool imports it
    tool = open(os.path.join(ROOT, "tools", "stretch_timing.py")).read()
    assert "def sokal_tau" not in tool and "from victor_amd.autocorr import" in tool


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
