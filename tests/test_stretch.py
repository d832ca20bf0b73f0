"""Stretch-move ensembles (victor_amd/chains.py ``move="stretch"``, vk_chain_begin_stretch) without a GPU: the half-step of
victor_amd/csrc/vk_stretch_step.h compiled on its own under g++ and driven on analytic functions, bit for bit against the NumPy
loop that defines the ensembles; that loop against ``EnsembleStretch``; cuts; the moment sums at the bound of tests/test_chains.py;
the refusals; and the C ABI's surface."""

import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_chains import HI, LO, NAMES, assert_sums, evaluate_of, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
W, D = 8, 3
# starts: the Gaussian's mean lies next to the face x_0 = 1 of the box [-1, 1]^3; the ensemble of "halfnan" starts wide enough
# to reach both the -inf half (x_0 < 0) and the NaN strip (0.3 < x_1 < 0.4)
REF = {"gauss": ((0.8, -0.1, 0.1), 0.1), "halfnan": ((0.3, 0.15, 0.0), 0.2)}


def block_for(fn):
    loc, scale = REF[fn]
    return {n: {"prior": {"min": float(LO[j]), "max": float(HI[j])}, "ref": {"loc": loc[j], "scale": scale}, "proposal": 0.1}
            for j, n in enumerate(NAMES)}


def host(fn, n, seed=3, walkers=W, **kw):
    from victor_amd.chains import sample_chains
    return sample_chains(None, block_for(fn), n, walkers=walkers, seed=seed, move="stretch", device=False, evaluate=evaluate_of(fn), **kw)


def randoms(fn, seed, n, walkers=W, a=2.0):
    """The numbers a stretch run of one problem consumes, drawn again by the stated protocol: the start as
    ``EnsembleMetropolis.initialise`` draws it, then per block of 64 sweeps 128 times (random, integers, random)."""
    from victor_amd.chains import _draw_start
    rng = np.random.default_rng(seed)
    loc, scale = REF[fn]
    x0 = np.array([_draw_start(rng, np.array(loc), np.full(D, scale), LO, HI, "ref") for _ in range(walkers)])
    half = walkers // 2
    z, k, logu = [], [], []
    for _ in range(((n + 63) // 64) * 128):
        z.append(((a - 1.0) * rng.random(half) + 1.0) ** 2 / a)
        k.append(rng.integers(0, half, size=half))
        logu.append(np.log(rng.random(half)))
    shape = (-1, 2, half)
    return x0, np.array(z).reshape(shape)[:n], np.array(k).reshape(shape)[:n], np.array(logu).reshape(shape)[:n]


DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_stretch_step.h"

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

// usage: driver fn d W n burn thin in out  then d values each of lo, hi
// in:  doubles x0[W][d], z[n][2][W/2], lz, logu, partner (as doubles) alike
// out: doubles, per sweep: kept, accept[W], outside[W], x[W][d], lnl[W], chi2[W]; then n_accept[W], n_steps[W], n_kept[W],
//      sum1[W][d], sum2[W][d(d+1)/2].  The state is held structure-of-arrays with stride W, the proposals with stride W/2, as the
//      device holds them.
int main(int argc, char** argv) {
  const char* fn = argv[1];
  vkchain::Box box{};
  box.d = atoi(argv[2]);
  const int d = box.d, W = atoi(argv[3]), n = atoi(argv[4]), half = W / 2;
  const long long burn = atoll(argv[5]), thin = atoll(argv[6]);
  int a = 9;
  for (int j = 0; j < d; ++j) box.lo[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < d; ++j) box.hi[j] = strtod(argv[a++], nullptr);
  const size_t per = (size_t)n * 2 * half;
  std::vector<double> in((size_t)W * d + 4 * per);
  FILE* fi = fopen(argv[7], "rb");
  if (!fi || fread(in.data(), sizeof(double), in.size(), fi) != in.size()) return 2;
  fclose(fi);
  const double *x0 = in.data(), *z = x0 + (size_t)W * d, *lz = z + per, *logu = lz + per, *partner = logu + per;
  const int T = vkchain::n_tri(d);
  std::vector<double> x((size_t)d * W), lnl(W), chi2(W), pivot((size_t)d * W), sum1((size_t)d * W), sum2((size_t)T * W);
  std::vector<double> prop((size_t)d * half);
  std::vector<int64_t> n_accept(W), n_steps(W), n_kept(W);
  auto view = [&](int c) {
    vkchain::View s{};
    s.stride = (size_t)W;
    s.x = x.data() + c; s.lnl = lnl.data() + c; s.chi2 = chi2.data() + c; s.pivot = pivot.data() + c;
    s.sum1 = sum1.data() + c; s.sum2 = sum2.data() + c;
    s.n_accept = n_accept.data() + c; s.n_steps = n_steps.data() + c; s.n_kept = n_kept.data() + c;
    return s;
  };
  FILE* fo = fopen(argv[8], "wb");
  if (!fo) return 2;
  auto put = [&](double v) { fwrite(&v, sizeof(double), 1, fo); };
  for (int c = 0; c < W; ++c) {
    vkchain::View s = view(c);
    vkchain::start(box, s, x0 + (size_t)c * d);
    const double l = lnl_of(fn, x0 + (size_t)c * d);
    vkchain::adopt(s, l, -2.0 * l);
  }
  std::vector<double> acc(W), out(W), res_l(half), res_c(half);
  for (int t = 0; t < n; ++t) {
    const bool kept = vkchain::is_kept(t, burn, thin);
    for (int side = 0; side < 2; ++side) {
      const size_t at = ((size_t)t * 2 + side) * half;
      for (int i = 0; i < half; ++i) {                       // the proposals of the whole half first, as the propose kernel does
        const int c = side * half + i, p = (1 - side) * half + (int)partner[at + i];
        const vkchain::View s = view(c);
        const bool in = vkchain::propose(box, s, x.data() + p, z[at + i], prop.data() + i, (size_t)half);
        double row[vkchain::kMaxP];
        for (int j = 0; j < d; ++j) row[j] = in ? prop[(size_t)j * half + i] : s.x[j * s.stride];
        res_l[i] = lnl_of(fn, row);
        res_c[i] = -2.0 * res_l[i];
        out[c] = in ? 0.0 : 1.0;
      }
      for (int i = 0; i < half; ++i) {
        const int c = side * half + i;
        vkchain::View s = view(c);
        acc[c] = vkchain::stretch_transition(box, s, prop.data() + i, (size_t)half, lz[at + i], logu[at + i], res_l[i], res_c[i], kept)
                     ? 1.0 : 0.0;
      }
    }
    put(kept ? 1.0 : 0.0);
    for (int c = 0; c < W; ++c) put(acc[c]);
    for (int c = 0; c < W; ++c) put(out[c]);
    for (int c = 0; c < W; ++c)
      for (int j = 0; j < d; ++j) put(x[(size_t)j * W + c]);
    for (int c = 0; c < W; ++c) put(lnl[c]);
    for (int c = 0; c < W; ++c) put(chi2[c]);
  }
  for (int c = 0; c < W; ++c) put((double)n_accept[c]);
  for (int c = 0; c < W; ++c) put((double)n_steps[c]);
  for (int c = 0; c < W; ++c) put((double)n_kept[c]);
  for (int c = 0; c < W; ++c)
    for (int j = 0; j < d; ++j) put(sum1[(size_t)j * W + c]);
  for (int c = 0; c < W; ++c)
    for (int i = 0; i < T; ++i) put(sum2[(size_t)i * W + c]);
  fclose(fo);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("stretch_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(fn, x0, z, k, logu, burn=0, thin=1):
        n, _, half = z.shape
        Wn = 2 * half
        lz = (D - 1) * np.log(z)
        fin, fout = d / "in.bin", d / "out.bin"
        np.concatenate([x0.ravel(), z.ravel(), lz.ravel(), logu.ravel(), k.astype(np.float64).ravel()]).astype(np.float64).tofile(str(fin))
        args = [str(exe), fn, str(D), str(Wn), str(n), str(burn), str(thin), str(fin), str(fout)]
        args += [repr(float(v)) for v in LO] + [repr(float(v)) for v in HI]
        subprocess.run(args, check=True)
        out = np.fromfile(str(fout), dtype=np.float64)
        per = 1 + Wn * (D + 4)
        steps, tail = out[: n * per].reshape(n, per), out[n * per:]
        T = D * (D + 1) // 2
        tri = tail[3 * Wn + Wn * D:].reshape(Wn, T)
        sum2 = np.empty((Wn, D, D))
        i = 0
        for j in range(D):
            for kk in range(j, D):
                sum2[:, j, kk] = sum2[:, kk, j] = tri[:, i]
                i += 1
        o = 1
        res = {"kept": steps[:, 0] == 1.0}
        for name, width in (("accept", Wn), ("outside", Wn), ("x", Wn * D), ("lnl", Wn), ("chi2", Wn)):
            res[name] = steps[:, o:o + width]
            o += width
        res["accept"], res["outside"], res["x"] = res["accept"] == 1.0, res["outside"] == 1.0, res["x"].reshape(n, Wn, D)
        res.update(n_accept=tail[:Wn].astype(np.int64), n_steps=tail[Wn:2 * Wn].astype(np.int64),
                   n_kept=tail[2 * Wn:3 * Wn].astype(np.int64), sum1=tail[3 * Wn:3 * Wn + Wn * D].reshape(Wn, D), sum2=sum2)
        return res
    return run


# ------------------------------------------------------------------ 1. the transition, bit for bit ------------------------
@pytest.mark.parametrize("fn", ["gauss", "halfnan"])
def test_transition_against_numpy_bit_for_bit(driver, fn):
    n, seed = 220, 3
    ch = host(fn, n, seed=seed)
    assert ch.move == "stretch" and ch.n_steps == n
    x0, z, k, logu = randoms(fn, seed, n)
    got = driver(fn, x0, z, k, logu)
    assert same_bytes(ch.pivot[0], x0)
    assert same_bytes(got["x"], ch.chain[:, 0]), fn                                   # every position of every sweep
    assert same_bytes(got["lnl"], ch.lnl_chain[:, 0]) and same_bytes(got["chi2"], ch.chi2_chain[:, 0])
    before = np.concatenate([x0[None], ch.chain[:-1, 0]])
    moved = np.any(ch.chain[:, 0] != before, axis=2)
    assert np.array_equal(got["accept"], moved), fn                                   # every decision
    assert np.array_equal(got["n_accept"], ch.n_accept[0]) and np.array_equal(got["n_accept"], moved.sum(axis=0))
    assert np.all(got["kept"]) and np.all(got["n_steps"] == n) and np.all(got["n_kept"] == n) and ch.n_kept == n
    assert np.all((got["x"] >= LO) & (got["x"] <= HI))
    assert np.array_equal(got["outside"].sum(axis=0), ch.n_outside[0])
    assert got["outside"].sum() > 0, "no proposal left the box: the test does not reach that rule"
    assert not np.any(got["accept"] & got["outside"])
    assert 0.05 < moved.mean() < 0.95, moved.mean()
    if fn == "halfnan":
        assert not np.any(np.isnan(got["lnl"]))
        assert np.all((got["x"][..., 0] >= 0.0) | (got["lnl"] == -INF))               # (a walker may START in the -inf half)
        assert np.all((got["x"][..., 1] <= 0.3) | (got["x"][..., 1] >= 0.4))           # never onto the NaN strip
        # ... which proposals did reach, as they reached the -inf half: rebuilt from the walk and the numbers
        hit_nan = hit_inf = 0
        for t in range(n):
            x = before[t].copy()
            for h in range(2):
                mv = np.arange(4) + 4 * h
                p = x[np.arange(4) + 4 * (1 - h)][k[t, h]]
                prop = p + z[t, h][:, None] * (x[mv] - p)
                inside = ((prop >= LO) & (prop <= HI)).all(axis=1)
                hit_inf += int(np.sum(inside & (prop[:, 0] < 0)))
                hit_nan += int(np.sum(inside & (prop[:, 0] >= 0) & (prop[:, 1] > 0.3) & (prop[:, 1] < 0.4)))
                x[mv] = ch.chain[t, 0][mv]
        assert hit_nan > 0 and hit_inf > 0, (hit_nan, hit_inf)


@pytest.mark.parametrize("burn,thin", [(10, 3), (37, 7), (300, 2)])
def test_kept_sweeps_follow_burn_and_thin(driver, burn, thin):
    n, seed = 220, 3
    full = host("gauss", n, seed=seed)
    ch = host("gauss", n, seed=seed, burn=burn, thin=thin)
    got = driver("gauss", *randoms("gauss", seed, n), burn, thin)
    want = list(range(burn, n, thin))
    assert np.array_equal(np.flatnonzero(got["kept"]), want)
    assert ch.n_kept == len(want) and np.all(got["n_kept"] == len(want))
    assert same_bytes(ch.chain, full.chain[want]) and same_bytes(ch.lnl_chain, full.lnl_chain[want])
    assert same_bytes(got["x"][want], ch.chain[:, 0]) and np.array_equal(got["n_accept"], ch.n_accept[0])
    if want:
        assert_sums(got["sum1"], got["sum2"], ch.chain[:, 0], ch.pivot[0], "driver")


# ------------------------------------------------------------------ 2. the definition route is EnsembleStretch's chain -----
def test_definition_route_is_the_chain_of_ensemble_stretch():
    from victor_amd.chains import sample_chains
    from victor_amd.sampler import EnsembleStretch, parse_cobaya_params
    block = dict(block_for("gauss"), scale=2.0)

    def f(batch):                                     # elementwise arithmetic only: a row's value does not depend on the batch
        u, v, w = batch["a"] - 0.93, batch["b"] + 0.2, batch["c"] - 0.1
        return -0.5 * batch["scale"] * (9.0 * (u * u) + 7.0 * (u * v) + 4.0 * (v * v) + 25.0 * (w * w))
    specs, fixed = parse_cobaya_params(block)
    for seed, a in ((0, 2.0), (11, 2.0), (5, 1.5)):
        es = EnsembleStretch(f, specs, W, seed=seed, fixed=fixed, a=a).initialise()
        start = es.x.copy()
        chain, lnl = es.run(150)
        ch = sample_chains(None, block, 150, walkers=W, seed=seed, move="stretch", stretch_a=a, device=False, evaluate=f)
        assert ch.names == es.names and ch.fixed == {"scale": 2.0} and ch.move == "stretch"
        assert same_bytes(ch.pivot[0], start)
        assert same_bytes(ch.chain[:, 0], chain) and same_bytes(ch.lnl_chain[:, 0], lnl)
        assert int(ch.n_accept.sum()) == es.n_accept and abs(ch.acceptance[0] - es.acceptance) < 1e-15
        assert ch.n_outside.sum() > 0
        more, more_lnl = es.run(70)
        ch.extend(70)
        assert same_bytes(ch.chain[150:, 0], more) and same_bytes(ch.lnl_chain[150:, 0], more_lnl)


# ------------------------------------------------------------------ 3. cuts ------------------------------------------------
@pytest.mark.parametrize("cuts", [(40, 50), (1, 63, 1, 25), (64, 26)])
def test_a_run_does_not_depend_on_how_it_is_cut(cuts):
    whole = host("gauss", 90, burn=5, thin=2)
    ch = host("gauss", cuts[0], burn=5, thin=2)
    for k in cuts[1:]:
        ch.extend(k)
    for a in ("x", "lnl", "chi2", "chain", "lnl_chain", "chi2_chain", "n_accept", "n_outside", "sum1", "sum2", "mean", "cov"):
        assert same_bytes(getattr(ch, a), getattr(whole, a)), (cuts, a)
    assert ch.n_steps == 90 and ch.n_kept == whole.n_kept == len(range(5, 90, 2)) and ch.decision_margin == whole.decision_margin
    assert same_bytes(ch.chain, host("gauss", 90).chain[5::2])                      # burn and thin count over the object's life


# ------------------------------------------------------------------ 4. moments and bookkeeping -----------------------------
def test_moment_sums_and_bookkeeping():
    n = 150
    for burn, thin in ((0, 1), (10, 3)):
        ch = host("gauss", n, burn=burn, thin=thin)
        assert_sums(ch.sum1[0], ch.sum2[0], ch.chain[:, 0], ch.pivot[0], "definition route")
        assert ch.rhat is None                                                      # the walkers are not independent chains
        assert ch.acceptance[0] == ch.n_accept[0].sum() / (n * W)
        assert ch.chain.shape == (ch.n_kept, 1, W, D) and ch.x.shape == (1, W, D) and ch.n_outside.shape == (1, W)
        assert np.isfinite(ch.decision_margin)
    lean = host("gauss", n, burn=10, thin=3, keep_chain=False)
    assert lean.chain is None and lean.rhat is None
    for a in ("x", "lnl", "chi2", "mean", "cov", "n_accept", "sum1", "sum2", "pivot"):
        assert same_bytes(getattr(lean, a), getattr(ch, a)), a
    from victor_amd.chains import sample_chains
    m = sample_chains(None, block_for("gauss"), 20, walkers=4, seed=1, device=False, evaluate=evaluate_of("gauss"))
    assert m.move == "metropolis" and m.rhat is not None


# ------------------------------------------------------------------ 5. refusals --------------------------------------------
def test_refusals():
    from victor_amd import InputError
    from victor_amd.chains import sample_chains
    block, f = block_for("gauss"), evaluate_of("gauss")

    def call(n=10, **kw):
        kw = dict(dict(walkers=W, move="stretch", device=False, evaluate=f), **kw)
        return sample_chains(None, block, n, **kw)
    with pytest.raises(InputError, match="even number of walkers"):
        call(walkers=9)
    with pytest.raises(InputError, match=r"at least 2 \(n_params \+ 1\) = 8"):
        call(walkers=6)
    for a in (1.0, 0.5, math.nan):
        with pytest.raises(InputError, match="stretch_a"):
            call(stretch_a=a)
    with pytest.raises(InputError, match="proposal"):
        call(proposal={"a": 0.1})
    at = {"a": 0.5, "b": -0.3, "c": 0.2}
    with pytest.raises(InputError, match="scatter must be > 0"):
        call(start=at, scatter=0)
    with pytest.raises(InputError, match="scatter must be > 0"):
        call(start=at, scatter={"b": 0.0})
    with pytest.raises(InputError, match="move must be"):
        call(move="walk")
    with pytest.raises(InputError, match="device=False"):
        call(device=True)
    ok = call(start=at)                               # the default scatter: the block's proposal widths
    assert np.all(ok.pivot != np.array([0.5, -0.3, 0.2])) and ok.n_steps == 10
    assert call(stretch_a=1.5).stretch_a == 1.5


def test_fit_entry_points_refuse_before_any_device_call():
    import inspect

    import victor_amd
    from tests import cases
    from victor_amd import InputError
    params = cases.cobaya_info()["params"]
    fit = victor_amd.CCFFit(*cases.boss_options("config"))

    def boom(*a, **k):
        raise AssertionError("sample_chains reached the device before refusing its input")
    fit._get_engine = boom
    with pytest.raises(InputError, match="even number of walkers"):
        fit.sample_chains(params, 10, walkers=8, move="stretch")                     # d = 4 needs 10
    with pytest.raises(InputError, match="stretch_a"):
        fit.sample_chains(params, 10, walkers=10, move="stretch", stretch_a=1.0)
    with pytest.raises(InputError, match="proposal"):
        fit.sample_chains(params, 10, walkers=10, move="stretch", proposal={"beta": 0.1})
    with pytest.raises(InputError, match="move must be"):
        fit.sample_chains(params, 10, move="gibbs")
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for cls in (victor_amd.CCFFit, Realisations, JointFit, JointRealisations):
        sig = inspect.signature(cls.sample_chains).parameters
        assert sig["move"].default == "metropolis" and sig["stretch_a"].default == 2.0, cls


# ------------------------------------------------------------------ 6. the C ABI's surface ---------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    decl = re.search(r"int vk_chain_begin_stretch\(([^)]*)\);", header)
    assert decl, "include/victor_hip.h does not declare vk_chain_begin_stretch"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["vk_chain* f", "int32_t n_steps", "int32_t walkers", "const double* z", "const double* lz", "const double* logu",
                    "const int32_t* partner", "int64_t first_step", "int64_t burn", "int64_t thin", "int32_t want_history",
                    "int32_t* n_kept"]
    ctype = {"vk_chain*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "const double*": C.POINTER(C.c_double),
             "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32)}
    res, proto = N.SYMBOLS["vk_chain_begin_stretch"]
    assert res is C.c_int and proto == [ctype[a.rsplit(" ", 1)[0]] for a in args]
    # the existing entry points keep their signatures
    assert re.search(r"int vk_chain_begin\(vk_chain\* f, int32_t n_steps, const double\* dz, const double\* logu, int64_t first_step, "
                     r"int64_t burn,\s+int64_t thin, int32_t want_history, int32_t\* n_kept\);", header)
