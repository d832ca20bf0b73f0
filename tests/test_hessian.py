"""Hessians and Laplace covariances (victor_amd/laplace.py, vk_fit_hessian) without a GPU: the statistic of
victor_amd/csrc/vk_hessian.h compiled on its own under g++ against the NumPy statement, bit for bit - the stencil's decoding and
points, A, the Cholesky factor, the Hessian, the covariance and the status -; an exact quadratic; every status and their
precedence; the host's policy at the faces of the box, ``refine``, the evidence of a Gaussian with a known integral, correlated
Metropolis proposals from a ``Laplace`` on the definition route; the refusals, raised before any device call; and the C ABI's
surface.
"""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.test_chains import HI, LO, NAMES, WIDTH, block_for, evaluate_of, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_hessian_rows", "vk_fit_hessian")
U = 2.0 ** -53

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_hessian.h"

static std::vector<double> in;
static FILE* fo;
static void put(double v) { fwrite(&v, sizeof(double), 1, fo); }

// stencil d      in: x[d], h[d]                               out: M, then per point m: j, k, sj, sk, coord[d]
// asm d n        in: lo[d], hi[d], then n x (x[d], h[d], v[M])  out: per problem status, A, hess, cov, L, W (each [d][d])
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
  const int d = atoi(argv[2]), M = vkhess::n_points(d);
  if (!strcmp(mode, "stencil")) {
    const double *x = p, *h = p + d;
    put((double)M);
    for (int m = 0; m < M; ++m) {
      const vkhess::Point pt = vkhess::decode(d, m);
      put(pt.j), put(pt.k), put(pt.sj), put(pt.sk);
      for (int i = 0; i < d; ++i) put(vkhess::coord(pt, i, x[i], h[i]));
    }
  } else if (!strcmp(mode, "asm")) {
    const int n = atoi(argv[3]);
    const double *lo = p, *hi = p + d;
    p += 2 * d;
    std::vector<double> A(d * d), H(d * d), Cv(d * d), L(d * d), W(d * d), S(d * d);
    for (int i = 0; i < n; ++i, p += 2 * d + M) {
      const int st = vkhess::assemble(d, p + 2 * d, p, p + d, lo, hi, A.data(), H.data(), Cv.data(), L.data(), W.data(), S.data());
      put((double)st);
      for (auto* a : {&A, &H, &Cv, &L, &W})
        for (double v : *a) put(v);
    }
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
    d = tmp_path_factory.mktemp("hessian_driver")
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


def driver_assemble(driver, values, x, h, lo, hi):
    """The g++ build of vkhess::assemble over R problems: (status, A, hess, cov, L, W)."""
    R, d = x.shape
    out = driver(["asm", d, R], [lo, hi, np.concatenate([x, h, values], axis=1)]).reshape(R, 1 + 5 * d * d)
    mats = out[:, 1:].reshape(R, 5, d, d)
    return out[:, 0].astype(np.int32), mats[:, 0], mats[:, 1], mats[:, 2], mats[:, 3], mats[:, 4]


def quadratic_values(Q, centre, x, h, noise=None, lo=None, hi=None):
    """lnL = -1/2 (p - centre)^T Q (p - centre) at the stencil points of every problem, plus noise: (R, M)."""
    from victor_amd.laplace import stencil_points
    pts = stencil_points(x, h, lo, hi) - centre
    v = -0.5 * np.einsum("rmj,jk,rmk->rm", pts, Q, pts)
    return v if noise is None else v + noise


# ------------------------------------------------------------------ 1. the header under g++ against the mirror --------------
@pytest.mark.parametrize("d", [1, 2, 4, 7, 10])
def test_stencil_decoding_and_points_bit_for_bit(driver, d):
    from victor_amd import laplace as L
    rng = np.random.default_rng(d)
    x, h = rng.uniform(-1, 1, d), rng.uniform(0.01, 0.3, d)
    out = driver(["stencil", d], [x, h])
    M = int(out[0])
    assert M == 2 * d * d + 1 == L.n_points(d)
    rec = out[1:].reshape(M, 4 + d)
    pts = L.stencil_points(x[None], h[None])[0]
    assert pts.shape == (M, d) and same_bytes(rec[:, 4:], pts)
    seen = set()
    for m in range(M):
        j, k, sj, sk = (int(v) for v in rec[m, :4])
        assert (j, k, sj, sk) == L.decode(d, m), m
        seen.add((j, k, sj, sk))
        if m == 0:
            assert (j, k) == (-1, -1) and same_bytes(pts[m], x)
        elif k < 0:
            assert m == L.at_axis(j, 0 if sj > 0 else 1) and 0 <= j < d
            want = x.copy()
            want[j] = x[j] + h[j] if sj > 0 else x[j] - h[j]
            assert same_bytes(pts[m], want)
        else:
            assert 0 <= j < k < d and m == L.at_pair(d, j, k, (0 if sj > 0 else 2) + (0 if sk > 0 else 1))
            want = x.copy()
            want[j] = x[j] + h[j] if sj > 0 else x[j] - h[j]
            want[k] = x[k] + h[k] if sk > 0 else x[k] - h[k]
            assert same_bytes(pts[m], want)
    assert len(seen) == M                                         # every index decodes to a point of its own
    pairs = [(j, k) for j in range(d) for k in range(j + 1, d)]
    assert [L.pair_index(d, j, k) for j, k in pairs] == list(range(len(pairs)))


@pytest.mark.parametrize("d", [1, 2, 4, 7, 10])
def test_assemble_against_numpy_bit_for_bit(driver, d):
    """Random SPD quadratics plus noise: A, L, W, hess, cov and status of the g++ build are the mirror's bytes."""
    from victor_amd import laplace as L
    rng = np.random.default_rng(10 + d)
    R = 33
    a = rng.standard_normal((d, d))
    Q = a @ a.T + d * np.eye(d)
    lo, hi = np.full(d, -10.0), np.full(d, 10.0)
    x, h = rng.uniform(-1, 1, (R, d)), rng.uniform(0.05, 0.5, (R, d))
    v = quadratic_values(Q, rng.uniform(-0.2, 0.2, d), x, h, 1e-9 * rng.standard_normal((R, L.n_points(d))))
    # (problems of other statuses among them: a stencil outside the box, a value that is not finite, a negative curvature)
    x[1, 0], v[2, L.n_points(d) - 1] = 9.9, -np.inf
    v[3, L.at_axis(d - 1, 0)] += 50.0
    st, A, H, Cv, Lc, W = driver_assemble(driver, v, x, h, lo, hi)
    m = L.assemble(v, x, h, lo, hi)
    assert st[1] == L.AT_BOUND and st[2] == L.NOT_FINITE and st[3] == L.NOT_POSDEF and np.all(st[4:] == L.OK) and st[0] == L.OK
    assert np.array_equal(st, m.status)
    assert same_bytes(A, m.a) and same_bytes(H, m.hess) and same_bytes(Cv, m.cov)
    ok = st == L.OK
    assert same_bytes(Lc[ok], m.chol[ok]) and same_bytes(W[ok], m.winv[ok])
    assert d * (d + 1) // 2 <= 55
    # ... and the statement is the inverse Hessian of the quadratic, to the noise
    want = np.linalg.inv(Q)
    assert np.allclose(m.cov[ok], want, rtol=0, atol=1e-4 * np.abs(want).max())
    assert np.allclose(m.hess[ok], -Q, rtol=0, atol=1e-4 * np.abs(Q).max())
    assert np.all(np.swapaxes(m.a[ok], 1, 2) == m.a[ok]) and np.all(np.swapaxes(m.cov[ok], 1, 2) == m.cov[ok])


# ------------------------------------------------------------------ 2. an exact quadratic -----------------------------------
def test_exact_quadratic(driver):
    """Dyadic coefficients, centre and steps: every value of the stencil is exact, so A is -H o (h h^T) exactly, and
    cov (-hess) = I to 64 u kappa(A) (steps that are powers of two scale exactly)."""
    from victor_amd import laplace as L
    Q = np.array([[4.0, 1.0, 0.5, 0.0], [1.0, 3.0, 0.25, 0.5], [0.5, 0.25, 2.0, 1.0], [0.0, 0.5, 1.0, 5.0]])
    centre = np.array([0.25, -0.5, 0.125, 0.0])
    x = np.array([[0.5, 0.25, -0.25, 0.75], centre])
    h = np.array([[0.25, 0.5, 0.125, 0.25], [0.5, 0.5, 0.25, 1.0]])
    lo, hi = np.full(4, -8.0), np.full(4, 8.0)
    v = quadratic_values(Q, centre, x, h)
    m = L.assemble(v, x, h, lo, hi)
    st, A, H, Cv, _, _ = driver_assemble(driver, v, x, h, lo, hi)
    assert np.all(m.status == L.OK) and np.array_equal(st, m.status)
    want = Q[None] * h[:, :, None] * h[:, None, :]
    assert np.array_equal(m.a, want) and np.array_equal(A, want)
    assert np.array_equal(m.hess, np.broadcast_to(-Q, (2, 4, 4))) and same_bytes(H, m.hess) and same_bytes(Cv, m.cov)
    for r in range(2):
        kappa = np.linalg.cond(want[r])
        err = np.abs(m.cov[r] @ -m.hess[r] - np.eye(4)).max()
        print("problem", r, "kappa", kappa, "|cov (-hess) - I|", err, "bound", 64 * U * kappa)
        assert err <= 64 * U * kappa


# ------------------------------------------------------------------ 3. each status ------------------------------------------
def test_each_status_and_their_precedence(driver):
    from victor_amd import laplace as L
    d = 3
    Q = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.5], [0.0, 0.5, 2.0]])
    lo, hi = np.full(d, -1.0), np.full(d, 1.0)
    x = np.tile([0.5, 0.0, 0.0], (8, 1))
    h = np.full((8, d), 0.25)
    h[4, 0] = 0.5                              # x + h == hi: still inside
    h[5, 0] = 0.5 + 2.0 ** -52                 # one ulp beyond the face
    h[6, 0] = h[7, 0] = 0.5 + 2.0 ** -52
    assert x[5, 0] + h[5, 0] == np.nextafter(1.0, 2.0)
    v = quadratic_values(Q, np.zeros(d), x, h)
    v[1, 7] = -np.inf                          # one value -inf
    v[2, 11] = np.nan                          # one value NaN
    saddle = Q.copy()
    saddle[2, 2] = -2.0
    v[3] = quadratic_values(saddle, np.zeros(d), x[3:4], h[3:4])[0]
    v[6, 3] = np.nan                           # at the bound AND not finite: at the bound
    v[7] = v[3]                                # at the bound AND a saddle
    v[2, :] = np.where(np.isnan(v[2]), np.nan, quadratic_values(saddle, np.zeros(d), x[2:3], h[2:3])[0])   # not finite AND a saddle
    m = L.assemble(v, x, h, lo, hi)
    st, A, H, Cv, _, _ = driver_assemble(driver, v, x, h, lo, hi)
    assert m.status.tolist() == [L.OK, L.NOT_FINITE, L.NOT_FINITE, L.NOT_POSDEF, L.OK, L.AT_BOUND, L.AT_BOUND, L.AT_BOUND]
    assert np.array_equal(st, m.status) and same_bytes(A, m.a) and same_bytes(H, m.hess) and same_bytes(Cv, m.cov)
    for r in (1, 2, 5, 6, 7):                  # not finite, at the bound: nothing is given
        assert np.all(np.isnan(m.hess[r])) and np.all(np.isnan(m.cov[r])) and np.all(np.isnan(m.a[r]))
    assert np.all(np.isfinite(m.hess[3])) and np.all(np.isfinite(m.a[3])) and np.all(np.isnan(m.cov[3]))    # a saddle: hess, no cov
    assert np.allclose(m.hess[3], -saddle, rtol=0, atol=1e-12)
    for r in (0, 4):
        assert np.all(np.isfinite(m.cov[r])) and np.allclose(m.cov[r], np.linalg.inv(Q), rtol=1e-10)
    # x itself outside the box
    out = L.assemble(v[:1], np.array([[1.5, 0.0, 0.0]]), h[:1], lo, hi)
    assert out.status[0] == L.AT_BOUND
    # at the bound every point of the stencil is x: the rows the device evaluates
    pts = L.stencil_points(x, h, lo, hi)
    assert np.all(pts[5] == x[5]) and not np.all(pts[4] == x[4])


# ------------------------------------------------------------------ 4. host logic -------------------------------------------
def gauss3():
    """lnL of tests/test_chains.py's "gauss", its precision matrix and its mean."""
    P = np.array([[9.0, 3.5, 0.0], [3.5, 4.0, 0.0], [0.0, 0.0, 25.0]])
    return P, np.array([0.93, -0.2, 0.1])


def test_face_policy():
    from victor_amd import laplace as L
    lo, hi = np.array([0.0, 0.0]), np.array([1.0, 1.0])
    h = np.array([[0.1, 0.2]] * 4)
    x = np.array([[0.5, 0.5], [1.0 - 0.05, 0.5], [0.5, 0.2 / 16], [1.0 - 0.1 / 16, 0.1]])
    got = L.face_steps(x, h, lo, hi, 8)
    assert same_bytes(got[0], h[0])                                        # far from every face: the steps as asked
    assert got[1, 0] == 0.999 * (1.0 - x[1, 0]) and got[1, 1] == 0.2          # at distance h / 2: shrunk
    assert got[2, 1] == 0.2 and got[2, 0] == 0.1                              # at distance h / 16: left alone ...
    assert got[3, 0] == 0.1 and got[3, 1] == 0.999 * 0.1                      # (at the lower face, distance h / 2)
    bound = L.at_bound(x, got, lo, hi)
    assert bound.tolist() == [False, False, True, True]                      # ... so that the stencil is flagged
    # through the call: the problem at h / 2 is OK with its step shrunk, the one at h / 16 is AT_BOUND
    P, mu = gauss3()
    block = block_for("gauss")
    at = {"a": np.array([0.5, 1.0 - WIDTH[0] / 2, 1.0 - WIDTH[0] / 16]), "b": -0.2, "c": 0.1}
    lap = L.laplace(None, block, at, device=False, evaluate=evaluate_of("gauss"))
    assert lap.status.tolist() == [L.OK, L.OK, L.AT_BOUND] and lap.ok.tolist() == [True, True, False]
    assert lap.step[0, 0] == WIDTH[0] and lap.step[1, 0] == 0.999 * (1.0 - at["a"][1]) and lap.step[2, 0] == WIDTH[0]
    assert np.allclose(lap.cov[:2], np.linalg.inv(P), rtol=1e-8) and np.all(np.isnan(lap.cov[2])) and np.all(np.isnan(lap.sigma[2]))
    assert lap.names == NAMES and lap.point(1) == {"a": float(at["a"][1]), "b": -0.2, "c": 0.1}
    assert lap.values is None and lap.x.shape == (3, 3) and lap.corr.shape == (3, 3, 3)
    assert np.allclose(np.einsum("rjj->rj", lap.corr[:2]), 1.0)


def test_refine_steps():
    from victor_amd import laplace as L
    P, mu = gauss3()
    block = block_for("gauss")
    at = {"a": np.array([0.5, 0.9]), "b": -0.2, "c": 0.1}
    kw = dict(device=False, evaluate=evaluate_of("gauss"), keep_values=True)
    first = L.laplace(None, block, at, **kw)
    second = L.laplace(None, block, at, refine=1, **kw)
    x = np.stack([at["a"], np.full(2, -0.2), np.full(2, 0.1)], axis=1)
    assert same_bytes(first.step, L.face_steps(x, np.tile(WIDTH, (2, 1)), LO, HI, 8))
    assert same_bytes(second.step, L.face_steps(x, 0.5 * first.sigma, LO, HI, 8))
    half_sigma = 0.5 * np.sqrt(np.diag(np.linalg.inv(P)))
    assert np.allclose(second.step[0], half_sigma, rtol=1e-6) and np.allclose(second.step[1, 1:], half_sigma[1:], rtol=1e-6)
    assert second.step[1, 0] == 0.999 * (1.0 - 0.9)               # (half a sigma reaches past the face: shrunk again)
    assert second.values.shape == (2, 19) and np.allclose(second.cov, np.linalg.inv(P), rtol=1e-8)
    # a pass that was not OK keeps its steps
    far = L.laplace(None, block, {"a": 1.0 - WIDTH[0] / 16, "b": -0.2, "c": 0.1}, refine=2, **kw)
    assert far.status[0] == L.AT_BOUND and same_bytes(far.step[0], WIDTH)


def test_evidence_of_a_gaussian_and_none_under_a_prior():
    from victor_amd import GaussianPrior
    from victor_amd import laplace as L
    P, mu = gauss3()
    block = block_for("gauss")
    lap = L.laplace(None, block, dict(zip(NAMES, mu - [0.1, 0.0, 0.0])), device=False, evaluate=evaluate_of("gauss"))
    # the integral of exp(lnL) over the whole space is (2 pi)^(3/2) det(P)^(-1/2) wherever the expansion is made; the uniform
    # prior's density is 1 / 8.  The stencil of a quadratic is exact to the rounding of its values (|v| <= 1, entries of A
    # 1e-2 and more: 1e-13 relative)
    want = 1.5 * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(P)[1] - np.log(8.0)
    lnl_at = -0.5 * 9.0 * 0.01
    assert lap.status[0] == L.OK and abs(lap.lnpost[0] - lnl_at) <= 1e-15
    laplace_value = lap.ln_evidence[0] - lap.lnpost[0]
    assert abs(laplace_value - want) <= 1e-10, (laplace_value, want)
    assert np.all(lap.lnprior == 0.0) and same_bytes(lap.lnl, lap.lnpost) and same_bytes(lap.chi2, -2.0 * lap.lnpost)
    prior = GaussianPrior(["b"], [-0.1], sigma=[0.2])
    post = L.laplace(None, block, dict(zip(NAMES, mu)), prior=prior, device=False, evaluate=evaluate_of("gauss"))
    assert post.ln_evidence is None
    assert np.allclose(post.hessian[0], -(P + np.diag([0.0, 25.0, 0.0])), rtol=0, atol=1e-9)
    assert post.lnprior[0] == -0.5 * (0.1 / 0.2) ** 2 or abs(post.lnprior[0] + 0.125) <= 1e-15
    assert same_bytes(post.lnl, post.lnpost - post.lnprior)
    # a problem that is not OK has no evidence
    far = L.laplace(None, block, {"a": 1.0 - WIDTH[0] / 16, "b": -0.2, "c": 0.1}, device=False, evaluate=evaluate_of("gauss"))
    assert np.isnan(far.ln_evidence[0])


def test_correlated_proposals_on_the_definition_route():
    from victor_amd import laplace as L
    from victor_amd.chains import sample_chains
    block = block_for("gauss")
    kw = dict(walkers=64, seed=3, device=False, evaluate=evaluate_of("gauss"))
    before = sample_chains(None, block, 20, **kw)                    # (before any Laplace is constructed)
    P, mu = gauss3()
    lap = L.laplace(None, block, {"a": 0.8, "b": -0.2, "c": 0.1}, device=False, evaluate=evaluate_of("gauss"))
    assert lap.status[0] == L.OK
    after = sample_chains(None, block, 20, proposal=None, **kw)
    widths = sample_chains(None, block, 20, proposal={"a": float(WIDTH[0])}, **kw)
    for a in ("chain", "lnl_chain", "x", "n_accept", "sum1", "sum2"):
        assert same_bytes(getattr(after, a), getattr(before, a)) and same_bytes(getattr(widths, a), getattr(before, a)), a
    ch = sample_chains(None, block, 20, proposal=lap, **kw)
    assert not same_bytes(ch.chain, before.chain) and same_bytes(ch.pivot, before.pivot)       # the same starts, other increments
    dz, logu = ch._draw_block()
    assert dz.shape == (64, 64, 3) and logu.shape == (64, 64)
    z = dz.reshape(4096, 3)
    want = 2.38 ** 2 / 3 * lap.cov[0]
    emp = z.T @ z / len(z)
    se = np.sqrt((np.outer(np.diag(want), np.diag(want)) + want ** 2) / len(z))
    print("empirical - wanted, in standard errors:", (emp - want) / se)
    assert np.all(np.abs(emp - want) <= 6 * se)
    assert np.allclose(lap.proposal_factors(WIDTH)[0] @ lap.proposal_factors(WIDTH)[0].T, want, rtol=1e-12)
    # a problem whose status is not OK falls back to the widths: the increments of a run without a proposal
    far = L.laplace(None, block, {"a": 1.0 - WIDTH[0] / 16, "b": -0.2, "c": 0.1}, device=False, evaluate=evaluate_of("gauss"))
    assert far.status[0] == L.AT_BOUND and np.array_equal(far.proposal_factors(WIDTH)[0], np.diag(WIDTH))
    fallback = sample_chains(None, block, 20, proposal=far, **kw)
    assert np.array_equal(fallback.chain, before.chain)
    # a BestFit carrying a Laplace is taken for it
    from victor_amd.fitting import BestFit
    bf = BestFit(NAMES, lap.x, {}, lap.lnpost, lap.chi2, np.zeros(1, np.int32), np.ones(1, np.int32), np.ones(1, np.int64))
    assert bf.laplace is None and bf.cov is None and bf.sigma is None and "laplace" not in vars(bf)
    bf.laplace = lap
    assert same_bytes(sample_chains(None, block, 20, proposal=bf, **kw).chain, ch.chain)


def boom(*a, **k):
    raise AssertionError("the call reached the device before refusing its input")


def test_refusals_come_before_any_device_call():
    import victor_amd
    from victor_amd import InputError
    from victor_amd import laplace as L
    from victor_amd.chains import sample_chains
    params = cases.cobaya_info()["params"]
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    fit._get_engine = boom
    at = {"fsigma8": 0.47, "beta": 0.4, "sigma_v": 380.0, "epsilon": 1.0}
    with pytest.raises(InputError, match="at= is needed"):
        fit.laplace(params, None)
    with pytest.raises(InputError, match="gives no value of beta"):
        fit.laplace(params, {k: v for k, v in at.items() if k != "beta"})
    with pytest.raises(InputError, match="not sampled"):
        fit.laplace(params, dict(at, sigma_w=3.0))
    with pytest.raises(InputError, match="outside its prior"):
        fit.laplace(params, dict(at, sigma_v=1e4))
    with pytest.raises(InputError, match="not finite"):
        fit.laplace(params, dict(at, sigma_v=np.nan))
    with pytest.raises(InputError, match="different lengths"):
        fit.laplace(params, dict(at, sigma_v=np.array([380.0, 390.0]), beta=np.array([0.4, 0.41, 0.42])))
    with pytest.raises(InputError, match="step must be finite and > 0"):
        fit.laplace(params, at, step={"beta": 0.0})
    with pytest.raises(InputError, match="step must be finite and > 0"):
        fit.laplace(params, at, step={"beta": np.inf})
    with pytest.raises(InputError, match="step names parameters"):
        fit.laplace(params, at, step={"gamma": 0.1})
    with pytest.raises(InputError, match="shrink"):
        fit.laplace(params, at, shrink=0.5)
    with pytest.raises(InputError, match="refine"):
        fit.laplace(params, at, refine=-1)
    with pytest.raises(InputError, match="refine"):
        fit.laplace(params, at, refine=1.5)
    with pytest.raises(InputError, match="every parameter is fixed"):
        fit.laplace(params, at, fixed=at)
    with pytest.raises(InputError, match="GaussianPrior or a list"):
        fit.laplace(params, at, prior={"sigma_v": (380.0, 20.0)})
    with pytest.raises(InputError, match="need a JointFit"):
        fit.laplace(dict(params, **{"sigma_v@1": params["sigma_v"]}), dict(at, **{"sigma_v@1": 380.0}))
    with pytest.raises(InputError, match="host route only"):
        L.laplace(None, block_for("gauss"), {"a": 0.5, "b": 0.0, "c": 0.0}, evaluate=evaluate_of("gauss"))
    with pytest.raises(InputError, match="a fit or an evaluate callable"):
        L.laplace(None, block_for("gauss"), {"a": 0.5, "b": 0.0, "c": 0.0}, device=False)
    wide = {f"p{j}": {"prior": {"min": 0.0, "max": 1.0}, "ref": {"loc": 0.5, "scale": 0.1}, "proposal": 0.1} for j in range(11)}
    with pytest.raises(InputError, match="at most 10"):
        L.laplace(None, wide, {n: 0.5 for n in wide}, device=False, evaluate=lambda b: -b["p0"] ** 2)
    # at= a BestFit of other parameters
    from victor_amd.fitting import BestFit
    one = np.zeros(1)
    bf = BestFit(["fsigma8", "beta"], np.array([[0.47, 0.4]]), {}, one, one, np.zeros(1, np.int32), np.ones(1, np.int32), np.ones(1, np.int64))
    with pytest.raises(InputError, match="pass the same params block and the same fixed"):
        fit.laplace(params, bf)
    with pytest.raises(AssertionError, match="reached the device"):          # good arguments go on to the device
        fit.laplace(params, at, step={"beta": 0.01}, refine=1, shrink=4)
    with pytest.raises(AssertionError, match="reached the device"):
        fit.laplace(params, bf, fixed={"sigma_v": 380.0, "epsilon": 1.0})
    # best_fit(covariance=...)
    with pytest.raises(InputError, match="covariance must be True or a dict"):
        fit.best_fit(params, covariance="yes")
    with pytest.raises(InputError, match="unknown keys"):
        fit.best_fit(params, covariance={"steps": {}})
    with pytest.raises(InputError, match="step must be finite and > 0"):
        fit.best_fit(params, covariance={"step": {"beta": -1.0}})
    with pytest.raises(InputError, match="shrink"):
        fit.best_fit(params, covariance={"shrink": 0})
    with pytest.raises(AssertionError, match="reached the device"):
        fit.best_fit(params, covariance={"refine": 1})
    # sample_chains(proposal=...)
    lap = L.laplace(None, block_for("gauss"), {"a": 0.5, "b": 0.0, "c": 0.0}, device=False, evaluate=evaluate_of("gauss"))
    kw = dict(device=False, evaluate=evaluate_of("gauss"))
    with pytest.raises(InputError, match="proposal must be a dict"):
        sample_chains(None, block_for("gauss"), 5, proposal=[0.1, 0.1, 0.1], **kw)
    with pytest.raises(InputError, match="proposal must be a dict"):
        sample_chains(None, block_for("gauss"), 5, proposal=bf, **kw)          # a BestFit without a Laplace
    with pytest.raises(InputError, match="holds the parameters"):
        sample_chains(None, block_for("gauss"), 5, proposal=lap, fixed={"c": 0.1}, **kw)
    with pytest.raises(InputError, match="mean nothing under move='stretch'"):
        sample_chains(None, block_for("gauss"), 5, proposal=lap, move="stretch", walkers=8, **kw)
    two = L.laplace(None, block_for("gauss"), {"a": np.array([0.5, 0.6]), "b": 0.0, "c": 0.0}, **kw)
    with pytest.raises(InputError, match="holds 2 problems"):
        sample_chains(None, block_for("gauss"), 5, proposal=two, **kw)
    with pytest.raises(InputError, match="holds the parameters"):
        fit.sample_chains(params, 5, proposal=lap)


def test_the_methods_are_on_all_four_classes():
    import inspect

    import victor_amd
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for cls in (victor_amd.CCFFit, Realisations, JointFit, JointRealisations):
        sig = inspect.signature(cls.laplace).parameters
        assert list(sig)[:10] == ["self", "params", "at", "step", "fixed", "prior", "shrink", "refine", "keep_values", "kwargs"], cls
        assert sig["shrink"].default == 8 and sig["refine"].default == 0 and sig["keep_values"].default is False
        assert inspect.signature(cls.best_fit).parameters["covariance"].default is None, cls
    assert victor_amd.Laplace is victor_amd.laplace.Laplace


# ------------------------------------------------------------------ 5. the C ABI's surface ----------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    dp, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    decl = re.search(r"int64_t vk_hessian_rows\(([^)]*)\);", header)
    assert decl and decl.group(1).strip() == "int32_t n_params"
    assert N.SYMBOLS["vk_hessian_rows"] == (C.c_int64, [C.c_int32])
    decl = re.search(r"int vk_fit_hessian\(([^)]*)\);", header)
    assert decl, "include/victor_hip.h does not declare vk_fit_hessian"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["vk_fit* f", "const double* x", "const double* h", "double* values", "double* a", "double* hess", "double* cov",
                    "double* lnpost", "double* chi2", "int32_t* status"]
    ctype = {"vk_fit*": C.c_void_p, "const double*": dp, "double*": dp, "int32_t*": i32}
    assert N.SYMBOLS["vk_fit_hessian"] == (C.c_int, [ctype[a.rsplit(" ", 1)[0]] for a in args])
    for name, value in (("OK", 0), ("AT_BOUND", 1), ("NOT_FINITE", 2), ("NOT_POSDEF", 3)):
        assert re.search(r"#define VK_HESS_%s %d\b" % (name, value), header) and getattr(N, "VK_HESS_" + name) == value
    src = open(os.path.join(ROOT, "victor_amd", "csrc", "vk_hessian.h")).read()
    assert "hip/hip_runtime.h" not in src and "#pragma clang fp contract(off)" in src
    for name, value in (("kOk", 0), ("kAtBound", 1), ("kNotFinite", 2), ("kNotPosdef", 3)):
        assert re.search(r"\b%s = %d\b" % (name, value), src), name


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
    rows = lib.vk_hessian_rows
    rows.restype, rows.argtypes = C.c_int64, [C.c_int32]
    assert [rows(d) for d in (1, 4, 10)] == [3, 33, 201] and rows(0) == 0 and rows(11) == 0
