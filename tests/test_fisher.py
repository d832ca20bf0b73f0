"""Fisher matrices from model-vector Jacobians (victor_amd/fisher.py, vk_fit_fisher) without a GPU: the statistic of
victor_amd/csrc/vk_fisher.h compiled on its own under g++ against the NumPy statement, bit for bit - the stencil's points, D, G,
S, fisher, A, the Cholesky factor, its inverse, the covariance and the status, with one slice and with blended slices of a
deliberately non-symmetric precision, padded rows, two diagonal blocks, with and without a prior, the scale of the four
likelihood forms and the covariance bracket -; an exactly representable linear model; every status and their precedence; the
face policy; the refusals, raised before any device call on all four classes; the signatures; and the C ABI's surface.
"""

import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_joint_cov import correlated
from tests.test_joint_realisations import write_stacks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_fisher_rows", "vk_fit_fisher")
U = 2.0 ** -53

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vk_fisher.h"

static std::vector<double> in;
static FILE* fo;
static void put(double v) { fwrite(&v, sizeof(double), 1, fo); }

// stencil d        in: x[d], h[d]                         out: M, then per point m: coord[d]
// scale n          in: n x (form, nm, np, nd)             out: n x c
// bracket n m      in: g[n], beta[m]                      out: m x (lo, t)
// asm d N B n      in: lo[d], hi[d], c, prior.on, mu[10], pp[55], B x (n_b, ld_b, off_b), then
//                      n x (x[d], h[d], v[M][N], B x (t, P_lo[n_b][ld_b], P_last[n_b][ld_b]))
//                  out: per problem status, D[N][d], G[N][d], then S, fisher, A, cov, L, W (each [d][d])
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
  if (!strcmp(mode, "stencil")) {
    const int d = atoi(argv[2]), M = vkfisher::n_rows(d);
    const double *x = p, *h = p + d;
    put((double)M);
    for (int m = 0; m < M; ++m) {
      const vkhess::Point pt = vkhess::decode(d, m);
      for (int i = 0; i < d; ++i) put(vkhess::coord(pt, i, x[i], h[i]));
    }
  } else if (!strcmp(mode, "scale")) {
    const int n = atoi(argv[2]);
    for (int i = 0; i < n; ++i, p += 4) put(vkfisher::form_scale((int)p[0], p[1], p[2], p[3]));
  } else if (!strcmp(mode, "bracket")) {
    const int n = atoi(argv[2]), m = atoi(argv[3]);
    for (int i = 0; i < m; ++i) {
      int lo;
      double t;
      vkfisher::bracket(p, n, p[n + i], &lo, &t);
      put((double)lo), put(t);
    }
  } else if (!strcmp(mode, "asm")) {
    const int d = atoi(argv[2]), N = atoi(argv[3]), B = atoi(argv[4]), n = atoi(argv[5]), M = vkfisher::n_rows(d);
    const double *lo = p, *hi = p + d;
    p += 2 * d;
    const double c = *p++;
    vkprior::Prior prior{};
    prior.on = (int)*p++;
    for (int j = 0; j < vkprior::kMaxP; ++j) prior.mu[j] = *p++;
    for (int j = 0; j < vkprior::kMaxTri; ++j) prior.pp[j] = *p++;
    std::vector<vkfisher::Block> blocks(B);
    for (int b = 0; b < B; ++b, p += 3) blocks[b].n = (int)p[0], blocks[b].ld = (int)p[1], blocks[b].off = (int)p[2];
    std::vector<double> D(N * d), G(N * d), S(d * d), F(d * d), A(d * d), Cv(d * d), L(d * d), W(d * d), T(d * d);
    for (int i = 0; i < n; ++i) {
      const double *x = p, *h = p + d, *v = p + 2 * d;
      p += 2 * d + (size_t)M * N;
      for (int b = 0; b < B; ++b) {
        const size_t sz = (size_t)blocks[b].n * blocks[b].ld;
        blocks[b].t = *p++;
        blocks[b].lo = p;
        blocks[b].last = p + sz;
        p += 2 * sz;
      }
      const int st = vkfisher::assemble(d, N, v, x, h, lo, hi, blocks.data(), B, c, prior, D.data(), G.data(), S.data(), F.data(),
                                        A.data(), Cv.data(), L.data(), W.data(), T.data());
      put((double)st);
      for (auto* a : {&D, &G, &S, &F, &A, &Cv, &L, &W})
        for (double w : *a) put(w);
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
    d = tmp_path_factory.mktemp("fisher_driver")
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


def driver_assemble(driver, v, x, h, lo, hi, blocks, c=1.0, prior=None):
    """The g++ build of vkfisher::assemble over R problems.  ``blocks``: a list of (off, t (R,), P_lo (R, n, ld), P_last
    (R, n, ld)) - rows padded to ld.  Returns (status, D, G, S, fisher, A, cov, L, W)."""
    R, d = x.shape
    N = v.shape[2]
    head = [lo, hi, [c], [0.0 if prior is None else 1.0], np.zeros(10) if prior is None else np.pad(prior.mu, (0, 10 - d)),
            np.zeros(55) if prior is None else np.pad(prior.pp, (0, 55 - len(prior.pp)))]
    for off, t, p_lo, p_last in blocks:
        head.append([p_lo.shape[1], p_lo.shape[2], off])
    body = []
    for r in range(R):
        body += [x[r], h[r], v[r]]
        for off, t, p_lo, p_last in blocks:
            body += [[t[r]], p_lo[r], p_last[r]]
    out = driver(["asm", d, N, len(blocks), R], head + body).reshape(R, 1 + 2 * N * d + 6 * d * d)
    D, G = out[:, 1:1 + N * d].reshape(R, N, d), out[:, 1 + N * d:1 + 2 * N * d].reshape(R, N, d)
    mats = out[:, 1 + 2 * N * d:].reshape(R, 6, d, d)
    return (out[:, 0].astype(np.int32), D, G) + tuple(mats[:, i] for i in range(6))


def mirror_blocks(blocks):
    from victor_amd.fisher import Block
    return [Block(off, p_lo[:, :, :p_lo.shape[1]], p_last[:, :, :p_lo.shape[1]], t) for off, t, p_lo, p_last in blocks]


def random_problems(rng, R, d, N, sizes, pad=3):
    """R problems of a smooth model with N entries over the diagonal blocks ``sizes``: vectors (R, M, N), x, h, the box, and
    blocks with NON-SYMMETRIC slices, rows padded by ``pad``, weights t = 0 for even problems and in (0, 1) for odd ones."""
    from victor_amd.fisher import stencil_points
    lo, hi = np.full(d, -10.0), np.full(d, 10.0)
    x, h = rng.uniform(-1, 1, (R, d)), rng.uniform(0.05, 0.5, (R, d))
    J = rng.standard_normal((N, d))
    pts = stencil_points(x, h, lo, hi)
    v = rng.standard_normal(N) + np.einsum("ak,rmk->rma", J, pts) + 0.05 * np.sin(np.einsum("ak,rmk->rma", J[::-1], pts))
    blocks, off = [], 0
    for n in sizes:
        def slices():
            a = rng.standard_normal((R, n, n))
            p = np.einsum("rij,rkj->rik", a, a) + n * np.eye(n) + 0.3 * rng.standard_normal((R, n, n))      # not symmetric
            return np.concatenate([p, 7.0 + rng.standard_normal((R, n, pad))], axis=2)                    # the padding is never read
        t = np.where(np.arange(R) % 2 == 0, 0.0, rng.uniform(0.05, 0.95, R))
        blocks.append((off, t, slices(), slices()))
        off += n
    assert off == N
    return v, x, h, lo, hi, blocks


def compare(got, m, tag):
    st, D, G, S, F, A, Cv, L, W = got
    assert np.array_equal(st, m.status), tag
    for name, a, b in (("D", D, m.D), ("G", G, m.G), ("S", S, m.S), ("fisher", F, m.fisher), ("A", A, m.a), ("cov", Cv, m.cov)):
        assert same_bytes(a, b), (tag, name)
    ok = st == 0
    assert same_bytes(L[ok], m.chol[ok]) and same_bytes(W[ok], m.winv[ok]), tag


# ------------------------------------------------------------------ 1. the header under g++ against the mirror --------------
@pytest.mark.parametrize("d", [1, 2, 4, 7, 10])
def test_stencil_points_bit_for_bit(driver, d):
    from victor_amd import fisher as F
    from victor_amd import laplace as L
    rng = np.random.default_rng(d)
    x, h = rng.uniform(-1, 1, d), rng.uniform(0.01, 0.3, d)
    out = driver(["stencil", d], [x, h])
    M = int(out[0])
    assert M == 2 * d + 1 == F.n_rows(d)
    pts = F.stencil_points(x[None], h[None])[0]
    assert pts.shape == (M, d) and same_bytes(out[1:].reshape(M, d), pts)
    assert same_bytes(pts, L.stencil_points(x[None], h[None])[0][:M])          # the first 2 d + 1 points of the Hessian's stencil
    assert same_bytes(pts[0], x)
    for j in range(d):
        for s, disp in ((0, x[j] + h[j]), (1, x[j] - h[j])):
            want = x.copy()
            want[j] = disp
            assert same_bytes(pts[1 + 2 * j + s], want)


@pytest.mark.parametrize("N", [1, 2, 7, 60, 130])
@pytest.mark.parametrize("d", [1, 2, 4, 7, 10])
def test_assemble_against_numpy_bit_for_bit(driver, d, N):
    """One block, rows padded: problems with one slice (t = 0) and with blended slices, a non-symmetric P; then the same under a
    prior and a scale that is no power of two.  Among the problems one of every other status."""
    from victor_amd import fisher as F
    from victor_amd.priors import GaussianPrior, resolve_prior
    rng = np.random.default_rng(100 * d + N)
    R = 8
    v, x, h, lo, hi, blocks = random_problems(rng, R, d, N, [N])
    x[1, 0] = 9.99                                       # the stencil leaves the box
    v[2, 2 * d, N - 1] = np.inf                           # an entry of the last vector
    v[3, 2 * d - 1] = v[3, 2 * d]                         # the theory does not depend on the last parameter: D_(., d-1) = 0
    names = [f"p{j}" for j in range(d)]
    cv = rng.standard_normal((d, d))
    prior = resolve_prior(GaussianPrior(names, np.zeros(d), cov=cv @ cv.T + d * np.eye(d)), "test", names, lo, hi)
    for c, pr in ((1.0, None), (0.8341, prior)):
        got = driver_assemble(driver, v, x, h, lo, hi, blocks, c, pr)
        m = F.assemble(v, x, h, lo, hi, mirror_blocks(blocks), c, None if pr is None else pr.pp)
        compare(got, m, (d, N, c))
        want = [F.OK, F.AT_BOUND, F.NOT_FINITE, F.NOT_POSDEF if pr is None else F.OK] + [F.OK] * 4
        if N >= 2 * d:                                   # (few entries against the parameters: J^T P J is singular or close to it)
            assert m.status.tolist() == want, (m.status, c)
        assert m.status[1] == F.AT_BOUND and m.status[2] == F.NOT_FINITE and (pr is not None or m.status[3] == F.NOT_POSDEF)
        assert np.all(m.S[3, d - 1, :] == 0.0) and np.all(np.isfinite(m.fisher[3]))
        if pr is None:
            assert np.all(np.isnan(m.cov[3])) and same_bytes(m.a[3], 0.25 * m.S[3])
        for r in (1, 2):
            assert all(np.all(np.isnan(a[r])) for a in (m.fisher, m.a, m.cov))
    # a transposed read of P would show: the mirror with P^T differs
    if N > 1 and d > 0:
        flipped = [(off, t, np.concatenate([np.swapaxes(lo_[:, :, :N], 1, 2), lo_[:, :, N:]], axis=2), last) for off, t, lo_, last in blocks]
        assert not same_bytes(F.assemble(v, x, h, lo, hi, mirror_blocks(flipped)).G[0], m.G[0])
    # the blend is (1 - t) P_lo + t P_last, each product rounded, and P_lo itself where t == 0
    b = mirror_blocks(blocks)[0]
    P = b.precision(R)
    assert same_bytes(P[0], blocks[0][2][0][:, :N])
    t1 = blocks[0][1][1]
    assert same_bytes(P[1], (1.0 - t1) * blocks[0][2][1][:, :N] + t1 * blocks[0][3][1][:, :N])


@pytest.mark.parametrize("d,sizes", [(3, [7, 5]), (10, [60, 70]), (1, [1, 1])])
def test_two_diagonal_blocks_bit_for_bit(driver, d, sizes):
    """Block-diagonal P: G is formed block by block, S sums through the concatenated vector; each block its own weight."""
    from victor_amd import fisher as F
    rng = np.random.default_rng(7 * d + sizes[0])
    v, x, h, lo, hi, blocks = random_problems(rng, 6, d, sum(sizes), sizes)
    blocks[1] = (blocks[1][0], blocks[1][1][::-1].copy()) + blocks[1][2:]       # (block 1 blended where block 0 is not)
    got = driver_assemble(driver, v, x, h, lo, hi, blocks, 0.97)
    m = F.assemble(v, x, h, lo, hi, mirror_blocks(blocks), 0.97)
    compare(got, m, (d, sizes))
    assert np.all(m.status == F.OK)
    # ... and it is the dense statement with a block-diagonal matrix, to rounding
    n0 = sizes[0]
    for r in range(6):
        P = np.zeros((sum(sizes), sum(sizes)))
        P[:n0, :n0], P[n0:, n0:] = mirror_blocks(blocks)[0].precision(6)[r], mirror_blocks(blocks)[1].precision(6)[r]
        dense = np.tril(m.D[r].T @ P @ m.D[r])
        assert np.allclose(np.tril(m.S[r]), dense, rtol=1e-11, atol=1e-11 * np.abs(dense).max())


def test_form_scale_of_the_four_forms(driver):
    from victor_amd import _native as N
    from victor_amd import fisher as F
    cases_ = [(form, nm, npar, nd) for form in ("gaussian", "sellentin", "hartlap", "percival")
              for nm, npar, nd in ((1000.0, 4.0, 60.0), (513.0, 10.0, 150.0), (2048.0, 3.0, 1.0))]
    out = driver(["scale", len(cases_)], [[N.LIKE[f], nm, npar, nd] for f, nm, npar, nd in cases_])
    for got, (form, nm, npar, nd) in zip(out, cases_):
        assert same_bytes(got, F.form_scale(form, nm, npar, nd)), form
        if form == "gaussian":
            assert got == 1.0
        elif form == "sellentin":
            assert got == nm / (nm - 1.0)
        elif form == "hartlap":
            assert got == (nm - nd - 2.0) / (nm - 1.0)
        else:
            B = (nm - nd - 2.0) / ((nm - nd - 1.0) * (nm - nd - 4.0))
            assert got == (npar + 2.0 + (nm - 1.0 + B * (nd - npar)) / (1.0 + B * (nd - npar))) / (nm - 1.0)
    # it is -2 dlnL/dchi2 at chi2 = 0 of the forms' lnL (the symbols of like_form), by a difference quotient
    nm, npar, nd, e = 1000.0, 4.0, 60.0, 1e-6
    lnl = {"gaussian": lambda c2: -0.5 * c2, "hartlap": lambda c2: -0.5 * c2 * ((nm - nd - 2.0) / (nm - 1.0)),
           "sellentin": lambda c2: -nm * np.log1p(c2 / (nm - 1.0)) / 2.0,
           "percival": lambda c2: -(F.form_scale("percival", nm, npar, nd) * (nm - 1.0)) * np.log1p(c2 / (nm - 1.0)) / 2.0}
    for form, f in lnl.items():
        assert abs(-2.0 * (f(e) - f(0.0)) / e - F.form_scale(form, nm, npar, nd)) <= 1e-6, form


def test_bracket_is_the_fits_own(driver):
    """vkfisher::bracket against ``CCFFit._bracket``: below, above, on every node, between nodes."""
    import victor_amd

    class Grid:
        beta_covmat = np.array([0.2, 0.25, 0.3, 0.4, 0.55])
    g = Grid.beta_covmat
    betas = np.concatenate([[0.1, 0.9, 0.2, 0.55, np.nextafter(0.3, 1.0), np.nextafter(0.3, 0.0)], g, np.linspace(0.21, 0.54, 17)])
    out = driver(["bracket", len(g), len(betas)], [g, betas]).reshape(len(betas), 2)
    for (lo, t), beta in zip(out, betas):
        want = victor_amd.CCFFit._bracket(Grid, beta)
        assert int(lo) == want[0] and same_bytes(t, float(want[1])), beta
    assert out[0].tolist() == [0.0, 0.0] and out[1].tolist() == [4.0, 0.0] and np.any(out[:, 1] != 0.0)


# ------------------------------------------------------------------ 2. an exactly representable linear model ----------------
def linear_block(d, lo=-8.0, hi=8.0, width=0.25):
    return {f"p{j}": {"prior": {"min": lo, "max": hi}, "ref": {"loc": 0.0, "scale": 0.1}, "proposal": width} for j in range(d)}


def linear_model(Mx, t0):
    names = [f"p{j}" for j in range(Mx.shape[1])]
    return lambda b: t0 + np.stack(np.broadcast_arrays(*[np.asarray(b[n], dtype=float) for n in names]), axis=1) @ Mx.T


def test_exact_linear_model():
    """t(x) = t0 + M x with small-integer M and P, dyadic points and power-of-two steps: every vector entry, every difference
    and every sum is exact, so jacobian == M and fisher == M^T P M exactly.  cov (fisher + Lambda) = diag(h) (B A) diag(1/h) with
    the power-of-two scalings exact; B is A^-1 through a Cholesky factor, two triangular stages of sums of at most d terms: the
    residual |B A - I| is at most 8 d^2 u kappa_2(A) (three stages, each d-term sums with relative error (d + 1) u at most,
    amplified by kappa, and a factor for max-entry against 2-norm), times max h / min h."""
    from victor_amd import GaussianPrior
    from victor_amd import fisher as F
    Mx = np.array([[1.0, 2, 0, -1], [0, 1, -1, 2], [3, 0, 1, 1], [1, 1, 1, 0], [2, -1, 0, 1], [0, 2, 2, -1], [1, 0, -3, 1]])
    P = np.array([[6.0, 1, 0, 0, 1, 0, 0], [2, 5, 0, 1, 0, 0, 0], [0, 0, 4, 0, 0, 1, 0], [0, 1, 0, 5, 1, 0, 0], [1, 0, 0, 1, 6, 0, 2],
                  [0, 0, 1, 0, 0, 3, 0], [0, 0, 0, 0, 1, 0, 7]])          # small integers, NOT symmetric
    t0 = np.arange(7.0)
    at = {"p0": np.array([0.5, -0.25]), "p1": np.array([0.25, 0.0]), "p2": -0.125, "p3": 1.0}
    step = {"p0": 0.25, "p1": 0.5, "p2": 0.125, "p3": np.array([0.25, 1.0])}
    kw = dict(device=False, evaluate=linear_model(Mx, t0), precision=P, keep_vectors=True)
    res = F.fisher(None, linear_block(4), at, step=step, **kw)
    assert np.all(res.status == F.OK) and res.scale == 1.0 and res.jacobian.shape == (2, 7, 4) and res.vectors.shape == (2, 9, 7)
    want = Mx.T @ P @ Mx
    sym = np.tril(want) + np.tril(want, -1).T              # the statement forms S_jk for j >= k and mirrors it
    for r in range(2):
        assert np.array_equal(res.jacobian[r], Mx) and np.array_equal(res.fisher[r], sym)
        assert np.array_equal(res.model[r], t0 + Mx @ res.x[r])
        kappa = np.linalg.cond(res.a[r])
        err = np.abs(res.cov[r] @ res.fisher[r] - np.eye(4)).max()
        bound = 8 * 16 * U * kappa * res.step[r].max() / res.step[r].min()
        print("problem", r, "kappa", kappa, "|cov fisher - I|", err, "bound", bound)
        assert err <= bound
    assert np.allclose(res.conditional_sigma, 1.0 / np.sqrt(np.diag(sym))[None]) and np.all(res.conditional_sigma <= res.sigma)
    assert res.names == ["p0", "p1", "p2", "p3"] and res.point(1) == {"p0": -0.25, "p1": 0.0, "p2": -0.125, "p3": 1.0}
    # under a prior: Lambda = diag(0, 4, 0, 0) (sigma = 1/2), exactly representable
    prior = GaussianPrior(["p1"], [0.0], sigma=[0.5])
    post = F.fisher(None, linear_block(4), at, step=step, prior=prior, **kw)
    lam = np.diag([0.0, 4.0, 0.0, 0.0])
    for r in range(2):
        assert np.array_equal(post.fisher[r], sym)                              # the likelihood's information, without the prior
        hh = np.outer(post.step[r], post.step[r])
        assert np.array_equal(post.a[r], 0.25 * (4.0 * (sym + lam) * hh))
        kappa = np.linalg.cond(post.a[r])
        err = np.abs(post.cov[r] @ (post.fisher[r] + lam) - np.eye(4)).max()
        assert err <= 8 * 16 * U * kappa * post.step[r].max() / post.step[r].min()
        assert post.conditional_sigma[r, 1] == 1.0 / np.sqrt(sym[1, 1] + 4.0)
    no_keep = F.fisher(None, linear_block(4), at, step=step, device=False, evaluate=linear_model(Mx, t0), precision=P)
    assert no_keep.jacobian is None and no_keep.vectors is None and same_bytes(no_keep.fisher, res.fisher)


# ------------------------------------------------------------------ 3. each status, the precedence, the faces ---------------
def test_each_status_their_precedence_and_the_face_policy(driver):
    from victor_amd import fisher as F
    Mx = np.array([[1.0, 2, 0], [0, 1, 0], [3, 0, 0], [1, 1, 0], [2, -1, 0]])               # the third parameter moves nothing
    P = np.diag([2.0, 3.0, 1.0, 4.0, 5.0])
    block = linear_block(3, -1.0, 1.0, 0.25)

    def model(b):
        out = linear_model(Mx, np.ones(5))(b)
        out[np.asarray(b["p1"]) == 0.5 + 0.25, 2] = np.nan         # one displaced point of the problems at p1 = 0.5 is not finite
        return out
    kw = dict(device=False, evaluate=model, precision=P, keep_vectors=True)
    dep = F.fisher(None, block, {"p0": 0.0, "p1": 0.0}, fixed={"p2": 0.0}, **kw)
    assert dep.status[0] == F.OK and np.all(np.isfinite(dep.cov[0]))
    # a zero column: S_22 = 0 exactly, NOT_POSDEF, fisher given, cov NaN
    flat = F.fisher(None, block, {"p0": 0.0, "p1": 0.0, "p2": 0.0}, **kw)
    assert flat.status[0] == F.NOT_POSDEF and not flat.ok[0]
    assert np.all(flat.fisher[0, 2] == 0.0) and np.all(np.isfinite(flat.fisher[0])) and np.all(np.isnan(flat.cov[0]))
    assert same_bytes(flat.fisher[0, :2, :2], dep.fisher[0]) and np.all(np.isnan(flat.sigma[0]))
    assert flat.conditional_sigma[0, 2] == np.inf
    # NaN beats the zero column; the face beats both
    at = {"p0": np.array([0.0, 0.0, 1.0 - 0.25 / 16]), "p1": np.array([0.5, 0.0, 0.5]), "p2": 0.0}
    res = F.fisher(None, block, at, **kw)
    assert res.status.tolist() == [F.NOT_FINITE, F.NOT_POSDEF, F.AT_BOUND]
    for r in (0, 2):
        assert all(np.all(np.isnan(a[r])) for a in (res.fisher, res.a, res.cov))
    assert np.all(res.vectors[2] == res.vectors[2, :1]) and not np.all(res.vectors[1] == res.vectors[1, :1])   # every row at x
    # the face policy through shrink: at distance h / 2 the step is shrunk, at h / 16 it is left alone and the device flags
    near = {"p0": np.array([0.5, 1.0 - 0.25 / 2, 1.0 - 0.25 / 16]), "p1": 0.0}
    res = F.fisher(None, block, near, fixed={"p2": 0.0}, **kw)
    assert res.status.tolist() == [F.OK, F.OK, F.AT_BOUND]
    assert res.step[0, 0] == 0.25 and res.step[1, 0] == 0.999 * (1.0 - near["p0"][1]) and res.step[2, 0] == 0.25
    assert np.allclose(res.fisher[1], res.fisher[0], rtol=1e-12)                         # a linear model: any step serves
    res = F.fisher(None, block, near, fixed={"p2": 0.0}, shrink=32, **kw)
    assert res.status.tolist() == [F.OK, F.OK, F.OK] and res.step[2, 0] == 0.999 * (0.25 / 16)
    res = F.fisher(None, block, near, fixed={"p2": 0.0}, shrink=1, **kw)
    assert res.status.tolist() == [F.OK, F.AT_BOUND, F.AT_BOUND]
    # the header agrees on the precedence: at the bound AND not finite AND a zero column
    lo, hi = np.full(2, -1.0), np.full(2, 1.0)
    x, h = np.array([[0.9, 0.0], [0.0, 0.0], [0.0, 0.0]]), np.full((3, 2), 0.25)
    v = np.ones((3, 5, 4))
    v[:, 1] = 2.0                                        # D_(., 0) = 1, D_(., 1) = 0
    v[0, 3, 1] = v[1, 3, 1] = np.nan
    Pm = np.broadcast_to(np.eye(4), (3, 4, 4)).copy()
    blocks = [(0, np.zeros(3), Pm, Pm)]
    got = driver_assemble(driver, v, x, h, lo, hi, blocks)
    m = F.assemble(v, x, h, lo, hi, mirror_blocks(blocks))
    compare(got, m, "precedence")
    assert m.status.tolist() == [F.AT_BOUND, F.NOT_FINITE, F.NOT_POSDEF]


# ------------------------------------------------------------------ 4. refusals before any evaluation -----------------------
def boom(*a, **k):
    raise AssertionError("the call reached the device before refusing its input")


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """A CCFFit, its Realisations, a JointFit (block-diagonal and under a covariance) and their JointRealisations, none of
    which can reach a device."""
    import victor_amd
    from victor_amd.joint import JointFit
    opts = write_stacks(tmp_path_factory.mktemp("fisher"), [cases.dsplit_options(q) for q in range(3)], 5, tag="dsplit")
    fits = [victor_amd.CCFFit(*o) for o in opts]
    for f in fits:
        f._get_engine = boom
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    fit._get_engine = boom
    joint = JointFit(fits)
    under = JointFit(fits, covariance=correlated([f.covmat for f in fits]))
    return fit, fits[0].realisations(), joint, joint.realisations(), under, under.realisations()


def test_refusals_come_before_any_device_call(four):
    from victor_amd import InputError
    from victor_amd import fisher as F
    from victor_amd.fitting import BestFit
    params = cases.cobaya_info()["params"]
    at = {"fsigma8": 0.47, "beta": 0.4, "sigma_v": 380.0, "epsilon": 1.0}
    fit, real, joint, jreal, under, ureal = four
    for target in four:
        with pytest.raises(InputError, match="at= is needed"):
            target.fisher(params, None)
        with pytest.raises(InputError, match="gives no value of beta"):
            target.fisher(params, {k: v for k, v in at.items() if k != "beta"})
        with pytest.raises(InputError, match="not sampled"):
            target.fisher(params, dict(at, sigma_w=3.0))
        with pytest.raises(InputError, match="outside its prior"):
            target.fisher(params, dict(at, sigma_v=1e4))
        with pytest.raises(InputError, match="not finite"):
            target.fisher(params, dict(at, sigma_v=np.nan))
        with pytest.raises(InputError, match="step must be finite and > 0"):
            target.fisher(params, at, step={"beta": 0.0})
        with pytest.raises(InputError, match="step must be finite and > 0"):
            target.fisher(params, at, step={"beta": np.inf})
        with pytest.raises(InputError, match="step names parameters"):
            target.fisher(params, at, step={"gamma": 0.1})
        with pytest.raises(InputError, match="shrink"):
            target.fisher(params, at, shrink=0.5)
        with pytest.raises(InputError, match="every parameter is fixed"):
            target.fisher(params, at, fixed=at)
        with pytest.raises(InputError, match="GaussianPrior or a list"):
            target.fisher(params, at, prior={"sigma_v": (380.0, 20.0)})
        with pytest.raises(InputError, match="no column"):
            target.fisher(dict(params, alpha={"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0}, "proposal": 0.01}), dict(at, alpha=1.0))
        with pytest.raises(AssertionError, match="reached the device"):          # good arguments go on to the device
            target.fisher(params, at, step={"beta": 0.01}, shrink=4, keep_vectors=True)
    for target in (fit, joint, under):
        with pytest.raises(InputError, match="different lengths"):
            target.fisher(params, dict(at, sigma_v=np.array([380.0, 390.0]), beta=np.array([0.4, 0.41, 0.42])))
    for target in (real, jreal, ureal):
        with pytest.raises(InputError, match="fixed values must be scalars"):
            target.fisher(params, {k: v for k, v in at.items() if k != "beta"}, fixed={"beta": np.full(5, 0.4)})
        with pytest.raises(InputError, match="one value per problem"):
            target.fisher(params, dict(at, beta=np.array([0.4, 0.41])))
    for target in (fit, real):
        with pytest.raises(InputError, match="need a JointFit"):
            target.fisher(dict(params, **{"sigma_v@1": params["sigma_v"]}), dict(at, **{"sigma_v@1": 380.0}))
    with pytest.raises(InputError, match="names block 3"):
        joint.fisher(dict(params, **{"sigma_v@3": params["sigma_v"]}), dict(at, **{"sigma_v@3": 380.0}), fixed={"sigma_v": 380.0})
    if laplace_refuses_likelihood_mode(fit, params, at):
        with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
            fit.fisher(params, at, beta_interpolation="likelihood")
    # a block-diagonal joint fit under a form whose scale depends on the blocks' lengths: equal lengths pass, and go on
    like = {"form": "hartlap", "nmocks": 1000}
    with pytest.raises(AssertionError, match="reached the device"):
        joint.fisher(params, at, likelihood=like)
    # at= a BestFit of other parameters, or of another number of problems
    one = np.zeros(1)
    bf = BestFit(["fsigma8", "beta"], np.array([[0.47, 0.4]]), {}, one, one, np.zeros(1, np.int32), np.ones(1, np.int32), np.ones(1, np.int64))
    with pytest.raises(InputError, match="pass the same params block and the same fixed"):
        fit.fisher(params, bf)
    with pytest.raises(InputError, match="holds 1 problems, there are 5 realisations"):
        real.fisher(params, bf, fixed={"sigma_v": 380.0, "epsilon": 1.0})
    with pytest.raises(AssertionError, match="reached the device"):
        fit.fisher(params, bf, fixed={"sigma_v": 380.0, "epsilon": 1.0})
    # the function's own
    blk, ev = linear_block(2), linear_model(np.eye(2), np.zeros(2))
    with pytest.raises(InputError, match="host route only"):
        F.fisher(None, blk, {"p0": 0.0, "p1": 0.0}, evaluate=ev, precision=np.eye(2))
    with pytest.raises(InputError, match="a fit or an evaluate callable"):
        F.fisher(None, blk, {"p0": 0.0, "p1": 0.0}, device=False)
    with pytest.raises(InputError, match="go together"):
        F.fisher(None, blk, {"p0": 0.0, "p1": 0.0}, device=False, evaluate=ev)
    with pytest.raises(InputError, match=r"\(N, N\) array"):
        F.fisher(None, blk, {"p0": 0.0, "p1": 0.0}, device=False, evaluate=ev, precision=np.ones(2))
    with pytest.raises(InputError, match="must return"):
        F.fisher(None, blk, {"p0": 0.0, "p1": 0.0}, device=False, evaluate=ev, precision=np.eye(3))
    wide = linear_block(11)
    with pytest.raises(InputError, match="at most 10"):
        F.fisher(None, wide, {n: 0.5 for n in wide}, device=False, evaluate=boom, precision=np.eye(2))
    # sample_chains takes no Fisher for a proposal
    from victor_amd.chains import sample_chains
    res = F.fisher(None, blk, {"p0": 0.0, "p1": 0.0}, device=False, evaluate=ev, precision=np.eye(2))
    with pytest.raises(InputError, match="proposal must be a dict"):
        sample_chains(None, blk, 5, proposal=res, device=False, evaluate=lambda b: (-b["p0"] ** 2, 2 * b["p0"] ** 2))


def laplace_refuses_likelihood_mode(fit, params, at):
    from victor_amd import InputError
    try:
        fit.laplace(params, at, beta_interpolation="likelihood")
    except InputError as e:
        return "beta_interpolation 'likelihood'" in str(e)
    except AssertionError:
        return False
    return False


def test_unequal_blocks_have_no_one_scale(four):
    """hartlap / percival scale a block's chi-square by a factor of its length: blocks of different lengths are refused, gaussian
    and sellentin (and a joint covariance, whose form takes p = NT) are not."""
    from victor_amd import InputError
    from victor_amd import fisher as F

    class Block:
        def __init__(self, n, form):
            self.s, self.poles_s, self.form = np.zeros(n), [0], form

        def _merged_fit(self, kwargs):
            return {"likelihood": {"form": self.form, "nmocks": 500, "nparams": 4}}

    from victor_amd.joint import JointFit
    for form, refused in (("gaussian", False), ("sellentin", False), ("hartlap", True), ("percival", True)):
        joint = JointFit.__new__(JointFit)
        joint.fits, joint.covariance = [Block(30, form), Block(40, form)], None
        if refused:
            with pytest.raises(InputError, match="no one scale"):
                F.resolve_scale(joint, {})
        else:
            assert F.resolve_scale(joint, {}) == F.form_scale(form, 500, 4, 30)
        joint.fits = [Block(30, form), Block(30, form)]
        assert F.resolve_scale(joint, {}) == F.form_scale(form, 500, 4, 30)
    under = four[4]
    assert F.resolve_scale(under, {"likelihood": {"form": "hartlap", "nmocks": 1000}}) == F.form_scale("hartlap", 1000, 0, under.n_data)


# ------------------------------------------------------------------ 5. signatures -------------------------------------------
def test_the_methods_are_on_all_four_classes():
    import victor_amd
    from victor_amd.joint import JointFit, JointRealisations
    from victor_amd.realisations import Realisations
    for cls in (victor_amd.CCFFit, Realisations, JointFit, JointRealisations):
        sig = inspect.signature(cls.fisher).parameters
        assert list(sig) == ["self", "params", "at", "step", "fixed", "prior", "shrink", "keep_vectors", "kwargs"], cls
        assert sig["step"].default is None and sig["fixed"].default is None and sig["prior"].default is None
        assert sig["shrink"].default == 8 and sig["keep_vectors"].default is False
        assert sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert victor_amd.Fisher is victor_amd.fisher.Fisher and "Fisher" in victor_amd.__all__
    sig = inspect.signature(victor_amd.fisher.fisher).parameters
    assert list(sig) == ["fit", "params", "at", "step", "fixed", "prior", "shrink", "keep_vectors", "kwargs", "realisations", "device",
                         "evaluate", "precision"]
    assert sig["device"].default is True and sig["evaluate"].default is None and sig["precision"].default is None
    assert "refine" not in sig


# ------------------------------------------------------------------ 6. the C ABI's surface ----------------------------------
def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    dp, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    decl = re.search(r"int64_t vk_fisher_rows\(([^)]*)\);", header)
    assert decl and decl.group(1).strip() == "int32_t n_params"
    assert N.SYMBOLS["vk_fisher_rows"] == (C.c_int64, [C.c_int32])
    decl = re.search(r"int vk_fit_fisher\(([^)]*)\);", header)
    assert decl, "include/victor_hip.h does not declare vk_fit_fisher"
    args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
    assert args == ["vk_fit* f", "const double* x", "const double* h", "double* vectors", "double* fisher", "double* a", "double* cov",
                    "double* scale", "int32_t* status"]
    ctype = {"vk_fit*": C.c_void_p, "const double*": dp, "double*": dp, "int32_t*": i32}
    assert N.SYMBOLS["vk_fit_fisher"] == (C.c_int, [ctype[a.rsplit(" ", 1)[0]] for a in args])
    csrc = os.path.join(ROOT, "victor_amd", "csrc")
    src = open(os.path.join(csrc, "vk_fisher.h")).read()
    assert "hip/hip_runtime.h" not in src and "hip_runtime" not in src and "#pragma clang fp contract(off)" in src
    assert '#include "vk_hessian.h"' in src
    for reused in ("chol_update", "w_entry", "b_entry", "cov_entry", "at_bound", "finite"):
        assert re.search(r"vkhess::%s\(" % reused, src), reused
    for code in ("kOk", "kAtBound", "kNotFinite", "kNotPosdef"):
        assert "vkhess::" + code in src, code
    kern = open(os.path.join(csrc, "vk_kernel_fisher.h")).read()
    assert "atomic" not in kern and "vk_fisher_rows_kernel" in kern and "vk_fisher_assemble_kernel" in kern
    assert '#include "vk_kernel_fisher.h"' in open(os.path.join(csrc, "vk_sampled.hip")).read()
    for name, value in (("gaussian", "kGaussian"), ("sellentin", "kSellentin"), ("hartlap", "kHartlap"), ("percival", "kPercival")):
        assert re.search(r"\b%s = %d\b" % (value, N.LIKE[name]), src), name


def test_library_exports_the_new_symbols():
    from victor_amd import _native as N
    lib = C.CDLL(N.library_path())
    for name in NEW:
        assert hasattr(lib, name), name
    fn = lib.vk_abi_version
    fn.restype = C.c_int
    assert fn() == 22
    rows = lib.vk_fisher_rows
    rows.restype, rows.argtypes = C.c_int64, [C.c_int32]
    assert [rows(d) for d in (1, 4, 10)] == [3, 9, 21] and rows(0) == 0 and rows(11) == 0
