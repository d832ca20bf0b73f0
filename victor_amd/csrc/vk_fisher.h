// vk_fisher.h - the Fisher matrix F = J^T P J of a theory vector at a point, J = d(theory vector)/d(theta) by central differences,
// the statistic behind vk_fit_fisher (include/victor_hip.h): the errors a model, a binning and a covariance allow, independent of
// any data vector.  Header-only and free of HIP, like vk_hessian.h, whose stencil, Cholesky and inverse routines it reuses: the
// kernels of vk_kernel_fisher.h call it, and tests/test_fisher.py compiles it on its own under g++ against the NumPy statement
// of victor_amd/fisher.py, bit for bit.
//
// A problem has d <= 10 sampled parameters, the point x, the steps h and theory vectors of N entries (of a joint fit: the blocks'
// vectors concatenated in block order).
//   Stencil    M = 2 d + 1 points, the first 2 d + 1 of the Hessian stencil (vkhess::decode, coord): 0 is x, 1 + 2 j + s is
//              x +- h_j e_j (s = 0: +); a displaced coordinate is the rounded sum or difference.  n_rows(d) = M.
//   D          D_ak = t_a(x + h_k e_k) - t_a(x - h_k e_k)                                                          (d_entry)
//              The division by 2 h is never performed on the vector: it is folded into the d x d scaling below.
//   P          the precision at the CENTRE's beta: of a fixed covariance its one slice; of a beta-gridded one, with the bracket
//              (lo, t) of cov_bracket (vk_kernel_like.h: lower slice lo, weight t, upper slice the LAST one; bracket() here),
//              P_ab = P_lo,ab when t == 0, else ((1 - t) P_lo,ab) + (t P_last,ab): 1 - t rounded, each product rounded, then the
//              sum (p_entry).  P is read as stored, P_ab = slice[a * ld + b]: nothing assumes it symmetric.
//              P is block-diagonal over one or more blocks (Block): one block of N entries for a single fit and for a joint fit
//              under one covariance; the blocks of a block-diagonal joint fit, each with its own bracket.
//   G          G_ak = sum_b P_ab D_bk, b ascending through the block a belongs to                                  (g_entry)
//   S          S_jk = sum_a D_aj G_ak, a ascending through the whole vector, for j >= k, mirrored                  (s_entry)
//              Every sum starts from its first term; each product is rounded, then added.
//   c          -2 dlnL/dchi2 at chi2 = 0 of the likelihood form (form_scale; the symbols of like_form, vk_kernel_like.h):
//              gaussian 1, hartlap (nm - nd - 2) / (nm - 1), sellentin nm / (nm - 1), percival m / (nm - 1).  Exact for a
//              forecast: with data = model at x the residual term of the curvature vanishes.  One number per problem set: a
//              block-diagonal joint fit whose blocks would have different c (hartlap / percival with blocks of different
//              length) is refused by the entry point.
//   fisher     q = 0.25 c;  fisher_jk = (q S_jk) / (h_j h_k)                                                       (fisher_entry)
//   A          A_jk = q S_jk, plus Lambda_jk (h_j h_k) under a Gaussian prior (each product rounded; a_entry), Lambda the prior's
//              precision matrix (lambda_entry: vk_prior.h stores its off-diagonal entries doubled; halving is exact)
//   cov        Cholesky of A, W = L^-1, B = W^T W by the routines of vk_hessian.h;  cov_jk = (h_j h_k) B_jk
// Status, in this precedence (the codes of vk_hessian.h):
//   kAtBound    the stencil leaves the box or x is outside it (vkhess::at_bound): every row of the problem is formed at x
//   kNotFinite  some entry of the M vectors is not finite
//   kNotPosdef  a Cholesky pivot fails > 0: fisher and A are given, cov is NaN.  A parameter the theory does not depend on has
//               D_aj = 0 for every a, so S_jj = 0 exactly, and reads this.
//   kOk         otherwise
// On kAtBound and kNotFinite fisher, A and cov are NaN (vkhess::nan()).
//
// Bits: products feed sums here - what a compiler contracts into fused multiply-adds.  The routines forbid it (hipcc: the pragma;
// the CPU tests build with -ffp-contract=off); sqrt and / are IEEE's.  So hipcc, g++ and NumPy produce the same bits from the
// same vectors.
//
// assemble() is the whole statistic of one problem in plain serial C++ (the CPU test's subject); vk_fisher_assemble_kernel
// spreads the same per-entry routines over a workgroup, with D and G in LDS.
#pragma once
#include <cstddef>

#include "vk_hessian.h"
#include "vk_prior.h"

namespace vkfisher {

constexpr int kMaxP = vkhess::kMaxP;
constexpr int kMaxRows = 2 * kMaxP + 1;      // 21
constexpr int kGaussian = 0, kSellentin = 1, kHartlap = 2, kPercival = 3;      // VK_LIKE_* of include/victor_hip.h

VK_HESS_HD constexpr int n_rows(int d) { return 2 * d + 1; }

// one diagonal block of the precision: entries off .. off + n - 1 of the vector; row a of the slices at lo + a * ld, last + a * ld
struct Block {
  const double *lo, *last;   // slice `lo` of the bracket and the LAST slice (not read when t == 0)
  double t;                  // the bracket's weight
  int n, ld, off;
};

// -2 dlnL/dchi2 at chi2 = 0; nd: entries of the vector the form is applied to
inline double form_scale(int form, double nm, double np, double nd) {
  if (form == kSellentin) return nm / (nm - 1.0);
  if (form == kHartlap) return (nm - nd - 2.0) / (nm - 1.0);
  if (form == kPercival) {
    const double B = (nm - nd - 2.0) / ((nm - nd - 1.0) * (nm - nd - 4.0));
    const double m = np + 2.0 + (nm - 1.0 + B * (nd - np)) / (1.0 + B * (nd - np));
    return m / (nm - 1.0);
  }
  return 1.0;
}

// The bracket of beta in the covariance grid g [n], the rule of cov_bracket (vk_kernel_like.h, whose kernels this header cannot
// bring along) and of CCFFit._bracket: below / above the grid the first / last slice, on a grid value that slice, else slice lo
// = the last grid value below beta, blended with the LAST slice with weight t = (beta - g_lo) / (g_last - g_lo).
VK_HESS_HD inline void bracket(const double* g, int n, double beta, int* lo_out, double* t_out) {
  int lo = 0;
  double t = 0.0;
  const int last = n - 1;
  if (beta < g[0]) {
    lo = 0;
  } else if (beta > g[last]) {
    lo = last;
  } else {
    int exact = -1, below = 0;
    for (int i = 0; i <= last; ++i) {
      if (g[i] == beta && exact < 0) exact = i;
      if (g[i] < beta) below = i;
    }
    if (exact >= 0) {
      lo = exact;
    } else {
      lo = below;
      t = (beta - g[lo]) / (g[last] - g[lo]);
    }
  }
  *lo_out = lo;
  *t_out = t;
}

VK_HESS_HD inline double d_entry(double t_plus, double t_minus) { return t_plus - t_minus; }

VK_HESS_HD inline double p_entry(double p_lo, double p_last, double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (t == 0.0) return p_lo;
  const double u = (1.0 - t) * p_lo;
  const double v = t * p_last;
  return u + v;
}

// G_ak of a block: row_lo, row_last are row a of its slices (n entries), dcol the block's first D_bk, consecutive b ldd apart
VK_HESS_HD inline double g_entry(const double* row_lo, const double* row_last, double t, int n, const double* dcol, int ldd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double s = p_entry(row_lo[0], t == 0.0 ? 0.0 : row_last[0], t) * dcol[0];
  for (int b = 1; b < n; ++b) {
    const double u = p_entry(row_lo[b], t == 0.0 ? 0.0 : row_last[b], t) * dcol[(size_t)b * ldd];
    s = s + u;
  }
  return s;
}

// S_jk from D and G, both [N][ldd]
VK_HESS_HD inline double s_entry(const double* D, const double* G, int ldd, int N, int j, int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double s = D[j] * G[k];
  for (int a = 1; a < N; ++a) {
    const double u = D[(size_t)a * ldd + j] * G[(size_t)a * ldd + k];
    s = s + u;
  }
  return s;
}

// Lambda_jk, j >= k, of the prior (0 without one)
VK_HESS_HD inline double lambda_entry(const vkprior::Prior& p, int d, int j, int k) {
  if (!p.on) return 0.0;
  const double v = p.pp[vkprior::tri(d, k, j)];
  return j == k ? v : 0.5 * v;
}

VK_HESS_HD inline double fisher_entry(double c, double s_jk, double hj, double hk) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double q = 0.25 * c;
  const double u = q * s_jk;
  return u / (hj * hk);
}

// A_jk; with_prior false: the prior term is absent (not a zero added)
VK_HESS_HD inline double a_entry(double c, double s_jk, bool with_prior, double lambda_jk, double hj, double hk) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double q = 0.25 * c;
  const double u = q * s_jk;
  if (!with_prior) return u;
  const double hh = hj * hk;
  const double v = lambda_jk * hh;
  return u + v;
}

// The statistic of one problem, serially: the vectors v [M][N], x, h, the box lo, hi (each [d]), the precision's blocks, the
// scale c and the prior.  Out: D, G [N][d], S, fisher, A, cov (each [d][d], symmetric), the factor L and its inverse W (lower
// triangles; meaningful when the status is kOk), and the status, returned.  T is d * d doubles of working space.
inline int assemble(int d, int N, const double* v, const double* x, const double* h, const double* lo, const double* hi,
                    const Block* blocks, int n_blocks, double c, const vkprior::Prior& prior, double* D, double* G, double* S,
                    double* fisher, double* A, double* cov, double* L, double* W, double* T) {
  const int M = n_rows(d);
  for (int i = 0; i < d * d; ++i) S[i] = fisher[i] = A[i] = cov[i] = vkhess::nan(), L[i] = W[i] = T[i] = 0.0;
  for (int i = 0; i < N * d; ++i) D[i] = G[i] = vkhess::nan();
  if (vkhess::at_bound(d, [&](int j) { return x[j]; }, [&](int j) { return h[j]; }, [&](int j) { return lo[j]; },
                       [&](int j) { return hi[j]; }))
    return vkhess::kAtBound;
  for (int i = 0; i < M * N; ++i)
    if (!vkhess::finite(v[i])) return vkhess::kNotFinite;
  for (int a = 0; a < N; ++a)
    for (int k = 0; k < d; ++k)
      D[a * d + k] = d_entry(v[(size_t)vkhess::at_axis(k, 0) * N + a], v[(size_t)vkhess::at_axis(k, 1) * N + a]);
  for (int q = 0; q < n_blocks; ++q) {
    const Block& b = blocks[q];
    for (int a = 0; a < b.n; ++a)
      for (int k = 0; k < d; ++k)
        G[(b.off + a) * d + k] = g_entry(b.lo + (size_t)a * b.ld, b.last + (size_t)a * b.ld, b.t, b.n, D + (size_t)b.off * d + k, d);
  }
  for (int j = 0; j < d; ++j)
    for (int k = 0; k <= j; ++k) {
      const double s = s_entry(D, G, d, N, j, k);
      S[j * d + k] = S[k * d + j] = s;
      fisher[j * d + k] = fisher[k * d + j] = fisher_entry(c, s, h[j], h[k]);
      A[j * d + k] = A[k * d + j] = T[j * d + k] = a_entry(c, s, prior.on != 0, lambda_entry(prior, d, j, k), h[j], h[k]);
    }
  for (int cc = 0; cc < d; ++cc) {
    if (!(T[cc * d + cc] > 0.0)) return vkhess::kNotPosdef;
    const double lcc = __builtin_sqrt(T[cc * d + cc]);
    L[cc * d + cc] = lcc;
    for (int j = cc + 1; j < d; ++j) L[j * d + cc] = T[j * d + cc] / lcc;
    for (int j = cc + 1; j < d; ++j)
      for (int k = cc + 1; k <= j; ++k) T[j * d + k] = vkhess::chol_update(T[j * d + k], L[j * d + cc], L[k * d + cc]);
  }
  for (int cc = 0; cc < d; ++cc)
    for (int j = cc; j < d; ++j) W[j * d + cc] = vkhess::w_entry(L, W, d, j, cc);
  for (int j = 0; j < d; ++j)
    for (int k = 0; k <= j; ++k) cov[j * d + k] = cov[k * d + j] = vkhess::cov_entry(vkhess::b_entry(W, d, d, j, k), h[j], h[k]);
  return vkhess::kOk;
}

}  // namespace vkfisher
