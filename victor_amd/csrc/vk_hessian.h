// vk_hessian.h - the central-difference Hessian of lnL + ln prior at a point and its inverse, the statistic behind vk_fit_hessian
// (include/victor_hip.h): the local Gaussian (Laplace) approximation of a posterior around its best fit.  Header-only and free of
// HIP, like vk_prior.h and vk_autocorr.h: the kernels of vk_kernel_hessian.h call it, and tests/test_hessian.py compiles it on its
// own under g++ against the NumPy statement of victor_amd/laplace.py, bit for bit.
//
// The stencil of one problem at x with steps h, d <= 10 sampled parameters, has M = 2 d^2 + 1 points:
//   m = 0                     x
//   m = 1 + 2 j + s           x +- h_j e_j             (s = 0: +, s = 1: -)
//   m = 1 + 2 d + 4 q + c     x_j and x_k displaced    (q: the pair j < k in the order (0,1), (0,2), .., (0,d-1), (1,2), ..;
//                                                       c = 0, 1, 2, 3: the signs (+,+), (+,-), (-,+), (-,-))
// A displaced coordinate is the rounded sum x_j + h_j or the rounded difference x_j - h_j (decode, coord).
//
// From the values v of the points, the scaled negative Hessian A = -H o (h h^T) - no division:
//   A_jj = ((v0 + v0) - v(+j)) - v(-j)                                       (a_diag)
//   A_jk = 0.25 * ((v(+-) - v(++)) + (v(-+) - v(--))),  mirrored              (a_off)
// Status, in this precedence:
//   kAtBound (1)    some x_j - h_j < lo_j or x_j + h_j > hi_j, or x itself outside the box (at_bound): the stencil is not
//                   formed, every row of the problem is evaluated at x
//   kNotFinite (2)  some value of the M is not finite
//   kNotPosdef (3)  a Cholesky pivot fails > 0
//   kOk (0)         otherwise
// Cholesky A = L L^T, right-looking, on a working copy S of A's lower triangle: for c = 0 .. d - 1
//   L_cc = sqrt(S_cc);  L_jc = S_jc / L_cc for j > c;  S_jk = S_jk - L_jc * L_kc for c < k <= j (the product rounded, then the
//   difference: chol_update).
// Inverse: W = L^-1 by forward substitution, W_cc = 1 / L_cc, W_jc = -(sum_{m = c}^{j - 1} L_jm W_mc) / L_jj (w_entry); then
//   B = W^T W, B_jk = sum_{m = max(j, k)}^{d - 1} W_mj W_mk (b_entry).  Every sum starts from its first term and runs in ascending m.
// Outputs: hess_jk = -A_jk / (h_j * h_k), cov_jk = (h_j * h_k) * B_jk.  On kAtBound or kNotFinite A, hess and cov are NaN (the
//   quiet NaN of nan()); on kNotPosdef A and hess are given and cov is NaN.
// The definition is per entry and independent of layout: matrices here are row-major with a leading dimension `ld`.
//
// Bits: products feed sums and differences here - what a compiler contracts into fused multiply-adds.  The routines forbid it
// (hipcc: the pragma below; the CPU tests build with -ffp-contract=off); sqrt and / are IEEE's, correctly rounded.  So hipcc,
// g++ and NumPy produce the same bits from the same values.
//
// assemble() is the whole statistic of one problem in plain serial C++ (the CPU test's subject and the statement the kernel is
// held to); vk_hess_assemble_kernel spreads the same per-entry routines over the lanes of a wave, with its matrices in LDS.
#pragma once

#if defined(__HIPCC__)
#define VK_HESS_HD __host__ __device__
#else
#define VK_HESS_HD
#endif

namespace vkhess {

constexpr int kMaxP = 10;                          // sampled parameters, as vkfit::kMaxP
constexpr int kMaxPoints = 2 * kMaxP * kMaxP + 1;  // 201
constexpr int kMaxTri = kMaxP * (kMaxP + 1) / 2;   // 55: the packed triangle fits the 64 lanes of a wave
constexpr int kOk = 0, kAtBound = 1, kNotFinite = 2, kNotPosdef = 3;

VK_HESS_HD constexpr int n_points(int d) { return 2 * d * d + 1; }
// number of the pair (j, k), j < k
VK_HESS_HD constexpr int pair(int d, int j, int k) { return j * d - j * (j + 1) / 2 + (k - j - 1); }
VK_HESS_HD constexpr int at_axis(int j, int s) { return 1 + 2 * j + s; }
VK_HESS_HD constexpr int at_pair(int d, int j, int k, int c) { return 1 + 2 * d + 4 * pair(d, j, k) + c; }

// what point m displaces: coordinate j by sj h_j and coordinate k by sk h_k (sj, sk = +1 / -1); j < 0: nothing (the centre),
// k < 0: one coordinate only
struct Point {
  int j, k, sj, sk;
};

VK_HESS_HD inline Point decode(int d, int m) {
  Point p{-1, -1, 0, 0};
  if (m <= 0) return p;
  if (m < 1 + 2 * d) {
    p.j = (m - 1) / 2;
    p.sj = (m - 1) % 2 ? -1 : 1;
    return p;
  }
  const int t = m - 1 - 2 * d, c = t % 4;
  int rem = t / 4, j = 0;
  while (rem >= d - 1 - j) {
    rem -= d - 1 - j;
    ++j;
  }
  p.j = j;
  p.k = j + 1 + rem;
  p.sj = c / 2 ? -1 : 1;
  p.sk = c % 2 ? -1 : 1;
  return p;
}

// coordinate i of the point: x, or the rounded x + h / x - h
VK_HESS_HD inline double coord(const Point& p, int i, double x, double h) {
  const int s = i == p.j ? p.sj : i == p.k ? p.sk : 0;
  return s > 0 ? x + h : s < 0 ? x - h : x;
}

// does the stencil leave the box?  x(j), h(j), lo(j), hi(j): getters
template <class X, class H, class Lo, class Hi>
VK_HESS_HD inline bool at_bound(int d, X x, H h, Lo lo, Hi hi) {
  bool out = false;
  for (int j = 0; j < d; ++j) {
    const double xj = x(j), hj = h(j);
    if (!(xj >= lo(j)) || !(xj <= hi(j)) || xj - hj < lo(j) || xj + hj > hi(j)) out = true;
  }
  return out;
}

VK_HESS_HD inline bool finite(double v) { return v - v == 0.0; }
VK_HESS_HD inline double nan() { return __builtin_nan(""); }

VK_HESS_HD inline double a_diag(double v0, double vp, double vm) { return ((v0 + v0) - vp) - vm; }
VK_HESS_HD inline double a_off(double vpp, double vpm, double vmp, double vmm) { return 0.25 * ((vpm - vpp) + (vmp - vmm)); }

// entry (j, k), j >= k, of A from the values v(m)
template <class V>
VK_HESS_HD inline double a_entry(int d, int j, int k, V v) {
  if (j == k) return a_diag(v(0), v(at_axis(j, 0)), v(at_axis(j, 1)));
  return a_off(v(at_pair(d, k, j, 0)), v(at_pair(d, k, j, 1)), v(at_pair(d, k, j, 2)), v(at_pair(d, k, j, 3)));
}

// the trailing update of column c: S_jk - L_jc * L_kc, the product rounded first
VK_HESS_HD inline double chol_update(double s_jk, double l_jc, double l_kc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double t = l_jc * l_kc;
  return s_jk - t;
}

// W_jc, j >= c, from L and the entries W_cc .. W_(j-1)c of the column above it
VK_HESS_HD inline double w_entry(const double* L, const double* W, int ld, int j, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (j == c) return 1.0 / L[c * ld + c];
  double s = L[j * ld + c] * W[c * ld + c];
  for (int m = c + 1; m < j; ++m) {
    const double t = L[j * ld + m] * W[m * ld + c];
    s = s + t;
  }
  return -s / L[j * ld + j];
}

// B_jk = sum_{m = max(j, k)}^{d - 1} W_mj W_mk
VK_HESS_HD inline double b_entry(const double* W, int ld, int d, int j, int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int m0 = j > k ? j : k;
  double s = W[m0 * ld + j] * W[m0 * ld + k];
  for (int m = m0 + 1; m < d; ++m) {
    const double t = W[m * ld + j] * W[m * ld + k];
    s = s + t;
  }
  return s;
}

VK_HESS_HD inline double hess_entry(double a_jk, double hj, double hk) { return -a_jk / (hj * hk); }
VK_HESS_HD inline double cov_entry(double b_jk, double hj, double hk) { return (hj * hk) * b_jk; }

// The statistic of one problem, serially: values v [M], the point x, steps h, the box lo, hi (each [d]).  Out: A, hess, cov
// (each [d][d], ld == d), the factor L and its inverse W (lower triangles; the rest zero; meaningful when the status is kOk), and
// the status, returned.  S is d * d doubles of working space.
VK_HESS_HD inline int assemble(int d, const double* v, const double* x, const double* h, const double* lo, const double* hi,
                               double* A, double* hess, double* cov, double* L, double* W, double* S) {
  const int M = n_points(d);
  for (int i = 0; i < d * d; ++i) A[i] = hess[i] = cov[i] = nan(), L[i] = W[i] = S[i] = 0.0;
  if (at_bound(d, [&](int j) { return x[j]; }, [&](int j) { return h[j]; }, [&](int j) { return lo[j]; },
               [&](int j) { return hi[j]; }))
    return kAtBound;
  for (int m = 0; m < M; ++m)
    if (!finite(v[m])) return kNotFinite;
  for (int j = 0; j < d; ++j)
    for (int k = 0; k <= j; ++k) {
      const double a = a_entry(d, j, k, [&](int m) { return v[m]; });
      A[j * d + k] = A[k * d + j] = S[j * d + k] = a;
      hess[j * d + k] = hess[k * d + j] = hess_entry(a, h[j], h[k]);
    }
  for (int c = 0; c < d; ++c) {
    if (!(S[c * d + c] > 0.0)) return kNotPosdef;
    const double lcc = __builtin_sqrt(S[c * d + c]);
    L[c * d + c] = lcc;
    for (int j = c + 1; j < d; ++j) L[j * d + c] = S[j * d + c] / lcc;
    for (int j = c + 1; j < d; ++j)
      for (int k = c + 1; k <= j; ++k) S[j * d + k] = chol_update(S[j * d + k], L[j * d + c], L[k * d + c]);
  }
  for (int c = 0; c < d; ++c)
    for (int j = c; j < d; ++j) W[j * d + c] = w_entry(L, W, d, j, c);
  for (int j = 0; j < d; ++j)
    for (int k = 0; k <= j; ++k) cov[j * d + k] = cov[k * d + j] = cov_entry(b_entry(W, d, d, j, k), h[j], h[k]);
  return kOk;
}

}  // namespace vkhess
