// vk_kernel_hessian.h: the Hessian stencil of vk_fit_hessian (include/victor_hip.h) on the device - part of libvictor_hip.so
// (see vk_sampled.hip for the host side, vk_hessian.h for the statistic, DESIGN.md section 7a for the measurements).
//
// vk_hess_rows_kernel forms the parameter rows of a chunk of the R M stencil rows, one thread per row: global row g belongs to
// problem p = g / M and is its stencil point m = g % M (vkhess::decode, coord), written through sampled_row like every other
// sampled row - epsilon becomes the Alcock-Paczynski factors, a joint fit's row sets and param_block apply.  A problem whose
// stencil leaves the box (vkhess::at_bound) has all its rows formed at x: the launch shape never depends on the data, the rule
// the chains follow for a proposal outside the box.
//
// vk_hess_assemble_kernel turns the R M values into A, the Hessian, the covariance and the status: one wave-sized workgroup per
// problem (the idiom of vk_chain_series_kernel).  The values - lnL, plus ln prior at the point as the rows kernel formed it when
// the handle has a prior - are staged in LDS; lane t < d (d + 1) / 2 owns entry (j >= k) of the packed triangle and computes its
// A, its Cholesky updates, its B and its outputs with the routines of vk_hessian.h, so every entry sees the arithmetic of
// vkhess::assemble; the matrices S, L, W live in three 10 x 10 LDS tiles that the lanes read each other's entries from, with a
// workgroup barrier between dependent phases (one wave: the barrier is a wait).  The columns of W = L^-1 are independent and
// run one per lane.  Plain loads and vector stores, no atomics, no local arrays: nothing indexes a register file at run time.
#pragma once
#include "vk_common.h"
#include "vk_hessian.h"
#include "vk_prior.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kHessBlock = 64;
static_assert(vkhess::kMaxTri <= kHessBlock, "one lane per entry of the packed triangle");
static_assert(vkhess::kMaxP == vkrow::kMaxP && vkhess::kMaxP == vkprior::kMaxP, "the stencil covers the sampled parameters");

struct HessArgs {
  int d, M;                 // sampled parameters, stencil points of a problem (2 d^2 + 1)
  int R;                    // problems
  double lo[vkhess::kMaxP], hi[vkhess::kMaxP];
  const double* x;          // [R][d]: the points
  const double* h;          // [R][d]: the steps
  // rows kernel
  long long g0, n;          // the chunk: global rows g0 .. g0 + n - 1 land in pending rows 0 .. n - 1
  const double* base;       // [R][VK_NPAR] per row set
  double* rows;             // [rows_max][VK_NPAR] per row set
  int* row_which;           // [rows_max], or NULL (the fit's own data vector)
  const int* which;         // [R], or NULL
  int col[vkhess::kMaxP];
  double alpha;
  vkrow::Blocks blocks;
  // assemble kernel
  vkprior::Prior prior;
  double* values;           // [R][M]: in lnL of every stencil row, out the values the statistic used (lnL + ln prior)
  const double* chis;       // [R][M]: chi-square of every stencil row
  double *a, *hess, *cov;   // [R][d][d]
  double *lnpost, *chi2;    // [R]: the centre
  int* status;              // [R]
};

// does problem p's stencil leave the box?
__device__ __forceinline__ bool hess_at_bound(const HessArgs& a, size_t p) {
  const double *x = a.x + p * a.d, *h = a.h + p * a.d;
  return vkhess::at_bound(a.d, [&](int j) { return x[j]; }, [&](int j) { return h[j]; }, [&](int j) { return a.lo[j]; },
                          [&](int j) { return a.hi[j]; });
}

__global__ void __launch_bounds__(kHessBlock) vk_hess_rows_kernel(HessArgs a) {
  const long long i = (long long)blockIdx.x * kHessBlock + threadIdx.x;
  if (i >= a.n) return;
  const long long g = a.g0 + i;
  const size_t p = (size_t)(g / a.M);
  const int m = (int)(g - (long long)p * a.M);
  const vkhess::Point pt = hess_at_bound(a, p) ? vkhess::decode(a.d, 0) : vkhess::decode(a.d, m);
  const double *x = a.x + p * a.d, *h = a.h + p * a.d;
  sampled_row(a.blocks, a.base, p, a.rows, (size_t)i, a.col, a.d, a.alpha, [&](int j) { return vkhess::coord(pt, j, x[j], h[j]); });
  if (a.row_which) a.row_which[i] = a.which[p];
}

__global__ void __launch_bounds__(kHessBlock) vk_hess_assemble_kernel(HessArgs a) {
  constexpr int ld = vkhess::kMaxP;
  __shared__ double val[vkhess::kMaxPoints];
  __shared__ double S[ld * ld], L[ld * ld], W[ld * ld];
  const size_t p = blockIdx.x;
  const int lane = threadIdx.x, d = a.d, M = a.M;
  const double *x = a.x + p * d, *h = a.h + p * d;
  const bool bound = hess_at_bound(a, p);
  // the values: lnL of the row, plus ln prior at the point the rows kernel formed
  bool bad = false;
  for (int m = lane; m < M; m += kHessBlock) {
    double v = a.values[p * M + m];
    if (a.prior.on) {
      const vkhess::Point pt = bound ? vkhess::decode(d, 0) : vkhess::decode(d, m);
      v = v + vkprior::lnprior(a.prior, d, [&](int j) { return vkhess::coord(pt, j, x[j], h[j]); });
      a.values[p * M + m] = v;
    }
    val[m] = v;
    bad = bad || !vkhess::finite(v);
  }
  const bool not_finite = __syncthreads_or(bad) != 0;      // (the barrier behind the staging, too)
  // lane -> entry (j >= k) of the packed lower triangle, row by row
  int j = 0;
  while ((j + 1) * (j + 2) / 2 <= lane) ++j;
  const int k = lane - j * (j + 1) / 2;
  const bool mine = j < d;
  int status = bound ? vkhess::kAtBound : not_finite ? vkhess::kNotFinite : vkhess::kOk;
  const double hh_j = mine ? h[j] : 1.0, hh_k = mine ? h[k] : 1.0;
  double av = vkhess::nan(), hv = vkhess::nan(), cv = vkhess::nan();
  if (status == vkhess::kOk) {                     // (uniform over the workgroup: every barrier below is reached by all lanes)
    if (mine) {
      av = vkhess::a_entry(d, j, k, [&](int m) { return val[m]; });
      hv = vkhess::hess_entry(av, hh_j, hh_k);
      S[j * ld + k] = av;
    }
    __syncthreads();
    for (int c = 0; c < d; ++c) {
      const double scc = S[c * ld + c];
      if (!(scc > 0.0)) {                          // (every lane reads the same pivot)
        status = vkhess::kNotPosdef;
        break;
      }
      const double lcc = __builtin_sqrt(scc);
      if (mine && k == c) L[j * ld + c] = j == c ? lcc : S[j * ld + c] / lcc;
      __syncthreads();
      if (mine && k > c) S[j * ld + k] = vkhess::chol_update(S[j * ld + k], L[j * ld + c], L[k * ld + c]);
      __syncthreads();
    }
    if (status == vkhess::kOk) {
      if (lane < d)                                // column `lane` of W = L^-1, top to bottom
        for (int r = lane; r < d; ++r) W[r * ld + lane] = vkhess::w_entry(L, W, ld, r, lane);
      __syncthreads();
      if (mine) cv = vkhess::cov_entry(vkhess::b_entry(W, ld, d, j, k), hh_j, hh_k);
    }
  }
  if (mine) {
    const size_t at = p * d * d;
    a.a[at + j * d + k] = a.a[at + k * d + j] = av;
    a.hess[at + j * d + k] = a.hess[at + k * d + j] = hv;
    a.cov[at + j * d + k] = a.cov[at + k * d + j] = cv;
  }
  if (lane == 0) {
    a.lnpost[p] = val[0];
    a.chi2[p] = a.chis[p * M];
    a.status[p] = status;
  }
}

}  // namespace vk
