// vk_kernel_fisher.h: the Jacobian stencil and the Fisher matrix of vk_fit_fisher (include/victor_hip.h) on the device - part of
// libvictor_hip.so (see vk_sampled.hip for the host side, vk_fisher.h for the statistic, DESIGN.md section 7a for the
// measurements).
//
// vk_fisher_rows_kernel forms the parameter rows of a chunk of the R M stencil rows, M = 2 d + 1, one thread per row, exactly as
// vk_hess_rows_kernel does for the first 2 d + 1 points of its stencil: global row g is point g % M of problem g / M, written
// through sampled_row; a problem whose stencil leaves the box has all its rows formed at x.
//
// vk_fisher_assemble_kernel turns the R M theory vectors into fisher, A, cov and the status: one workgroup of kFisherBlock
// threads per problem.  The vectors arrive in segments - one for a single fit, one per block of a joint fit, each the workspace
// [R M][N_q] of that block's theory launches - and the precision in the same segments: FisherSeg says which rows and columns of
// which slices a segment's entries meet (the whole padded joint matrix under one covariance, the block's own matrix otherwise).
//   1. thread (a, k) of N d, in a loop, stages D_ak in LDS and tests its two vectors' entries (and, for k = 0, the centre's) for
//      finiteness; thread q < n_seg brackets segment q's covariance at the centre's beta (vkfisher::bracket).
//   2. thread (a, k) forms G_ak, its sum over b run serially (vkfisher::g_entry): the d threads of an `a` read the same address of
//      P (one request), the 64 / d rows of a wave distinct lines that serve 16 consecutive b each; D_bk comes from LDS, the same
//      word for every a of a wave and consecutive words over k - no bank conflict.  P is read R times, from L2 after the first.
//   3. thread t < d (d + 1) / 2 owns entry (j >= k): S_jk by vkfisher::s_entry over LDS, fisher and A, then the d Cholesky steps,
//      W = L^-1 and B through three 10 x 10 LDS tiles with a barrier between dependent phases, as vk_hess_assemble_kernel - so
//      every entry sees the arithmetic of vkfisher::assemble.
// LDS: 2 N d doubles (D, G) and the tiles, dynamic, beside 640 static bytes (the brackets, the workgroup vote):
// fisher_lds_doubles(N, d) <= kFisherLdsDoubles keeps the workgroup within the 160 KiB of a gfx950 CU (above 64 KiB by the
// per-kernel opt-in every large-LDS kernel of the library takes), i.e. N d <= 10026 - N <= 1002 at d = 10; vk_fit_fisher
// refuses more.  The five density-split blocks at d = 10 (N = 600) hold 96 KiB: one workgroup per CU, 4 waves.
// Plain loads and vector stores, nothing read-modify-write across threads, no local arrays.
#pragma once
#include "vk_common.h"
#include "vk_fisher.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kFisherBlock = 256;
constexpr int kFisherMaxSeg = 32;                 // the blocks of a joint fit (sampled_create)
constexpr int kFisherRowsBlock = 64;
constexpr int kFisherLdsDoubles = 20480 - 128;    // 160 KiB less 1 KiB for the kernel's static LDS (640 bytes)
static_assert(vkhess::kMaxTri <= kFisherBlock && kFisherMaxSeg <= kFisherBlock, "one thread per entry of the triangle, per segment");

__host__ __device__ constexpr size_t fisher_lds_doubles(int N, int d) { return 2 * (size_t)N * d + 3 * vkhess::kMaxP * vkhess::kMaxP; }

struct FisherSeg {
  const double* theory;     // [R M][N]: this segment's vectors of every stencil row
  const double* prec;       // the precision slices its entries meet: [max(n_beta_c, 1)] matrices `slice` doubles apart, rows of ld
  const double* beta_c;     // [n_beta_c], or NULL
  long long slice;
  int n_beta_c;             // 0: one fixed covariance
  int N, off;               // entries, offset in the concatenated vector
  int ld, prow0;            // entry e's row of P is prow0 + e
  int poff, pn;             // ... and meets the entries poff .. poff + pn - 1 of the vector, columns 0 .. pn - 1 of that row
  int set;                  // the row set whose beta brackets the covariance
};

struct FisherArgs {
  int d, M;                 // sampled parameters, stencil points of a problem (2 d + 1)
  int R, N, n_seg;          // problems, entries of the concatenated vector, segments
  double lo[vkhess::kMaxP], hi[vkhess::kMaxP];
  const double* x;          // [R][d]: the points
  const double* h;          // [R][d]: the steps
  // rows kernel
  long long g0, n;          // the chunk: global rows g0 .. g0 + n - 1 land in pending rows 0 .. n - 1
  const double* base;       // [R][VK_NPAR] per row set
  double* rows;             // [rows_max][VK_NPAR] per row set
  int* row_which;           // [rows_max], or NULL: the rows' realisations, for a context whose xi^r tables are selected per row
  const int* which;         // [R], or NULL     (vk_set_model_realisations) - the forecast itself reads no data
  int col[vkhess::kMaxP];
  double alpha;
  vkrow::Blocks blocks;
  // assemble kernel
  vkprior::Prior prior;
  double c;                 // vkfisher::form_scale
  FisherSeg seg[kFisherMaxSeg];
  double *fisher, *a, *cov; // [R][d][d]
  int* status;              // [R]
};

static_assert(sizeof(FisherArgs) <= 4096, "kernel arguments");

__device__ __forceinline__ bool fisher_at_bound(const FisherArgs& a, size_t p) {
  const double *x = a.x + p * a.d, *h = a.h + p * a.d;
  return vkhess::at_bound(a.d, [&](int j) { return x[j]; }, [&](int j) { return h[j]; }, [&](int j) { return a.lo[j]; },
                          [&](int j) { return a.hi[j]; });
}

__global__ void __launch_bounds__(kFisherRowsBlock) vk_fisher_rows_kernel(FisherArgs a) {
  const long long i = (long long)blockIdx.x * kFisherRowsBlock + threadIdx.x;
  if (i >= a.n) return;
  const long long g = a.g0 + i;
  const size_t p = (size_t)(g / a.M);
  const int m = (int)(g - (long long)p * a.M);
  const vkhess::Point pt = fisher_at_bound(a, p) ? vkhess::decode(a.d, 0) : vkhess::decode(a.d, m);
  const double *x = a.x + p * a.d, *h = a.h + p * a.d;
  sampled_row(a.blocks, a.base, p, a.rows, (size_t)i, a.col, a.d, a.alpha, [&](int j) { return vkhess::coord(pt, j, x[j], h[j]); });
  if (a.row_which) a.row_which[i] = a.which[p];
}

__global__ void __launch_bounds__(kFisherBlock) vk_fisher_assemble_kernel(FisherArgs a) {
  constexpr int ld = vkhess::kMaxP;
  extern __shared__ double fisher_lds[];
  __shared__ double seg_t[kFisherMaxSeg];
  __shared__ int seg_lo[kFisherMaxSeg];
  const size_t p = blockIdx.x;
  const int tid = threadIdx.x, d = a.d, M = a.M, N = a.N;
  double* D = fisher_lds;
  double* G = D + (size_t)N * d;
  double* S = G + (size_t)N * d;
  double* L = S + ld * ld;
  double* W = L + ld * ld;
  const double *x = a.x + p * d, *h = a.h + p * d;
  const bool bound = fisher_at_bound(a, p);
  // the bracket of every segment's covariance at the centre's beta: the beta of the centre's row in the segment's row set
  if (tid < a.n_seg) {
    const FisherSeg& s = a.seg[tid];
    int lo = 0;
    double t = 0.0;
    if (s.n_beta_c > 0) {
      double beta = a.base[(size_t)s.set * a.blocks.base_stride + p * VK_NPAR + VK_P_BETA];
      for (int j = 0; j < d; ++j)
        if (a.col[j] == VK_P_BETA && vkrow::applies(a.blocks, j, s.set)) beta = x[j];
      vkfisher::bracket(s.beta_c, s.n_beta_c, beta, &lo, &t);
    }
    seg_lo[tid] = lo;
    seg_t[tid] = t;
  }
  // D, and the finiteness of every entry of the M vectors
  bool bad = false;
  for (int idx = tid; idx < N * d; idx += kFisherBlock) {
    const int e_all = idx / d, k = idx - e_all * d;
    int q = 0;
    while (q + 1 < a.n_seg && e_all >= a.seg[q + 1].off) ++q;
    const FisherSeg& s = a.seg[q];
    const int e = e_all - s.off;
    const double* th = s.theory + p * M * s.N + e;
    const double tp = th[(size_t)vkhess::at_axis(k, 0) * s.N], tm = th[(size_t)vkhess::at_axis(k, 1) * s.N];
    bad = bad || !vkhess::finite(tp) || !vkhess::finite(tm) || (k == 0 && !vkhess::finite(th[0]));
    D[idx] = vkfisher::d_entry(tp, tm);
  }
  const bool not_finite = __syncthreads_or(bad) != 0;      // (the barrier behind the staging and the brackets, too)
  int status = bound ? vkhess::kAtBound : not_finite ? vkhess::kNotFinite : vkhess::kOk;
  // thread -> entry (j >= k) of the packed lower triangle, row by row
  int j = 0;
  while ((j + 1) * (j + 2) / 2 <= tid) ++j;
  const int k = tid - j * (j + 1) / 2;
  const bool mine = j < d;
  const double hh_j = mine ? h[j] : 1.0, hh_k = mine ? h[k] : 1.0;
  double fv = vkhess::nan(), av = vkhess::nan(), cv = vkhess::nan();
  if (status == vkhess::kOk) {                     // (uniform over the workgroup: every barrier below is reached by all threads)
    for (int idx = tid; idx < N * d; idx += kFisherBlock) {
      const int e_all = idx / d, kk = idx - e_all * d;
      int q = 0;
      while (q + 1 < a.n_seg && e_all >= a.seg[q + 1].off) ++q;
      const FisherSeg& s = a.seg[q];
      const size_t row = (size_t)(s.prow0 + e_all - s.off) * s.ld;
      const int last = s.n_beta_c > 0 ? s.n_beta_c - 1 : 0;
      G[idx] = vkfisher::g_entry(s.prec + (size_t)seg_lo[q] * s.slice + row, s.prec + (size_t)last * s.slice + row, seg_t[q], s.pn,
                                 D + (size_t)s.poff * d + kk, d);
    }
    __syncthreads();
    if (mine) {
      const double s = vkfisher::s_entry(D, G, d, N, j, k);
      fv = vkfisher::fisher_entry(a.c, s, hh_j, hh_k);
      av = vkfisher::a_entry(a.c, s, a.prior.on != 0, vkfisher::lambda_entry(a.prior, d, j, k), hh_j, hh_k);
      S[j * ld + k] = av;
    }
    __syncthreads();
    for (int c = 0; c < d; ++c) {
      const double scc = S[c * ld + c];
      if (!(scc > 0.0)) {                          // (every thread reads the same pivot)
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
      if (tid < d)                                 // column `tid` of W = L^-1, top to bottom
        for (int r = tid; r < d; ++r) W[r * ld + tid] = vkhess::w_entry(L, W, ld, r, tid);
      __syncthreads();
      if (mine) cv = vkhess::cov_entry(vkhess::b_entry(W, ld, d, j, k), hh_j, hh_k);
    }
  }
  if (mine) {
    const size_t at = p * d * d;
    a.fisher[at + j * d + k] = a.fisher[at + k * d + j] = fv;
    a.a[at + j * d + k] = a.a[at + k * d + j] = av;
    a.cov[at + j * d + k] = a.cov[at + k * d + j] = cv;
  }
  if (tid == 0) a.status[p] = status;
}

}  // namespace vk
