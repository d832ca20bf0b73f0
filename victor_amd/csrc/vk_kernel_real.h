// vk_kernel_real.h: chi-square / log-likelihood of one theory vector against MANY data vectors (simulation realisations) - part of
// libvictor_hip.so (see victor_hip.hip for the overview, DESIGN.md section 5 for the measurements).
//
// CCFFit reads one realisation of a stacked data file (ccf_fit.py:59-61,93-100: `simulation_number`); validating a model on
// mocks means the same parameter points against every realisation.  The theory vector t_p does not depend on the realisation,
// so a point costs one theory evaluation (the existing theory launch, into the workspace) and then, for M realisations,
//     chi2[p][m] = r_m^T Q(beta_p) r_m,   r_m = t_p - D_m(beta_p)
// the column sums of R o (Q R) for the N x M residual block R: a batched N x N x M product, 2 N^2 M flops per point.
//
// Layout: one workgroup per point.  The precision at beta_p (slice blend as in vk_like_kernel, cov_bracket) is formed once in
// LDS, K-major (Qk[k][i] = Q[i][k], rows of Np + 2 doubles, N padded with zeros to Np = a multiple of 16), next to the theory
// vector; the log-det factor (logdet_term, block_sum4) is taken once per point and shared by its realisations.  Realisations
// go through in tiles of 16 - the columns of v_mfma_f64_16x16x4_f64: the workgroup evaluates the tile's data vectors at beta_p
// (Horner on the PCHIP pieces, as LikePrefetch) into an Np x 16 block of LDS, the four waves take the 16-row blocks of Q R
// round-robin (wave w: row blocks w, w + 4, ...), multiply the block on the matrix cores (Np / 4 MFMAs of K = 4 per row block)
// and dot the accumulators with the matching residuals; the four waves' partial sums are added in wave order.
//
// Pairs mode (point p against realisation which[p] only) is the same kernel with a tile of one live column; that column is
// the one the realisation occupies in cross mode (which[p] mod 16), so every sum of the pair is formed in the same order as
// in cross mode and the two modes return the same bits.
//
// f64 MFMA operand maps (cdna_hip_programming.md section 3; NOT the f32 C/D map): lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; result register q of lane l is C[(l >> 4) + 4 q][l & 15].
#pragma once
#include "vk_kernel_like.h"

namespace vk {

constexpr int kRealCols = 16;                                        // realisations per tile: the MFMA's N

struct RealArgs {
  LikeArgs like;            // theory [n][N], params, grids, precision slices, log det, eig, form; lnl / chi2 are the outputs
  const double* real;       // [n_real][block]: data vector of each realisation in the layout of vk_tables.data
  long long block;          // doubles per realisation
  int n_real;
  const int* which;         // pairs mode: [n] realisation of each point; NULL: every realisation (outputs [n][n_real])
};

__host__ __device__ constexpr int real_np(int N) { return (N + 15) & ~15; }
__host__ __device__ constexpr int real_qs(int N) { return real_np(N) + 2; }       // row stride of Qk (breaks the bank pattern)
// LDS: Qk [Np][Np + 2] | theory [Np] | residual tile [Np][16] | wave partials [kWaves][16] | kLikeRed
__host__ __device__ constexpr size_t real_lds_doubles(int N) {
  return (size_t)real_np(N) * real_qs(N) + real_np(N) + (size_t)real_np(N) * kRealCols + kWaves * kRealCols + kLikeRed;
}

typedef double real_d4 __attribute__((ext_vector_type(4)));

// Q R for row block rb of the tile; lane l's four results are rows 16 rb + (l >> 4) + 4 q of column l & 15
template <bool MFMA>
__device__ __forceinline__ real_d4 real_block_product(const double* Qk, int qs, const double* Rt, int Np, int rb, int lane) {
  real_d4 acc = {0.0, 0.0, 0.0, 0.0};
  const int col = lane & 15, grp = lane >> 4;
  if (MFMA) {
    const double* a = Qk + (size_t)grp * qs + rb * 16 + col;         // A[i = 16 rb + col][k = 4 ks + grp]
    const double* b = Rt + grp * kRealCols + col;                     // B[k = 4 ks + grp][j = col]
    for (int ks = 0; ks < Np / 4; ++ks)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(size_t)ks * 4 * qs], b[ks * 4 * kRealCols], acc, 0, 0, 0);
  } else {
    // the VALU yardstick of the same tiling: every lane forms its own four entries, k in order
    const int row = rb * 16 + grp;
    for (int k = 0; k < Np; ++k) {
      const double r = Rt[k * kRealCols + col];
      const double* q = Qk + (size_t)k * qs + row;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fma(q[4 * j], r, acc[j]);
    }
  }
  return acc;
}

template <bool MFMA>
__global__ __launch_bounds__(kBlock) void vk_like_real_kernel(RealArgs ra) {
  extern __shared__ double lds[];
  const LikeArgs& a = ra.like;
  const long long point = blockIdx.x;                 // one point per workgroup (the host launches n of them)
  if (point >= a.n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, Np = real_np(N), qs = real_qs(N);
  double* Qk = lds;
  double* th = Qk + (size_t)Np * qs;
  double* Rt = th + Np;
  double* part = Rt + (size_t)Np * kRealCols;
  double* red = part + kWaves * kRealCols;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double beta = a.params[point * VK_NPAR + VK_P_BETA];

  // precision at beta (ccf_fit.py:230-260), K-major, zero-padded; the blend as in vk_like_kernel
  int lo = 0;
  double t = 0.0;
  if (a.n_beta_c > 0) cov_bracket(a, beta, &lo, &t);
  const double omt = 1.0 - t;
  const double* P0 = a.prec + (a.n_beta_c > 0 ? (size_t)lo * N * N : 0);
  const double* P1 = a.prec + (a.n_beta_c > 0 ? (size_t)(a.n_beta_c - 1) * N * N : 0);
  for (int idx = tid; idx < Np * Np; idx += kBlock) {
    const int i = idx / Np, k = idx - i * Np;
    double q = 0.0;
    if (i < N && k < N) {
      const size_t at = (size_t)i * N + k;
      q = (t != 0.0) ? omt * P0[at] + t * P1[at] : P0[at];
    }
    Qk[(size_t)k * qs + i] = q;
  }
  for (int e = tid; e < Np; e += kBlock) th[e] = e < N ? a.theory[point * N + e] : 0.0;

  // -1/2 log det of the blended covariance, once per point (ccf_fit.py:445-451; sign rule of logdet_term)
  double sums[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.n_beta_c > 0 && t != 0.0) {
    int neg = 0, bad = 0;
    for (int e = tid; e < N; e += kBlock) sums[1] += logdet_term(fma(t, a.eig[(size_t)lo * N + e], omt), &neg, &bad);
    sums[2] = (double)neg;
    sums[3] = (double)bad;
  }
  block_sum4(sums, red);                                // (its barriers also publish Qk and th)
  double factor = 0.0;
  bool singular = false;
  if (a.n_beta_c > 0) {
    const int neg = (int)sums[2], bad = (int)sums[3];
    singular = (neg & 1) || bad || !(fabs(a.logdet[lo]) < inf);
    factor = -0.5 * (a.logdet[lo] + sums[1]);
  }

  // the PCHIP piece of the data vectors at beta (ccf_fit.py:166-193), as vk_like_kernel finds it
  int kb = 0;
  for (int i = 1; i < a.n_beta_d - 1; ++i) kb = (beta >= a.beta_d[i]) ? i : kb;
  const double db = a.n_beta_d > 0 ? beta - a.beta_d[kb] : 0.0;

  const bool pairs = ra.which != nullptr;
  const int mine = pairs ? ra.which[point] : 0;
  const long long tiles = pairs ? 1 : (ra.n_real + kRealCols - 1) / kRealCols;
  for (long long tile = 0; tile < tiles; ++tile) {
    const long long m0 = pairs ? (long long)(mine & ~(kRealCols - 1)) : tile * kRealCols;
    // residual block Rt[k][j] = t_k - D_(m0 + j)(beta)_k; lanes along k (coalesced pieces), zeros outside the data
    for (int idx = tid; idx < Np * kRealCols; idx += kBlock) {
      const int j = idx / Np, k = idx - j * Np;
      const long long m = m0 + j;
      const bool live = k < N && (pairs ? m == mine : m < ra.n_real);
      double r = 0.0;
      if (live) {
        const double* blk = ra.real + m * ra.block;
        if (a.n_beta_d > 0) {
          const double* c = blk + ((size_t)kb * N + k) * 4;
          r = th[k] - fma(fma(fma(c[3], db, c[2]), db, c[1]), db, c[0]);
        } else {
          r = th[k] - blk[k];
        }
      }
      Rt[k * kRealCols + j] = r;
    }
    __syncthreads();
    // chi2 of column j: sum over the row blocks of this wave, register by register, then over the four lane groups
    double acc = 0.0;
    for (int rb = wave; rb < Np / 16; rb += kWaves) {
      const real_d4 y = real_block_product<MFMA>(Qk, qs, Rt, Np, rb, lane);
      const int row = rb * 16 + (lane >> 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) acc = fma(Rt[(row + 4 * q) * kRealCols + (lane & 15)], y[q], acc);
    }
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (lane < kRealCols) part[wave * kRealCols + lane] = acc;
    __syncthreads();
    if (tid < kRealCols) {
      const long long m = m0 + tid;
      if (pairs ? m == mine : m < ra.n_real) {
        double chisq = part[tid];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) chisq += part[w * kRealCols + tid];
        double lnl = like_form(a, chisq, factor);
        double chi_out = chisq;
        if (singular || lnl != lnl) {  // ccf_fit.py:448-450, 477-481
          lnl = -inf;
          chi_out = inf;
        }
        const long long at = pairs ? point : point * ra.n_real + m;
        if (a.lnl) a.lnl[at] = lnl;
        if (a.chi2) a.chi2[at] = chi_out;
      }
    }
    // (the next tile's residuals overwrite Rt: every wave has passed the barrier above, so its reads of Rt are done)
  }
}

}  // namespace vk
