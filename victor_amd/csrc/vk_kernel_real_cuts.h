// vk_kernel_real_cuts.h: the realisation kernel of vk_kernel_real.h under SCALE CUTS - one theory vector against every
// (cut, realisation) pair - part of libvictor_hip.so (see victor_hip.hip for the overview, DESIGN.md for the measurements).
//
// A cut k keeps n_k of the N entries of the data vector (an s range, a set of multipoles, a mask): idx_k[0 .. n_k - 1], strictly
// increasing.  Its precision is the inverse of the SUB-covariance C[idx, idx] - not a sub-block of the full precision -, its log
// determinant and blend eigenvalues are the sub-covariance's, and the likelihood forms count n_k data points (Hartlap, Percival).
// The host (vk_set_cuts) keeps those tables per cut; the theory vector does not depend on the cut, so a point still costs one
// theory evaluation, and then for cut k and realisation m
//     chi2[p][k R + m] = r^T Q_k(beta_p) r,   r_e = t_p[idx_k[e]] - D_m(beta_p)[idx_k[e]],  e < n_k.
// A problem is the flat index v = k R + m, cut-major: cross mode writes [point][K R], pairs mode takes which[point] = v.
//
// Layout: vk_like_real_kernel's, once per cut.  One workgroup per point; the covariance bracket and the PCHIP piece depend on beta
// alone and are found once.  Per cut: Q_k at beta_p goes into LDS K-major with Np_k = real_np(n_k) and stride real_qs(n_k) - the
// fill and the MFMA loop shrink with the cut -, the log-det factor and the singular flag are taken from the cut's tables
// (logdet_term, block_sum4), then the tiles of 16 realisations go through real_block_product exactly as in the uncut kernel, the
// residual gathered through idx_k (the PCHIP pieces are indexed by the FULL entry).  The theory vector keeps all N entries in LDS
// behind the space of the full Qk, so the LDS need is real_lds_doubles(N) whatever the cuts.
//
// Shapes: n_k <= 16 is one row block - wave 0 multiplies, the other three add zeros to the wave-ordered sum; a count
// of row blocks that is no multiple of four (Np_k not a multiple of 64) leaves the last round of the round-robin short.  Both
// are the uncut kernel's behaviour at such an N, kept for the sake of one order of summation.
//
// Pairs mode is the cut which / R with a tile of one live column, the column which % R mod 16 the realisation occupies in cross
// mode: the same bits as cross mode.  Operand maps: real_block_product (vk_kernel_real.h).
#pragma once
#include "vk_kernel_real.h"

namespace vk {

struct CutArgs {
  RealArgs real;            // the uncut kernel's arguments: like.prec / logdet / eig are NOT read, the tables below are
  int n_cuts;
  int n_slices;             // max(n_beta_c, 1)
  const int* n_keep;        // [n_cuts]
  const int* index;         // [n_cuts][N]: idx_k, the first n_k entries of row k
  const double* prec;       // [n_cuts][n_slices][N N]: the n_k x n_k precision of slice j, compact (row stride n_k), at (k n_slices + j) N N
  const double* logdet;     // [n_cuts][n_beta_c] (NULL: fixed covariance)
  const double* eig;        // [n_cuts][n_beta_c][N]: the first n_k of each row
};

// like_form (vk_kernel_like.h) with the number of data points given: a cut counts the entries it keeps
__device__ __forceinline__ double like_form_nd(const LikeArgs& a, double chisq, double factor, double nd) {
  const double nm = a.nmocks, np = a.nparams;
  if (a.like_form == VK_LIKE_SELLENTIN) return -nm * log(1.0 + chisq / (nm - 1.0)) / 2.0 + factor;
  if (a.like_form == VK_LIKE_HARTLAP) return -0.5 * chisq * ((nm - nd - 2.0) / (nm - 1.0)) + factor;
  if (a.like_form == VK_LIKE_PERCIVAL) {
    const double B = (nm - nd - 2.0) / ((nm - nd - 1.0) * (nm - nd - 4.0));
    const double m = np + 2.0 + (nm - 1.0 + B * (nd - np)) / (1.0 + B * (nd - np));
    return -m * log(1.0 + chisq / (nm - 1.0)) / 2.0 + factor;
  }
  return -0.5 * chisq + factor;
}

// (Named vk_cuts_*: the vk_like_* kernels are the chi-square kernels of the instance matrix, tests/kernel_matrix.py, one recipe each
// per count of data poles; this one is reached through vk_set_cuts alone and has tests of its own, as the joint kernels have.)
template <bool MFMA>
__global__ __launch_bounds__(kBlock) void vk_cuts_real_kernel(CutArgs ca) {
  extern __shared__ double lds[];
  const RealArgs& ra = ca.real;
  const LikeArgs& a = ra.like;
  const long long point = blockIdx.x;                 // one point per workgroup (the host launches n of them)
  if (point >= a.n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N, R = ra.n_real;
  double* Qk = lds;                                    // the cut's [Np_k][qs_k], inside the space of the full [Np][qs]
  double* th = Qk + (size_t)real_np(N) * real_qs(N);   // all N entries: a cut gathers from it
  double* Rt = th + real_np(N);
  double* part = Rt + (size_t)real_np(N) * kRealCols;
  double* red = part + kWaves * kRealCols;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double beta = a.params[point * VK_NPAR + VK_P_BETA];

  // what depends on beta alone: the covariance bracket (ccf_fit.py:213-228) and the PCHIP piece of the data vectors (:166-193)
  int lo = 0;
  double t = 0.0;
  if (a.n_beta_c > 0) cov_bracket(a, beta, &lo, &t);
  const double omt = 1.0 - t;
  int kb = 0;
  for (int i = 1; i < a.n_beta_d - 1; ++i) kb = (beta >= a.beta_d[i]) ? i : kb;
  const double db = a.n_beta_d > 0 ? beta - a.beta_d[kb] : 0.0;
  for (int e = tid; e < N; e += kBlock) th[e] = a.theory[point * N + e];

  const bool pairs = ra.which != nullptr;
  const int flat = pairs ? ra.which[point] : 0;
  const int mine = pairs ? flat % R : 0;
  const int k_first = pairs ? flat / R : 0, k_end = pairs ? k_first + 1 : ca.n_cuts;
  const long long per_point = (long long)ca.n_cuts * R;
  const long long tiles = pairs ? 1 : (R + kRealCols - 1) / kRealCols;
  for (int kc = k_first; kc < k_end; ++kc) {
    const int n = ca.n_keep[kc], Np = real_np(n), qs = real_qs(n);
    const int* idx = ca.index + (size_t)kc * N;
    // precision of the cut at beta, K-major, zero-padded; the blend as in vk_like_kernel.  (Every wave is past the last barrier
    // of the previous cut's last tile, so its reads of Qk and Rt are done.)
    const double* Pc = ca.prec + (size_t)kc * ca.n_slices * N * N;
    const double* P0 = Pc + (a.n_beta_c > 0 ? (size_t)lo * N * N : 0);
    const double* P1 = Pc + (a.n_beta_c > 0 ? (size_t)(a.n_beta_c - 1) * N * N : 0);
    for (int at = tid; at < Np * Np; at += kBlock) {
      const int i = at / Np, k = at - i * Np;
      double q = 0.0;
      if (i < n && k < n) {
        const size_t src = (size_t)i * n + k;
        q = (t != 0.0) ? omt * P0[src] + t * P1[src] : P0[src];
      }
      Qk[(size_t)k * qs + i] = q;
    }
    // -1/2 log det of the cut's blended covariance, once per (point, cut) (ccf_fit.py:445-451; sign rule of logdet_term)
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    if (a.n_beta_c > 0 && t != 0.0) {
      int neg = 0, bad = 0;
      const double* ev = ca.eig + ((size_t)kc * a.n_beta_c + lo) * N;
      for (int e = tid; e < n; e += kBlock) sums[1] += logdet_term(fma(t, ev[e], omt), &neg, &bad);
      sums[2] = (double)neg;
      sums[3] = (double)bad;
    }
    block_sum4(sums, red);                              // (its barriers also publish Qk and th)
    double factor = 0.0;
    bool singular = false;
    if (a.n_beta_c > 0) {
      const double ld = ca.logdet[(size_t)kc * a.n_beta_c + lo];
      const int neg = (int)sums[2], bad = (int)sums[3];
      singular = (neg & 1) || bad || !(fabs(ld) < inf);
      factor = -0.5 * (ld + sums[1]);
    }

    for (long long tile = 0; tile < tiles; ++tile) {
      const long long m0 = pairs ? (long long)(mine & ~(kRealCols - 1)) : tile * kRealCols;
      // residual block Rt[k][j] = t_idx[k] - D_(m0 + j)(beta)_idx[k]; lanes along k, zeros outside the cut
      for (int at = tid; at < Np * kRealCols; at += kBlock) {
        const int j = at / Np, k = at - j * Np;
        const long long m = m0 + j;
        const bool live = k < n && (pairs ? m == mine : m < R);
        double r = 0.0;
        if (live) {
          const int e = idx[k];
          const double* blk = ra.real + m * ra.block;
          if (a.n_beta_d > 0) {
            const double* c = blk + ((size_t)kb * N + e) * 4;
            r = th[e] - fma(fma(fma(c[3], db, c[2]), db, c[1]), db, c[0]);
          } else {
            r = th[e] - blk[e];
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
        if (pairs ? m == mine : m < R) {
          double chisq = part[tid];
#pragma unroll
          for (int w = 1; w < kWaves; ++w) chisq += part[w * kRealCols + tid];
          double lnl = like_form_nd(a, chisq, factor, (double)n);
          double chi_out = chisq;
          if (singular || lnl != lnl) {  // ccf_fit.py:448-450, 477-481
            lnl = -inf;
            chi_out = inf;
          }
          const long long at = pairs ? point : point * per_point + (long long)kc * R + m;
          if (a.lnl) a.lnl[at] = lnl;
          if (a.chi2) a.chi2[at] = chi_out;
        }
      }
      // (the next tile's residuals overwrite Rt: every wave has passed the barrier above, so its reads of Rt are done)
    }
  }
}

}  // namespace vk
