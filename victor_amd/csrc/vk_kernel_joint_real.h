// vk_kernel_joint_real.h: chi-square / log-likelihood of a joint fit under ONE covariance against MANY simulation realisations
// of its data vectors (vk_joint_cov_eval_realisations) - part of libvictor_hip.so (see victor_hip.hip for the overview, DESIGN.md
// section 5 for the measurements).
//
// Joint realisation m is realisation m of every block (each block reads its own stacked file, ccf_fit.py:59-61,93-100), so the
// pair (point p, realisation m) has the residual r_pm = concat_q (t_q(theta_p) - d_{q,m}(beta_p)) and
//     chi2_pm = r_pm^T Psi(beta_p) r_pm,
// the problem of vk_joint_chi2_kernel (vk_kernel_joint.h) with rows = (point, realisation) pairs instead of points: 2 NT^2 n M
// flops.  The kernel below is that kernel with another row map; the matrix product, the per-row reduction and the slice loop
// are the same code shape, and a row's sum is formed in the same fixed order wherever the row sits:
//   - cross mode (which == NULL): tile T holds realisations 16 (T mod tpp) .. + 15 of point T / tpp, tpp = ceil(M / 16).  All
//     rows of a tile share one point, hence one covariance bracket: one quadratic form per row, two when blended, no sort.
//   - pairs mode (which[p]: the realisation of point p): the rows are points, ordered by covariance slice through the stable
//     counting sort of vk_kernel_joint.h (vk_joint_rank / offsets / scatter_kernel), as vk_joint_cov_eval_device_async does.
// The residuals are formed once per tile in LDS: the blocks' theory vectors from their theory launches' workspaces minus the
// realisation's data at beta_p (Horner on its PCHIP pieces, read from the realisation's block of the context's d_real).
//
// -1/2 log det C(beta_p) and its sign test depend on the point only: vk_joint_real_factor_kernel takes them once per point
// (one wave each, the arithmetic of vk_joint_chi2_kernel) into the workspace, and both modes read them from there.  With the
// same factor and the same row sum, pairs mode and cross mode return the same bits; nothing is accumulated with atomics.
#pragma once
#include "vk_kernel_joint.h"

namespace vk {

struct JointRealArgs {
  JointArgs joint;                       // like: params, n, N = NT, covariance grid and slices, form, outputs lnl / chi2;
                                         // perm: pairs mode's slice order (NULL: identity); blk[q].data: block q's realisations
  long long stride[kJointMaxBlocks];     // doubles per realisation of block q (the layout of vk_tables.data)
  int n_real;
  const int* which;                      // pairs mode: [n] realisation of each point; NULL: every realisation (outputs [n][n_real])
  const double* fac;                     // [n] -1/2 log det C(beta_p) (NULL: fixed covariance, 0)
  const int* bad;                        // [n] 1 where the blended covariance fails the sign test
};

// LDS: residuals [16][NTp + 4] | wave partials [kWaves][16] | per row: Q_lo, Q_last, t, factor [4][16], db [blocks][16] |
// ints: point, realisation, lo, singular [4][16], kb [blocks][16], need [max(n_beta, 1)]
__host__ __device__ constexpr size_t joint_real_lds_doubles(int NT, int n_blocks, int n_beta) {
  return (size_t)kJointRows * joint_rs(NT) + kWaves * kJointRows + 4 * kJointRows + (size_t)n_blocks * kJointRows +
         ((size_t)(4 + n_blocks) * kJointRows + (n_beta > 1 ? n_beta : 1) + 1) / 2 + 1;
}

// -1/2 log det of the covariance at beta_p and its sign test (ccf_fit.py:445-451): one wave per point, lanes over the
// generalised-eigenvalue factors, as vk_joint_chi2_kernel forms them
__global__ __launch_bounds__(kBlock) void vk_joint_real_factor_kernel(JointArgs ja, double* fac, int* bad_out) {
  const LikeArgs& a = ja.like;
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (p >= a.n) return;                                           // (uniform over the wave)
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const int NT = a.N;
  int lo = 0;
  double t = 0.0;
  cov_bracket(a, a.params[(size_t)p * VK_NPAR + VK_P_BETA], &lo, &t);
  const double omt = 1.0 - t;
  double sum = 0.0, neg = 0.0, bad = 0.0;
  if (t != 0.0) {
    int n_neg = 0, n_bad = 0;
    for (int e = lane; e < NT; e += 64) sum += logdet_term(fma(t, a.eig[(size_t)lo * NT + e], omt), &n_neg, &n_bad);
    neg = (double)n_neg;
    bad = (double)n_bad;
  }
  sum = wave_sum(sum);
  neg = wave_sum(neg);
  bad = wave_sum(bad);
  if (lane == 0) {
    fac[p] = -0.5 * (a.logdet[lo] + sum);
    bad_out[p] = (((int)neg & 1) || bad != 0.0 || !(fabs(a.logdet[lo]) < inf)) ? 1 : 0;
  }
}

__global__ __launch_bounds__(kBlock) void vk_joint_real_chi2_kernel(JointRealArgs jr) {
  extern __shared__ double lds[];
  const JointArgs& ja = jr.joint;
  const LikeArgs& a = ja.like;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = a.N, NTp = ja.NTp, rs = joint_rs(NT), nblk = ja.n_blocks;
  const int n_slices = a.n_beta_c > 0 ? a.n_beta_c : 1, last = n_slices - 1;
  const bool pairs = jr.which != nullptr;
  double* R = lds;
  double* part = R + (size_t)kJointRows * rs;
  double* q_lo = part + kWaves * kJointRows;
  double* q_last = q_lo + kJointRows;
  double* row_t = q_last + kJointRows;
  double* row_fac = row_t + kJointRows;
  double* row_db = row_fac + kJointRows;                          // [blocks][16]
  int* row_pt = reinterpret_cast<int*>(row_db + nblk * kJointRows);
  int* row_m = row_pt + kJointRows;
  int* row_lo = row_m + kJointRows;
  int* row_bad = row_lo + kJointRows;
  int* row_kb = row_bad + kJointRows;                             // [blocks][16]
  int* need = row_kb + nblk * kJointRows;                         // [n_slices]
  const double inf = __longlong_as_double(0x7ff0000000000000LL);

  // the tile's (point, realisation) rows, their covariance bracket and log-det factor, the PCHIP piece of every block's data
  for (int s = tid; s < n_slices; s += kBlock) need[s] = 0;
  if (tid < kJointRows) {
    int p = -1, m = 0, lo = 0, bad = 0;
    double t = 0.0, fac = 0.0;
    if (pairs) {
      const long long at = (long long)blockIdx.x * kJointRows + tid;
      if (at < a.n) {
        p = ja.perm ? ja.perm[at] : (int)at;
        if (p < 0 || p >= a.n) p = -1;                            // (a permutation always holds 0 .. n - 1; never read past it)
        if (p >= 0) m = jr.which[p];
      }
    } else {
      const long long tpp = (jr.n_real + kJointRows - 1) / kJointRows;
      const long long pt = (long long)blockIdx.x / tpp;
      const long long mm = ((long long)blockIdx.x - pt * tpp) * kJointRows + tid;
      if (pt < a.n && mm < jr.n_real) {
        p = (int)pt;
        m = (int)mm;
      }
    }
    if (m < 0 || m >= jr.n_real) p = -1;                          // (the host checked which[]; never read past the realisations)
    if (p >= 0 && a.n_beta_c > 0) {
      cov_bracket(a, a.params[(size_t)p * VK_NPAR + VK_P_BETA], &lo, &t);
      fac = jr.fac[p];
      bad = jr.bad[p];
    }
    row_pt[tid] = p;
    row_m[tid] = m;
    row_lo[tid] = lo;
    row_t[tid] = t;
    row_fac[tid] = fac;
    row_bad[tid] = bad;
  }
  __syncthreads();
  if (tid < kJointRows && row_pt[tid] >= 0) {
    need[row_lo[tid]] = 1;
    if (row_t[tid] != 0.0) need[last] = 1;
  }
  for (int idx = tid; idx < kJointRows * nblk; idx += kBlock) {
    const int r = idx & (kJointRows - 1), q = idx / kJointRows;
    const JointBlock& b = ja.blk[q];
    int kb = 0;
    double db = 0.0;
    if (row_pt[r] >= 0 && b.n_beta_d > 0) {
      const double beta = a.params[(size_t)row_pt[r] * VK_NPAR + VK_P_BETA];
      for (int i = 1; i < b.n_beta_d - 1; ++i) kb = (beta >= b.beta_d[i]) ? i : kb;
      db = beta - b.beta_d[kb];
    }
    row_kb[q * kJointRows + r] = kb;
    row_db[q * kJointRows + r] = db;
  }
  __syncthreads();

  // residuals R[r][k] = t_k - d_k(beta) of the row's realisation; zeros for padding and for rows past the last pair
  for (int idx = tid; idx < kJointRows * NTp; idx += kBlock) {
    const int r = idx / NTp, k = idx - r * NTp;
    const int p = row_pt[r];
    double v = 0.0;
    if (p >= 0 && k < NT) {
      int q = 0;
      while (q + 1 < nblk && k >= ja.blk[q + 1].off) ++q;
      const JointBlock& b = ja.blk[q];
      const int e = k - b.off;
      const double th = b.theory[(size_t)p * b.N + e];
      const double* d = b.data + (size_t)row_m[r] * jr.stride[q];
      if (b.n_beta_d > 0) {
        const double* c = d + ((size_t)row_kb[q * kJointRows + r] * b.N + e) * 4;
        const double db = row_db[q * kJointRows + r];
        v = th - fma(fma(fma(c[3], db, c[2]), db, c[1]), db, c[0]);
      } else {
        v = th - d[e];
      }
    }
    R[(size_t)r * rs + k] = v;
  }
  __syncthreads();

  // the quadratic form of every slice a row of the tile needs (the loop of vk_joint_chi2_kernel)
  const int col = lane & 15, grp = lane >> 4;
  for (int s = 0; s < n_slices; ++s) {
    if (!need[s]) continue;                                       // (LDS word: uniform over the workgroup)
    const double* P = a.prec + (size_t)s * NTp * NTp;
    joint_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int cb = wave; cb < NTp / 16; cb += kWaves) {
      joint_d4 y = {0.0, 0.0, 0.0, 0.0};
      const double* ar = R + (size_t)col * rs + grp;              // A[i = col][k = 4 ks + grp]
      const double* br = P + (size_t)grp * NTp + cb * 16 + col;   // B[k = 4 ks + grp][j = 16 cb + col]
      for (int ks = 0; ks < NTp / 4; ks += 4) {                  // (NTp / 4 is a multiple of 4: four B loads in flight)
        double bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[u] = br[(size_t)(ks + u) * 4 * NTp];
#pragma unroll
        for (int u = 0; u < 4; ++u) y = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[(ks + u) * 4], bv[u], y, 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fma(R[(size_t)(grp + 4 * q) * rs + cb * 16 + col], y[q], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double v = acc[q];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 8);
      if (col == 0) part[wave * kJointRows + grp + 4 * q] = v;
    }
    __syncthreads();
    if (tid < kJointRows) {
      double form = part[tid];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) form += part[w * kJointRows + tid];
      if (row_lo[tid] == s) q_lo[tid] = form;
      if (s == last && row_t[tid] != 0.0) q_last[tid] = form;
    }
    __syncthreads();                                              // (part is written again by the next slice)
  }

  if (tid < kJointRows && row_pt[tid] >= 0) {
    const int p = row_pt[tid];
    const double t = row_t[tid];
    const double chisq = (t != 0.0) ? (1.0 - t) * q_lo[tid] + t * q_last[tid] : q_lo[tid];
    double lnl = like_form(a, chisq, row_fac[tid]);
    double chi_out = chisq;
    if (row_bad[tid] || lnl != lnl) {                             // ccf_fit.py:448-450, 477-481
      lnl = -inf;
      chi_out = inf;
    }
    const long long at = pairs ? (long long)p : (long long)p * jr.n_real + row_m[tid];
    if (a.lnl) a.lnl[at] = lnl;
    if (a.chi2) a.chi2[at] = chi_out;
  }
}

}  // namespace vk
