// vk_kernel_joint.h: chi-square / log-likelihood of a joint fit under ONE covariance matrix across its data vectors
// (vk_joint_cov_eval_device_async) - part of libvictor_hip.so (see victor_hip.hip for the overview, DESIGN.md section 5 for the
// measurements).
//
// The blocks' theory vectors come from their own theory launches (theory-only mode, one workspace [n][N_q] per block).  The
// joint residual of point p is r_p = concat_q (t_q(theta_p) - d_q(beta_p)), NT = sum_q N_q entries in block order, and
//     chi2_p = r_p^T Psi(beta_p) r_p
// for all n points is the batched quadratic form of the n x NT residual matrix R: Y = R Psi, chi2_p = sum_i R[p][i] Y[p][i],
// 2 n NT^2 flops.  For NT = 600 a precision slice is 2.9 MB - far beyond LDS - so Psi is streamed from L2 / Infinity Cache.
//
// Layout: one workgroup per tile of 16 points - the rows (M) of v_mfma_f64_16x16x4_f64.  The tile's residuals are formed
// once in LDS (theory from the workspaces minus the data at beta, Horner on the PCHIP pieces as LikePrefetch), row-major with
// rows of NTp + 4 doubles (NT padded with zeros to NTp = a multiple of 16; the +4 puts the 16 rows of an A operand on distinct
// banks).  The four waves take the 16-column blocks of Y round-robin (wave w: column blocks w, w + 4, ...); a column block is
// NTp / 4 MFMAs of K = 4 whose A operand is read from the residuals in LDS and whose B operand - 64 doubles of Psi, four
// 128-byte row segments - straight from global memory: every element of Psi is used exactly once per workgroup, so a copy
// through LDS would add traffic and no reuse.  The accumulators are dotted with the matching residuals, summed over the 16
// lanes of a row (xor butterfly: every lane gets the same bits) and over the column blocks of the wave, and the four waves'
// partial sums are added in wave order by one thread per row.  A row's sum is formed in the same order whichever tile or row
// of a tile the point sits in, and nothing is accumulated with atomics: repeated calls return the same bits.
//
// beta-dependent covariance (CCFFit._bracket: below / above the grid the first / last slice, on the grid that slice, else slice
// lo blended with the LAST slice, weight t):
//     chi2 = (1 - t) r^T Psi_lo r + t r^T Psi_last r,
// which equals r^T ((1 - t) Psi_lo + t Psi_last) r up to rounding (the blend is not formed; the two forms are combined per
// point), and chi2 = r^T Psi_lo r where t = 0.  A tile evaluates only the slices its points need, so the points are first
// sorted by lo (vk_joint_rank_kernel, vk_joint_offsets_kernel, vk_joint_scatter_kernel: a stable counting sort over the n_beta
// buckets, integer arithmetic only) and the tiles load their points through that permutation.  Cost: one quadratic form per
// point on the grid or outside it, two when blended, plus at most one partial tile per bucket boundary.  The -1/2 log det of
// the blended covariance is the generalised-eigenvalue product of the single-fit kernels (logdet_term, the same sign rule),
// one wave per point of the tile.
//
// f64 MFMA operand maps (cdna_hip_programming.md section 3; NOT the f32 C/D map): lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; result register q of lane l is C[(l >> 4) + 4 q][l & 15].
#pragma once
#include "vk_kernel_like.h"

namespace vk {

constexpr int kJointRows = 16;           // points per workgroup: the MFMA's M
constexpr int kJointMaxBlocks = 32;      // data vectors of one joint fit (kernel arguments)
constexpr int kJointSortChunk = kBlock;  // points per workgroup of the counting sort

struct JointBlock {
  const double* theory;     // [n][N] theory vectors of this block (its theory launch's workspace)
  const double* data;       // data vector, layout of vk_tables.data
  const double* beta_d;     // [n_beta_d] or NULL
  int N, off, n_beta_d;     // entries, offset in the joint vector, data beta grid (0: fixed data)
};

struct JointArgs {
  LikeArgs like;            // params, n, N = NT, covariance grid (n_beta_c, beta_c), prec = padded slices [..][NTp][NTp],
                            // logdet, eig [n_beta_c][NT], likelihood form; lnl / chi2 are the outputs
  int NTp;                  // NT rounded up to a multiple of 16
  int n_blocks;
  const int* perm;          // [n] tile order of the points (sorted by their covariance slice), or NULL: identity
  JointBlock blk[kJointMaxBlocks];
};

__host__ __device__ constexpr int joint_ntp(int NT) { return (NT + 15) & ~15; }
__host__ __device__ constexpr int joint_rs(int NT) { return joint_ntp(NT) + 4; }
// LDS: residuals [16][NTp + 4] | wave partials [kWaves][16] | per row: Q_lo, Q_last, t, factor [4][16], db [blocks][16] |
// ints: point, lo, singular [3][16], kb [blocks][16], need [max(n_beta, 1)]
__host__ __device__ constexpr size_t joint_lds_doubles(int NT, int n_blocks, int n_beta) {
  return (size_t)kJointRows * joint_rs(NT) + kWaves * kJointRows + 4 * kJointRows + (size_t)n_blocks * kJointRows +
         ((size_t)(3 + n_blocks) * kJointRows + (n_beta > 1 ? n_beta : 1) + 1) / 2 + 1;
}

typedef double joint_d4 __attribute__((ext_vector_type(4)));

// counting sort of the points by covariance slice, step 1: slice of each point, its rank among the points of its chunk with the
// same slice, and the chunk's histogram hist[chunk][b]
__global__ __launch_bounds__(kBlock) void vk_joint_rank_kernel(JointArgs ja, int* lo_out, int* rank_out, int* hist) {
  __shared__ int s_lo[kJointSortChunk];
  const LikeArgs& a = ja.like;
  const int tid = threadIdx.x;
  const long long p = (long long)blockIdx.x * kJointSortChunk + tid;
  int lo = -1;
  if (p < a.n) {
    double t;
    cov_bracket(a, a.params[p * VK_NPAR + VK_P_BETA], &lo, &t);
  }
  s_lo[tid] = lo;
  __syncthreads();
  if (p < a.n) {
    int rank = 0;
    for (int j = 0; j < tid; ++j) rank += (s_lo[j] == lo) ? 1 : 0;
    lo_out[p] = lo;
    rank_out[p] = rank;
  }
  for (int b = tid; b < a.n_beta_c; b += kBlock) {
    int c = 0;
    for (int j = 0; j < kJointSortChunk; ++j) c += (s_lo[j] == b) ? 1 : 0;
    hist[(size_t)blockIdx.x * a.n_beta_c + b] = c;
  }
}

// step 2 (one workgroup): hist[chunk][b] becomes the position of the chunk's first point of slice b in the sorted order.  Each
// thread walks the n / 256 chunks of its buckets serially: 64 chunks (0.05 ms) at the 16384 points of a sampler's batch, linear
// in n beyond that - meant for batches up to about a million points (4096 chunks); the histograms, (n / 256 + 1) x n_beta ints
// of the workspace, grow the same way.
__global__ __launch_bounds__(kBlock) void vk_joint_offsets_kernel(int* hist, int n_chunks, int n_beta) {
  int* total = hist + (size_t)n_chunks * n_beta;          // [n_beta] behind the histograms
  for (int b = threadIdx.x; b < n_beta; b += kBlock) {
    int run = 0;
    for (int c = 0; c < n_chunks; ++c) {
      const int h = hist[(size_t)c * n_beta + b];
      hist[(size_t)c * n_beta + b] = run;
      run += h;
    }
    total[b] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int b = 0; b < n_beta; ++b) {
      const int h = total[b];
      total[b] = run;
      run += h;
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_beta; b += kBlock)
    for (int c = 0; c < n_chunks; ++c) hist[(size_t)c * n_beta + b] += total[b];
}

// step 3: perm[position] = point
__global__ void vk_joint_scatter_kernel(const int* lo, const int* rank, const int* hist, int n_beta, long long n, int* perm) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  perm[hist[(size_t)(p / kJointSortChunk) * n_beta + lo[p]] + rank[p]] = (int)p;
}

__global__ __launch_bounds__(kBlock) void vk_joint_chi2_kernel(JointArgs ja) {
  extern __shared__ double lds[];
  const LikeArgs& a = ja.like;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = a.N, NTp = ja.NTp, rs = joint_rs(NT), nblk = ja.n_blocks;
  const int n_slices = a.n_beta_c > 0 ? a.n_beta_c : 1, last = n_slices - 1;
  double* R = lds;
  double* part = R + (size_t)kJointRows * rs;
  double* q_lo = part + kWaves * kJointRows;
  double* q_last = q_lo + kJointRows;
  double* row_t = q_last + kJointRows;
  double* row_fac = row_t + kJointRows;
  double* row_db = row_fac + kJointRows;                          // [blocks][16]
  int* row_pt = reinterpret_cast<int*>(row_db + nblk * kJointRows);
  int* row_lo = row_pt + kJointRows;
  int* row_bad = row_lo + kJointRows;
  int* row_kb = row_bad + kJointRows;                             // [blocks][16]
  int* need = row_kb + nblk * kJointRows;                         // [n_slices]
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const long long first = (long long)blockIdx.x * kJointRows;

  // the tile's points, their covariance bracket and the PCHIP piece of every block's data at their beta
  for (int s = tid; s < n_slices; s += kBlock) need[s] = 0;
  if (tid < kJointRows) {
    const long long at = first + tid;
    int p = -1, lo = 0;
    double t = 0.0;
    if (at < a.n) {
      p = ja.perm ? ja.perm[at] : (int)at;
      if (p < 0 || p >= a.n) p = -1;                              // (a permutation always holds 0 .. n - 1; never read past it)
      if (p >= 0 && a.n_beta_c > 0) cov_bracket(a, a.params[(size_t)p * VK_NPAR + VK_P_BETA], &lo, &t);
    }
    row_pt[tid] = p;
    row_lo[tid] = lo;
    row_t[tid] = t;
  }
  __syncthreads();
  if (tid < kJointRows && row_pt[tid] >= 0) {
    need[row_lo[tid]] = 1;
    if (row_t[tid] != 0.0) need[last] = 1;
  }
  for (int idx = tid; idx < kJointRows * nblk; idx += kBlock) {  // (up to kJointMaxBlocks x 16 = 512 entries: more than one pass)
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

  // residuals R[r][k] = t_k - d_k(beta); zeros for padding and for the rows behind the last point
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
      if (b.n_beta_d > 0) {
        const double* c = b.data + ((size_t)row_kb[q * kJointRows + r] * b.N + e) * 4;
        const double db = row_db[q * kJointRows + r];
        v = th - fma(fma(fma(c[3], db, c[2]), db, c[1]), db, c[0]);
      } else {
        v = th - b.data[e];
      }
    }
    R[(size_t)r * rs + k] = v;
  }

  // -1/2 log det of the covariance at beta (ccf_fit.py:445-451): one wave per row, lanes over the eigenvalue factors
  if (a.n_beta_c > 0) {
    for (int r = wave; r < kJointRows; r += kWaves) {
      const int p = row_pt[r];
      if (p < 0) continue;                                        // (uniform over the wave)
      const int lo = row_lo[r];
      const double t = row_t[r], omt = 1.0 - t;
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
        row_fac[r] = -0.5 * (a.logdet[lo] + sum);
        row_bad[r] = (((int)neg & 1) || bad != 0.0 || !(fabs(a.logdet[lo]) < inf)) ? 1 : 0;
      }
    }
  } else if (tid < kJointRows) {
    row_fac[tid] = 0.0;
    row_bad[tid] = 0;
  }
  __syncthreads();

  // the quadratic form of every slice a point of the tile needs
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
    if (a.lnl) a.lnl[p] = lnl;
    if (a.chi2) a.chi2[p] = chi_out;
  }
}

}  // namespace vk
