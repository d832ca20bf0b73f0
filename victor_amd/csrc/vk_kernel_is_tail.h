// vk_kernel_is_tail.h: the tail of an importance sample on the device - per problem the K largest finite lnpost of the whole
// sample with their points, selected exactly while the chunks stream by (vk_is_set_tail / vk_is_tail, include/victor_hip.h) -
// part of libvictor_hip.so (see vk_sampled.hip for the host side, vk_is_tail.h for the order, the limits, the slices and the merge
// positions, victor_amd/importance.py rule 7 for the definition in NumPy, DESIGN.md section 7e for the mapping and the
// measurements).
//
// Per chunk of n points two launches on the context's stream, behind vk_is_max_kernel:
//   vk_is_tail_filter_kernel  the shape of vk_is_max_kernel with the chunk's rows over grid.y: a workgroup is pr problems (the
//                          problem the fastest-varying lane: a row of [n][R] and the thresholds coalesce) times 256 / pr slices
//                          of one block of rows (vkist::slice_of).  A thread walks its slice; lnpost is formed as every kernel
//                          of vk_kernel_importance.h forms it (one addition, not finite -> -inf); a value above the problem's
//                          threshold - the K-th held value, -inf while fewer than K are held - leaves its ROW in the slice's
//                          next slot of the problem's candidate array (the value is formed again by whoever reads the slot),
//                          and the slice stores its count.  In steady state a chunk adds K n / g0 candidates per problem in
//                          expectation, so this pass is one read of [n][R].
//   vk_is_tail_merge_kernel   one workgroup per problem.  It scans the slices' counts (one per thread, through LDS) and ends
//                          at once when nothing beat the threshold.  The candidates go through LDS in batches of kBatch: a
//                          batch is ranked by counting (every entry against every other, in the total order of vk_is_tail.h),
//                          then merged with the held list by positions (vk_is_tail.h: one binary search per entry) from the
//                          list's one buffer into its other - no entry is read from where another thread writes -, and the
//                          problem's side flips.  The last batch publishes the count, the side and, once K are held, the new
//                          threshold.
// The first chunks, and a K above the chunk, are the same code: the threshold is -inf until K entries are held, every finite
// value is a candidate, and the merge keeps whatever fits.  The candidate array holds `cap` = the handle's chunk rows per
// problem, which a chunk cannot exceed, and a slice's slots are the positions of its own rows; every index is bounded by n, R, K
// and cap, which vk_is_set_tail and the launch fix (a count read back is clamped to the slice's rows, a row read from a slot to
// the chunk).
// No atomics of any kind, plain vector stores, no scratch; what lies in which slot is fixed by the indices, and the held list is
// the unique sorted arrangement of its set: two runs give the same bytes.  The prior's own problem keeps no tail.
#pragma once
#include "vk_common.h"
#include "vk_importance.h"
#include "vk_is_tail.h"

namespace vk {

struct IsTailArgs {
  int n, R, K, cap;                  // the chunk's rows; problems; entries held per problem; candidate slots per problem
  int pr, gy;                        // problems of a filter workgroup; blocks of rows of the chunk (grid.y of the filter launch)
  long long g0;                      // the chunk: points g0 .. g0 + n - 1 are rows 0 .. n - 1
  const double* lnl;                 // [n][R]
  const double* lno;                 // [G]; a proposal per problem (own = R): [G][R]
  int own;                           // 0, or R: the stride of vkis::value_at, as IsArgs::own
  double* threshold;                 // [R]: the K-th held value, -inf while fewer are held
  int* count;                        // [R]: entries held
  int* side;                         // [R]: which of the two buffers holds the problem's list
  int* n_cand;                       // [kMaxSlices][R]: candidates of slice s of the chunk for problem r at s R + r
  int* cand;                         // [R][cap]: their rows, slice s's k-th at the slot of the slice's k-th row
  double* val[2];                    // [R][K]: the held values, sorted
  int* idx[2];                       // [R][K]: their points
};

// lnpost of row i for problem r: vk_kernel_importance.h's is_post, one addition
__device__ __forceinline__ double is_tail_post(const IsTailArgs& a, int i, int r) {
  double v = a.lnl[(size_t)i * a.R + r];
  v = v + a.lno[vkis::value_at(a.g0 + i, r, a.own)];
  return vkgrid::clean(v);
}

// the start of a run: nothing held, no threshold
__global__ void __launch_bounds__(vkist::kBlock) vk_is_tail_init_kernel(IsTailArgs a) {
  const int r = blockIdx.x * vkist::kBlock + threadIdx.x;
  if (r >= a.R) return;
  a.threshold[r] = vkgrid::neg_inf();
  a.count[r] = 0;
  a.side[r] = 0;
}

// grid: (problems / pr rounded up, gy)
__global__ void __launch_bounds__(vkist::kBlock) vk_is_tail_filter_kernel(IsTailArgs a) {
  const int pr = a.pr, per = vkist::slices_per_block(pr);
  const int rl = threadIdx.x % pr, sl = threadIdx.x / pr;
  const int r = blockIdx.x * pr + rl, s = blockIdx.y * per + sl;
  if (r >= a.R || (int)blockIdx.y >= a.gy) return;
  const vkist::Slice c = vkist::slice_of(a.n, pr, a.gy, s);
  const double threshold = a.threshold[r];
  int* slot = a.cand + (size_t)r * a.cap;
  int at = c.first, found = 0;                                   // the next slot of the slice: slots and rows share their positions
  for (int i = c.first; i < c.end; i += c.step) {
    if (vkist::enters(is_tail_post(a, i, r), threshold)) {
      slot[at] = i;                                              // (at <= i < n <= cap)
      at += c.step;
      found += 1;
    }
  }
  a.n_cand[(size_t)s * a.R + r] = found;
}

__global__ void __launch_bounds__(vkist::kBlock) vk_is_tail_merge_kernel(IsTailArgs a) {
  constexpr int kBlock = vkist::kBlock, kBatch = vkist::kBatch;
  __shared__ double s_v[2][kBatch];                             // a batch as it came, then sorted
  __shared__ int s_g[2][kBatch];
  __shared__ int s_scan[2][kBlock];                             // the slices' counts, then their running sums
  const int r = blockIdx.x, tid = threadIdx.x, K = a.K;
  if (r >= a.R) return;
  const int S = a.gy * vkist::slices_per_block(a.pr);           // (<= kMaxSlices <= kBlock: the launch fixes gy)
  int mine = 0;
  if (tid < S) {
    const int rows = vkist::rows_of(vkist::slice_of(a.n, a.pr, a.gy, tid));
    mine = a.n_cand[(size_t)tid * a.R + r];
    mine = mine < 0 ? 0 : (mine < rows ? mine : rows);
  }
  s_scan[0][tid] = mine;
  __syncthreads();
  int p = 0;
  for (int d = 1; d < kBlock; d <<= 1) {                        // an inclusive scan, log2(kBlock) = 8 steps: it ends in s_scan[0]
    int v = s_scan[p][tid];
    if (tid >= d) v += s_scan[p][tid - d];
    s_scan[p ^ 1][tid] = v;
    __syncthreads();
    p ^= 1;
  }
  const int* upto = s_scan[p];                                  // upto[s]: the candidates of slices 0 .. s
  const int c = upto[kBlock - 1];                               // (<= n: the slices' rows)
  if (c <= 0) return;                                           // (the whole workgroup: nothing beat the threshold)
  int h = a.count[r], side = a.side[r] & 1;
  h = h < 0 ? 0 : (h < K ? h : K);
  const int* cand = a.cand + (size_t)r * a.cap;
  for (int c0 = 0; c0 < c; c0 += kBatch) {
    const int b = c - c0 < kBatch ? c - c0 : kBatch;
    for (int k = tid; k < b; k += kBlock) {
      const int e = c0 + k;
      int lo = 0, hi = S - 1;                                   // the slice of candidate e: the first s with upto[s] > e
      while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (upto[mid] > e) hi = mid;
        else lo = mid + 1;
      }
      const vkist::Slice sc = vkist::slice_of(a.n, a.pr, a.gy, lo);
      int at = sc.first + (e - (lo ? upto[lo - 1] : 0)) * sc.step;
      at = at < 0 ? 0 : (at < a.n ? at : a.n - 1);
      int i = cand[at];
      i = i < 0 ? 0 : (i < a.n ? i : a.n - 1);
      s_v[0][k] = is_tail_post(a, i, r);
      s_g[0][k] = (int)(a.g0 + i);
    }
    __syncthreads();
    for (int k = tid; k < b; k += kBlock) {
      const double v = s_v[0][k];
      const int g = s_g[0][k];
      int rank = 0;
      for (int j = 0; j < b; ++j) rank += vkist::precedes(s_v[0][j], s_g[0][j], v, g) ? 1 : 0;
      s_v[1][rank] = v;                                         // (no two entries share a g: the ranks are 0 .. b - 1, each once)
      s_g[1][rank] = g;
    }
    __syncthreads();
    const double* from_v = a.val[side] + (size_t)r * K;
    const int* from_g = a.idx[side] + (size_t)r * K;
    double* to_v = a.val[side ^ 1] + (size_t)r * K;
    int* to_g = a.idx[side ^ 1] + (size_t)r * K;
    for (int j = tid; j < h; j += kBlock) {
      const double v = from_v[j];
      const int g = from_g[j];
      const int at = j + vkist::preceding(b, v, g, [&](int m, double& vm, int& gm) { vm = s_v[1][m]; gm = s_g[1][m]; });
      if (at < K) {
        to_v[at] = v;
        to_g[at] = g;
      }
    }
    for (int k = tid; k < b; k += kBlock) {
      const double v = s_v[1][k];
      const int g = s_g[1][k];
      const int at = k + vkist::preceding(h, v, g, [&](int m, double& vm, int& gm) { vm = from_v[m]; gm = from_g[m]; });
      if (at < K) {
        to_v[at] = v;
        to_g[at] = g;
      }
    }
    h = h + b < K ? h + b : K;
    side ^= 1;
    __syncthreads();                                            // the list just written is the next batch's source, the LDS its own
  }
  if (tid != 0) return;
  a.count[r] = h;
  a.side[r] = side;
  if (h == K) a.threshold[r] = a.val[side][(size_t)r * K + K - 1];
}

}  // namespace vk
