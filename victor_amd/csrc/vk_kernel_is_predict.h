// vk_kernel_is_predict.h: the posterior-predictive sums of an importance sample (vk_is_set_predictive, include/victor_hip.h) on
// the device - part of libvictor_hip.so (see vk_sampled.hip for the host side, vk_is_predict.h for the tile and index rules and
// the terms, victor_amd/importance.py for the definition in NumPy, DESIGN.md section 7e for the mapping and the measurements).
//
// vk_is_predict_kernel runs once per chunk behind vk_is_accumulate_kernel - of a joint handle once per block segment, on the
// lead stream behind the join of the blocks' streams - and forms the tall-skinny product of what the chunk left resident: the
// weights w [n][R] (which, with predictive on, vk_is_weight_kernel writes to an array of their own, so that the evaluation's
// chi-squares survive) and the segment's theory vectors T [n][N].
//   grid.x   tiles of pr problems (vkisp::problems_per_wave)
//   grid.y   tiles of 64 / pr x kTile entries, and - in the launch that keeps them - one more workgroup for the deviance sums
//   a lane   a problem and a tile of kTile entries: 2 kTile partial sums in registers.  At R >= 64 (kWide) the 64 lanes are 64
//            problems, their loads of a row of w coalesce, and the tile's entries are the same for the whole wave: their
//            addresses are formed from wave-uniform values only, so the theory values can travel as scalar operands; at
//            smaller R the lanes cover (problem, entry group) pairs, so a wave is busy at R = 1 too
//   a wave   one of the kSlices contiguous slices of the chunk's rows, in increasing order, kAhead rows at a time: the loads of
//            kAhead rows are issued before their terms are added, and the terms are selected, not branched on (vkisp::add), so
//            a wave waits for memory once per kAhead rows
//   combine  the waves' partial sums meet in LDS (kSlices x 2 kTile x 64 doubles, 16 KiB) and are added in slice order onto the
//            accumulator rescaled by the chunk's factor (vkisp::combine), each wave combining its share of the tile's entries
// The chunk that holds kept point 0 (`first`) takes the pivots - every lane from row 0 itself, the lanes of problem 0 store them
// - and starts its accumulators from zero, so a handle may run again.  A weight of zero selects zero terms: no NaN of a failed
// point can reach a sum.  No atomics, no scratch, plain vector stores; the order of the additions is fixed by the indices, so
// two runs give the same bytes.  Every index is bounded by n, R and N, which vk_is_set_predictive and the launch check; a lane
// without a problem reads problem R - 1, a tile past the end entry N - 1, and neither stores.
#pragma once
#include "vk_common.h"
#include "vk_is_predict.h"

namespace vk {

struct IsPredictArgs {
  int n, R, N, pr;                   // the chunk's rows; problems; entries of this segment; problems of a wave
  int first;                         // the chunk holds kept point 0: take the pivots, start from zero
  int deviance;                      // this launch keeps the deviance sums as well (grid.y has one workgroup more)
  const double* w;                   // [n][R]: the chunk's weights
  const double* th;                  // [n][N]: the segment's theory vectors
  const double* chi2;                // [n][R]
  const double* lnl;                 // [n][R]
  const vkgrid::Running* run;        // [R]: the chunk's rescale factors
  double* pivot_t;                   // [N]: the segment's part of the pivot vector
  double* pt;                        // [N][R]: the segment's rows of sum w v
  double* ptt;                       // [N][R]: ... of sum (w v) v
  double* pivots;                    // [2][R]: pivot_chi2 | pivot_lnl
  double* dev;                       // [kDeviance][R]
};

// kWide: pr == 64, a wave's lanes are 64 problems of one entry tile
template <bool kWide>
__global__ void __launch_bounds__(vkisp::kBlock) vk_is_predict_kernel(IsPredictArgs a) {
  constexpr int kTile = vkisp::kTile, kWave = vkisp::kWave, kSlices = vkisp::kSlices, kAhead = vkisp::kAhead;
  constexpr int kPart = 2 * kTile * kWave;                    // doubles of a slice's partial sums
  static_assert(kTile % kSlices == 0 && vkisp::kDeviance <= 2 * kTile, "each wave combines kTile / kSlices entries of a tile");
  __shared__ double s_part[kSlices * kPart];
  const int lane = threadIdx.x % kWave;
  const int slice = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);      // (wave-uniform, and known to be)
  const int pr = kWide ? kWave : a.pr, R = a.R, N = a.N;
  const int r = vkisp::problem_of(blockIdx.x, pr, lane);
  const bool has = r < R;
  const int rr = has ? r : R - 1;                             // (what a lane without a problem reads; it adds and stores nothing)
  const int i0 = vkisp::slice_begin(a.n, slice), i1 = vkisp::slice_begin(a.n, slice + 1);
  double* mine = s_part + slice * kPart + lane;               // partial sum j of this lane at mine[j kWave]
  const double factor = a.run[rr].factor;

  if ((int)blockIdx.y >= vkisp::entry_tiles(N, pr)) {
    // the deviance sums: the lanes of entry group 0, one problem each
    const bool work = has && lane < pr;
    const double pa = a.first ? vkisp::pivot_of(a.chi2[rr]) : a.pivots[rr];
    const double pb = a.first ? vkisp::pivot_of(a.lnl[rr]) : a.pivots[R + rr];
    double s[vkisp::kDeviance] = {0.0, 0.0, 0.0, 0.0};
    auto row = [&](double w, double chi2, double lnl) {
      vkisp::add(s[0], s[1], work && w > 0.0, w, chi2, pa);
      vkisp::add(s[2], s[3], work && w > 0.0, w, lnl, pb);
    };
    int i = i0;
    for (; i + kAhead <= i1; i += kAhead) {
      double w[kAhead], c[kAhead], l[kAhead];
#pragma unroll
      for (int b = 0; b < kAhead; ++b) {
        const size_t at = (size_t)(i + b) * R + rr;
        w[b] = a.w[at];
        c[b] = a.chi2[at];
        l[b] = a.lnl[at];
      }
#pragma unroll
      for (int b = 0; b < kAhead; ++b) row(w[b], c[b], l[b]);
    }
    for (; i < i1; ++i) {
      const size_t at = (size_t)i * R + rr;
      row(a.w[at], a.chi2[at], a.lnl[at]);
    }
#pragma unroll
    for (int j = 0; j < vkisp::kDeviance; ++j) mine[j * kWave] = s[j];
    __syncthreads();
    if (!work || slice != 0) return;
#pragma unroll
    for (int j = 0; j < vkisp::kDeviance; ++j) {
      double* slot = a.dev + (size_t)j * R + r;
      *slot = vkisp::combine(a.first ? 0.0 : *slot, factor, s_part + j * kWave + lane, kPart);
    }
    if (a.first) {
      a.pivots[r] = pa;
      a.pivots[R + r] = pb;
    }
    return;
  }

  // the tile's first entry: of a wide launch the same for every lane of the workgroup
  const int k0 = kWide ? (int)blockIdx.y * kTile : vkisp::first_entry(blockIdx.y, pr, lane);
  int kk[kTile];                                               // (clamped: a tile past the end reads entry N - 1 and stores nothing)
  double piv[kTile], s1[kTile], s2[kTile];
#pragma unroll
  for (int u = 0; u < kTile; ++u) {
    kk[u] = k0 + u < N ? k0 + u : N - 1;
    piv[u] = a.first ? vkisp::pivot_of(a.th[kk[u]]) : a.pivot_t[kk[u]];
    s1[u] = s2[u] = 0.0;
  }
  const double* wcol = a.w + rr;
  int i = i0;
  for (; i + kAhead <= i1; i += kAhead) {
    double w[kAhead], tv[kAhead][kTile];
#pragma unroll
    for (int b = 0; b < kAhead; ++b) {
      w[b] = wcol[(size_t)(i + b) * R];
      const double* t = a.th + (size_t)(i + b) * N;
#pragma unroll
      for (int u = 0; u < kTile; ++u) tv[b][u] = t[kk[u]];
    }
#pragma unroll
    for (int b = 0; b < kAhead; ++b) {
      const bool on = has && w[b] > 0.0;
#pragma unroll
      for (int u = 0; u < kTile; ++u) vkisp::add(s1[u], s2[u], on, w[b], tv[b][u], piv[u]);
    }
  }
  for (; i < i1; ++i) {
    const double w = wcol[(size_t)i * R];
    const double* t = a.th + (size_t)i * N;
    const bool on = has && w > 0.0;
#pragma unroll
    for (int u = 0; u < kTile; ++u) vkisp::add(s1[u], s2[u], on, w, t[kk[u]], piv[u]);
  }
#pragma unroll
  for (int u = 0; u < kTile; ++u) {
    mine[u * kWave] = s1[u];
    mine[(kTile + u) * kWave] = s2[u];
  }
  __syncthreads();
  // wave `slice` combines entries slice, slice + kSlices, ... of every lane's tile
#pragma unroll
  for (int u = 0; u < kTile; ++u) {
    if (u % kSlices != slice || !has || k0 + u >= N) continue;
    const size_t at = (size_t)(k0 + u) * R + r;
    a.pt[at] = vkisp::combine(a.first ? 0.0 : a.pt[at], factor, s_part + u * kWave + lane, kPart);
    a.ptt[at] = vkisp::combine(a.first ? 0.0 : a.ptt[at], factor, s_part + (kTile + u) * kWave + lane, kPart);
    if (a.first && r == 0) a.pivot_t[k0 + u] = piv[u];
  }
}

}  // namespace vk
