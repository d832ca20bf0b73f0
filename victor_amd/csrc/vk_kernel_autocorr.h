// vk_kernel_autocorr.h: the ensemble series of vk_chain_set_autocorr (include/victor_hip.h) on the device - part of
// libvictor_hip.so (see vk_sampled.hip for the host side, vk_autocorr.h for the statistic, DESIGN.md section 7b for the
// measurements).
//
// vk_chain_series_kernel runs behind the step kernel of every kept step (vk_chain_begin) and behind the second half's step
// kernel of every kept sweep (vk_chain_begin_stretch), on the handle's stream: the positions it sums were written by other
// threads and other workgroups of that step kernel, and stream order is the only hand-off between workgroups - the argument
// vk_kernel_stretch.h makes for the proposals of a half-step.  One wave-sized workgroup per series (problem r, parameter j),
// R d workgroups:
//   phase 1   the series value: lane l sums x[j][r W + w] over w = l, l + 64, ... (consecutive lanes read consecutive doubles),
//             then the xor butterfly of vk_autocorr.h with __shfl_xor - cross-lane moves, no LDS allocated, no barrier;
//   phase 2   the lanes stride over the lags 0 .. min(n, L - 1): each adds its product to its own acc[k], reading ring slots
//             that earlier launches wrote; lane 0 then writes the pivot (step 0), the sum, head[n] and ring[n mod L] - a slot no
//             lag of this step reads.
// Plain loads and vector stores, no atomics: nothing is handed over inside the launch.  The step count n is a kernel argument.
#pragma once
#include "vk_autocorr.h"
#include "vk_kernel_chain.h"

namespace vk {

struct SeriesArgs {
  vkac::Autocorr ac;        // group, max_lag, n and the state of the R d series
  const double* x;          // [d][C]: the chains' positions (ChainArgs::x)
  int C;                    // chains
  int d;                    // sampled parameters
};

static_assert(kChainBlock == vkac::kLanes, "one wave per series: the butterfly spans the workgroup");

__global__ void __launch_bounds__(kChainBlock) vk_chain_series_kernel(SeriesArgs a) {
  const int series = blockIdx.x, lane = threadIdx.x;
  const int r = series / a.d, j = series - r * a.d;
  const int W = a.ac.group, L = a.ac.max_lag;
  const double* xj = a.x + (size_t)j * a.C + (size_t)r * W;
  double v = vkac::lane_partial(W, lane, [&](int w) { return xj[w]; });
  for (int off = vkac::kLanes / 2; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  const long long n = a.ac.n;
  const double val = vkac::value(v, a.ac.pivot[series], n);
  const int slot = (int)(n % L), top = vkac::top_lag(n, L);
  const size_t at = (size_t)series * L;
  for (int k = lane; k <= top; k += vkac::kLanes) vkac::lag(a.ac.acc + at, a.ac.ring + at, val, slot, k, L);
  if (lane == 0) vkac::store(a.ac.pivot + series, a.ac.total + series, a.ac.head + at, a.ac.ring + at, v, val, n, slot, L);
}

}  // namespace vk
