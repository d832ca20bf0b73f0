// vk_kernel_predictive.h: the posterior-predictive sums of vk_chain_set_predictive (include/victor_hip.h) on the device - part
// of libvictor_hip.so (see vk_sampled.hip for the host side, vk_predictive.h for the rules, DESIGN.md section 7b for the
// measurements).
//
// vk_chain_hold_kernel runs behind EVERY step kernel (vk_chain_begin; each half of vk_chain_begin_stretch) and before the next
// evaluation overwrites the theory vectors: accepts happen on steps that are not kept.  One wave-sized workgroup per row of the
// launch just decided (M rows: C, or C / 2 in a half-step); the workgroup of row i serves chain c = vkpred::stretch_chain(i, half,
// side).  Every lane reads n_accept[c] and seen[c]; a barrier follows, so that no lane can still be reading seen[c] when lane 0
// writes it; then, if the counter moved (or `all`: the start), the lanes stride over the N entries - consecutive lanes copy
// consecutive doubles of th[i] into held[c] - and lane 0 writes seen[c].  The decision is uniform over the workgroup.
//
// vk_chain_predict_kernel runs behind the hold of every KEPT step (a kept sweep's second half), and once behind the start's hold
// with `start` set: one thread per (problem r, entry k), ceil(N / 64) workgroups per problem, consecutive lanes on consecutive k.
// At the start it writes the pivots.  On a kept step it loops over the problem's walkers in order, adding held[c][k] about the
// pivot for the chains whose chi2 and lnL are finite, with the sums in registers between one load and one store; the thread of
// entry 0 also keeps the problem's deviance sums and its two counters.
//
// Both read what other workgroups of the step kernel (and, the second, of the hold) wrote: stream order is the only hand-off,
// the argument vk_kernel_autocorr.h makes.  Plain loads and vector stores, no atomics, no LDS beyond the barrier, no scratch.
#pragma once
#include "vk_predictive.h"
#include "vk_kernel_chain.h"

namespace vk {

struct HoldArgs {
  vkpred::Predictive p;
  const double* th;             // [M][N]: the theory vectors of the launch just decided (Sampled::d_th)
  const long long* n_accept;    // [C]: ChainArgs::n_accept
  int M;                        // rows of that launch: workgroups
  int half;                     // W / 2 of a stretch half-step; 0: a Metropolis launch, row i is chain i
  int side;                     // which half moved
  int all;                      // the start: every chain takes its row
};

struct PredictArgs {
  vkpred::Predictive p;
  const double* chi2;           // [C]: ChainArgs::chi2
  const double* lnl;            // [C]: ChainArgs::lnl
  int R;                        // problems
  int start;                    // write the pivots instead of adding
};

__global__ void __launch_bounds__(kChainBlock) vk_chain_hold_kernel(HoldArgs a) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= a.M) return;                                   // (uniform: the grid has M workgroups)
  const int c = vkpred::stretch_chain(i, a.half, a.side);
  const long long now = a.n_accept[c], seen = a.p.seen[c];
  __syncthreads();
  if (!vkpred::changed(a.all != 0, now, seen)) return;
  const int N = a.p.N;
  const double* from = a.th + (size_t)i * N;
  double* to = a.p.held + (size_t)c * N;
  for (int k = lane; k < N; k += kChainBlock) to[k] = from[k];
  if (lane == 0) a.p.seen[c] = now;
}

__global__ void __launch_bounds__(kChainBlock) vk_chain_predict_kernel(PredictArgs a) {
  const int N = a.p.N, W = a.p.group;
  const int per = (N + kChainBlock - 1) / kChainBlock;    // workgroups of a problem
  const int r = blockIdx.x / per, k = (blockIdx.x - r * per) * kChainBlock + threadIdx.x;
  if (r >= a.R || k >= N) return;
  const size_t c0 = (size_t)r * W, at = (size_t)r * N + k;
  double* dev = a.p.dev + (size_t)r * vkpred::kDeviance;
  if (a.start) {
    a.p.pivot_t[at] = vkpred::pivot_of(a.p.held[c0 * N + k]);
    if (k == 0) {
      dev[0] = vkpred::pivot_of(a.chi2[c0]);
      dev[1] = vkpred::pivot_of(a.lnl[c0]);
    }
    return;
  }
  const double pivot = a.p.pivot_t[at];
  double s1 = a.p.sum_t[at], s2 = a.p.sum_tt[at];
  long long n = 0, skipped = 0;                           // (of this launch; kept by the thread of entry 0)
  for (int w = 0; w < W; ++w) {
    const double chi2 = a.chi2[c0 + w], lnl = a.lnl[c0 + w];            // (one address per wave: a broadcast)
    if (vkpred::counts(chi2, lnl)) {
      vkpred::add(&s1, &s2, a.p.held[(c0 + w) * N + k], pivot);
      if (k == 0) vkpred::add_deviance(dev, chi2, lnl);
      n += 1;
    } else {
      skipped += 1;
    }
  }
  a.p.sum_t[at] = s1;
  a.p.sum_tt[at] = s2;
  if (k == 0) {
    a.p.n[r] += n;
    a.p.n_skipped[r] += skipped;
  }
}

}  // namespace vk
