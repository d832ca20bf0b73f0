// vk_kernel_stretch.h: the stretch-move ensembles of vk_chain_begin_stretch (include/victor_hip.h) on the device - part of
// libvictor_hip.so (see vk_sampled.hip for the host side, DESIGN.md section 7b for the algorithm and the measurements).
//
// The C chains of a handle are R = C / W ensembles of W walkers, walker c = r W + w, in the state arrays of vk_kernel_chain.h.
// A sweep is two half-steps; half-step h moves the M = C / 2 walkers r W + h W/2 + m (m < W/2) against partners from the other
// half of the same ensemble, one thread per MOVING walker: thread i serves ensemble i / (W/2), member i % (W/2), and row i of the
// launch is its row.  Per half-step three things are enqueued on the handle's stream, in this order:
//   vk_stretch_propose_kernel   prop = p + z (x - p) (vkchain::propose: formed once, stored in prop[d][M]) and the walker's row -
//                               the proposal, or outside the box the walker's current position;
//   the evaluation of the M rows (the launches the Metropolis chains make for C rows);
//   vk_stretch_step_kernel      decides on the STORED proposal (vkchain::stretch_transition; under a Gaussian prior, a.c.prior.on,
//                               stretch_transition_prior with the prior at the stored proposal), accounts (with a.c.marg.on also in
//                               the marginal histograms of the walker's problem, vk_marginals.h) and fills the history slot.
// The proposals of a half read positions that the step kernel of the other half has just written, by other threads and other
// workgroups: that is why they are formed in a launch of their own behind it, and why the step kernel writes no rows - stream
// order is the only hand-off between workgroups.
#pragma once
#include "vk_kernel_chain.h"
#include "vk_stretch_step.h"

namespace vk {

struct StretchArgs {
  ChainArgs c;              // the chains' state, base rows, results, rows and history slots; c.kept: the sweep is kept
  int half;                 // W / 2: moving walkers of one ensemble
  int side;                 // which half moves: 0 or 1
  int M;                    // C / 2: threads, rows
  const double* z;          // [M]: stretch factors of this half-step
  const double* lz;         // [M]: (d - 1) log z
  const double* logu;       // [M]
  const int* partner;       // [M]: member of the other half, in [0, W / 2): checked on the host before any launch
  double* prop;             // [d][M]: the proposals of this half-step
};

// the walker thread i moves
__device__ __forceinline__ int stretch_walker(const StretchArgs& a, int i) {
  const int r = i / a.half, m = i - r * a.half;
  return (2 * r + a.side) * a.half + m;
}

__global__ void __launch_bounds__(kChainBlock) vk_stretch_propose_kernel(StretchArgs a) {
  const int i = blockIdx.x * kChainBlock + threadIdx.x;
  if (i >= a.M) return;
  const int c = stretch_walker(a, i);
  const int p = (2 * (i / a.half) + (1 - a.side)) * a.half + a.partner[i];
  const vkchain::View s = chain_view(a.c, c);
  const size_t M = (size_t)a.M;
  const bool in = vkchain::propose(a.c.box, s, a.c.x + p, a.z[i], a.prop + i, M);
  sampled_row(a.c.blocks, a.c.base, (size_t)c, a.c.rows, (size_t)i, a.c.col, a.c.box.d, a.c.alpha,
              [&](int j) { return in ? a.prop[j * M + i] : s.x[j * s.stride]; });
  if (a.c.row_which) a.c.row_which[i] = a.c.which[c];
}

__global__ void __launch_bounds__(kChainBlock) vk_stretch_step_kernel(StretchArgs a) {
  const int i = blockIdx.x * kChainBlock + threadIdx.x;
  if (i >= a.M) return;
  const int c = stretch_walker(a, i);
  vkchain::View s = chain_view(a.c, c);
  const int d = a.c.box.d;
  if (a.c.prior.on)
    vkchain::stretch_transition_prior(a.c.box, a.c.prior, s, a.prop + i, (size_t)a.M, a.lz[i], a.logu[i], a.c.res_lnl[i],
                                      a.c.res_chi2[i], a.c.kept != 0);
  else
    vkchain::stretch_transition(a.c.box, s, a.prop + i, (size_t)a.M, a.lz[i], a.logu[i], a.c.res_lnl[i], a.c.res_chi2[i], a.c.kept != 0);
  if (a.c.marg.on && a.c.kept) chain_count(a.c.marg, s, d, c);       // (a kept sweep, in the walker's own moving half-step)
  if (a.c.hist_x) {
    for (int j = 0; j < d; ++j) a.c.hist_x[(size_t)c * d + j] = s.x[j * s.stride];
    a.c.hist_lnl[c] = *s.lnl;
    a.c.hist_chi2[c] = *s.chi2;
  }
}

}  // namespace vk
