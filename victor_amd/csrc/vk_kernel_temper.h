// vk_kernel_temper.h: replica exchange on the chains of vk_chain_begin_tempered (include/victor_hip.h) - part of libvictor_hip.so
// (see vk_sampled.hip for the host side, DESIGN.md section 7b for the algorithm).
//
// Chain c = (r K + k) W + w is problem r, rung k, walker w (vk_temper_step.h).  vk_chain_step_tempered_kernel is
// vk_chain_step_kernel (vk_kernel_chain.h) with the tempered transition at the chain's own beta and, on a kept step, the energy
// sums thermodynamic integration reads: one thread per chain, the same structure-of-arrays state, the same history slots,
// histograms and next rows.  vk_chain_swap_kernel runs behind it on a swap step: one thread per candidate pair (r, k, w), the
// pair's two chains W doubles apart in every per-chain array, so the 64 lanes of a wave - neighbouring walkers of a rung, then
// the next pair of rungs - read and write consecutive doubles.  A chain belongs to at most one pair of an event (the lower rungs
// of an event share a parity), so the threads of a launch touch disjoint state: no atomics, no LDS, no evaluation.  On a swap step
// the step kernel writes no next row (dz_next == NULL): vk_chain_propose_kernel follows the swap and forms it from the exchanged
// state.
#pragma once
#include "vk_kernel_chain.h"
#include "vk_temper_step.h"

namespace vk {

struct TemperArgs {
  const double* betas;      // [K]: 1 = betas[0] > ... > betas[K - 1] >= 0
  int K, W;                 // rungs, walkers: C = R K W
  double* pivot_e;          // [C]: the energy sums of vk_temper_step.h
  double* e1;               // [C]
  double* e2;               // [C]
  long long* n_e;           // [C]
  long long* n_swap_try;    // [C]: counted on the lower chain of a pair
  long long* n_swap_acc;    // [C]
};

struct TemperStepArgs {
  ChainArgs c;
  TemperArgs t;
};

struct SwapArgs {
  int C, d;
  double* x;                // [d][C]
  double* lnl;              // [C]
  double* chi2;             // [C]
  TemperArgs t;
  const double* logs;       // [C]: the event's acceptance levels; a pair reads its lower chain's
  int parity;               // the lower rungs of the event: k = parity (mod 2)
  int pairs;                // candidate pairs of a ladder at this parity (vktemper::pairs_of), >= 1
  int n;                    // threads: R * pairs * W
};

// one tempered step per chain, then the chain's next row unless a swap follows
__global__ void __launch_bounds__(kChainBlock) vk_chain_step_tempered_kernel(TemperStepArgs g) {
  const ChainArgs& a = g.c;
  const int c = blockIdx.x * kChainBlock + threadIdx.x;
  if (c >= a.C) return;
  vkchain::View s = chain_view(a, c);
  const int d = a.box.d;
  const double beta = g.t.betas[vktemper::rung_of(c, g.t.K, g.t.W)];
  vktemper::transition(a.box, a.prior, s, beta, a.dz + (size_t)c * d, a.logu[c], a.res_lnl[c], a.res_chi2[c], a.kept != 0);
  if (a.kept) {
    vktemper::Energy e{g.t.pivot_e + c, g.t.e1 + c, g.t.e2 + c, reinterpret_cast<int64_t*>(g.t.n_e + c)};
    vktemper::energy_add(e, *s.lnl);
  }
  if (a.marg.on && a.kept) chain_count(a.marg, s, d, c);
  if (a.hist_x) {
    for (int j = 0; j < d; ++j) a.hist_x[(size_t)c * d + j] = s.x[j * s.stride];
    a.hist_lnl[c] = *s.lnl;
    a.hist_chi2[c] = *s.chi2;
  }
  if (a.dz_next) chain_emit(a, s, c, a.dz_next + (size_t)c * d);
}

// one candidate pair per thread: thread i is walker i % W of pair (i / W) % pairs of problem i / (W pairs)
__global__ void __launch_bounds__(kChainBlock) vk_chain_swap_kernel(SwapArgs a) {
  const int i = blockIdx.x * kChainBlock + threadIdx.x;
  if (i >= a.n) return;
  const int W = a.t.W, K = a.t.K;
  const int w = i % W, q = (i / W) % a.pairs, r = i / (W * a.pairs);
  const int k = a.parity + 2 * q;                           // k + 1 < K by the count of pairs
  const int lo = (r * K + k) * W + w, hi = lo + W;          // hi <= (r K + K - 1) W + w < C
  vkchain::View s{}, u{};
  s.stride = u.stride = (size_t)a.C;
  s.x = a.x + lo;
  s.lnl = a.lnl + lo;
  s.chi2 = a.chi2 + lo;
  u.x = a.x + hi;
  u.lnl = a.lnl + hi;
  u.chi2 = a.chi2 + hi;
  vktemper::swap_pair(a.d, s, u, a.t.betas[k], a.t.betas[k + 1], a.logs[lo], reinterpret_cast<int64_t*>(a.t.n_swap_try + lo),
                      reinterpret_cast<int64_t*>(a.t.n_swap_acc + lo));
}

}  // namespace vk
