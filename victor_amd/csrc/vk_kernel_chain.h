// vk_kernel_chain.h: the Metropolis chains of vk_chain_begin (include/victor_hip.h) on the device - part of libvictor_hip.so
// (see vk_sampled.hip for the host side, DESIGN.md section 7b for the algorithm and the measurements).
//
// One thread per chain.  The chains' state lives in device memory, structure-of-arrays (x[j][c], sum1[j][c], sum2[jk][c], ...:
// the 64 lanes of a wave touch consecutive doubles); the transition itself is vkchain::transition (vk_chain_step.h) on a strided
// view of it.  Between two step kernels the library evaluates the C rows (the fit's own data vector: the theory launch with its
// chi-square; a realisation: the theory launch and vk_like_real_kernel in pairs mode).  The step kernel reads the (lnL, chi2) of
// its chain's row, decides, accounts (accept count, moment sums and the history slot of a kept step) and writes the chain's next
// row from the increment of the following step: the base row with the sampled columns overwritten and epsilon turned into the
// Alcock-Paczynski factors by sampled_row (vk_sampled_row.h), as the best fits' rows are - with the device's pow, so a row
// with a sampled epsilon equals the host's row (libm's pow through vk_epsilon_to_ap) to rounding, any other row bit for bit.
// A proposal outside the box is not evaluated: its row carries the chain's current position and the step kernel ignores what
// comes back.  Under a Gaussian prior (a.prior.on, vk_prior.h) the step kernel decides on lnL + ln prior (transition_prior); the
// state and the history keep the log-likelihood.  With marginal histograms set (a.marg.on, vk_marginals.h) a kept step also counts
// the position the moment sums have just taken, in the histograms of the chain's problem: integer atomic increments on global memory.
#pragma once
#include "vk_common.h"
#include "vk_chain_step.h"
#include "vk_marginals.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kChainBlock = 64;            // threads per workgroup: one wave

struct ChainArgs {
  vkchain::Box box;
  int C;                    // chains
  double* x;                // [d][C]
  double* lnl;              // [C]
  double* chi2;             // [C]
  double* pivot;            // [d][C]
  double* sum1;             // [d][C]
  double* sum2;             // [d (d + 1) / 2][C]
  long long* n_accept;      // [C]
  long long* n_steps;       // [C]
  long long* n_kept;        // [C]
  const double* base;       // [C][VK_NPAR]: fixed parameters and defaults of each chain's rows (per row set)
  const int* which;         // [C]: realisation of each chain, or NULL (the fit's own data vector)
  const double* x0;         // [C][d]: starts (vk_chain_init_kernel)
  const double* res_lnl;    // [C]: results of the launch just evaluated
  const double* res_chi2;
  const double* dz;         // [C][d]: increments of the step being decided (step kernel) / proposed (propose kernel)
  const double* logu;       // [C]
  const double* dz_next;    // [C][d]: increments of the following step, or NULL: no next row (the block ends)
  double* rows;             // [C][VK_NPAR]: the next launch's rows (per row set, blocks.row_stride apart)
  int* row_which;           // [C]: realisation of each row, or NULL
  double* hist_x;           // [C][d]: history slot of this step, or NULL (not kept, or no history wanted)
  double* hist_lnl;         // [C]
  double* hist_chi2;        // [C]
  int kept;                 // this step enters the moment sums
  int adopt;                // the launch just evaluated held the start positions: take its results, no decision
  int col[vkchain::kMaxP];  // row column of each sampled parameter; VK_WALK_EPSILON: epsilon -> aperp, apar, epsilon
  double alpha;
  vkrow::Blocks blocks;     // the row sets of base and rows (one, or one per block of a joint fit) and each parameter's set
  vkprior::Prior prior;     // the Gaussian prior of the sampled parameters (vk_chain_set_prior); on == 0: none
  vkmarg::Marginals marg;   // the marginal histograms of the kept positions (vk_chain_set_marginals); on == 0: none
};

static_assert(sizeof(long long) == sizeof(int64_t), "the chain counters are 64-bit");
static_assert(sizeof(unsigned long long) == sizeof(int64_t) && vkmarg::kMaxP == vkchain::kMaxP, "the histograms count in 64 bits");

static_assert(sizeof(unsigned long) == sizeof(unsigned long long), "the atomic increment below is 64 bits wide");

// The position vkchain::accumulate has just taken for chain c, counted in the histograms of the chain's problem.  The count is
// the 64-bit atomic increment with its wrap bound at 2^64 - 1 - a plain + 1, global_atomic_inc_x2, no value returned - and not
// atomicAdd(at, 1): global_atomic_add in this library's code objects is the completion counter of the theory kernels' hand-off
// between workgroups, whose ordering tests/test_host.py checks on the shipped ISA of every kernel that contains one.  A count
// hands nothing over: nothing is read back inside the launch, and the host reads the histograms behind a stream synchronise.
__device__ __forceinline__ void chain_count(const vkmarg::Marginals& m, const vkchain::View& s, int d, int c) {
  vkmarg::count(m, d, (size_t)(c / m.group), [&](int j) { return s.x[j * s.stride]; }, [](unsigned long long* at) {
    __builtin_amdgcn_atomic_inc64(reinterpret_cast<unsigned long*>(at), ~0ul, __ATOMIC_RELAXED, "agent");
  });
}

__device__ __forceinline__ vkchain::View chain_view(const ChainArgs& a, int c) {
  vkchain::View s;
  s.stride = (size_t)a.C;
  s.x = a.x + c;
  s.lnl = a.lnl + c;
  s.chi2 = a.chi2 + c;
  s.pivot = a.pivot + c;
  s.sum1 = a.sum1 + c;
  s.sum2 = a.sum2 + c;
  s.n_accept = reinterpret_cast<int64_t*>(a.n_accept + c);
  s.n_steps = reinterpret_cast<int64_t*>(a.n_steps + c);
  s.n_kept = reinterpret_cast<int64_t*>(a.n_kept + c);
  return s;
}

// the row of chain c at x (+ dz when dz is given and x + dz is inside the box)
__device__ __forceinline__ void chain_emit(const ChainArgs& a, const vkchain::View& s, int c, const double* dz) {
  const bool move = dz != nullptr && vkchain::proposal_inside(a.box, s, dz);
  sampled_row(a.blocks, a.base, (size_t)c, a.rows, (size_t)c, a.col, a.box.d, a.alpha, [&](int j) {
    const double v = s.x[j * s.stride];
    return move ? v + dz[j] : v;
  });
  if (a.row_which) a.row_which[c] = a.which[c];
}

// fresh chains at their starts, and the rows that evaluate the starts
__global__ void __launch_bounds__(kChainBlock) vk_chain_init_kernel(ChainArgs a) {
  const int c = blockIdx.x * kChainBlock + threadIdx.x;
  if (c >= a.C) return;
  vkchain::View s = chain_view(a, c);
  vkchain::start(a.box, s, a.x0 + (size_t)c * a.box.d);
  chain_emit(a, s, c, nullptr);
}

// the first rows of a block of steps: the chains' proposals under a.dz
__global__ void __launch_bounds__(kChainBlock) vk_chain_propose_kernel(ChainArgs a) {
  const int c = blockIdx.x * kChainBlock + threadIdx.x;
  if (c >= a.C) return;
  const vkchain::View s = chain_view(a, c);
  chain_emit(a, s, c, a.dz + (size_t)c * a.box.d);
}

// one step per chain (or the adoption of the start's results), then the chain's next row
__global__ void __launch_bounds__(kChainBlock) vk_chain_step_kernel(ChainArgs a) {
  const int c = blockIdx.x * kChainBlock + threadIdx.x;
  if (c >= a.C) return;
  vkchain::View s = chain_view(a, c);
  const int d = a.box.d;
  if (a.adopt) {
    vkchain::adopt(s, a.res_lnl[c], a.res_chi2[c]);
    return;
  }
  if (a.prior.on) vkchain::transition_prior(a.box, a.prior, s, a.dz + (size_t)c * d, a.logu[c], a.res_lnl[c], a.res_chi2[c], a.kept != 0);
  else vkchain::transition(a.box, s, a.dz + (size_t)c * d, a.logu[c], a.res_lnl[c], a.res_chi2[c], a.kept != 0);
  if (a.marg.on && a.kept) chain_count(a.marg, s, d, c);
  if (a.hist_x) {
    for (int j = 0; j < d; ++j) a.hist_x[(size_t)c * d + j] = s.x[j * s.stride];
    a.hist_lnl[c] = *s.lnl;
    a.hist_chi2[c] = *s.chi2;
  }
  if (a.dz_next) chain_emit(a, s, c, a.dz_next + (size_t)c * d);
}

}  // namespace vk
