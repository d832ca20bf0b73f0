// vk_kernel_fit.h: the bounded Nelder-Mead search of vk_fit_run (include/victor_hip.h) on the device - part of libvictor_hip.so
// (see vk_sampled.hip for the host side, DESIGN.md section 7a for the algorithm and the measurements).
//
// One thread per problem.  The search's state lives in device memory (vkfit::State, one per problem); between two of these
// kernels the library evaluates the S rows of every active problem (the fit's own data vector: the theory launch with its
// chi-square; a realisation: the theory launch and vk_like_real_kernel in pairs mode).  The step kernel reads those S
// (lnL, chi2) pairs, applies vkfit::transition and writes the problem's next S rows - the base row with the sampled columns
// overwritten and epsilon turned into the Alcock-Paczynski factors (sampled_row, vk_sampled_row.h) - and, against realisations,
// each row's realisation index.  Rows of launch position k are rows k S .. k S + S - 1; the host keeps the list of active
// problems (in problem order) and, when it shrinks, lays the rows out again with vk_fit_emit_kernel.  Under a Gaussian prior
// (a.prior.on, vk_prior.h) the value handed to vkfit::transition for a live slot is lnL + ln prior at the slot's point: the search
// and its State are unchanged, f is minus the log-posterior.
#pragma once
#include "vk_common.h"
#include "vk_fit_simplex.h"
#include "vk_prior.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kFitBlock = 64;

struct FitArgs {
  vkfit::Params q;
  vkfit::State* state;      // [n_problems]
  const double* base;       // [n_problems][VK_NPAR]: fixed parameters and defaults of each problem's rows (per row set)
  const double* x0;         // [n_problems][d]: starts (vk_fit_init_kernel)
  const int* active;        // [n_active]: problem at each launch position (NULL: position = problem)
  int n_active;
  const double* lnl;        // [n_active * S] results of the launch just evaluated
  const double* chi2;
  double* rows;             // [n_active * S][VK_NPAR]: the next launch's rows (per row set, blocks.row_stride apart)
  int* row_which;           // [n_active * S]: realisation of each row, or NULL (the fit's own data vector)
  const int* which;         // [n_problems]: realisation of each problem, or NULL
  int* status;              // [n_problems]: -1 while the problem runs, then its VK_FIT_* status
  int col[vkfit::kMaxP];    // row column of each sampled parameter; VK_WALK_EPSILON: epsilon -> aperp, apar, epsilon
  double alpha;
  vkrow::Blocks blocks;     // the row sets of base and rows (one, or one per block of a joint fit) and each parameter's set
  vkprior::Prior prior;     // the Gaussian prior of the sampled parameters (vk_fit_set_prior); on == 0: none
  double* post;             // [n_active * S]: with a prior, lnL + ln prior of each live row (the results buffer itself: lnl == post)
};
static_assert(vkprior::kMaxP == vkfit::kMaxP, "a prior covers the sampled parameters");

__device__ __forceinline__ void fit_emit(const FitArgs& a, const vkfit::State& s, int p, int k) {
  const int S = a.q.S;
  for (int slot = 0; slot < S; ++slot) {
    const size_t r = (size_t)k * S + slot;
    sampled_row(a.blocks, a.base, (size_t)p, a.rows, r, a.col, a.q.d, a.alpha, [&](int j) { return s.pt[slot][j]; });
    if (a.row_which) a.row_which[r] = a.which[p];
  }
}

// the start simplex of every problem (launch position = problem)
__global__ void __launch_bounds__(kFitBlock) vk_fit_init_kernel(FitArgs a) {
  const int p = blockIdx.x * kFitBlock + threadIdx.x;
  if (p >= a.n_active) return;
  vkfit::State& s = a.state[p];
  vkfit::start(s, a.q, a.x0 + (size_t)p * a.q.d);
  a.status[p] = -1;
  fit_emit(a, s, p, p);
}

// one transition per active problem, then its next rows at its launch position
__global__ void __launch_bounds__(kFitBlock) vk_fit_step_kernel(FitArgs a) {
  const int k = blockIdx.x * kFitBlock + threadIdx.x;
  if (k >= a.n_active) return;
  const int p = a.active[k];
  vkfit::State& s = a.state[p];
  if (s.phase == vkfit::kDone) return;
  const int S = a.q.S;
  if (a.prior.on) {
    // the search maximises the posterior: a live slot's value becomes lnL + lp(pt[slot]), written over the result it came from
    // (global memory: no local array, no scratch); chi2 stays the chi-square of the row
    for (int slot = 0; slot < S; ++slot)
      if (s.live[slot]) {
        const size_t r = (size_t)k * S + slot;
        a.post[r] = a.post[r] + vkprior::lnprior(a.prior, a.q.d, [&](int j) { return s.pt[slot][j]; });
      }
  }
  vkfit::transition(s, a.q, a.lnl + (size_t)k * S, a.chi2 + (size_t)k * S);
  if (s.phase == vkfit::kDone) {
    a.status[p] = s.status;
    return;
  }
  fit_emit(a, s, p, k);
}

// the pending rows of the active problems at their new launch positions (after the host has dropped finished problems)
__global__ void __launch_bounds__(kFitBlock) vk_fit_emit_kernel(FitArgs a) {
  const int k = blockIdx.x * kFitBlock + threadIdx.x;
  if (k >= a.n_active) return;
  const int p = a.active[k];
  fit_emit(a, a.state[p], p, k);
}

}  // namespace vk
