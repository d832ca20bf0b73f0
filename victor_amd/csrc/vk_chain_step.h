// vk_chain_step.h - one chain's Metropolis step behind vk_chain_begin (include/victor_hip.h): given the chain's state, the
// proposal increment and acceptance level of the step and the (lnL, chi2) its row evaluated to, decide, move and account.
// Header-only and free of HIP: vk_kernel_chain.h calls it from one thread per chain, and tests/test_chains.py compiles it on
// its own under g++ and drives it on analytic functions against a NumPy restatement.
//
// The rules (victor_amd/chains.py states them in NumPy; that loop is the definition):
//   prop = x + dz;  a proposal outside the box [lo, hi] was evaluated at the chain's current position (so that every launch
//   has one row per chain, the rule of vk_walk_run), its result is discarded and it reads lnL = -inf;
//   accept  <=>  logu < lnL' - lnL   with IEEE semantics (a NaN difference - both -inf, or a NaN lnL' - rejects);
//   on accept x, lnL, chi2 are replaced.  A NaN lnL at the start is stored as -inf, as the likelihood returns a failed row.
// A KEPT step (the caller decides: step >= burn and (step - burn) % thin == 0) adds the position after the decision to the
// chain's moment sums about its pivot p (its start): n, sum (x_j - p_j), sum (x_j - p_j)(x_k - p_k) for j <= k, plain double sums
// in step order.
//
// Bits: the decision arithmetic is one addition per parameter, two comparisons per parameter, one subtraction and one
// comparison - nothing a compiler could contract into an fma, so hipcc and g++ take the same decisions from the same inputs.
// The moment sums hold products: a compiler may contract them, which removes roundings (tests/test_chains.py bounds them
// against extended precision, it does not compare them bit for bit).
//
// Layout: a chain's state is addressed through a View - element j of a per-parameter array sits at [j * stride] - so the same
// code serves the device's structure-of-arrays state (stride = number of chains: the 64 lanes of a wave touch consecutive
// doubles) and a test's single chain (stride 1).  Nothing here indexes a local array, so the device code needs no scratch.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "vk_prior.h"

#if defined(__HIPCC__)
#define VK_CHAIN_HD __host__ __device__
#else
#define VK_CHAIN_HD
#endif

namespace vkchain {

constexpr int kMaxP = 10;              // sampled parameters, as vkfit::kMaxP
constexpr int kBlock = 64;             // steps whose random numbers travel together (EnsembleMetropolis.BLOCK)
static_assert(vkprior::kMaxP == kMaxP, "a prior covers the sampled parameters");

struct Box {
  int d;
  double lo[kMaxP], hi[kMaxP];
};

// one chain inside (possibly strided) storage; the pointers address the chain's own first element
struct View {
  size_t stride;
  double* x;                 // [d]
  double* lnl;               // lnL and chi-square at x
  double* chi2;
  double* pivot;             // [d]
  double* sum1;              // [d]
  double* sum2;              // [d (d + 1) / 2]: (j, k), j <= k, at tri(d, j, k)
  int64_t* n_accept;
  int64_t* n_steps;
  int64_t* n_kept;
};

VK_CHAIN_HD inline double neg_inf() { return -__builtin_inf(); }

// position of (j, k), j <= k, in the packed upper triangle of a d x d matrix, row by row
VK_CHAIN_HD inline int tri(int d, int j, int k) { return j * d - j * (j - 1) / 2 + (k - j); }

VK_CHAIN_HD inline int n_tri(int d) { return d * (d + 1) / 2; }

VK_CHAIN_HD inline double stored(double lnl) { return lnl != lnl ? neg_inf() : lnl; }

VK_CHAIN_HD inline bool in_box(const Box& b, const double* x) {
  bool in = true;
  for (int j = 0; j < b.d; ++j) in = in && x[j] >= b.lo[j] && x[j] <= b.hi[j];      // (a NaN is outside)
  return in;
}

// is x + dz inside the box?  (a NaN is outside)
VK_CHAIN_HD inline bool proposal_inside(const Box& b, const View& s, const double* dz) {
  bool in = true;
  for (int j = 0; j < b.d; ++j) {
    const double p = s.x[j * s.stride] + dz[j];
    in = in && p >= b.lo[j] && p <= b.hi[j];
  }
  return in;
}

// a fresh chain at x0 (inside the box: the caller checks it); its lnL and chi-square follow with adopt()
VK_CHAIN_HD inline void start(const Box& b, View& s, const double* x0) {
  for (int j = 0; j < b.d; ++j) {
    s.x[j * s.stride] = x0[j];
    s.pivot[j * s.stride] = x0[j];
    s.sum1[j * s.stride] = 0.0;
  }
  for (int i = 0; i < n_tri(b.d); ++i) s.sum2[i * s.stride] = 0.0;
  *s.lnl = neg_inf();
  *s.chi2 = __builtin_inf();
  *s.n_accept = 0;
  *s.n_steps = 0;
  *s.n_kept = 0;
}

// the start's own evaluation
VK_CHAIN_HD inline void adopt(View& s, double lnl_row, double chi2_row) {
  *s.lnl = stored(lnl_row);
  *s.chi2 = chi2_row;
}

VK_CHAIN_HD inline void accumulate(const Box& b, View& s) {
  const size_t st = s.stride;
  for (int j = 0; j < b.d; ++j) {
    const double dj = s.x[j * st] - s.pivot[j * st];
    s.sum1[j * st] += dj;
    for (int k = j; k < b.d; ++k) {
      const double dk = s.x[k * st] - s.pivot[k * st];
      s.sum2[tri(b.d, j, k) * st] += dj * dk;
    }
  }
  *s.n_kept += 1;
}

// One step: dz [d] and logu of this step, (lnl_row, chi2_row) what the chain's row of the launch evaluated to (the proposal if
// it was inside the box, else the current position: ignored).  Returns whether the proposal was accepted.
VK_CHAIN_HD inline bool transition(const Box& b, View& s, const double* dz, double logu, double lnl_row, double chi2_row, bool kept) {
  const bool in = proposal_inside(b, s, dz);
  const double lnl_prop = in ? lnl_row : neg_inf();
  const bool accept = logu < lnl_prop - *s.lnl;            // false for a NaN difference
  if (accept) {
    for (int j = 0; j < b.d; ++j) s.x[j * s.stride] = s.x[j * s.stride] + dz[j];
    *s.lnl = lnl_prop;
    *s.chi2 = chi2_row;
    *s.n_accept += 1;
  }
  *s.n_steps += 1;
  if (kept) accumulate(b, s);
  return accept;
}

// One step under a Gaussian prior (vk_prior.h) multiplied onto the box: the posterior decides,
//   accept  <=>  logu < (lnL' + lp') - (lnL + lp)
// with lp' the prior at the proposal x + dz and lp the prior recomputed at the current position - one addition on each side, one
// subtraction and one comparison.  The state still holds the log-LIKELIHOOD of the chain's position.  A proposal outside the box
// reads lnL' = -inf as in transition(), and -inf plus a finite lp' is -inf; a NaN lnL' rejects.  Without a prior (pr.on == 0)
// this is transition().
VK_CHAIN_HD inline bool transition_prior(const Box& b, const vkprior::Prior& pr, View& s, const double* dz, double logu,
                                         double lnl_row, double chi2_row, bool kept) {
  if (!pr.on) return transition(b, s, dz, logu, lnl_row, chi2_row, kept);
  const bool in = proposal_inside(b, s, dz);
  const double lnl_prop = in ? lnl_row : neg_inf();
  const double lp_prop = vkprior::lnprior(pr, b.d, [&](int j) { return s.x[j * s.stride] + dz[j]; });
  const double lp = vkprior::lnprior(pr, b.d, [&](int j) { return s.x[j * s.stride]; });
  const double post_prop = lnl_prop + lp_prop, post = *s.lnl + lp;
  const bool accept = logu < post_prop - post;             // false for a NaN difference
  if (accept) {
    for (int j = 0; j < b.d; ++j) s.x[j * s.stride] = s.x[j * s.stride] + dz[j];
    *s.lnl = lnl_prop;
    *s.chi2 = chi2_row;
    *s.n_accept += 1;
  }
  *s.n_steps += 1;
  if (kept) accumulate(b, s);
  return accept;
}

// "kept" as victor_amd/chains.py defines it, over the whole life of a chain
VK_CHAIN_HD inline bool is_kept(int64_t step, int64_t burn, int64_t thin) { return step >= burn && (step - burn) % thin == 0; }

}  // namespace vkchain
