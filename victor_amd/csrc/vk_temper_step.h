// vk_temper_step.h - replica exchange (parallel tempering) on the chains of vk_chain_begin_tempered (include/victor_hip.h): the
// tempered Metropolis step of one chain, the energy sums thermodynamic integration reads, and the exchange of two neighbouring
// rungs.  Header-only and free of HIP, like vk_chain_step.h: vk_kernel_temper.h calls it from one thread per chain (step) and one
// thread per candidate pair (swap), and tests/test_tempering.py compiles it on its own under g++ against the NumPy statement of
// victor_amd/tempering.py, which is the definition.
//
// Layout: chain c = (r K + k) W + w is problem r, rung k, walker w; rung k samples  L^beta_k x prior  with
// 1 = beta_0 > beta_1 > ... > beta_(K-1) >= 0.  The W ladders of a problem never interact.
//
// The tempered step (transition): with lnL' = the row's value inside the box, -inf outside (vk_chain_step.h),
//   post' = beta * lnL' (+ lp'),   post = beta * lnL (+ lp)      each product and each sum rounded on its own,
//   accept  <=>  the proposal is inside the box  and  logu < post' - post           (a NaN difference rejects),
// lp' and lp the Gaussian prior (vk_prior.h) at the proposal and recomputed at the current position.  1 * v == v exactly, so at
// beta = 1 this is vkchain::transition / transition_prior bit for bit.  At beta = 0 without a prior post' - post = 0 - 0 for every
// finite pair: every proposal inside the box with a finite lnL' is accepted; 0 * -inf and 0 * NaN are NaN, so a row that failed
// is never moved onto.  THE DEAD END: a chain whose STORED lnL is -inf at beta = 0 has post = NaN and never moves by a step
// (a swap can still carry the state to a colder rung, where -inf loses to anything finite).  State, history and chi2 keep the
// log-LIKELIHOOD; accept counts and moment sums are vkchain's.
//
// The energy sums (energy_add): at every KEPT step, after the decision and before any swap, a chain whose stored lnL is finite
// counts it: n_e += 1; the first such value becomes pivot_e; a = lnL - pivot_e; e1 += a; e2 += a * a (the product rounded before
// the sum).  <lnL>_beta and Var(lnL)_beta of a rung follow on the host from the sums of its W chains.
//
// The swap (swap_pair): a swap event follows the step with life-long index s when swap_every > 0 and (s + 1) % swap_every == 0;
// event e = (s + 1) / swap_every - 1 has parity e % 2 and pairs rung k with rung k + 1, walker for walker, for every
// k = parity, parity + 2, ... with k + 1 < K:
//   accept  <=>  logs < (beta_k - beta_(k+1)) * (lnL_(k+1) - lnL_k)     one subtraction each, one product; a NaN rejects,
// logs the entry of the LOWER rung's chain.  On accept x, lnL and chi2 are exchanged (the untempered prior cancels in the ratio);
// temperatures, pivots, moment sums, energy sums and counters stay with the rung.  The lower chain counts n_swap_try, n_swap_acc.
//
// Bits: every product that feeds a sum or a difference sits under `fp contract(off)` (hipcc; the CPU tests build with
// -ffp-contract=off), so hipcc, g++ and NumPy take the same decisions and form the same sums from the same inputs.
#pragma once

#include "vk_chain_step.h"

namespace vktemper {

// the energy sums and swap counters of one chain: pointers to the chain's own elements
struct Energy {
  double* pivot_e;
  double* e1;
  double* e2;
  int64_t* n_e;
};

// rung of chain c in the layout above
VK_CHAIN_HD inline int rung_of(int c, int K, int W) { return (c / W) % K; }

// does a swap event follow the step with life-long index `step`?  (swap_every == 0: never)
VK_CHAIN_HD inline bool is_swap(int64_t step, int64_t swap_every) { return swap_every > 0 && (step + 1) % swap_every == 0; }

// ... and its parity: the lower rungs k of its pairs are k = parity (mod 2)
VK_CHAIN_HD inline int swap_parity(int64_t step, int64_t swap_every) { return (int)(((step + 1) / swap_every - 1) % 2); }

// candidate pairs per ladder at a parity: the k = parity, parity + 2, ... with k + 1 < K
VK_CHAIN_HD inline int pairs_of(int K, int parity) { return K - parity > 0 ? (K - parity) / 2 : 0; }

// post' - post of the decision
VK_CHAIN_HD inline double gain(double beta, double lnl_prop, double lnl, bool with_prior, double lp_prop, double lp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double post_prop = beta * lnl_prop;
  double post = beta * lnl;
  if (with_prior) {
    post_prop = post_prop + lp_prop;
    post = post + lp;
  }
  return post_prop - post;
}

// One tempered step of a chain at inverse temperature beta; arguments and return as vkchain::transition_prior.
VK_CHAIN_HD inline bool transition(const vkchain::Box& b, const vkprior::Prior& pr, vkchain::View& s, double beta, const double* dz,
                                   double logu, double lnl_row, double chi2_row, bool kept) {
  const bool in = vkchain::proposal_inside(b, s, dz);
  const double lnl_prop = in ? lnl_row : vkchain::neg_inf();
  double lp_prop = 0.0, lp = 0.0;
  if (pr.on) {
    lp_prop = vkprior::lnprior(pr, b.d, [&](int j) { return s.x[j * s.stride] + dz[j]; });
    lp = vkprior::lnprior(pr, b.d, [&](int j) { return s.x[j * s.stride]; });
  }
  const bool accept = in && logu < gain(beta, lnl_prop, *s.lnl, pr.on != 0, lp_prop, lp);      // false for a NaN difference
  if (accept) {
    for (int j = 0; j < b.d; ++j) s.x[j * s.stride] = s.x[j * s.stride] + dz[j];
    *s.lnl = lnl_prop;
    *s.chi2 = chi2_row;
    *s.n_accept += 1;
  }
  *s.n_steps += 1;
  if (kept) vkchain::accumulate(b, s);
  return accept;
}

// the stored lnL of a kept step enters the chain's energy sums
VK_CHAIN_HD inline void energy_add(const Energy& e, double lnl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!__builtin_isfinite(lnl)) return;                     // -inf (and a NaN, which is never stored): not counted
  if (*e.n_e == 0) *e.pivot_e = lnl;
  *e.n_e += 1;
  const double a = lnl - *e.pivot_e;
  const double a2 = a * a;
  *e.e1 = *e.e1 + a;
  *e.e2 = *e.e2 + a2;
}

// the decision of a swap between rung k (lnl_lo, beta_lo) and rung k + 1 (lnl_hi, beta_hi)
VK_CHAIN_HD inline bool swap_accepts(double beta_lo, double beta_hi, double lnl_lo, double lnl_hi, double logs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double db = beta_lo - beta_hi;
  const double dl = lnl_hi - lnl_lo;
  const double g = db * dl;
  return logs < g;                                          // false for a NaN
}

// One candidate pair: `lo` the chain of rung k, `hi` the chain of rung k + 1 (same problem, same walker), both views of the same
// strided state.  Returns whether the states were exchanged.
VK_CHAIN_HD inline bool swap_pair(int d, vkchain::View& lo, vkchain::View& hi, double beta_lo, double beta_hi, double logs,
                                  int64_t* n_swap_try, int64_t* n_swap_acc) {
  *n_swap_try += 1;
  if (!swap_accepts(beta_lo, beta_hi, *lo.lnl, *hi.lnl, logs)) return false;
  for (int j = 0; j < d; ++j) {
    const double t = lo.x[j * lo.stride];
    lo.x[j * lo.stride] = hi.x[j * hi.stride];
    hi.x[j * hi.stride] = t;
  }
  const double l = *lo.lnl, c = *lo.chi2;
  *lo.lnl = *hi.lnl;
  *lo.chi2 = *hi.chi2;
  *hi.lnl = l;
  *hi.chi2 = c;
  *n_swap_acc += 1;
  return true;
}

}  // namespace vktemper
