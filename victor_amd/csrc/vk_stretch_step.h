// vk_stretch_step.h - one walker's half-step of the affine-invariant stretch move (Goodman & Weare 2010, the two-half parallel
// form of victor_amd.sampler.EnsembleStretch) behind vk_chain_begin_stretch (include/victor_hip.h): form the proposal from the
// walker and its partner, and - given the (lnL, chi2) the walker's row evaluated to - decide, move and account.  Header-only and
// free of HIP, like vk_chain_step.h, whose Box, View, accumulate and is_kept it uses: vk_kernel_stretch.h calls it from one
// thread per moving walker, and tests/test_stretch.py compiles it on its own under g++ and drives it on analytic functions
// against a NumPy restatement.
//
// The rules (victor_amd/chains.py states them in NumPy; that loop is the definition).  An ensemble of W walkers (W even) is split
// into half 0 (walkers w < W / 2) and half 1; a sweep moves half 0 against half 1, then half 1 against the updated half 0.  For
// one moving walker at x with partner p (a walker of the other half of the same problem), stretch z, lz = (d - 1) log z (formed
// on the host) and acceptance level logu:
//   prop = p + z (x - p);  a proposal outside the box [lo, hi] was evaluated at the walker's current position, its result is
//   discarded and it reads lnL = -inf (the rule of vk_chain_step.h: every launch has one row per moving walker);
//   accept  <=>  logu < (lz + lnL') - lnL   with IEEE semantics (a NaN on the right rejects);
//   on accept x, lnL, chi2 are replaced.
// A walker's position after its own half-step is its position at the end of the sweep (the other half does not move it), so a
// KEPT sweep adds it to the walker's moment sums right there (vkchain::accumulate).
//
// Bits: z (x - p) is a product that feeds an addition - the one place where a compiler may contract to an fma and change the
// proposal's last bit.  propose() forbids it (hipcc: the pragma below; the CPU tests build with -ffp-contract=off) and is the
// ONLY place the proposal is formed: the caller stores what it returns, builds the row from it and hands the same numbers to
// transition().  The decision is two additions and a comparison.
#pragma once

#include "vk_chain_step.h"

namespace vkchain {

// prop[j * prop_stride] = p_j + z (x_j - p_j), j < d: x the moving walker (s), p its partner (element j at partner[j * s.stride],
// the same storage).  Returns whether the proposal lies inside the box (a NaN is outside).
VK_CHAIN_HD inline bool propose(const Box& b, const View& s, const double* partner, double z, double* prop, size_t prop_stride) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool in = true;
  for (int j = 0; j < b.d; ++j) {
    const double p = partner[j * s.stride];
    const double step = z * (s.x[j * s.stride] - p);
    const double v = p + step;
    prop[j * prop_stride] = v;
    in = in && v >= b.lo[j] && v <= b.hi[j];
  }
  return in;
}

// is the stored proposal inside the box?  (comparisons only: the same answer wherever it is asked)
VK_CHAIN_HD inline bool stored_inside(const Box& b, const double* prop, size_t prop_stride) {
  bool in = true;
  for (int j = 0; j < b.d; ++j) {
    const double v = prop[j * prop_stride];
    in = in && v >= b.lo[j] && v <= b.hi[j];
  }
  return in;
}

// One half-step of one moving walker: prop as propose() stored it, lz = (d - 1) log z and logu of this half-step, (lnl_row,
// chi2_row) what the walker's row of the launch evaluated to (the proposal if it was inside the box, else the current position:
// ignored).  kept: the sweep enters the moment sums.  Returns whether the proposal was accepted.
VK_CHAIN_HD inline bool stretch_transition(const Box& b, View& s, const double* prop, size_t prop_stride, double lz, double logu,
                                           double lnl_row, double chi2_row, bool kept) {
  const bool in = stored_inside(b, prop, prop_stride);
  const double lnl_prop = in ? lnl_row : neg_inf();
  const double gain = lz + lnl_prop;
  const bool accept = logu < gain - *s.lnl;                // false for a NaN
  if (accept) {
    for (int j = 0; j < b.d; ++j) s.x[j * s.stride] = prop[j * prop_stride];
    *s.lnl = lnl_prop;
    *s.chi2 = chi2_row;
    *s.n_accept += 1;
  }
  *s.n_steps += 1;
  if (kept) accumulate(b, s);
  return accept;
}

// The half-step under a Gaussian prior (vk_prior.h): accept  <=>  logu < (lz + (lnL' + lp')) - (lnL + lp), lp' the prior at the
// STORED proposal (formed only by propose()), lp the prior recomputed at the walker's position.  Outside the box lnL' = -inf as
// above.  Without a prior (pr.on == 0) this is stretch_transition().
VK_CHAIN_HD inline bool stretch_transition_prior(const Box& b, const vkprior::Prior& pr, View& s, const double* prop, size_t prop_stride,
                                                 double lz, double logu, double lnl_row, double chi2_row, bool kept) {
  if (!pr.on) return stretch_transition(b, s, prop, prop_stride, lz, logu, lnl_row, chi2_row, kept);
  const bool in = stored_inside(b, prop, prop_stride);
  const double lnl_prop = in ? lnl_row : neg_inf();
  const double lp_prop = vkprior::lnprior(pr, b.d, [&](int j) { return prop[j * prop_stride]; });
  const double lp = vkprior::lnprior(pr, b.d, [&](int j) { return s.x[j * s.stride]; });
  const double post_prop = lnl_prop + lp_prop, post = *s.lnl + lp;
  const double gain = lz + post_prop;
  const bool accept = logu < gain - post;                  // false for a NaN
  if (accept) {
    for (int j = 0; j < b.d; ++j) s.x[j * s.stride] = prop[j * prop_stride];
    *s.lnl = lnl_prop;
    *s.chi2 = chi2_row;
    *s.n_accept += 1;
  }
  *s.n_steps += 1;
  if (kept) accumulate(b, s);
  return accept;
}

}  // namespace vkchain
