// vk_is_predict.h - the tile and index rules and the term arithmetic of the posterior-predictive sums of an importance sample
// (vk_is_set_predictive / vk_is_predictive, include/victor_hip.h; victor_amd/importance.py states the definition in NumPy,
// DESIGN.md section 7e the kernel mapping).  Header-only and free of HIP, like vk_importance.h: the kernel of
// vk_kernel_is_predict.h calls it, and tests/test_importance_predictive.py compiles it on its own under g++ (-ffp-contract=off)
// against the NumPy statement.
//
// Per chunk of n points the weights w [n][R] of the step (vk_importance.h) and the points' theory vectors T [n][N] - of a joint
// handle N_b entries of block segment b - give, per problem r and entry k, about the pivot vector (the theory vector of kept
// point 0 where finite, else 0; shared by all problems):
//   pt[k][r]  = pt[k][r] f_r  + sum_i w[i][r] v[i][k]              v = T - pivot
//   ptt[k][r] = ptt[k][r] f_r + sum_i (w[i][r] v[i][k]) v[i][k]
// and the four deviance sums of the problem about pivots of its own (chi2 and lnL of kept point 0 for problem r where finite,
// else 0): w a, (w a) a, w b, (w b) b with a = chi2 - pivot_chi2[r], b = lnl - pivot_lnl[r].  f_r is the chunk's rescale factor,
// applied ONCE to each (every term is linear in w).  A point with w == 0 adds nothing, so no NaN of a failed point reaches a sum.
// Every product and difference is rounded on its own (fp contract(off)), so NumPy, g++ and hipcc form the same terms from the
// same w and T; the ORDER of the additions is the mapping's and fixed:
//   lanes    a wave's 64 lanes hold pr problems (the power of two >= R, at most 64; the problem the fastest-varying lane, so a row
//            of [n][R] coalesces) times 64 / pr entry groups, each lane a tile of kTile consecutive entries: at R >= 64 a
//            workgroup covers 64 problems x kTile entries, at R = 1 one problem x 64 kTile entries; a lane that has no
//            problem or whose tile lies past N adds with `on` false and stores nothing
//   slices   the workgroup's kSlices waves take the chunk's rows in kSlices contiguous slices, slice s the rows
//            slice_begin(n, s) .. slice_begin(n, s + 1) - 1 in increasing order from zero; the partial sums are then added in
//            slice order, ((p0 + p1) + p2) + p3, and that sum to the rescaled accumulator: acc f + p.
#pragma once
#include "vk_grid.h"

namespace vkisp {

constexpr int kWave = 64;
constexpr int kSlices = 4;             // waves of a workgroup: slices of the chunk
constexpr int kBlock = kWave * kSlices;
constexpr int kTile = 4;               // entries of a lane (two accumulators each)
constexpr int kAhead = 8;              // rows whose loads a wave keeps in flight
constexpr int kDeviance = 4;           // sums of a problem: w a, (w a) a, w b, (w b) b
constexpr int kMaxEntries = 1 << 17;   // entries of a segment (a theory vector): its entry tiles are a launch's grid.y

// problems of a wave: the power of two >= R, at most 64 (the max kernel's pr)
VK_GRID_HD inline int problems_per_wave(int R) {
  int pr = 1;
  while (pr < kWave && pr < R) pr *= 2;
  return pr;
}
VK_GRID_HD inline int groups(int pr) { return kWave / pr; }                       // entry groups of a wave
VK_GRID_HD inline int entries_per_block(int pr) { return groups(pr) * kTile; }
VK_GRID_HD inline int entry_tiles(int N, int pr) { return (N + entries_per_block(pr) - 1) / entries_per_block(pr); }
VK_GRID_HD inline int problem_tiles(int R, int pr) { return (R + pr - 1) / pr; }
// what a lane holds: its problem (>= R: none) and the first entry of its tile (entries k .. k + kTile - 1 below N)
VK_GRID_HD inline int problem_of(int rtile, int pr, int lane) { return rtile * pr + lane % pr; }
VK_GRID_HD inline int first_entry(int etile, int pr, int lane) { return (etile * groups(pr) + lane / pr) * kTile; }
// the first row of slice s of a chunk of n rows (s = kSlices: n)
VK_GRID_HD inline int slice_begin(int n, int s) { return (int)((long long)n * s / kSlices); }

VK_GRID_HD inline double pivot_of(double v) { return __builtin_isfinite(v) ? v : 0.0; }

// One point's terms into a pair of sums: v = t - pivot, s1 += w v, s2 += (w v) v - if `on` (the point's w > 0), else nothing:
// the terms are formed either way and SELECTED, so a loop over rows has no branch to wait for, and what a point of weight 0
// holds (NaN, inf) is never added.  (A partial sum starts at +0.0 and is never -0.0, so adding +0.0 changes no bit.)
VK_GRID_HD inline void add(double& s1, double& s2, bool on, double w, double t, double pivot) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double v = t - pivot;
  const double wv = w * v;
  const double wvv = wv * v;
  s1 = s1 + (on ? wv : 0.0);
  s2 = s2 + (on ? wvv : 0.0);
}

// the partial sums of the slices in slice order, then onto the rescaled accumulator
VK_GRID_HD inline double combine(double acc, double factor, const double* part, int stride) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double p = part[0];
  for (int s = 1; s < kSlices; ++s) p = p + part[(long long)s * stride];
  const double scaled = acc * factor;
  return scaled + p;
}

}  // namespace vkisp
