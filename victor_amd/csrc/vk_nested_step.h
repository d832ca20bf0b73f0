// vk_nested_step.h - nested sampling behind vk_nested_begin (include/victor_hip.h): the total order of a problem's live points
// and the rank of one, the range of the live set, the survivor a replacement walker starts from, the constrained step of one
// walker and its commit into the slot of a dead point.  Header-only and free of HIP, like vk_chain_step.h: vk_kernel_nested.h
// calls it from one workgroup per problem (select) and one thread per walker (step, commit), and tests/test_nested.py compiles
// it on its own under g++ against the NumPy statement of victor_amd/nested.py, which is the definition.
//
// Layout: a problem has L live points, K of which are replaced per iteration (K divides L, K <= L / 2) by K walkers that take
// S constrained steps each; row r K + k of every launch is walker k of problem r.
//
// One iteration of one problem:
//   range_j = max_i x_ij - min_i x_ij over all L live points                              comparisons and one subtraction;
//   the K live points smallest in (lnL, index) - a total order: lnL is never NaN (a NaN is stored as -inf), ties go to the
//   smaller index - are the dead points 0 .. K - 1 in that order, L* = lnL of dead point K - 1;
//   walker k starts at survivor number  min(floor(pick_k (L - K)), L - K - 1)  of the L - K survivors in increasing index and
//   takes its x, lnL, chi2;
//   a step:  prop_j = y_j + (scale range_j) dz_j      each product and the sum rounded on its own (`fp contract(off)`);
//   a proposal outside the box [lo, hi] was evaluated at the walker's current position and is discarded (the chains' rule);
//   accept  <=>  the proposal is inside the box  and  lnL' > L*                           strict; a NaN lnL' rejects;
//   after step S walker k's (y, lnL, chi2) replaces dead point k in its slot, and a walker that never moved counts in n_stuck.
//
// Bits: the decision arithmetic is two products, one sum and comparisons, the products under `fp contract(off)` (hipcc; the CPU
// tests build with -ffp-contract=off): hipcc, g++ and NumPy take the same decisions from the same inputs.
//
// Under a Gaussian prior (vk_prior.h; the second forms of transition and commit below) the run still samples the uniform box and
// orders, kills and constrains on lnpost = lnL + ln prior, ONE rounded addition (-inf + finite is -inf): before() and rank_of()
// are used unchanged on lnpost, L* is the lnpost of dead point K - 1, a walker carries the ln prior of its position beside lnL
// and chi2, and a step accepts  <=>  inside the box  and  lnL' + lnprior(prop) > L*, ln prior taken at exactly the values
// proposed() produces and the acceptance stores.
//
// Nothing here indexes a local array (ranges and live values are read through callables or strided pointers), so the device
// code needs no scratch.
#pragma once

#include "vk_chain_step.h"
#include "vk_prior.h"

namespace vknest {

constexpr int kMaxP = vkchain::kMaxP;  // sampled parameters
constexpr int kMaxLive = 4096;         // live points of a problem: their lnL fit the select kernel's LDS
constexpr int kBlock = 8;              // iterations whose random numbers travel together (victor_amd.nested.BLOCK)

enum Status { kOk = 0, kMaxIter = 1, kNoFinite = 2 };

// one walker inside (possibly strided) storage; the pointers address the walker's own first element
struct Walker {
  size_t stride;
  double* y;                 // [d]
  double* lnl;               // lnL and chi-square at y
  double* chi2;
  int64_t* n_accept;
  int64_t* n_steps;
  int64_t* n_stuck;
  int32_t* moved;            // accepted steps of the current iteration
  double* lnprior;           // ln prior at y (runs under a prior; not read otherwise)
};

// (la, ia) before (lb, ib) in the total order of live points
VK_CHAIN_HD inline bool before(double la, int ia, double lb, int ib) { return la < lb || (la == lb && ia < ib); }

// live points before point i: i's rank (0: the lowest).  lnl(m): the lnL of live point m
template <class Lnl>
VK_CHAIN_HD inline int rank_of(int L, int i, Lnl lnl) {
  const double li = lnl(i);
  int n = 0;
  for (int m = 0; m < L; ++m) n += before(lnl(m), m, li, i) ? 1 : 0;
  return n;
}

// max - min of one parameter over the live points.  x(i): the parameter of live point i
template <class X>
VK_CHAIN_HD inline double range_of(int L, X x) {
  double lo = x(0), hi = lo;
  for (int i = 1; i < L; ++i) {
    const double v = x(i);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  return hi - lo;
}

// which of the L - K survivors (in increasing index) a pick u in [0, 1) names
VK_CHAIN_HD inline int pick_of(double u, int L, int K) {
  const int n = L - K;
  int q = (int)(u * (double)n);
  q = q < 0 ? 0 : q;
  return q > n - 1 ? n - 1 : q;
}

// the live index of survivor number q.  rank(i): the rank of live point i (a survivor has rank >= K)
template <class Rank>
VK_CHAIN_HD inline int survivor_of(int L, int K, int q, Rank rank) {
  int seen = 0;
  for (int i = 0; i < L; ++i) {
    if (rank(i) < K) continue;
    if (seen == q) return i;
    ++seen;
  }
  return -1;                                               // (q < L - K: not reached)
}

VK_CHAIN_HD inline double proposed(double y, double scale, double range, double dz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double w = scale * range;
  const double s = w * dz;
  return y + s;
}

// is the walker's proposal under dz inside the box?  (a NaN is outside.)  range(j): the live range of parameter j
template <class Range>
VK_CHAIN_HD inline bool proposal_inside(const vkchain::Box& b, const Walker& w, double scale, Range range, const double* dz) {
  bool in = true;
  for (int j = 0; j < b.d; ++j) {
    const double p = proposed(w.y[j * w.stride], scale, range(j), dz[j]);
    in = in && p >= b.lo[j] && p <= b.hi[j];
  }
  return in;
}

// walker k of an iteration starts at a survivor: its x(j), lnL and chi2
template <class X>
VK_CHAIN_HD inline void start(int d, Walker& w, X x, double lnl, double chi2) {
  for (int j = 0; j < d; ++j) w.y[j * w.stride] = x(j);
  *w.lnl = lnl;
  *w.chi2 = chi2;
  *w.moved = 0;
}

// One constrained step: dz [d] of this step, (lnl_row, chi2_row) what the walker's row of the launch evaluated to (the proposal
// if it was inside the box, else the current position: ignored).  Returns whether the proposal was accepted.
template <class Range>
VK_CHAIN_HD inline bool transition(const vkchain::Box& b, Walker& w, double scale, Range range, const double* dz, double lstar,
                                   double lnl_row, double chi2_row) {
  const bool in = proposal_inside(b, w, scale, range, dz);
  const double lnl_prop = in ? lnl_row : vkchain::neg_inf();
  const bool accept = in && lnl_prop > lstar;              // strict; false for a NaN
  if (accept) {
    for (int j = 0; j < b.d; ++j) w.y[j * w.stride] = proposed(w.y[j * w.stride], scale, range(j), dz[j]);
    *w.lnl = lnl_prop;
    *w.chi2 = chi2_row;
    *w.n_accept += 1;
    *w.moved += 1;
  }
  *w.n_steps += 1;
  return accept;
}

// ... under a prior: the decision is taken on lnL' + ln prior at the proposal, one rounded addition
template <class Range>
VK_CHAIN_HD inline bool transition(const vkchain::Box& b, const vkprior::Prior& prior, Walker& w, double scale, Range range,
                                   const double* dz, double lstar, double lnl_row, double chi2_row) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool in = proposal_inside(b, w, scale, range, dz);
  const double lnl_prop = in ? lnl_row : vkchain::neg_inf();
  const double lp = vkprior::lnprior(prior, b.d, [&](int j) { return proposed(w.y[j * w.stride], scale, range(j), dz[j]); });
  const double post = lnl_prop + lp;
  const bool accept = in && post > lstar;                  // strict; false for a NaN
  if (accept) {
    for (int j = 0; j < b.d; ++j) w.y[j * w.stride] = proposed(w.y[j * w.stride], scale, range(j), dz[j]);
    *w.lnl = lnl_prop;
    *w.chi2 = chi2_row;
    *w.lnprior = lp;
    *w.n_accept += 1;
    *w.moved += 1;
  }
  *w.n_steps += 1;
  return accept;
}

// after step S: the walker replaces its dead point.  x: the slot's first element in the live points' storage, live_stride apart
VK_CHAIN_HD inline void commit(int d, Walker& w, double* x, size_t live_stride, double* lnl, double* chi2) {
  for (int j = 0; j < d; ++j) x[j * live_stride] = w.y[j * w.stride];
  *lnl = *w.lnl;
  *chi2 = *w.chi2;
  if (*w.moved == 0) *w.n_stuck += 1;
}

// ... under a prior: its ln prior goes into the slot with the rest
VK_CHAIN_HD inline void commit(int d, Walker& w, double* x, size_t live_stride, double* lnl, double* chi2, double* lnprior) {
  commit(d, w, x, live_stride, lnl, chi2);
  *lnprior = *w.lnprior;
}

}  // namespace vknest
