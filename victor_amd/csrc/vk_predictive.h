// vk_predictive.h - the posterior-predictive sums behind vk_chain_set_predictive (include/victor_hip.h): per problem, the sum
// and the sum of squares of the THEORY VECTOR at the kept positions of the problem's W chains (walkers), and of chi2 and lnL
// there - what the posterior band of the model drawn through the data, the mean chi-square quoted beside it and the deviance
// information criterion are read from when no history is kept.  Header-only and free of HIP, like vk_chain_step.h and
// vk_autocorr.h: the two kernels of vk_kernel_predictive.h call it, and tests/test_predictive.py compiles it on its own under g++
// against a NumPy restatement (victor_amd/predictive.py states the same rules; that statement is the definition).
//
// A problem r owns `group` chains, c = r group + w.  State of a problem: pivot_t[N], sum_t[N], sum_tt[N]; dev[6] = pivot_chi2,
// pivot_lnl, s_chi2, s_chi2sq, s_lnl, s_lnlsq; the counters n and n_skipped.  State of a chain: held[N], the theory vector at
// the chain's CURRENT position, and seen, the value of the chain's accept counter when held was last brought up to date.
//
// Hold.  The theory vector of every proposal is in memory when its step is decided (th[rows][N]) and overwritten one launch
//   later.  After the start's evaluation held[c] = th[row of c] and seen[c] = n_accept[c] for every chain (hold with all).  After
//   every decision: n_accept[c] != seen[c]  =>  held[c] = th[row of c], seen[c] = n_accept[c] (changed).  The accept counter is
//   the hand-off: the step kernels know nothing of this header.  A rejected proposal, and one outside the box (whose row carries
//   the chain's current position and is never accepted), leaves held alone.  Row of c: c in a Metropolis launch; in half-step
//   `side` of a stretch sweep row i serves walker stretch_chain(i, half, side), half = group / 2.
// Pivot.  At the start pivot_t[r][k] = held[r group][k] if finite, else 0; pivot_chi2 and pivot_lnl the same way from the start
//   of chain r group (pivot_of).
// Accumulate, on a kept step, or on a kept sweep after its second half - the moment the series of vk_autocorr.h is taken.  For
//   w = 0 .. group - 1 in that order, with c = r group + w: if chi2[c] and lnl[c] are both finite (counts),
//     v = held[c][k] - pivot_t[k];  sum_t[k] += v;  sum_tt[k] += v v   for every k (add),
//     the four deviance sums likewise about their pivots (add_deviance), n += 1;
//   otherwise n_skipped += 1 and nothing is summed.
// All sums are plain doubles in (step, walker) order: a run does not depend on how it is cut into blocks.
//
// Bits: v v feeds a sum, which a compiler may contract into an fma and so remove a rounding; the tests bound the sums against
// extended precision, they do not compare them bit for bit (as the moment sums of vk_chain_step.h).
//
// Memory: (C + 3 R) N doubles, 6 R doubles, C + 2 R 64-bit counters - C = 65536 chains of 8 walkers at N = 120: 87 MB.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VK_PRED_HD __host__ __device__
#else
#define VK_PRED_HD
#endif

namespace vkpred {

constexpr int kDeviance = 6;           // pivot_chi2, pivot_lnl, s_chi2, s_chi2sq, s_lnl, s_lnlsq

struct Predictive {
  int on;                              // 0: none (nothing else is read)
  int group;                           // W: chains per problem, chain c belongs to problem c / group
  int N;                               // entries of a theory vector
  double* pivot_t;                     // [R][N]
  double* sum_t;                       // [R][N]
  double* sum_tt;                      // [R][N]
  double* held;                        // [C][N]
  double* dev;                         // [R][6]
  long long* n;                        // [R]
  long long* n_skipped;                // [R]
  long long* seen;                     // [C]
};

// doubles and 64-bit counters of a handle's state, in the order of the struct
inline size_t state_doubles(size_t C, size_t R, size_t N) { return (C + 3 * R) * N + kDeviance * R; }
inline size_t state_counters(size_t C, size_t R) { return C + 2 * R; }

// the walker that row i of half-step `side` serves: ensemble i / half, member i % half of the moving half (vk_kernel_stretch.h);
// half == 0: a Metropolis launch, row i is chain i
VK_PRED_HD inline int stretch_chain(int i, int half, int side) {
  if (half == 0) return i;
  const int r = i / half, m = i - r * half;
  return (2 * r + side) * half + m;
}

// does the chain's held vector need its row of the launch just decided?
VK_PRED_HD inline bool changed(bool all, long long n_accept, long long seen) { return all || n_accept != seen; }

VK_PRED_HD inline bool finite(double v) { return v - v == 0.0; }       // (false for a NaN and for either infinity)

VK_PRED_HD inline double pivot_of(double v) { return finite(v) ? v : 0.0; }

// does the chain's position enter the sums of a kept step?
VK_PRED_HD inline bool counts(double chi2, double lnl) { return finite(chi2) && finite(lnl); }

// one entry of one chain's held vector into the problem's sums
VK_PRED_HD inline void add(double* sum_t, double* sum_tt, double held, double pivot) {
  const double v = held - pivot;
  *sum_t += v;
  *sum_tt += v * v;
}

// one chain's chi2 and lnL into the problem's deviance sums
VK_PRED_HD inline void add_deviance(double* dev, double chi2, double lnl) {
  const double a = chi2 - dev[0], b = lnl - dev[1];
  dev[2] += a;
  dev[3] += a * a;
  dev[4] += b;
  dev[5] += b * b;
}

// ---- the same rules over whole arrays, one thing after the other: what the kernels do with a thread per entry ----------------

// the hold behind a launch of M rows: th [M][N], n_accept [C]
inline void hold(const Predictive& p, const double* th, const long long* n_accept, int M, int half, int side, bool all) {
  for (int i = 0; i < M; ++i) {
    const int c = stretch_chain(i, half, side);
    if (!changed(all, n_accept[c], p.seen[c])) continue;
    for (int k = 0; k < p.N; ++k) p.held[(size_t)c * p.N + k] = th[(size_t)i * p.N + k];
    p.seen[c] = n_accept[c];
  }
}

// the pivots of R problems from the held vectors and the state of each problem's first chain
inline void pivots(const Predictive& p, const double* chi2, const double* lnl, int R) {
  for (int r = 0; r < R; ++r) {
    const size_t c = (size_t)r * p.group;
    for (int k = 0; k < p.N; ++k) p.pivot_t[(size_t)r * p.N + k] = pivot_of(p.held[c * p.N + k]);
    p.dev[(size_t)r * kDeviance + 0] = pivot_of(chi2[c]);
    p.dev[(size_t)r * kDeviance + 1] = pivot_of(lnl[c]);
  }
}

// one kept step (one kept sweep) of R problems
inline void accumulate(const Predictive& p, const double* chi2, const double* lnl, int R) {
  for (int r = 0; r < R; ++r)
    for (int w = 0; w < p.group; ++w) {
      const size_t c = (size_t)r * p.group + w;
      if (!counts(chi2[c], lnl[c])) {
        p.n_skipped[r] += 1;
        continue;
      }
      for (int k = 0; k < p.N; ++k)
        add(p.sum_t + (size_t)r * p.N + k, p.sum_tt + (size_t)r * p.N + k, p.held[c * p.N + k], p.pivot_t[(size_t)r * p.N + k]);
      add_deviance(p.dev + (size_t)r * kDeviance, chi2[c], lnl[c]);
      p.n[r] += 1;
    }
}

}  // namespace vkpred
