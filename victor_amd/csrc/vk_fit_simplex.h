// vk_fit_simplex.h - one problem's step of the bounded Nelder-Mead search behind vk_fit_run (include/victor_hip.h): given the
// problem's state and the log-likelihoods of the S rows its last launch evaluated, take the decision, move the simplex and lay
// out the points of its next launch.  Header-only and free of HIP: vk_kernel_fit.h calls it from one thread per problem, and
// tests/test_best_fit.py compiles it on its own under g++ and drives it on analytic functions.
//
// The rules are those of Lagarias et al. (1998), as scipy.optimize's Nelder-Mead takes them: minimise f = -lnL over the d
// sampled parameters, vertices v_0 .. v_d sorted by f (ties by vertex index), centroid c of the best d, candidates
//   r = c + (c - v_d),  e = c + 2 (c - v_d),  oc = c + (c - v_d) / 2,  ic = c - (c - v_d) / 2
// and the decision of decide() below.  All four candidates travel in ONE launch (speculation): a problem owns
// S = max(4, d + 1) row slots and every launch is an init (the d + 1 start vertices), a candidate (r, e, oc, ic) or a shrink
// (the d shrunk vertices) launch.  The trajectory is textbook Nelder-Mead evaluated one point at a time, up to the rounding of lnL.
//
// Bits: every product here is by 2 or 1/2 (exact), the centroid is a sum and a division, the rest are additions and comparisons -
// nothing a compiler could contract into an fma, so hipcc and g++ produce the same bits from the same inputs.
#pragma once

#include <stdint.h>

#include "victor_hip.h"

#if defined(__HIPCC__)
#define VK_FIT_HD __host__ __device__
#else
#define VK_FIT_HD
#endif

namespace vkfit {

constexpr int kMaxP = 10;              // sampled parameters: the row columns other than aperp / apar / epsilon, plus epsilon
constexpr int kMaxS = kMaxP + 1;       // row slots per problem: max(4, d + 1)

// phases: what the rows of the pending launch hold
constexpr int kInit = 0, kCand = 1, kShrink = 2, kDone = 3;
// candidate slots
constexpr int kR = 0, kE = 1, kOC = 2, kIC = 3;
// decisions (the test compares them launch by launch with a NumPy restatement)
enum Decision { kVertices = 0, kExpand, kReflect, kOutside, kInside, kShrunk, kRestart, kConverged, kMaxIter, kNoFiniteStart };

// what is shared by every problem of a run
struct Params {
  int d, S;
  int max_iter, restarts;
  double ftol;
  double lo[kMaxP], hi[kMaxP], step[kMaxP], xtol[kMaxP];
};

// one problem (device memory in vk_fit_run; one thread reads and writes it)
struct State {
  int32_t phase, status, iter, restarts_left;
  int32_t live[kMaxS];        // slot s of the pending launch holds a point the search uses (else a copy of v_0, value ignored)
  int64_t n_evals;            // rows whose value the search used
  double f[kMaxS];            // f = -lnL of each vertex (+inf: failed or outside the box)
  double chi[kMaxS];          // chi-square of each vertex
  double v[kMaxS][kMaxP];     // vertices, sorted by f
  double pt[kMaxS][kMaxP];    // points of the pending launch's slots
  double x0[kMaxP];           // the problem's start
};

VK_FIT_HD inline int slots(int d) { return d + 1 > 4 ? d + 1 : 4; }

VK_FIT_HD inline double inf() { return __builtin_inf(); }

VK_FIT_HD inline bool in_box(const Params& q, const double* x) {
  bool in = true;
  for (int j = 0; j < q.d; ++j) in = in && x[j] >= q.lo[j] && x[j] <= q.hi[j];      // (a NaN is outside)
  return in;
}

VK_FIT_HD inline void copy(double* dst, const double* src, int d) {
  for (int j = 0; j < d; ++j) dst[j] = src[j];
}

// A slot carries point x if it is inside the box; otherwise a copy of the best vertex, and its value is ignored.
VK_FIT_HD inline void put(State& s, const Params& q, int slot, const double* x) {
  const bool in = in_box(q, x);
  s.live[slot] = in ? 1 : 0;
  copy(s.pt[slot], in ? x : s.v[0], q.d);
}

// Vertex j of the simplex around v_0 (the start, or the best vertex at a restart): v_0 + step_j e_j, else v_0 - step_j e_j, else
// the coordinate clamped to the box face with more room.
VK_FIT_HD inline void lay_start(State& s, const Params& q) {
  s.phase = kInit;
  for (int i = 1; i <= q.d; ++i) {
    const int j = i - 1;
    copy(s.v[i], s.v[0], q.d);
    const double up = s.v[0][j] + q.step[j], down = s.v[0][j] - q.step[j];
    s.v[i][j] = up <= q.hi[j] ? up : (down >= q.lo[j] ? down : (q.hi[j] - s.v[0][j] >= s.v[0][j] - q.lo[j] ? q.hi[j] : q.lo[j]));
  }
  for (int i = 0; i < q.S; ++i) put(s, q, i, s.v[i <= q.d ? i : 0]);
  for (int i = q.d + 1; i < q.S; ++i) s.live[i] = 0;                   // spare slots repeat the start
}

// A fresh problem at x0 (inside the box: vk_fit_run checks it).
VK_FIT_HD inline void start(State& s, const Params& q, const double* x0) {
  s.status = -1;
  s.iter = 0;
  s.restarts_left = q.restarts;
  s.n_evals = 0;
  copy(s.x0, x0, q.d);
  copy(s.v[0], x0, q.d);
  lay_start(s, q);
}

VK_FIT_HD inline double f_of(double lnl) { return __builtin_isfinite(lnl) ? -lnl : inf(); }    // -inf / NaN / +inf lnL: failed

// insertion sort of the d + 1 vertices by f; equal values keep their order (stable: ties by vertex index)
VK_FIT_HD inline void sort(State& s, const Params& q) {
  for (int i = 1; i <= q.d; ++i)
    for (int k = i; k > 0 && s.f[k] < s.f[k - 1]; --k) {
      const double tf = s.f[k], tc = s.chi[k];
      s.f[k] = s.f[k - 1];
      s.chi[k] = s.chi[k - 1];
      s.f[k - 1] = tf;
      s.chi[k - 1] = tc;
      for (int j = 0; j < q.d; ++j) {
        const double t = s.v[k][j];
        s.v[k][j] = s.v[k - 1][j];
        s.v[k - 1][j] = t;
      }
    }
}

// scipy's test: every parameter's spread max_i |v_i - v_0|_j <= xtol_j and max_i (f_i - f_0) <= ftol
VK_FIT_HD inline bool converged(const State& s, const Params& q) {
  bool ok = true;
  for (int i = 1; i <= q.d; ++i) {
    ok = ok && s.f[i] - s.f[0] <= q.ftol;
    for (int j = 0; j < q.d; ++j) ok = ok && __builtin_fabs(s.v[i][j] - s.v[0][j]) <= q.xtol[j];
  }
  return ok;
}

// the candidates around the centroid of the best d vertices, into slots r, e, oc, ic
VK_FIT_HD inline void lay_candidates(State& s, const Params& q) {
  s.phase = kCand;
  const int d = q.d;
  for (int j = 0; j < d; ++j) {
    double c = 0.0;
    for (int i = 0; i < d; ++i) c += s.v[i][j];
    c = c / d;
    const double g = c - s.v[d][j];
    s.pt[kR][j] = c + g;
    s.pt[kE][j] = c + 2.0 * g;
    s.pt[kOC][j] = c + 0.5 * g;
    s.pt[kIC][j] = c - 0.5 * g;
  }
  for (int k = 0; k < 4; ++k) {
    const bool in = in_box(q, s.pt[k]);
    s.live[k] = in ? 1 : 0;
    if (!in) copy(s.pt[k], s.v[0], d);
  }
  for (int i = 4; i < q.S; ++i) {
    s.live[i] = 0;
    copy(s.pt[i], s.v[0], d);
  }
}

// v_i <- v_0 + (v_i - v_0) / 2 for i >= 1, into slots 0 .. d - 1
VK_FIT_HD inline void lay_shrink(State& s, const Params& q) {
  s.phase = kShrink;
  for (int i = 1; i <= q.d; ++i)
    for (int j = 0; j < q.d; ++j) s.v[i][j] = s.v[0][j] + 0.5 * (s.v[i][j] - s.v[0][j]);
  for (int i = 0; i < q.S; ++i) put(s, q, i, s.v[i < q.d ? i + 1 : 0]);
  for (int i = q.d; i < q.S; ++i) s.live[i] = 0;
}

VK_FIT_HD inline void take(State& s, const Params& q, int slot, double f, double chi) {
  copy(s.v[q.d], s.pt[slot], q.d);
  s.f[q.d] = f;
  s.chi[q.d] = chi;
}

// The decision on the candidates' values (Lagarias et al. 1998, section 2; scipy.optimize._optimize._minimize_neldermead).
// Returns kShrunk when the simplex must shrink (the caller lays out the shrink launch).
VK_FIT_HD inline int decide(State& s, const Params& q, const double* fc, const double* cc) {
  const int d = q.d;
  const double fr = fc[kR];
  if (fr < s.f[0]) {
    if (fc[kE] < fr) {
      take(s, q, kE, fc[kE], cc[kE]);
      return kExpand;
    }
    take(s, q, kR, fr, cc[kR]);
    return kReflect;
  }
  if (fr < s.f[d - 1]) {
    take(s, q, kR, fr, cc[kR]);
    return kReflect;
  }
  if (fr < s.f[d]) {
    if (fc[kOC] <= fr) {
      take(s, q, kOC, fc[kOC], cc[kOC]);
      return kOutside;
    }
    return kShrunk;
  }
  if (fc[kIC] < s.f[d]) {
    take(s, q, kIC, fc[kIC], cc[kIC]);
    return kInside;
  }
  return kShrunk;
}

// One transition: the values lnl / chi2 [S] of the pending launch's slots -> the next launch's slots (or the end).  Returns the
// decision taken (Decision).  A problem in kDone is left alone.
VK_FIT_HD inline int transition(State& s, const Params& q, const double* lnl, const double* chi2) {
  if (s.phase == kDone) return kConverged;
  const int d = q.d;
  s.iter += 1;
  int dec = kVertices;                                                 // start or shrunk vertices evaluated
  if (s.phase == kInit) {
    for (int i = 0; i <= d; ++i) {
      s.f[i] = s.live[i] ? f_of(lnl[i]) : inf();
      s.chi[i] = s.live[i] ? chi2[i] : inf();
      s.n_evals += s.live[i];
    }
    bool any = false;
    for (int i = 0; i <= d; ++i) any = any || s.f[i] < inf();
    if (!any) {
      copy(s.v[0], s.x0, d);
      s.f[0] = inf();
      s.chi[0] = inf();
      s.status = VK_FIT_NO_FINITE_START;
      s.phase = kDone;
      return kNoFiniteStart;
    }
  } else if (s.phase == kCand) {
    double fc[4], cc[4];
    for (int k = 0; k < 4; ++k) {
      fc[k] = s.live[k] ? f_of(lnl[k]) : inf();
      cc[k] = s.live[k] ? chi2[k] : inf();
    }
    // the rows a one-point-at-a-time search would have evaluated: r, then e (r better than the best) or oc / ic (r no better
    // than the second worst) - counted when inside the box
    s.n_evals += s.live[kR];
    if (fc[kR] < s.f[0]) s.n_evals += s.live[kE];
    else if (!(fc[kR] < s.f[d - 1])) s.n_evals += fc[kR] < s.f[d] ? s.live[kOC] : s.live[kIC];
    dec = decide(s, q, fc, cc);
    if (dec == kShrunk) {
      if (s.iter >= q.max_iter) {
        s.status = VK_FIT_MAX_ITER;
        s.phase = kDone;
        return kMaxIter;
      }
      lay_shrink(s, q);
      return kShrunk;
    }
  } else {                                                             // kShrink: slots 0 .. d - 1 hold v_1 .. v_d
    for (int i = 1; i <= d; ++i) {
      s.f[i] = s.live[i - 1] ? f_of(lnl[i - 1]) : inf();
      s.chi[i] = s.live[i - 1] ? chi2[i - 1] : inf();
      s.n_evals += s.live[i - 1];
    }
  }
  sort(s, q);
  if (converged(s, q)) {
    if (s.restarts_left > 0 && s.iter < q.max_iter) {
      s.restarts_left -= 1;
      lay_start(s, q);
      return kRestart;
    }
    s.status = VK_FIT_CONVERGED;
    s.phase = kDone;
    return kConverged;
  }
  if (s.iter >= q.max_iter) {
    s.status = VK_FIT_MAX_ITER;
    s.phase = kDone;
    return kMaxIter;
  }
  lay_candidates(s, q);
  return dec;
}

}  // namespace vkfit
