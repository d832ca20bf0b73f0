// vk_grid.h - the index rules and the accumulation step of the grid posteriors behind vk_grid_create / vk_grid_run
// (include/victor_hip.h; victor_amd/grid.py states the definition in NumPy, DESIGN.md section 7c the kernel mapping).
// Header-only and free of HIP, like vk_marginals.h and vk_prior.h: the kernels of vk_kernel_grid.h call it, and
// tests/test_grid.py compiles it on its own under g++ (-ffp-contract=off) against the NumPy statement.
//
// The grid: d axes of n[j] nodes, flat index g in [0, G), G = prod n[j], ROW-MAJOR - the last axis varies fastest:
//   g = sum_j k_j stride[j],  stride[d - 1] = 1,  stride[j] = stride[j + 1] n[j + 1],  k_j = (g / stride[j]) % n[j].
//
// Cells.  The accumulators of a problem are the total, one cell per node of every axis, and one cell per node pair of every
// requested axis pair.  The flat indices of node k of axis j are runs of stride[j] consecutive indices, one run every
// n[j] stride[j] (the axis' period), the first at k stride[j].  For a pair (ja < jb) a run of axis ja starts at a multiple of axis
// jb's period (stride[ja] is a multiple of n[jb] stride[jb]), so the pair's indices are the runs of axis jb inside the runs of
// axis ja.  for_axis_cell / for_pair_cell call f(g) for the indices of a cell inside a chunk [g0, g1), IN INCREASING ORDER: the
// order of the additions is part of the definition.
//
// The step, per chunk and problem, with M the running maximum (-inf at the start):
//   M' = max(M, max over the chunk of lnpost);  M' = -inf: nothing else happens
//   M' > M: every accumulator is multiplied by exp(M - M') (rescale_factor; exp(-inf) = 0, and 0 * 0 = 0), then M = M'
//   every accumulator adds exp(lnpost[g] - M) for its indices of the chunk, one at a time in increasing g (add), and the
//   profile cells take the maximum of lnpost.
// A value that is not finite counts as -inf (clean): the evaluators report a failed point as -inf, and no NaN can enter a sum.
// exp is the caller's: the device's in the kernels, libm's in a host test.
#pragma once

#if defined(__HIPCC__)
#define VK_GRID_HD __host__ __device__
#else
#define VK_GRID_HD
#endif

namespace vkgrid {

constexpr int kMaxP = 10;              // axes, as vkrow::kMaxP
constexpr int kMaxBins = 1024;         // nodes of an axis
constexpr int kMaxBins2 = 128;         // ... of an axis of a pair
constexpr int kMaxPairs = 45;
constexpr long long kMaxPoints = 1LL << 40;
constexpr int kMaxChunk = 65536;

struct Shape {
  int d;
  int n[kMaxP];
  long long stride[kMaxP];
  long long G;
};

// the shape of d axes with n[j] nodes (the caller has checked 1 <= n[j] <= kMaxBins and the product)
VK_GRID_HD inline Shape make_shape(int d, const int* n) {
  Shape s{};
  s.d = d;
  long long stride = 1;
  for (int j = d - 1; j >= 0; --j) {
    s.n[j] = n[j];
    s.stride[j] = stride;
    stride *= n[j];
  }
  s.G = stride;
  return s;
}

VK_GRID_HD inline double neg_inf() { return -__builtin_inf(); }

// node of axis j at flat index g
VK_GRID_HD inline int node(const Shape& s, int j, long long g) { return (int)((g / s.stride[j]) % s.n[j]); }

// a value as the accumulators see it
VK_GRID_HD inline double clean(double v) { return __builtin_isfinite(v) ? v : neg_inf(); }

// the runs [lo, hi) of consecutive indices of node k of axis j inside [g0, g1), increasing: f(lo, hi), lo < hi
template <class F>
VK_GRID_HD inline void for_axis_runs(const Shape& s, int j, int k, long long g0, long long g1, F f) {
  const long long run = s.stride[j], period = run * s.n[j];
  for (long long start = (g0 / period) * period + k * run; start < g1; start += period) {
    const long long lo = start > g0 ? start : g0, hi = start + run < g1 ? start + run : g1;
    if (lo < hi) f(lo, hi);
  }
}

// ... of node ka of axis ja and node kb of axis jb, ja < jb: the runs of axis jb inside the runs of axis ja (a run of axis ja
// starts at a multiple of axis jb's period, so clipping to it keeps axis jb's pattern)
template <class F>
VK_GRID_HD inline void for_pair_runs(const Shape& s, int ja, int ka, int jb, int kb, long long g0, long long g1, F f) {
  for_axis_runs(s, ja, ka, g0, g1, [&](long long lo, long long hi) { for_axis_runs(s, jb, kb, lo, hi, f); });
}

// the indices themselves, one at a time: f(g)
template <class F>
VK_GRID_HD inline void for_axis_cell(const Shape& s, int j, int k, long long g0, long long g1, F f) {
  for_axis_runs(s, j, k, g0, g1, [&](long long lo, long long hi) {
    for (long long g = lo; g < hi; ++g) f(g);
  });
}
template <class F>
VK_GRID_HD inline void for_pair_cell(const Shape& s, int ja, int ka, int jb, int kb, long long g0, long long g1, F f) {
  for_pair_runs(s, ja, ka, jb, kb, g0, g1, [&](long long lo, long long hi) {
    for (long long g = lo; g < hi; ++g) f(g);
  });
}

// the factor the accumulators of a problem are multiplied by when its maximum moves from m_old to m_new >= m_old
template <class Exp>
VK_GRID_HD inline double rescale_factor(double m_old, double m_new, Exp e) {
  return m_new > m_old ? e(m_old - m_new) : 1.0;
}

// the weight of a value under the maximum m (finite): what every accumulator holding the index adds
template <class Exp>
VK_GRID_HD inline double weight(double lnpost, double m, Exp e) { return e(lnpost - m); }

// One rescale of an accumulator, one addition, one update of a profile cell.  A rescale feeds the chunk's first addition - a
// product into a sum, which a compiler contracts into a fused multiply-add: both forbid it (hipcc: the pragma; the CPU tests
// build with -ffp-contract=off), so each is rounded on its own, as NumPy rounds them.
VK_GRID_HD inline void rescale(double& acc, double factor) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  acc = acc * factor;
}
VK_GRID_HD inline void add(double& acc, double w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  acc = acc + w;
}
VK_GRID_HD inline void take_max(double& p, double lnpost) {
  if (lnpost > p) p = lnpost;
}

// A chunk's maximum, its first arg max and its count of finite values merged from two parts: the larger maximum, of equal maxima
// the smaller index (exact, whatever the order of the merges)
struct Best {
  double max;
  long long arg;       // -1: none yet
  long long n_finite;
};
VK_GRID_HD inline Best none() { return Best{neg_inf(), -1, 0}; }
VK_GRID_HD inline void see(Best& b, double lnpost, long long g) {
  if (lnpost > neg_inf()) {
    b.n_finite += 1;
    if (lnpost > b.max || (lnpost == b.max && (b.arg < 0 || g < b.arg))) {
      b.max = lnpost;
      b.arg = g;
    }
  }
}
VK_GRID_HD inline Best merge(const Best& a, const Best& b) {
  Best r = a;
  if (b.arg >= 0 && (a.arg < 0 || b.max > a.max || (b.max == a.max && b.arg < a.arg))) {
    r.max = b.max;
    r.arg = b.arg;
  }
  r.n_finite = a.n_finite + b.n_finite;
  return r;
}

// The running state of a problem, and the update the max kernel makes once per chunk: the maximum, its first index (changed on a
// strict increase only), the count, and the factor for the accumulators.
struct Running {
  double m;            // -inf at the start
  long long arg;       // -1 at the start
  long long n_finite;
  double factor;       // of the chunk just seen
};
VK_GRID_HD inline Running start() { return Running{neg_inf(), -1, 0, 1.0}; }
template <class Exp>
VK_GRID_HD inline void advance(Running& r, const Best& chunk, Exp e) {
  r.n_finite += chunk.n_finite;
  if (chunk.arg >= 0 && chunk.max > r.m) {
    r.factor = rescale_factor(r.m, chunk.max, e);
    r.m = chunk.max;
    r.arg = chunk.arg;
  } else {
    r.factor = 1.0;
  }
}

}  // namespace vkgrid
