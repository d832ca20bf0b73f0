// vk_importance.h - the accumulator index rules, the list walk and the terms of the importance-sampled posteriors behind
// vk_is_create / vk_is_run (include/victor_hip.h; victor_amd/importance.py states the definition in NumPy, DESIGN.md section 7e
// the kernel mapping).  Header-only and free of HIP, like vk_grid.h, whose step it generalises from lattice nodes to scattered
// points: the kernels of vk_kernel_importance.h call it, and tests/test_importance.py compiles it on its own under g++
// (-ffp-contract=off) against the NumPy statement.
//
// The sample: G points x[g][0 .. d), kept in the order they were drawn, with y[g][j] = x[g][j] - centre[j] and
// lno[g] = ln prior(x_g) - ln q(x_g).  What a lattice gave for free is stated by the caller here:
//   cells   a point's slot in the histogram of axis j (0: below the range, 1 .. n_j: the bins, n_j + 1: above) and its cell in a
//           pair's m x m histogram come from the host's binning rule (victor_amd/marginals.py); per chunk and list (the d axes,
//           then the pairs) the chunk's points are LISTED BY CELL, in increasing g inside a cell, with the cells' offsets:
//           cell k of a list holds entries off[k] .. off[k + 1] - 1 of the chunk's segment of the list, each the point's index
//           inside the chunk (g - g0).  walk calls f(g) for them in that order: the order of the additions is the definition.
//   nodes   x, y and the host's eps^(-2/3) are looked up by g
//   density lno carries the proposal; the step adds it to lnL once
//
// The accumulators of a problem, in the order the kernels and vk_is_result index them (accumulator a of problem r):
//   0                  total = sum w                     w = exp(lnpost - M), the step of vk_grid.h
//   1                  sq    = sum w w                   (rescaled by the factor TWICE, each product rounded: rescale_sq)
//   2 + j              s1[j] = sum w y_j
//   2 + d + tri(j, k)  s2[j][k] = sum (w y_j) y_k,  j <= k, the packed upper triangle row by row
//   whole(d) + c       histogram cell c: the slots of axis 0, of axis 1, ..., then the cells of the pairs;  += w over its list
// The first whole(d) = 2 + d + d (d + 1) / 2 walk the whole chunk, the others their lists.  Each term's products are rounded on
// their own (fp contract(off), as vkgrid::add and vkgrid::rescale), so NumPy, g++ and hipcc form the same bits from the same w.
#pragma once
#include "vk_grid.h"

#if defined(__clang__)
#define VK_IS_UNROLL _Pragma("unroll")
#else
#define VK_IS_UNROLL
#endif

namespace vkis {

constexpr int kMaxP = vkgrid::kMaxP;
constexpr int kMaxBins = vkgrid::kMaxBins;           // bins of an axis (its list has two more cells: below, above)
constexpr int kMaxBins2 = vkgrid::kMaxBins2;         // ... of an axis of a pair
constexpr int kMaxPairs = vkgrid::kMaxPairs;
constexpr int kMaxLists = kMaxP + kMaxPairs;
constexpr long long kMaxPoints = 1LL << 24;          // the sample lives on the device: x, y and one list entry per point and list
constexpr int kMaxChunk = vkgrid::kMaxChunk;
constexpr long long kMaxOffsets = 1LL << 27;         // offsets of all chunks together

enum { kTotal = 0, kSq = 1, kFirst = 2 };

VK_GRID_HD inline int tri(int d, int j, int k) { return j * d - j * (j - 1) / 2 + (k - j); }
VK_GRID_HD inline int whole(int d) { return kFirst + d + d * (d + 1) / 2; }
VK_GRID_HD inline int first(int j) { return kFirst + j; }
VK_GRID_HD inline int second(int d, int j, int k) { return kFirst + d + tri(d, j, k); }
// (j, k), j <= k, of second-moment accumulator a
VK_GRID_HD inline void second_of(int d, int a, int& j, int& k) {
  int t = a - kFirst - d;
  j = 0;
  while (t >= d - j) {
    t -= d - j;
    ++j;
  }
  k = j + t;
}

// the indices of a cell inside the chunk that starts at g0: entries lo .. hi - 1 of the chunk's segment, in the list's order
template <class F>
VK_GRID_HD inline void walk(const int* segment, int lo, int hi, long long g0, F f) {
  for (int e = lo; e < hi; ++e) f(g0 + segment[e]);
}

// The same walk with B loads in flight: a thread's walk is a chain of additions, and the loads need not wait for it.  load(g)
// gives the term of index g, add(v) takes the terms IN THE LIST'S ORDER.  range_ahead: the whole chunk, rows i0 .. i1 - 1.
template <int B, class Load, class Add>
VK_GRID_HD inline void walk_ahead(const int* segment, int lo, int hi, long long g0, Load load, Add add) {
  int e = lo;
  for (; e + B <= hi; e += B) {
    double v[B];
VK_IS_UNROLL
    for (int u = 0; u < B; ++u) v[u] = load(g0 + segment[e + u]);
VK_IS_UNROLL
    for (int u = 0; u < B; ++u) add(v[u]);
  }
  for (; e < hi; ++e) add(load(g0 + segment[e]));
}
template <int B, class Load, class Add>
VK_GRID_HD inline void range_ahead(int i0, int i1, Load load, Add add) {
  int i = i0;
  for (; i + B <= i1; i += B) {
    double v[B];
VK_IS_UNROLL
    for (int u = 0; u < B; ++u) v[u] = load(i + u);
VK_IS_UNROLL
    for (int u = 0; u < B; ++u) add(v[u]);
  }
  for (; i < i1; ++i) add(load(i));
}

// the terms: every product rounded on its own
VK_GRID_HD inline double square_term(double w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return w * w;
}
VK_GRID_HD inline double first_term(double w, double yj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return w * yj;
}
VK_GRID_HD inline double second_term(double w, double yj, double yk) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double t = w * yj;
  return t * yk;
}
// the sum of squares when the maximum rises: w w carries the factor twice
VK_GRID_HD inline void rescale_sq(double& acc, double factor) {
  vkgrid::rescale(acc, factor);
  vkgrid::rescale(acc, factor);
}

// ---- a proposal per problem (vk_is_create_own; victor_amd/importance.py rule 8) ------------------------------------------------
// Every problem r has its own n points: what was one value per point g is one per (g, r), the problem the fastest-varying index,
// so the lanes of a wave - consecutive problems of one point - read consecutive values.
//   x, y                 [G][R][d]   point (g, r) at (g R + r) d
//   eps_pow, lno, lnop   [G][R]      value_at(g, r, R); with stride 0 the same call names the shared mode's one value per point
//   rows, lnL, w         [n][R]      row i R + r of a chunk is point g0 + i of problem r, evaluated against realisation which[r]
//   lists                [R][n_lists][G]            problem r's list l at own_list(r, l, n_lists, G)
//   offsets              [n_chunks][R][cells + n_lists]   chunk c, problem r at own_offsets(c, r, R, cells + n_lists)
// Under a prior problem R + r is problem r's prior problem (prior_of): lnpost = lnop[g][r], a total alone.
VK_GRID_HD inline long long value_at(long long g, int r, int stride) { return stride ? g * stride + r : g; }
VK_GRID_HD inline long long own_row(long long i, int r, int R) { return i * R + r; }
VK_GRID_HD inline long long own_list(int r, int l, int n_lists, long long G) { return ((long long)r * n_lists + l) * G; }
VK_GRID_HD inline long long own_offsets(long long c, int r, int R, long long per_chunk) { return (c * R + r) * per_chunk; }
// the problem whose sample (points, y, lists, weights' row) problem r of the Rp = R or 2 R reads, and is it a prior problem
VK_GRID_HD inline int prior_of(int r, int R) { return r >= R ? r - R : r; }

// One chunk's segment of a list against its offsets, as vk_is_create checks every one before a kernel may index with them: n the
// chunk's points, cells the list's cells, off[0 .. cells].  0: off[0] = 0, the offsets never decrease, off[cells] <= n, every
// entry is a point of the chunk and the entries of a cell increase.  1: the offsets are wrong, at offset *where; 2: an entry is,
// at entry *where of the segment.
inline int check_list(const int* segment, const int* off, int cells, int n, long long* where) {
  *where = 0;
  if (off[0] != 0) return 1;
  for (int k = 0; k < cells; ++k)
    if (off[k + 1] < off[k] || off[k + 1] > n) {
      *where = k + 1;
      return 1;
    }
  for (int k = 0; k < cells; ++k)
    for (int e = off[k]; e < off[k + 1]; ++e)
      if (segment[e] < 0 || segment[e] >= n || (e > off[k] && segment[e] <= segment[e - 1])) {
        *where = e;
        return 2;
      }
  return 0;
}

}  // namespace vkis
