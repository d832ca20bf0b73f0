// vk_marginals.h - the binning rule of the marginal histograms behind vk_chain_set_marginals (include/victor_hip.h): where a
// kept position of a chain is counted, in the 1-D histogram of every sampled parameter and in the 2-D histograms of chosen pairs.
// Header-only and free of HIP, like vk_chain_step.h and vk_prior.h: the step kernels of vk_kernel_chain.h and vk_kernel_stretch.h
// call it right behind vkchain::accumulate, and tests/test_marginals.py compiles it on its own under g++ against the NumPy
// statement of victor_amd/marginals.py.
//
// Parameter j is binned over a range [a_j, b_j], in n_bins bins (1-D) or n_bins2 bins (2-D).  The host forms
// inv_j = n_bins / (b_j - a_j) and inv2_j = n_bins2 / (b_j - a_j), one IEEE division each, once (inverse_width()); the kernels get those
// doubles.  The slot of a value v among the n + 2 slots of a 1-D histogram:
//   v < a_j      slot 0, "below";
//   v > b_j      slot n + 1, "above" (so does a NaN, which no chain holds: the comparison is !(v <= b_j));
//   otherwise    slot 1 + min(n - 1, (int)((v - a_j) * inv_j)):  v == b_j lands in the last bin.
// A sample enters the 2-D histogram of the pair (j, k) only when it lies inside BOTH ranges, in cell (bin_j, bin_k) with
// bin = min(n_bins2 - 1, (int)((v - a) * inv2)).
//
// Bits: one subtraction, one multiplication and one conversion (the product is non-negative and at most a rounding above n, the
// conversion truncates) - nothing a compiler could contract into an fma, so hipcc, g++ and NumPy choose the same slot from the
// same bits.
//
// Counts are 64-bit integers and the increment is the caller's: count() hands every slot's address to `add` - on the device an
// atomic + 1 on unsigned long long (vk_kernel_chain.h; integer adds commute: the histogram does not depend on the order the
// chains arrive in), under g++ a plain += 1.  The histograms of a handle are pooled per problem: h1 [problems][d][n_bins + 2] and
// h2 [problems][n_pairs][n_bins2][n_bins2].  x is read through a getter, x(j), as in vk_prior.h; nothing here indexes a local
// array, so the device code needs no scratch; the ranges and the pair list are kernel arguments, read with scalar loads.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define VK_MARG_HD __host__ __device__
#else
#define VK_MARG_HD
#endif

namespace vkmarg {

constexpr int kMaxP = 10;              // sampled parameters, as vkchain::kMaxP
constexpr int kMaxPairs = kMaxP * (kMaxP - 1) / 2;
constexpr int kMaxBins = 1024;         // bins of a 1-D histogram
constexpr int kMaxBins2 = 128;         // bins per axis of a 2-D histogram

struct Marginals {
  int on;                              // 0: no histograms (nothing else is read)
  int group;                           // chains per problem: chain c adds to problem c / group
  int n_bins, n_bins2, n_pairs;
  double a[kMaxP], b[kMaxP];           // the range of each sampled parameter
  double inv[kMaxP], inv2[kMaxP];      // n_bins / (b - a), n_bins2 / (b - a)
  int pair[kMaxPairs][2];              // (j, k), j < k
  unsigned long long* h1;              // [problems][d][n_bins + 2]
  unsigned long long* h2;              // [problems][n_pairs][n_bins2][n_bins2]
};

// the one division of a parameter's range
inline double inverse_width(int n, double a, double b) { return (double)n / (b - a); }

VK_MARG_HD inline bool inside(double v, double a, double b) { return !(v < a) && v <= b; }

// the bin of a value inside [a, b], in 0 .. n - 1
VK_MARG_HD inline int bin(double v, double a, double inv, int n) {
  const double t = (v - a) * inv;
  const int i = (int)t;
  return i < n - 1 ? i : n - 1;
}

// the slot of a value among the n + 2 slots of a 1-D histogram
VK_MARG_HD inline int slot(double v, double a, double b, double inv, int n) {
  if (v < a) return 0;
  if (!(v <= b)) return n + 1;
  return 1 + bin(v, a, inv, n);
}

// the cell of (vj, vk) in a pair's n x n histogram, row bin_j, or -1 when the sample is outside either range
VK_MARG_HD inline int cell(double vj, double aj, double bj, double invj, double vk, double ak, double bk, double invk, int n) {
  if (!inside(vj, aj, bj) || !inside(vk, ak, bk)) return -1;
  return bin(vj, aj, invj, n) * n + bin(vk, ak, invk, n);
}

// one kept position x(0) .. x(d - 1) of a chain of `problem`: d + n_pairs increments at most
template <class Get, class Add>
VK_MARG_HD inline void count(const Marginals& m, int d, size_t problem, Get x, Add add) {
  const size_t n1 = (size_t)m.n_bins + 2;
  unsigned long long* h1 = m.h1 + problem * (size_t)d * n1;
  for (int j = 0; j < d; ++j) add(h1 + (size_t)j * n1 + slot(x(j), m.a[j], m.b[j], m.inv[j], m.n_bins));
  const size_t n2 = (size_t)m.n_bins2 * m.n_bins2;
  unsigned long long* h2 = m.h2 + problem * (size_t)m.n_pairs * n2;
  for (int p = 0; p < m.n_pairs; ++p) {
    const int j = m.pair[p][0], k = m.pair[p][1];
    const int at = cell(x(j), m.a[j], m.b[j], m.inv2[j], x(k), m.a[k], m.b[k], m.inv2[k], m.n_bins2);
    if (at >= 0) add(h2 + (size_t)p * n2 + at);
  }
}

}  // namespace vkmarg
