// vk_autocorr.h - the running autocorrelation of the ensemble series behind vk_chain_set_autocorr (include/victor_hip.h): per
// problem and sampled parameter, the series of the per-step sum over the problem's W chains (walkers), and the lagged products of
// that series up to a fixed lag - what an integrated autocorrelation time and an effective sample size are read from when no
// history is kept.  Header-only and free of HIP, like vk_chain_step.h and vk_marginals.h: vk_chain_series_kernel
// (vk_kernel_autocorr.h) calls it from one wave per series, and tests/test_autocorr.py compiles it on its own under g++ against
// the NumPy statement of victor_amd/autocorr.py, bit for bit.
//
// The series value of a kept step is s = the sum over the W chains of the problem, in a fixed shape:
//   lane l of 64 starts from +0.0 and adds the chains w = l, l + 64, l + 128, ... in increasing w (lane_partial);
//   a xor butterfly over the 64 partials follows, offsets 32, 16, 8, 4, 2, 1, v = v + v_partner (combine states it in plain C++;
//   the kernel does it with cross-lane moves); a lane without a chain carries +0.0.  No division by W: the autocorrelation does
//   not depend on scale.
// At the first kept step (n = 0) the pivot is p = s and the value is a_0 = 0; after that a_n = s - p (value).  Per series the
// state is  pivot, total = sum a_t, head[L] = a_0 .. a_{L - 1}, ring[L] (slot u mod L holds a_u) and acc[L], and kept step n does
//   acc[k] += a_n * a_{n - k}   for every lag 0 <= k <= min(n, L - 1) (lag: lag 0 takes a_n itself, lag k >= 1 reads ring[(n - k) mod L]),
//   total += a_n;  head[n] = a_n if n < L;  ring[n mod L] = a_n   (store).
// The slot written at step n is read by no lag of that step, so the lags of a step are independent of each other and of the
// store.  The count n is the same for every series of a handle and lives on the host.
//
// Bits: every product feeds a sum, which a compiler may contract into an fma and so change the last bit.  lag() forbids it
// (hipcc: the pragma below; the CPU test builds with -ffp-contract=off), as vkchain::propose does.  Everything else is one
// addition or one subtraction at a time.
#pragma once

#include <stddef.h>

#if defined(__HIPCC__)
#define VK_AC_HD __host__ __device__
#else
#define VK_AC_HD
#endif

namespace vkac {

constexpr int kLanes = 64;             // partial sums of a series value: the lanes of a wave
constexpr int kMaxLag = 1024;          // most lags a handle keeps

struct Autocorr {
  int on;                              // 0: no series (nothing else is read)
  int group;                           // W: chains per problem, chain c belongs to problem c / group
  int max_lag;                         // L
  long long n;                         // kept steps the series hold: the index of the step being added
  // series (problem r, parameter j) is number r d + j
  double* pivot;                       // [series]
  double* total;                       // [series]
  double* head;                        // [series][L]
  double* ring;                        // [series][L]
  double* acc;                         // [series][L]
};

// doubles of a handle's state: (3 L + 2) per series
inline size_t state_doubles(size_t series, int L) { return series * (3 * (size_t)L + 2); }

// the partial sum of lane `lane`: +0.0 plus the chains lane, lane + 64, ... < W in increasing order; x(w): chain w of the problem
template <class Get>
VK_AC_HD inline double lane_partial(int W, int lane, Get x) {
  double v = 0.0;
  for (int w = lane; w < W; w += kLanes) v = v + x(w);
  return v;
}

// the butterfly over the 64 partials, as the lanes of a wave do it: afterwards every entry holds the series value
inline void combine(double v[kLanes]) {
  for (int off = kLanes / 2; off > 0; off >>= 1) {
    double next[kLanes];
    for (int l = 0; l < kLanes; ++l) next[l] = v[l] + v[l ^ off];
    for (int l = 0; l < kLanes; ++l) v[l] = next[l];
  }
}

// a_n from the series value s and the pivot (which step 0 sets to s)
VK_AC_HD inline double value(double s, double pivot, long long n) { return n == 0 ? 0.0 : s - pivot; }

// most recent lag step n adds to
VK_AC_HD inline int top_lag(long long n, int L) { return n < (long long)(L - 1) ? (int)n : L - 1; }

// lag k of step n, 0 <= k <= top_lag(n, L): acc[k] += a_n a_{n - k}; slot = n mod L
VK_AC_HD inline void lag(double* acc, const double* ring, double a, int slot, int k, int L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int at = slot - k;
  if (at < 0) at += L;                 // (n - k) mod L: k <= L - 1
  const double other = k == 0 ? a : ring[at];
  const double prod = a * other;
  acc[k] = acc[k] + prod;
}

// the end of step n: the pivot (step 0), the sum, the head and the ring
VK_AC_HD inline void store(double* pivot, double* total, double* head, double* ring, double s, double a, long long n, int slot, int L) {
  if (n == 0) *pivot = s;
  *total = *total + a;
  if (n < (long long)L) head[n] = a;
  ring[slot] = a;
}

// one series, one kept step, every lag one after the other: what the wave of vk_chain_series_kernel does with its lanes striding
// over the lags
inline void step(double* pivot, double* total, double* head, double* ring, double* acc, double s, long long n, int L) {
  const double a = value(s, *pivot, n);
  const int slot = (int)(n % L), top = top_lag(n, L);
  for (int k = 0; k <= top; ++k) lag(acc, ring, a, slot, k, L);
  store(pivot, total, head, ring, s, a, n, slot, L);
}

}  // namespace vkac
