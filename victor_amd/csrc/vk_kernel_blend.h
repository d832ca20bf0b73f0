// vk_kernel_blend.h: the two kernels of LIKELIHOOD-LEVEL BETA INTERPOLATION on a sampled handle (VK_OPT_BETA_BLEND,
// include/victor_hip.h; the reference: ccf_fit.py:383-440) - part of libvictor_hip.so (see vk_sampled.hip, sampled_evaluate, for
// the host side; CCFFit._run_likelihood_interp / Realisations._likelihood_interp of victor_amd for the definition in NumPy;
// DESIGN.md section 7f for the layout).
//
// A handle in blend mode evaluates its m pending rows as 2 m rows - every row at the two nodes of the data vector's beta grid
// that bracket its beta - and blends lnL and chi-square linearly.  Around the unchanged evaluation, on the context's stream:
//   vk_blend_split_kernel  one thread per pending row i: finds lo = the last node with g < beta and hi = the first node with
//                          g >= beta (the reference's rule: a beta on a node gives hi = that node and t = 1), writes row i with
//                          beta = g[lo] to rows2[i] and with beta = g[hi] to rows2[m + i], the row's realisation index to
//                          which2[i] and which2[m + i], t[i] = (beta - g[lo]) / (g[hi] - g[lo]) and fail[i] = 0.  Without a
//                          bracket - beta <= g[0], beta > g[last] or NaN, where the host route raises IndexError - fail[i] = 1,
//                          t[i] = 0 and both rows carry g[0]: they are evaluated like any other row and their values dropped.
//   vk_blend_merge_kernel  one thread per output k of the m x per_row (cross mode: per_row = n_real, the row's t serves every
//                          realisation of it; otherwise 1): (1 - t) lo + t hi of lnL and of chi-square, with lo = raw[k] and
//                          hi = raw[m per_row + k].  A failed row, or a non-finite lnL at either end, gives (-inf, +inf)
//                          (ccf_fit.py:402-410).  Products and sum are rounded one by one (fp contract off: no fma),
//                          as NumPy evaluates the host expression: the same bits whenever the same theory kernel
//                          served both routes.
// No LDS, no atomics, nothing shared between threads; every index is below the bound the thread checked first.
#pragma once
#include <hip/hip_runtime.h>

#include "vk_common.h"

namespace vk {

constexpr int kBlendBlock = 256;

struct BlendArgs {
  const double* grid;                // [n_grid]: the data vector's beta nodes, increasing
  int n_grid;
  long long m;                       // pending rows
  long long per_row;                 // outputs of a row: 1, or n_real in cross mode
  const double* rows;                // [m][VK_NPAR]
  const int* row_which;              // [m] or NULL (the data vector, cross mode)
  double* rows2;                     // [2 m][VK_NPAR]
  int* which2;                       // [2 m] (written with row_which alone)
  double* t;                         // [m]
  int* fail;                         // [m]
  const double *raw_lnl, *raw_chi;   // [2 m][per_row]: the evaluation of rows2
  double *lnl, *chi;                 // [m][per_row]
};

__global__ void __launch_bounds__(kBlendBlock) vk_blend_split_kernel(BlendArgs a) {
  const long long i = (long long)blockIdx.x * kBlendBlock + threadIdx.x;
  if (i >= a.m) return;
  const double* row = a.rows + i * VK_NPAR;
  const double beta = row[VK_P_BETA];
  int lo = -1, hi = -1;
  for (int k = 0; k < a.n_grid; ++k) {
    const double g = a.grid[k];
    if (g < beta) lo = k;
    if (hi < 0 && g >= beta) hi = k;
  }
  const bool ok = lo >= 0 && hi >= 0;                     // (NaN compares false both ways: no bracket)
  const double g_lo = a.grid[ok ? lo : 0], g_hi = a.grid[ok ? hi : 0];
  double* out_lo = a.rows2 + i * VK_NPAR;
  double* out_hi = a.rows2 + (a.m + i) * VK_NPAR;
  for (int c = 0; c < VK_NPAR; ++c) {
    const double v = row[c];
    out_lo[c] = c == VK_P_BETA ? g_lo : v;
    out_hi[c] = c == VK_P_BETA ? g_hi : v;
  }
  if (a.row_which) {
    const int w = a.row_which[i];
    a.which2[i] = w;
    a.which2[a.m + i] = w;
  }
  a.t[i] = ok ? (beta - g_lo) / (g_hi - g_lo) : 0.0;
  a.fail[i] = ok ? 0 : 1;
}

// (1 - t) lo + t hi as NumPy evaluates it: the difference, the two products and the sum each rounded on its own.  (HIP's __dmul_rn
// and __dadd_rn are plain operators the compiler contracts into an fma like any others; the pragma is what keeps them apart.)
__device__ __forceinline__ double blend_uncontracted(double t, double lo, double hi) {
#pragma clang fp contract(off)
  const double u = 1.0 - t;
  const double a = u * lo;
  const double b = t * hi;
  return a + b;
}

__global__ void __launch_bounds__(kBlendBlock) vk_blend_merge_kernel(BlendArgs a) {
  const long long k = (long long)blockIdx.x * kBlendBlock + threadIdx.x;
  const long long n = a.m * a.per_row;
  if (k >= n) return;
  const long long i = k / a.per_row;
  const double t = a.t[i];
  const double l_lo = a.raw_lnl[k], l_hi = a.raw_lnl[n + k];
  const bool bad = a.fail[i] != 0 || !__builtin_isfinite(l_lo) || !__builtin_isfinite(l_hi);
  const double inf = __builtin_inf();
  a.lnl[k] = bad ? -inf : blend_uncontracted(t, l_lo, l_hi);
  a.chi[k] = bad ? inf : blend_uncontracted(t, a.raw_chi[k], a.raw_chi[n + k]);
}

}  // namespace vk
