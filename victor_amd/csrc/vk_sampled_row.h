// vk_sampled_row.h: the one place where a parameter row is formed on the device from sampled values - part of libvictor_hip.so
// (vk_sampled.hip; fit_emit of vk_kernel_fit.h and chain_emit of vk_kernel_chain.h call it).
//
// include/victor_hip.h promises that such a row equals the row the host forms from the same values (CCFFit._fit_rows) bit for
// bit - to rounding where epsilon is sampled: the device's pow stands where the host has libm's.
#pragma once
#include "vk_common.h"

namespace vk {

// row = base with column col[j] overwritten by value(j), j < d; col[j] < 0 (VK_WALK_EPSILON): value(j) is epsilon and becomes
// apar = alpha eps^(-2/3), aperp = eps apar as vk_epsilon_to_ap forms them (ccf_model.py:589-592)
template <class Value>
__device__ __forceinline__ void sampled_row(const double* base, double* row, const int* col, int d, double alpha, Value value) {
  for (int c = 0; c < VK_NPAR; ++c) row[c] = base[c];
  for (int j = 0; j < d; ++j) {
    const double x = value(j);
    const int c = col[j];
    if (c >= 0) {
      row[c] = x;
    } else {
      double ap = pow(x, -2.0 / 3.0);
      if (alpha != 1.0) ap = alpha * ap;
      row[VK_P_APAR] = ap;
      row[VK_P_APERP] = x * ap;
      row[VK_P_EPSILON] = x;
    }
  }
}

}  // namespace vk
