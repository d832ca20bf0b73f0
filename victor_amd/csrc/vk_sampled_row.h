// vk_sampled_row.h: the one place where a parameter row is formed on the device from sampled values - part of libvictor_hip.so
// (vk_sampled.hip; fit_emit of vk_kernel_fit.h, chain_emit of vk_kernel_chain.h and the propose kernel of vk_kernel_stretch.h
// call it).
//
// include/victor_hip.h promises that such a row equals the row the host forms from the same values (CCFFit._fit_rows) bit for
// bit - to rounding where epsilon is sampled: the device's pow stands where the host has libm's.
#pragma once
#include "vk_common.h"
#include "vk_row_select.h"

namespace vk {

static_assert(vkrow::kNpar == VK_NPAR && vkrow::kAperp == VK_P_APERP && vkrow::kApar == VK_P_APAR && vkrow::kEpsilon == VK_P_EPSILON,
              "vk_row_select.h restates the row layout of include/victor_hip.h");

// Row r of every row set of the handle (b: one set, or one per block of a joint fit) from base row p of that set: the base with
// column col[j] overwritten by value(j), j < d, in the sets parameter j belongs to (vkrow::form_rows states the rule);
// col[j] < 0 (VK_WALK_EPSILON): value(j) is epsilon and becomes apar = alpha eps^(-2/3), aperp = eps apar as vk_epsilon_to_ap
// forms them (ccf_model.py:589-592)
template <class Value>
__device__ __forceinline__ void sampled_row(const vkrow::Blocks& b, const double* base, size_t p, double* rows, size_t r, const int* col,
                                            int d, double alpha, Value value) {
  vkrow::form_rows(b, base, (long long)p, rows, (long long)r, col, d, alpha, value, [](double x) { return pow(x, -2.0 / 3.0); });
}

}  // namespace vk
