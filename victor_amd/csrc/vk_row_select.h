// vk_row_select.h - which sampled value lands in which block's parameter row: the selection rule behind the per-block rows of a
// joint fit's best fits and chains (vk_fit_create_joint_blocks / vk_chain_create_joint_blocks, include/victor_hip.h).
// Header-only and free of HIP: sampled_row (vk_sampled_row.h) calls it from the kernels that form rows, and
// tests/test_joint_blocks.py compiles it on its own under g++ against a NumPy restatement.
//
// The rule: a handle keeps n row sets - one per block of the joint fit, or one for all of them - each with base rows of its own.
// Sampled parameter j carries a row column col[j] (col[j] < 0: epsilon, which sets the columns aperp, apar and epsilon) and a
// block param_block[j]: -1 for every row set, else the one set it is written to.  The row of set q is that set's base row with
// value j written wherever param_block[j] < 0 or param_block[j] == q, in the order of j.
//
// Bits: copies, and for epsilon one power (the caller's: the device's pow in the kernels, libm's in a host test), one
// multiplication by alpha when alpha != 1 and one by epsilon - the arithmetic vk_epsilon_to_ap does.  With n == 1 and every
// param_block[j] == -1 the stores are those of a handle without row sets.
#pragma once

#if defined(__HIPCC__)
#define VK_ROW_HD __host__ __device__
#else
#define VK_ROW_HD
#endif

namespace vkrow {

constexpr int kMaxP = 10;              // sampled parameters, as vkfit::kMaxP
constexpr int kNpar = 12;              // VK_NPAR
constexpr int kAperp = 2, kApar = 3, kEpsilon = 4;     // VK_P_APERP, VK_P_APAR, VK_P_EPSILON

// the row sets of a handle, passed to the kernels by value
struct Blocks {
  int n;                     // row sets: 1, or the blocks of the joint fit
  long long row_stride;      // doubles between two sets of pending rows (fixed per handle: the largest launch's rows)
  long long base_stride;     // doubles between two sets of base rows
  int param_block[kMaxP];    // -1: the value goes to every set; q: to set q alone
};

VK_ROW_HD inline Blocks one_set() {
  Blocks b{};
  b.n = 1;
  for (int j = 0; j < kMaxP; ++j) b.param_block[j] = -1;
  return b;
}

VK_ROW_HD inline bool applies(const Blocks& b, int j, int q) { return b.param_block[j] < 0 || b.param_block[j] == q; }

// row = base with the values that apply to set q; power(x) = x^(-2/3)
template <class Value, class Power>
VK_ROW_HD inline void form_row(const Blocks& b, int q, const double* base, double* row, const int* col, int d, double alpha,
                               Value value, Power power) {
  for (int c = 0; c < kNpar; ++c) row[c] = base[c];
  for (int j = 0; j < d; ++j) {
    if (!applies(b, j, q)) continue;
    const double x = value(j);
    const int c = col[j];
    if (c >= 0) {
      row[c] = x;
    } else {
      double ap = power(x);
      if (alpha != 1.0) ap = alpha * ap;
      row[kApar] = ap;
      row[kAperp] = x * ap;
      row[kEpsilon] = x;
    }
  }
}

// row r of every set from base row p of every set
template <class Value, class Power>
VK_ROW_HD inline void form_rows(const Blocks& b, const double* base, long long p, double* rows, long long r, const int* col, int d,
                                double alpha, Value value, Power power) {
  for (int q = 0; q < b.n; ++q)
    form_row(b, q, base + q * b.base_stride + p * kNpar, rows + q * b.row_stride + r * kNpar, col, d, alpha, value, power);
}

}  // namespace vkrow
