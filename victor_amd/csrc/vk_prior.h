// vk_prior.h - the Gaussian prior of the sampled parameters behind vk_fit_set_prior / vk_chain_set_prior (include/victor_hip.h):
// ln prior = -1/2 (x - mu)^T P (x - mu), multiplied onto the uniform box, without a normalisation constant (a constant changes no
// decision and no maximum).  Header-only and free of HIP, like vk_chain_step.h: the step kernels of vk_kernel_fit.h,
// vk_kernel_chain.h and vk_kernel_stretch.h call it, and tests/test_priors.py compiles it on its own under g++ against the NumPy
// statement of victor_amd/priors.py.
//
// P is the d x d precision matrix of the sampled parameters in sampled order (zero rows for parameters without a prior), handed
// over as its upper triangle in tri() order with every OFF-DIAGONAL entry doubled (doubling is exact), so the quadratic form is
// one pass over the triangle.  The arithmetic order is part of the definition:
//   q = 0
//   for j in 0 .. d-1:  dj = x[j] - mu[j]
//       for k in j .. d-1:  t = pp[tri(d, j, k)] * dj;  t = t * (x[k] - mu[k]);  q = q + t
//   ln prior = -0.5 * q
//
// Bits: products feed sums here - what a compiler contracts into fused multiply-adds.  lnprior() forbids it (hipcc: the pragma
// below; the CPU tests build with -ffp-contract=off), so hipcc, g++ and NumPy (elementwise over the rows, the same operations in
// the same order) produce the same bits from the same inputs.
//
// x is read through a getter, x(j): the callers pass a strided view of a chain's state, a stored proposal or x + dz.  Nothing
// here indexes a local array, so the device code needs no scratch; mu and pp are kernel arguments, read with scalar loads.
#pragma once

#if defined(__HIPCC__)
#define VK_PRIOR_HD __host__ __device__
#else
#define VK_PRIOR_HD
#endif

namespace vkprior {

constexpr int kMaxP = 10;              // sampled parameters, as vkfit::kMaxP and vkchain::kMaxP
constexpr int kMaxTri = kMaxP * (kMaxP + 1) / 2;

// position of (j, k), j <= k, in the packed upper triangle of a d x d matrix, row by row: vkchain::tri's order
VK_PRIOR_HD constexpr int tri(int d, int j, int k) { return j * d - j * (j - 1) / 2 + (k - j); }

struct Prior {
  int on;                              // 0: no prior (mu and pp are not read)
  double mu[kMaxP];                    // the mean, in sampled order (0 for a parameter without a prior)
  double pp[kMaxTri];                  // the packed upper triangle of the precision matrix, off-diagonal entries doubled
};

// ln prior at x(0) .. x(d - 1)
template <class Get>
VK_PRIOR_HD inline double lnprior(const Prior& p, int d, Get x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double q = 0.0;
  for (int j = 0; j < d; ++j) {
    const double dj = x(j) - p.mu[j];
    for (int k = j; k < d; ++k) {
      double t = p.pp[tri(d, j, k)] * dj;
      t = t * (x(k) - p.mu[k]);
      q = q + t;
    }
  }
  return -0.5 * q;
}

}  // namespace vkprior
