// Standalone accuracy check of the shared reciprocals of vk_devmath.h (vkm::recip_shared2 / 3 / 4) on the GPU:
//   hipcc --offload-arch=gfx950 -O3 -I victor_amd/csrc tools/shared_recip_check.hip -o tools/shared_recip_check
// 2^20 blocks of 2, 3 and 4 operands - magnitudes log-uniform in [2^-8, 2^8], mixed signs, and blocks made of the edge values
// 1, powers of two and the neighbours of 1 - against 1.0 / x in double on the host.  Every result is held to
//   (k + 1) 2^-53 + e_max^3,   k = the multiplies on that operand's path (vk_devmath.h),
// with e_max the worst seed error |1 - P rcp(P)| the same run measures on the same products.  Prints one JSON line: per width the
// worst error, its bound and the worst margin (error / bound), e_max, and whether the signs came out right.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#include "vk_devmath.h"

// out[4 * i + j] = 1 / x[4 * i + j] for the first `width` operands of block i; seed[i] = 1 - P rcp(P) of the block's product
__global__ void run_shared(const double* x, double* out, double* seed, int n, int width) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = x[4 * i], b = x[4 * i + 1], c = x[4 * i + 2], d = x[4 * i + 3];
  double ra = 0.0, rb = 0.0, rc = 0.0, rd = 0.0, P;
  if (width == 2) {
    vkm::recip_shared2(a, b, ra, rb);
    P = a * b;
  } else if (width == 3) {
    vkm::recip_shared3(a, b, c, ra, rb, rc);
    P = (a * b) * c;
  } else {
    vkm::recip_shared4(a, b, c, d, ra, rb, rc, rd);
    P = (a * b) * (c * d);
  }
  out[4 * i] = ra; out[4 * i + 1] = rb; out[4 * i + 2] = rc; out[4 * i + 3] = rd;
  seed[i] = fma(-P, __builtin_amdgcn_rcp(P), 1.0);
}

int main() {
  const int n = 1 << 20;
  std::vector<double> x(4 * (size_t)n);
  unsigned long long s = 88172645463325252ULL;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
  const double edge[] = {1.0, -1.0, 2.0, 0.5, 256.0, 1.0 / 256.0, -4.0, 0.0625, 1.0 + 0x1p-52, 1.0 - 0x1p-53, -(1.0 + 0x1p-52),
                         1.0 + 0x1p-51, 1.0 - 0x1p-52, 2.0 - 0x1p-52, 0.5 + 0x1p-53};
  const int n_edge = (int)(sizeof edge / sizeof edge[0]);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 4; ++j) {
      double v = exp2((rnd() * 2 - 1) * 8.0) * (rnd() < 0.5 ? -1.0 : 1.0);       // 2^-8 .. 2^8, either sign
      const double r = rnd();
      if (i < 4096 || r < 1.0 / 16) v = edge[(int)(rnd() * n_edge) % n_edge];      // blocks of edge values, and edge values among the others
      x[4 * (size_t)i + j] = v;
    }
  double *dx, *dout, *dseed;
  const size_t nb = 4 * (size_t)n * sizeof(double);
  if (hipMalloc(&dx, nb) != hipSuccess || hipMalloc(&dout, nb) != hipSuccess || hipMalloc(&dseed, n * sizeof(double)) != hipSuccess) return 2;
  hipMemcpy(dx, x.data(), nb, hipMemcpyHostToDevice);
  std::vector<double> out(4 * (size_t)n), seed(n);
  // multiplies on the path of operand j of a block of `width` (vk_devmath.h: those that make P and those that lead from y to the
  // result; the factors an operand shares with P cancel, so this counts more roundings than act)
  const int k_path[5][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {2, 2, 0, 0}, {4, 4, 3, 0}, {5, 5, 5, 5}};
  const double u = 0x1p-53;
  printf("{");
  int all_ok = 1;
  for (int width = 2; width <= 4; ++width) {
    hipLaunchKernelGGL(run_shared, dim3(n / 256), dim3(256), 0, 0, dx, dout, dseed, n, width);
    if (hipMemcpy(out.data(), dout, nb, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    hipMemcpy(seed.data(), dseed, n * sizeof(double), hipMemcpyDeviceToHost);
    double e_max = 0.0;
    for (int i = 0; i < n; ++i) e_max = fmax(e_max, fabs(seed[i]));
    double worst_err = 0.0, worst_bound = 0.0, worst_margin = 0.0;
    int signs_ok = 1;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < width; ++j) {
        const double xv = x[4 * (size_t)i + j], got = out[4 * (size_t)i + j];
        const double want = 1.0 / xv;                                       // the reference: double division on the host
        const double err = fabs(got - want) / fabs(want);
        const double bound = (k_path[width][j] + 1) * u + e_max * e_max * e_max;
        if (!(err / bound <= worst_margin)) { worst_margin = err / bound; worst_err = err; worst_bound = bound; }   // (a NaN sticks)
        signs_ok &= (std::signbit(got) == std::signbit(xv));
      }
    all_ok &= signs_ok && worst_margin <= 1.0;
    printf("\"w%d\": {\"err\": %.4e, \"bound\": %.4e, \"margin\": %.4f, \"e_max\": %.4e, \"signs_ok\": %d}, ", width, worst_err, worst_bound,
           worst_margin, e_max, signs_ok);
  }
  printf("\"blocks\": %d, \"ok\": %d}\n", n, all_ok);
  return 0;
}
