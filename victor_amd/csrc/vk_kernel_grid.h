// vk_kernel_grid.h: the kernels of the grid posteriors (vk_grid_run, include/victor_hip.h) - part of libvictor_hip.so (see
// vk_sampled.hip for the host side, vk_grid.h for the index rules and the step, victor_amd/grid.py for the definition in NumPy,
// DESIGN.md section 7c for the mapping and the measurements).
//
// A chunk of n consecutive flat indices g0 .. g0 + n - 1 goes through five launches on the context's stream:
//   vk_grid_rows_kernel    one thread per grid point: decodes the flat index, LOOKS the nodes UP (the host's arrays are the
//                          definition: nothing recomputes a node), forms the parameter row through vkrow::form_rows - an epsilon
//                          axis with the host's own eps^(-2/3) of the node, so the row is CCFFit._fit_rows' bit for bit - and,
//                          with a prior, stores ln prior of the point (vkprior::lnprior)
//   (the evaluation)       sampled_evaluate: lnL of the rows, [n] against the data vector or [n][R] against every realisation
//   vk_grid_max_kernel     per problem the chunk's maximum, first arg max and finite count - a workgroup takes up to 64 problems
//                          (problem the fastest-varying lane: the loads of a row of [n][R] coalesce) times 256 / 64 slices of the
//                          chunk, merged through LDS with vkgrid::merge (exact in any order) - then the running state: M, arg
//                          max, count and the chunk's rescale factor, ONE exp per problem and chunk
//   vk_grid_weight_kernel  one thread per (point, problem): exp(lnpost - M), once, into the buffer the evaluation left its
//                          chi-squares in (the grid does not read them) - every accumulator that holds the point adds this value
//   vk_grid_accumulate_kernel  one thread per (cell, problem), problem the fastest-varying thread index: rescales its accumulator,
//                          then walks its cell's runs of indices of the chunk in increasing order (vkgrid::for_axis_runs /
//                          for_pair_runs), adding the weights one at a time and taking the maximum of lnpost - the loads of a
//                          few consecutive indices are issued together (a thread's walk is a chain of additions; the loads
//                          need not wait for it), the additions keep their order.  No LDS, no
//                          atomics, no cross-thread reduction: the order of the additions is the definition's by construction,
//                          and two runs give the same bytes.
// With a prior the Gaussian's own midpoint sum over the grid rides along as problem R (lnpost = ln prior; its total alone).
// exp is the library's: arguments <= 0 or -inf, within the 2.5 ULP tests/tolerances.py allows the device.
#pragma once
#include "vk_common.h"
#include "vk_grid.h"
#include "vk_prior.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kGridBlock = 256;
constexpr int kGridAhead = 32;         // loads the total's walk keeps in flight (vk_grid_accumulate_kernel)
static_assert(vkgrid::kMaxP == vkrow::kMaxP && vkgrid::kMaxP == vkprior::kMaxP, "a grid's axes are sampled parameters");

struct GridArgs {
  vkgrid::Shape shape;
  int R, Rp;                         // problems; with the prior's own (R + 1 with a prior, else R)
  long long g0;                      // the chunk: flat indices g0 .. g0 + n - 1 are rows 0 .. n - 1
  int n;
  // rows kernel
  const double* nodes;               // the axes' nodes, concatenated; axis j at axis_off[j]
  const double* eps_pow;             // [n of the epsilon axis]: the host's eps^(-2/3) per node (NULL: no epsilon axis)
  const double* base;                // [VK_NPAR]
  double* rows;                      // [chunk][VK_NPAR]
  int col[vkgrid::kMaxP];
  double alpha;
  vkprior::Prior prior;
  double* lnprior;                   // [chunk]: written with a prior only
  // values
  const double* lnl;                 // [n][R]
  double* w;                         // [n][R]: the weights
  double* wp;                        // [n]: the weights of the prior's own problem
  // state
  vkgrid::Running* run;              // [Rp]
  double* total;                     // [Rp]
  double *m1, *p1;                   // [R][n1], n1 = sum of the axes' nodes
  double *m2, *p2;                   // [R][n2], n2 = sum over the pairs of na nb
  int n1, n2, n_pairs, pr;           // pr: problems of a workgroup of the max kernel (a power of two <= 64)
  int axis_off[vkgrid::kMaxP];
  int pair[vkgrid::kMaxPairs][2];    // (ja < jb)
  int pair_off[vkgrid::kMaxPairs];
};

// lnpost of row i for problem r as every kernel reads it: one addition with a prior, the value itself without
__device__ __forceinline__ double grid_post(const GridArgs& a, int i, int r) {
  if (r >= a.R) return vkgrid::clean(a.lnprior[i]);
  double v = a.lnl[(size_t)i * a.R + r];
  if (a.prior.on) v = v + a.lnprior[i];
  return vkgrid::clean(v);
}
__device__ __forceinline__ double grid_weight(const GridArgs& a, int i, int r) { return r < a.R ? a.w[(size_t)i * a.R + r] : a.wp[i]; }

// the start of a run: nothing seen
__global__ void __launch_bounds__(kGridBlock) vk_grid_init_kernel(GridArgs a) {
  const long long t = (long long)blockIdx.x * kGridBlock + threadIdx.x;
  if (t < a.Rp) {
    a.run[t] = vkgrid::start();
    a.total[t] = 0.0;
  }
  if (t < (long long)a.R * a.n1) {
    a.m1[t] = 0.0;
    a.p1[t] = vkgrid::neg_inf();
  }
  if (t < (long long)a.R * a.n2) {
    a.m2[t] = 0.0;
    a.p2[t] = vkgrid::neg_inf();
  }
}

__global__ void __launch_bounds__(kGridBlock) vk_grid_rows_kernel(GridArgs a) {
  const int i = blockIdx.x * kGridBlock + threadIdx.x;
  if (i >= a.n) return;
  const long long g = a.g0 + i;
  const double* nodes = a.nodes;
  auto value = [&](int j) { return nodes[a.axis_off[j] + vkgrid::node(a.shape, j, g)]; };
  int eps_axis = 0;
  for (int j = 0; j < a.shape.d; ++j)
    if (a.col[j] < 0) eps_axis = j;
  const double* eps_pow = a.eps_pow;
  const int k_eps = vkgrid::node(a.shape, eps_axis, g);
  vkrow::form_rows(vkrow::one_set(), a.base, 0, a.rows, (long long)i, a.col, a.shape.d, a.alpha, value,
                   [=](double) { return eps_pow[k_eps]; });          // (called for an epsilon axis only)
  if (a.prior.on) a.lnprior[i] = vkprior::lnprior(a.prior, a.shape.d, value);
}

__global__ void __launch_bounds__(kGridBlock) vk_grid_max_kernel(GridArgs a) {
  __shared__ double s_max[kGridBlock];
  __shared__ long long s_arg[kGridBlock], s_cnt[kGridBlock];
  const int pr = a.pr, slices = kGridBlock / pr;
  const int rl = threadIdx.x % pr, sl = threadIdx.x / pr;
  const int r = blockIdx.x * pr + rl;
  vkgrid::Best b = vkgrid::none();
  if (r < a.Rp)
    for (int i = sl; i < a.n; i += slices) vkgrid::see(b, grid_post(a, i, r), a.g0 + i);
  s_max[threadIdx.x] = b.max;
  s_arg[threadIdx.x] = b.arg;
  s_cnt[threadIdx.x] = b.n_finite;
  __syncthreads();
  if (sl != 0 || r >= a.Rp) return;
  for (int s = 1; s < slices; ++s) {
    const int at = s * pr + rl;
    b = vkgrid::merge(b, vkgrid::Best{s_max[at], s_arg[at], s_cnt[at]});
  }
  vkgrid::Running run = a.run[r];
  vkgrid::advance(run, b, [](double x) { return exp(x); });
  a.run[r] = run;
}

__global__ void __launch_bounds__(kGridBlock) vk_grid_weight_kernel(GridArgs a) {
  const long long t = (long long)blockIdx.x * kGridBlock + threadIdx.x;
  if (t >= (long long)a.n * a.Rp) return;
  const int i = (int)(t / a.Rp), r = (int)(t - (long long)i * a.Rp);
  const double m = a.run[r].m;
  const double w = m > vkgrid::neg_inf() ? vkgrid::weight(grid_post(a, i, r), m, [](double x) { return exp(x); }) : 0.0;
  if (r < a.R) a.w[(size_t)i * a.R + r] = w;
  else a.wp[i] = w;
}

__global__ void __launch_bounds__(kGridBlock) vk_grid_accumulate_kernel(GridArgs a) {
  const long long t = (long long)blockIdx.x * kGridBlock + threadIdx.x;
  const long long cell = t / a.Rp;
  const int r = (int)(t - cell * a.Rp);
  if (cell >= 1 + (long long)a.n1 + a.n2) return;
  const vkgrid::Running run = a.run[r];
  const bool live = run.m > vkgrid::neg_inf();         // (nothing finite yet: every accumulator stays where it started)
  const long long g0 = a.g0, g1 = a.g0 + a.n;
  if (cell == 0) {
    double acc = a.total[r];
    vkgrid::rescale(acc, run.factor);
    if (live) {
      // The longest walk of the launch (the whole chunk): kGridAhead loads in flight, then their additions in order.  The two
      // inner loops unroll completely, so w[] lives in registers.
      int i = 0;
      for (; i + kGridAhead <= a.n; i += kGridAhead) {
        double w[kGridAhead];
#pragma unroll
        for (int u = 0; u < kGridAhead; ++u) w[u] = grid_weight(a, i + u, r);
#pragma unroll
        for (int u = 0; u < kGridAhead; ++u) vkgrid::add(acc, w[u]);
      }
      for (; i < a.n; ++i) vkgrid::add(acc, grid_weight(a, i, r));
    }
    a.total[r] = acc;
    return;
  }
  if (r >= a.R) return;                                // (the prior's own problem keeps a total alone)
  int c = (int)(cell - 1);
  double *macc, *pacc;
  int ja, ka, jb = -1, kb = 0;
  if (c < a.n1) {
    ja = 0;
    while (ja + 1 < a.shape.d && c >= a.axis_off[ja + 1]) ++ja;
    ka = c - a.axis_off[ja];
    macc = a.m1 + (size_t)r * a.n1 + c;
    pacc = a.p1 + (size_t)r * a.n1 + c;
  } else {
    c -= a.n1;
    int q = 0;
    while (q + 1 < a.n_pairs && c >= a.pair_off[q + 1]) ++q;
    ja = a.pair[q][0];
    jb = a.pair[q][1];
    const int at = c - a.pair_off[q];
    ka = at / a.shape.n[jb];
    kb = at - ka * a.shape.n[jb];
    macc = a.m2 + (size_t)r * a.n2 + c;
    pacc = a.p2 + (size_t)r * a.n2 + c;
  }
  double acc = *macc, p = *pacc;
  vkgrid::rescale(acc, run.factor);
  if (live) {
    auto visit = [&](long long lo, long long hi) {     // a run of consecutive indices: four loads in flight, additions in order
      int i = (int)(lo - g0);
      const int i1 = (int)(hi - g0);
      for (; i + 4 <= i1; i += 4) {
        const double w0 = grid_weight(a, i, r), w1 = grid_weight(a, i + 1, r), w2 = grid_weight(a, i + 2, r), w3 = grid_weight(a, i + 3, r);
        const double v0 = grid_post(a, i, r), v1 = grid_post(a, i + 1, r), v2 = grid_post(a, i + 2, r), v3 = grid_post(a, i + 3, r);
        vkgrid::add(acc, w0);
        vkgrid::add(acc, w1);
        vkgrid::add(acc, w2);
        vkgrid::add(acc, w3);
        vkgrid::take_max(p, v0);
        vkgrid::take_max(p, v1);
        vkgrid::take_max(p, v2);
        vkgrid::take_max(p, v3);
      }
      for (; i < i1; ++i) {
        vkgrid::add(acc, grid_weight(a, i, r));
        vkgrid::take_max(p, grid_post(a, i, r));
      }
    };
    if (jb < 0) vkgrid::for_axis_runs(a.shape, ja, ka, g0, g1, visit);
    else vkgrid::for_pair_runs(a.shape, ja, ka, jb, kb, g0, g1, visit);
  }
  *macc = acc;
  *pacc = p;
}

}  // namespace vk
