// vk_kernel_importance.h: the kernels of the importance-sampled posteriors (vk_is_run, include/victor_hip.h) - part of
// libvictor_hip.so (see vk_sampled.hip for the host side, vk_importance.h for the accumulator index rules, the list walk and the
// terms, vk_grid.h for the step they share with the grid, victor_amd/importance.py for the definition in NumPy, DESIGN.md section
// 7e for the mapping and the measurements).
//
// A chunk of n consecutive points g0 .. g0 + n - 1 of the uploaded sample goes through five launches on the context's stream:
//   vk_is_rows_kernel      one thread per point: reads x[g][.] and the host's eps^(-2/3) of the point and forms the parameter row
//                          through vkrow::form_rows - the row is CCFFit._fit_rows' bit for bit, epsilon sampled or not; of a
//                          joint handle with per-block axes a row per block (JointFit._block_rows' bit for bit): an axis goes to
//                          its own block's row, or to every block's
//   (the evaluation)       sampled_evaluate: lnL of the rows, [n] against the data vector or [n][R] against every realisation
//                          (of a joint fit: every joint realisation, under its covariance or block-diagonal)
//   vk_is_max_kernel       per problem the chunk's maximum of lnpost = lnL + lno[g], first arg max and finite count - the shape of
//                          vk_grid_max_kernel: up to 64 problems of a workgroup (problem the fastest-varying lane: the loads of a
//                          row of [n][R] coalesce) times 256 / 64 slices of the chunk, merged through LDS with vkgrid::merge
//                          (exact in any order) - then vkgrid::advance: M, arg max, count and the chunk's rescale factor
//   vk_is_weight_kernel    one thread per (point, problem): exp(lnpost - M), once, into the buffer the evaluation left its
//                          chi-squares in - every accumulator that holds the point reads this value
//   vk_is_accumulate_kernel  one thread per (accumulator, problem), problem the fastest-varying thread index: a row of [n][R]
//                          coalesces, and the lanes of a wave read the same list entry and the same y.  The thread rescales its
//                          accumulator (sq twice), then adds its terms one at a time in increasing g: total, sq, the d first and
//                          d (d + 1) / 2 second moments walk the whole chunk with kIsAhead loads in flight, a histogram or pair
//                          cell walks its list of the chunk with kIsListAhead.  No LDS, no atomics, no cross-thread
//                          floating-point reduction: the order of the additions is the definition's by construction, and two
//                          runs give the same bytes.
// With a prior its own problem (lnpost = lnop[g]; the total alone) rides along as problem R, as in the grid.
// exp is the library's: arguments <= 0 or -inf, within the 2.5 ULP tests/tolerances.py allows the device.
#pragma once
#include "vk_common.h"
#include "vk_importance.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kIsBlock = 256;
constexpr int kIsAhead = 16;           // loads a whole-chunk walk keeps in flight
constexpr int kIsListAhead = 4;        // ... a list walk
static_assert(vkis::kMaxP == vkrow::kMaxP, "a sample's axes are sampled parameters");

struct IsArgs {
  int d, R, Rp;                      // axes; problems; with the prior's own (R + 1 with a prior, else R; a proposal per problem: 2 R)
  int own;                           // 0: one sample for all problems; R: a proposal per problem (vk_kernel_is_own.h), values [G][R]
  long long G, g0;                   // the sample; the chunk: points g0 .. g0 + n - 1 are rows 0 .. n - 1
  int n;
  // rows kernel
  const double* x;                   // [G][d]
  const double* eps_pow;             // [G]: the host's eps^(-2/3) per point (NULL: epsilon is not sampled)
  const double* base;                // [VK_NPAR]; of a handle with a row per block (vk_is_create_joint_blocks) one base row per set
  double* rows;                      // [chunk][VK_NPAR]; ... a set per block, blocks.row_stride apart
  vkrow::Blocks blocks;              // the row sets and the set every axis is written to (one set: every axis to it)
  int col[vkis::kMaxP];
  double alpha;
  // values
  const double* y;                   // [G][d]
  const double* lno;                 // [G]
  const double* lnop;                // [G]: lnpost of the prior's own problem (NULL without one)
  const double* lnl;                 // [n][R]
  double* w;                         // [n][R]: the weights
  double* wp;                        // [n]: the weights of the prior's own problem
  // state
  vkgrid::Running* run;              // [Rp]
  double* acc;                       // [n_acc][Rp]: accumulator a of problem r at a Rp + r (the prior's own problem: a = 0 alone)
  int n_acc, whole, n_lists, pr;     // pr: problems of a workgroup of the max kernel (a power of two <= 64)
  const int* list;                   // [n_lists][G]: list l's segment of the chunk at l G + g0
  const int* off;                    // the chunk's offsets: list l's at cell_off[l] + l, one more than its cells
  int cell_off[vkis::kMaxLists + 1]; // the first cell of every list among the histogram cells, and their number
};

// lnpost of row i for problem r as every kernel reads it: one addition.  lno, lnop and the prior problems' weights are one value
// per point, or (a.own = R) one per point and problem: vkis::value_at names either
__device__ __forceinline__ double is_post(const IsArgs& a, int i, int r) {
  if (r >= a.R) return vkgrid::clean(a.lnop[vkis::value_at(a.g0 + i, r - a.R, a.own)]);
  double v = a.lnl[(size_t)i * a.R + r];
  v = v + a.lno[vkis::value_at(a.g0 + i, r, a.own)];
  return vkgrid::clean(v);
}
__device__ __forceinline__ double is_weight(const IsArgs& a, int i, int r) {
  return r < a.R ? a.w[(size_t)i * a.R + r] : a.wp[vkis::value_at(i, r - a.R, a.own)];
}

// the start of a run: nothing seen
__global__ void __launch_bounds__(kIsBlock) vk_is_init_kernel(IsArgs a) {
  const long long t = (long long)blockIdx.x * kIsBlock + threadIdx.x;
  if (t < a.Rp) a.run[t] = vkgrid::start();
  if (t < (long long)a.n_acc * a.Rp) a.acc[t] = 0.0;
}

__global__ void __launch_bounds__(kIsBlock) vk_is_rows_kernel(IsArgs a) {
  const int i = blockIdx.x * kIsBlock + threadIdx.x;
  if (i >= a.n) return;
  const long long g = a.g0 + i;
  const double* x = a.x + g * a.d;
  const double* eps_pow = a.eps_pow;
  // (block q's row at rows + q row_stride from its own base row; with one set the stores are those of vkrow::one_set())
  vkrow::form_rows(a.blocks, a.base, 0, a.rows, (long long)i, a.col, a.d, a.alpha, [=](int j) { return x[j]; },
                   [=](double) { return eps_pow[g]; });               // (called for a sampled epsilon only: shared by all blocks)
}

__global__ void __launch_bounds__(kIsBlock) vk_is_max_kernel(IsArgs a) {
  __shared__ double s_max[kIsBlock];
  __shared__ long long s_arg[kIsBlock], s_cnt[kIsBlock];
  const int pr = a.pr, slices = kIsBlock / pr;
  const int rl = threadIdx.x % pr, sl = threadIdx.x / pr;
  const int r = blockIdx.x * pr + rl;
  vkgrid::Best b = vkgrid::none();
  if (r < a.Rp)
    for (int i = sl; i < a.n; i += slices) vkgrid::see(b, is_post(a, i, r), a.g0 + i);
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

__global__ void __launch_bounds__(kIsBlock) vk_is_weight_kernel(IsArgs a) {
  const long long t = (long long)blockIdx.x * kIsBlock + threadIdx.x;
  if (t >= (long long)a.n * a.Rp) return;
  const int i = (int)(t / a.Rp), r = (int)(t - (long long)i * a.Rp);
  const double m = a.run[r].m;
  const double w = m > vkgrid::neg_inf() ? vkgrid::weight(is_post(a, i, r), m, [](double x) { return exp(x); }) : 0.0;
  if (r < a.R) a.w[(size_t)i * a.R + r] = w;
  else a.wp[vkis::value_at(i, r - a.R, a.own)] = w;
}

__global__ void __launch_bounds__(kIsBlock) vk_is_accumulate_kernel(IsArgs a) {
  const long long t = (long long)blockIdx.x * kIsBlock + threadIdx.x;
  const long long at = t / a.Rp;
  const int r = (int)(t - at * a.Rp);
  if (at >= a.n_acc) return;
  const int k = (int)at;
  if (r >= a.R && k != vkis::kTotal) return;             // (the prior's own problem keeps a total alone)
  const vkgrid::Running run = a.run[r];
  const bool live = run.m > vkgrid::neg_inf();           // (nothing finite yet: every accumulator stays where it started)
  double* slot = a.acc + (size_t)k * a.Rp + r;
  double acc = *slot;
  if (k == vkis::kSq) vkis::rescale_sq(acc, run.factor);
  else vkgrid::rescale(acc, run.factor);
  if (live) {
    auto add = [&](double v) { vkgrid::add(acc, v); };
    if (k == vkis::kTotal) {
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return is_weight(a, i, r); }, add);
    } else if (k == vkis::kSq) {
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return vkis::square_term(is_weight(a, i, r)); }, add);
    } else if (k < vkis::kFirst + a.d) {
      const double* yj = a.y + a.g0 * a.d + (k - vkis::kFirst);
      const int d = a.d;
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return vkis::first_term(is_weight(a, i, r), yj[(size_t)i * d]); }, add);
    } else if (k < a.whole) {
      int j, j2;
      vkis::second_of(a.d, k, j, j2);
      const double* y = a.y + a.g0 * a.d;
      const int d = a.d;
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return vkis::second_term(is_weight(a, i, r), y[(size_t)i * d + j], y[(size_t)i * d + j2]); },
                                  add);
    } else {
      const int c = k - a.whole;
      int l = 0;
      while (l + 1 < a.n_lists && c >= a.cell_off[l + 1]) ++l;
      const int* off = a.off + c + l;                    // (list l's offsets start at cell_off[l] + l; this cell is c - cell_off[l])
      const long long g0 = a.g0;
      vkis::walk_ahead<kIsListAhead>(a.list + (size_t)l * a.G + g0, off[0], off[1], g0, [&](long long g) { return is_weight(a, (int)(g - g0), r); },
                                     add);
    }
  }
  *slot = acc;
}

}  // namespace vk
