// vk_kernel_is_own.h: the kernels of importance-sampled posteriors with A PROPOSAL PER PROBLEM (vk_is_create_own,
// include/victor_hip.h) - part of libvictor_hip.so (see vk_sampled.hip for the host side, vk_importance.h for the layouts and the
// index rules host and device share, victor_amd/importance.py rule 8 for the definition in NumPy, DESIGN.md section 7e for the
// mapping).
//
// Every problem r has its own n points and is evaluated against realisation which[r]: a chunk of n consecutive points of every
// problem is n R rows, row i R + r point g0 + i of problem r.  Per chunk, on the context's stream:
//   vk_is_own_rows_kernel        one thread per (point, problem), the problem the fastest-varying index: reads x[g][r][.] and the
//                                host's eps^(-2/3) of the point and forms row i R + r through vkrow::form_rows from the one base
//                                row - CCFFit._fit_rows' bit for bit - and row_which[i R + r] = which[r]
//   (the evaluation)             sampled_evaluate in pairs mode over the n R rows: its [n R] output is the [n][R] array the max,
//                                weight and tail kernels of vk_kernel_importance.h / vk_kernel_is_tail.h read; they run as they
//                                are, with lno and lnop looked up at (g0 + i) R + r (IsArgs::own = R, vkis::value_at) and, under
//                                a prior, Rp = 2 R: problem R + r is problem r's prior problem
//   vk_is_own_accumulate_kernel  one thread per (accumulator, problem), the problem the fastest-varying index.  Totals and
//                                moments walk the chunk: the weights [n][R] and y [n][R][d] of the lanes of a wave are
//                                neighbours (the weights consecutive doubles, y d doubles apart).  A histogram or pair cell
//                                walks ITS OWN PROBLEM's list segment: the lanes read different lists at different lengths, so
//                                neither the entries nor the weights they name coalesce - the walk is G entries per list and
//                                problem over the whole run, small beside the n R theory evaluations, and left as it is.
//                                The additions go one at a time in increasing g with kIsAhead / kIsListAhead loads in flight.
//                                No LDS, no atomics, no cross-thread floating-point reduction: two runs give the same bytes.
#pragma once
#include "vk_kernel_importance.h"

namespace vk {

struct IsOwnArgs {
  IsArgs is;                         // the chunk as the shared kernels see it (is.own = R)
  const int* which;                  // [R]: the realisation of every problem
  int* row_which;                    // [chunk R]
  long long per_chunk;               // offsets of one problem in one chunk: cells + n_lists
};

__global__ void __launch_bounds__(kIsBlock) vk_is_own_rows_kernel(IsOwnArgs q) {
  const IsArgs& a = q.is;
  const long long t = (long long)blockIdx.x * kIsBlock + threadIdx.x;
  if (t >= (long long)a.n * a.R) return;
  const long long i = t / a.R;
  const int r = (int)(t - i * a.R);
  const long long at = vkis::value_at(a.g0 + i, r, a.R);
  const double* x = a.x + at * a.d;
  const double* eps_pow = a.eps_pow;
  vkrow::form_rows(vkrow::one_set(), a.base, 0, a.rows, vkis::own_row(i, r, a.R), a.col, a.d, a.alpha, [=](int j) { return x[j]; },
                   [=](double) { return eps_pow[at]; });              // (called for a sampled epsilon only)
  q.row_which[vkis::own_row(i, r, a.R)] = q.which[r];
}

__global__ void __launch_bounds__(kIsBlock) vk_is_own_accumulate_kernel(IsOwnArgs q) {
  const IsArgs& a = q.is;
  const long long t = (long long)blockIdx.x * kIsBlock + threadIdx.x;
  const long long at = t / a.Rp;
  const int r = (int)(t - at * a.Rp);
  if (at >= a.n_acc) return;
  const int k = (int)at;
  if (r >= a.R && k != vkis::kTotal) return;             // (a prior problem keeps a total alone)
  const int p = vkis::prior_of(r, a.R);                  // the problem whose points these are
  const vkgrid::Running run = a.run[r];
  const bool live = run.m > vkgrid::neg_inf();
  double* slot = a.acc + (size_t)k * a.Rp + r;
  double acc = *slot;
  if (k == vkis::kSq) vkis::rescale_sq(acc, run.factor);
  else vkgrid::rescale(acc, run.factor);
  if (live) {
    auto add = [&](double v) { vkgrid::add(acc, v); };
    const int R = a.R, d = a.d;
    const double* y = a.y + (a.g0 * R + p) * d;          // y of (g0 + i, p) at y[i R d + j]
    const size_t step = (size_t)R * d;
    if (k == vkis::kTotal) {
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return is_weight(a, i, r); }, add);
    } else if (k == vkis::kSq) {
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return vkis::square_term(is_weight(a, i, r)); }, add);
    } else if (k < vkis::kFirst + d) {
      const double* yj = y + (k - vkis::kFirst);
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return vkis::first_term(is_weight(a, i, r), yj[(size_t)i * step]); }, add);
    } else if (k < a.whole) {
      int j, j2;
      vkis::second_of(d, k, j, j2);
      vkis::range_ahead<kIsAhead>(0, a.n, [&](int i) { return vkis::second_term(is_weight(a, i, r), y[(size_t)i * step + j], y[(size_t)i * step + j2]); },
                                  add);
    } else {
      const int c = k - a.whole;
      int l = 0;
      while (l + 1 < a.n_lists && c >= a.cell_off[l + 1]) ++l;
      // (a.off: the chunk's offsets of problem 0; list l's start at cell_off[l] + l; this cell is c - cell_off[l])
      const int* off = a.off + vkis::own_offsets(0, r, R, q.per_chunk) + c + l;
      const long long g0 = a.g0;
      vkis::walk_ahead<kIsListAhead>(a.list + vkis::own_list(r, l, a.n_lists, a.G) + g0, off[0], off[1], g0,
                                     [&](long long g) { return is_weight(a, (int)(g - g0), r); }, add);
    }
  }
  *slot = acc;
}

}  // namespace vk
