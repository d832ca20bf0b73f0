// vk_kernel_nested.h: nested sampling of vk_nested_begin (include/victor_hip.h) on the device - part of libvictor_hip.so (see
// vk_sampled.hip for the host side, DESIGN.md section 7d for the algorithm, vk_nested_step.h for the rules).
//
// R problems of L live points each; per iteration K walkers per problem replace the K lowest points.  Live points are held
// structure-of-arrays over all problems (x[j][r L + i]), walkers likewise (y[j][r K + k]): the 64 lanes of a wave touch
// consecutive doubles.  Row r K + k of every launch of a run is walker k of problem r.
//
//   vk_nested_load_kernel / vk_nested_adopt_kernel   the start: pass p evaluates live points p K .. p K + K - 1 of every problem
//   vk_nested_select_kernel   one workgroup per problem: the live ranges (a min and a max per wave by lane exchange, the waves'
//                             through LDS), the rank of every live point by counting over the problem's lnL held in LDS (every
//                             lane of a wave reads the same word: a broadcast, no bank conflict, no divergence), the dead
//                             record, L*, the survivors in increasing index, the walkers' starts and their first rows
//   vk_nested_step_kernel     one thread per walker: decides on the row just evaluated, moves, writes its next row
//   vk_nested_commit_kernel   one thread per walker: the walker into its dead point's slot
// Between the launches the library evaluates the R K rows (sampled_evaluate).  A thread writes only its own walker, slot or
// record: no atomics, and every value a kernel indexes with was checked by the host (vk_nested_create) or is a rank < L.
//
// Every kernel is a template over its argument struct: NestedArgs (no prior) or NestedPriorArgs, which adds a vkprior::Prior by
// value (about 0.5 KiB of kernel arguments, read with scalar loads, as the chain kernels read theirs) and the ln prior of the
// live points, of the walkers and of the dead record.  `if constexpr (Args::kPrior)` keeps the prior's work out of the
// NestedArgs instantiations altogether: they are the kernels they were.  Under a prior the select kernel's s_lnl holds
// lnpost = lnL + ln prior (one rounded addition; no further LDS), L* is an lnpost, and the step kernel decides on the sum
// (the prior forms of vknest::transition / commit).  ln prior is always taken at the point's own sampled values - in a handle
// that blends in beta, at the point's own beta, never at the split rows' grid beta.
#pragma once
#include "vk_common.h"
#include "vk_nested_step.h"
#include "vk_prior.h"
#include "vk_sampled_row.h"

namespace vk {

constexpr int kNestedBlock = 64;           // threads per workgroup of the per-walker kernels: one wave
constexpr int kNestedSelect = 256;         // ... of the select kernel: four waves per problem
constexpr int kNestedWaves = kNestedSelect / 64;

struct NestedArgs {
  static constexpr bool kPrior = false;
  vkchain::Box box;
  int R, L, K;              // problems, live points of each, walkers of each
  double scale;
  double* lx;               // [d][R L]: the live points
  double* llnl;             // [R L]
  double* lchi;             // [R L]
  double* wx;               // [d][R K]: the walkers
  double* wlnl;             // [R K]
  double* wchi;             // [R K]
  int* wslot;               // [R K]: live index of the dead point walker k replaces
  int* wmoved;              // [R K]: accepted steps of the current iteration
  long long* n_accept;      // [R K]
  long long* n_steps;       // [R K]
  long long* n_stuck;       // [R K]
  double* lstar;            // [R]
  double* range;            // [d][R]
  const double* base;       // [R K][VK_NPAR]: fixed parameters and defaults of each row (per row set)
  const int* which;         // [R K]: realisation of each row, or NULL
  double* rows;             // [R K][VK_NPAR]: the next launch's rows (per row set)
  int* row_which;           // [R K], or NULL
  const double* res_lnl;    // [R K]: results of the launch just evaluated
  const double* res_chi2;
  const double* x0;         // [R][L][d]: the start (load kernel)
  int pass;                 // ... and which K of every problem's L points the launch holds
  const double* pick;       // [R K]: the iteration's survivor picks (select kernel)
  const double* dz;         // [R K][d]: increments of the step being decided (step kernel) / first proposed (select kernel)
  const double* dz_next;    // [R K][d]: increments of the following step, or NULL: the iteration ends
  double* dead_lnl;         // [R K]: the iteration's dead record
  double* dead_chi2;        // [R K]
  double* dead_x;           // [R K][d], or NULL
  int col[vknest::kMaxP];
  double alpha;
  vkrow::Blocks blocks;
};

struct NestedPriorArgs : NestedArgs {
  static constexpr bool kPrior = true;
  vkprior::Prior prior;
  double* llp;              // [R L]: ln prior of the live points
  double* wlp;              // [R K]: ... of the walkers
  double* dead_lp;          // [R K]: ... of the iteration's dead record
};

__device__ __forceinline__ vknest::Walker nested_walker(const NestedArgs& a, int c) {
  vknest::Walker w;
  w.stride = (size_t)a.R * a.K;
  w.y = a.wx + c;
  w.lnl = a.wlnl + c;
  w.chi2 = a.wchi + c;
  w.n_accept = reinterpret_cast<int64_t*>(a.n_accept + c);
  w.n_steps = reinterpret_cast<int64_t*>(a.n_steps + c);
  w.n_stuck = reinterpret_cast<int64_t*>(a.n_stuck + c);
  w.moved = a.wmoved + c;
  w.lnprior = nullptr;
  return w;
}
__device__ __forceinline__ vknest::Walker nested_walker(const NestedPriorArgs& a, int c) {
  vknest::Walker w = nested_walker(static_cast<const NestedArgs&>(a), c);
  w.lnprior = a.wlp + c;
  return w;
}

// the row of walker c at y (dz given and the proposal inside the box: at the proposal)
template <class Range>
__device__ __forceinline__ void nested_emit(const NestedArgs& a, const vknest::Walker& w, int c, Range range, const double* dz) {
  const bool move = dz != nullptr && vknest::proposal_inside(a.box, w, a.scale, range, dz);
  sampled_row(a.blocks, a.base, (size_t)c, a.rows, (size_t)c, a.col, a.box.d, a.alpha, [&](int j) {
    const double v = w.y[j * w.stride];
    return move ? vknest::proposed(v, a.scale, range(j), dz[j]) : v;
  });
  if (a.row_which) a.row_which[c] = a.which[c];
}

// the start, pass p: live point p K + k of problem r becomes row r K + k (and, on pass 0, fresh counters)
template <class Args>
__global__ void __launch_bounds__(kNestedBlock) vk_nested_load_kernel(Args a) {
  const int c = blockIdx.x * kNestedBlock + threadIdx.x;
  if (c >= a.R * a.K) return;
  const int r = c / a.K, k = c - r * a.K, d = a.box.d;
  const size_t at = (size_t)r * a.L + (size_t)a.pass * a.K + k, RL = (size_t)a.R * a.L;
  for (int j = 0; j < d; ++j) a.lx[j * RL + at] = a.x0[at * d + j];
  sampled_row(a.blocks, a.base, (size_t)c, a.rows, (size_t)c, a.col, d, a.alpha, [&](int j) { return a.x0[at * d + j]; });
  if (a.row_which) a.row_which[c] = a.which[c];
  if (a.pass == 0) {
    a.n_accept[c] = 0;
    a.n_steps[c] = 0;
    a.n_stuck[c] = 0;
    a.wmoved[c] = 0;
    a.wslot[c] = 0;
  }
}

template <class Args>
__global__ void __launch_bounds__(kNestedBlock) vk_nested_adopt_kernel(Args a) {
  const int c = blockIdx.x * kNestedBlock + threadIdx.x;
  if (c >= a.R * a.K) return;
  const int r = c / a.K, k = c - r * a.K;
  const size_t at = (size_t)r * a.L + (size_t)a.pass * a.K + k;
  a.llnl[at] = vkchain::stored(a.res_lnl[c]);
  a.lchi[at] = a.res_chi2[c];
  if constexpr (Args::kPrior) {
    const size_t RL = (size_t)a.R * a.L;
    a.llp[at] = vkprior::lnprior(a.prior, a.box.d, [&](int j) { return a.lx[j * RL + at]; });
  }
}

// one workgroup per problem (blockIdx.x = r)
template <class Args>
__global__ void __launch_bounds__(kNestedSelect) vk_nested_select_kernel(Args a) {
  __shared__ double s_lnl[vknest::kMaxLive];
  __shared__ int s_surv[vknest::kMaxLive];                 // the survivors' live indices, increasing
  __shared__ int s_dead[vknest::kMaxLive / 2];             // the live index of dead point k
  __shared__ double s_lo[kNestedWaves], s_hi[kNestedWaves];
  __shared__ double s_range[vknest::kMaxP];
  const int r = blockIdx.x, tid = threadIdx.x, L = a.L, K = a.K, d = a.box.d;
  const size_t RL = (size_t)a.R * L, first = (size_t)r * L;
  for (int i = tid; i < L; i += kNestedSelect) {
    if constexpr (Args::kPrior) s_lnl[i] = a.llnl[first + i] + a.llp[first + i];      // lnpost: what is ordered and constrained
    else s_lnl[i] = a.llnl[first + i];
    s_surv[i] = 0;                                         // (every index read below is one of the problem's, whatever lnL holds)
    if (i < K) s_dead[i] = 0;
  }
  // the ranges: per parameter a min and a max over the live points
  for (int j = 0; j < d; ++j) {
    const double* x = a.lx + j * RL + first;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (int i = tid; i < L; i += kNestedSelect) {
      const double v = x[i];
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const double lo2 = __shfl_xor(lo, m, 64), hi2 = __shfl_xor(hi, m, 64);
      lo = lo2 < lo ? lo2 : lo;
      hi = hi2 > hi ? hi2 : hi;
    }
    if ((tid & 63) == 0) {
      s_lo[tid >> 6] = lo;
      s_hi[tid >> 6] = hi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kNestedWaves; ++w) {
        lo = s_lo[w] < lo ? s_lo[w] : lo;
        hi = s_hi[w] > hi ? s_hi[w] : hi;
      }
      const double range = hi - lo;
      s_range[j] = range;
      a.range[(size_t)j * a.R + r] = range;
    }
    __syncthreads();
  }
  // ranks: the K lowest in (lnL, index) are the dead points, in that order  (s_lnl is complete: the barriers above)
  for (int i = tid; i < L; i += kNestedSelect) {
    const int rank = vknest::rank_of(L, i, [&](int m) { return s_lnl[m]; });
    if (rank < K) s_dead[rank] = i;
  }
  __syncthreads();
  // the survivors in increasing index: survivor i stands at i minus the dead points in front of it
  for (int i = tid; i < L; i += kNestedSelect) {
    int front = 0;
    bool dead = false;
    for (int k = 0; k < K; ++k) {
      const int at = s_dead[k];
      front += at < i ? 1 : 0;
      dead = dead || at == i;
    }
    if (!dead && front <= i) s_surv[i - front] = i;      // (front <= i whenever the ranks are a permutation: lnL holds no NaN)
  }
  __syncthreads();
  // the dead record, L*, and the walkers: their starts and first rows
  for (int k = tid; k < K; k += kNestedSelect) {
    const int c = r * K + k;
    const int gone = s_dead[k];
    if constexpr (Args::kPrior) {
      a.dead_lnl[c] = a.llnl[first + gone];
      a.dead_lp[c] = a.llp[first + gone];
    } else {
      a.dead_lnl[c] = s_lnl[gone];
    }
    a.dead_chi2[c] = a.lchi[first + gone];
    if (a.dead_x)
      for (int j = 0; j < d; ++j) a.dead_x[(size_t)c * d + j] = a.lx[j * RL + first + gone];
    a.wslot[c] = gone;
    if (k == K - 1) a.lstar[r] = s_lnl[gone];
    const int from = s_surv[vknest::pick_of(a.pick[c], L, K)];
    vknest::Walker w = nested_walker(a, c);
    if constexpr (Args::kPrior) {
      vknest::start(d, w, [&](int j) { return a.lx[j * RL + first + from]; }, a.llnl[first + from], a.lchi[first + from]);
      *w.lnprior = a.llp[first + from];
    } else {
      vknest::start(d, w, [&](int j) { return a.lx[j * RL + first + from]; }, s_lnl[from], a.lchi[first + from]);
    }
    nested_emit(a, w, c, [&](int j) { return s_range[j]; }, a.dz + (size_t)c * d);
  }
}

// one constrained step per walker, then the walker's next row
template <class Args>
__global__ void __launch_bounds__(kNestedBlock) vk_nested_step_kernel(Args a) {
  const int c = blockIdx.x * kNestedBlock + threadIdx.x;
  if (c >= a.R * a.K) return;
  const int r = c / a.K, d = a.box.d;
  vknest::Walker w = nested_walker(a, c);
  auto range = [&](int j) { return a.range[(size_t)j * a.R + r]; };
  if constexpr (Args::kPrior)
    vknest::transition(a.box, a.prior, w, a.scale, range, a.dz + (size_t)c * d, a.lstar[r], a.res_lnl[c], a.res_chi2[c]);
  else
    vknest::transition(a.box, w, a.scale, range, a.dz + (size_t)c * d, a.lstar[r], a.res_lnl[c], a.res_chi2[c]);
  if (a.dz_next) nested_emit(a, w, c, range, a.dz_next + (size_t)c * d);
}

// the walkers into the slots of their dead points
template <class Args>
__global__ void __launch_bounds__(kNestedBlock) vk_nested_commit_kernel(Args a) {
  const int c = blockIdx.x * kNestedBlock + threadIdx.x;
  if (c >= a.R * a.K) return;
  const int r = c / a.K;
  const size_t at = (size_t)r * a.L + a.wslot[c];
  vknest::Walker w = nested_walker(a, c);
  if constexpr (Args::kPrior) vknest::commit(a.box.d, w, a.lx + at, (size_t)a.R * a.L, a.llnl + at, a.lchi + at, a.llp + at);
  else vknest::commit(a.box.d, w, a.lx + at, (size_t)a.R * a.L, a.llnl + at, a.lchi + at);
}

}  // namespace vk
