// vk_sampled.hip - the drivers of libvictor_hip.so that step sets of sampled-parameter problems on the device: best fits
// (vk_fit_*) and Metropolis chains (vk_chain_*) of the C ABI (include/victor_hip.h), and what they share.  A problem names the
// row columns it samples inside a prior box, over a base row of its own, against the context's data vector or one of its
// realisations; its rows are formed on the device (vk_sampled_row.h) and evaluated by victor_hip.hip, which this unit reaches
// through vk_eval_batch_device_async and, in vk_host.h, enqueue_realisations / check_real_lds.  A handle made by
// vk_fit_create_joint / vk_chain_create_joint runs the same loops over a joint fit of several contexts - block-diagonal or under
// one covariance handle, against the blocks' data vectors or joint realisation which[i] (that realisation of every block) -
// through the joint entry points and their enqueue-only twins against realisations (vk_host.h).  vk_fit_set_prior /
// vk_chain_set_prior give any of these handles a Gaussian prior (vk_prior.h) that its step kernels add to lnL.  Their _blocks forms keep a row
// set per block (base rows and pending rows, par_stride() apart) and write each sampled parameter to the block it belongs to, or
// to all of them (vk_row_select.h); a handle of the other create calls has one row set and makes the launches it always made.
// The same object serves every flavour of the library.
//
// Host code, top to bottom: `Sampled` and what both kinds of handle share - Carve / carve_alloc lay every allocation out,
// sampled_create, sampled_ready, sampled_evaluate, sampled_launch makes every launch of the unit and sampled_home every download -;
// best fits, their Hessians and Fisher matrices; chains, whose optional state (marginals, autocorrelation, tempering, predictive sums, the stretch
// buffers) a DevBlock each owns, with the refusals the chain entry points share and the check, the history slot of a step and
// the ending of the three begin calls stated once.
//
// Device code lives in the headers next to this file:
//   vk_sampled_row.h     a parameter row from a base row and the sampled values
//   vk_kernel_fit.h      the best-fit search (vk_fit_run): start simplex, step and re-layout kernels, one thread per problem, over
//                        the one-problem transition of vk_fit_simplex.h (plain C++, also compiled on its own by the CPU tests)
//   vk_kernel_chain.h    Metropolis chains of the data vector or one realisation each (vk_chain_begin): start, propose and step
//                        kernels, one thread per chain, over the one-chain transition of vk_chain_step.h (plain C++, likewise)
//   vk_kernel_stretch.h  stretch-move ensembles on the same handles (vk_chain_begin_stretch): propose and step kernels of a
//                        half-step, one thread per moving walker, over the transition of vk_stretch_step.h (plain C++, likewise)
//   vk_prior.h           the Gaussian prior of the sampled parameters that the three step kernels add to lnL (plain C++, likewise)
//   vk_marginals.h       the binning rule of the marginal histograms the two chain step kernels count kept positions in
//                        (vk_chain_set_marginals; plain C++, likewise)
//   vk_kernel_autocorr.h the series kernel behind the step kernel of every kept step: the per-step sum over a problem's chains and
//                        its lagged products (vk_chain_set_autocorr), over the update of vk_autocorr.h (plain C++, likewise)
//   vk_kernel_hessian.h  the central-difference stencil of vk_fit_hessian on a best-fit handle: a rows kernel, one thread per
//                        stencil row, and an assemble kernel, one wave per problem, over the statistic of vk_hessian.h (plain
//                        C++, likewise)
//   vk_kernel_fisher.h   the Jacobian stencil of vk_fit_fisher on the same handles: a rows kernel, one thread per stencil row, and
//                        an assemble kernel, one workgroup per problem, which forms J^T P J from the rows' theory vectors over the
//                        statistic of vk_fisher.h (plain C++, likewise)
//   vk_kernel_temper.h   replica exchange on the same handles (vk_chain_begin_tempered): the tempered step kernel, one thread per
//                        chain, and the swap kernel, one thread per candidate pair of neighbouring rungs, over the transition,
//                        energy sums and swap of vk_temper_step.h (plain C++, likewise)
//   vk_kernel_predictive.h the posterior-predictive sums (vk_chain_set_predictive): the hold kernel behind every step kernel, one
//                        wave per row, which keeps each chain's theory vector, and the predict kernel behind every kept step, one
//                        thread per (problem, entry), over the rules of vk_predictive.h (plain C++, likewise)
//   vk_kernel_grid.h     grid posteriors (vk_grid_run; the third section from the end of this file): rows, max, weight and accumulate kernels of
//                        a chunk of grid points, over the index rules and the step of vk_grid.h (plain C++, likewise)
//   vk_kernel_importance.h importance-sampled posteriors (vk_is_run; the section behind the grid's): rows, max, weight and accumulate
//                        kernels of a chunk of an uploaded sample, over the index rules, the list walk and the terms of
//                        vk_importance.h (plain C++, likewise)
//   vk_kernel_is_own.h   ... with a proposal per problem (vk_is_create_own): the rows and accumulate kernels over [n][R] rows in
//                        pairs mode; the max, weight and tail kernels are the shared sample's, with a stride
//   vk_kernel_is_predict.h the posterior-predictive sums of an importance handle (vk_is_set_predictive): the product kernel behind
//                        every chunk's accumulate kernel, weights x theory vectors, over the tile and index rules and the terms
//                        of vk_is_predict.h (plain C++, likewise)
//   vk_kernel_is_tail.h  the tail of an importance handle (vk_is_set_tail): behind every chunk's max kernel the filter kernel, a
//                        thread per (slice of the chunk, problem), and the merge kernel, one workgroup per problem, which keep
//                        each problem's K largest lnpost and their points, over the order, the slices and the merge positions of
//                        vk_is_tail.h (plain C++, likewise)
//   vk_kernel_nested.h   nested sampling (vk_nested_begin; the last section of this file): the select kernel, one workgroup per
//                        problem, and the step and commit kernels, one thread per replacement walker, over the order, the pick,
//                        the constrained step and the commit of vk_nested_step.h (plain C++, likewise)
//   vk_kernel_blend.h    likelihood-level beta interpolation on any single-fit handle (VK_OPT_BETA_BLEND; sampled_evaluate_blend):
//                        the split kernel, one thread per pending row, and the merge kernel, one thread per output, around the
//                        unchanged evaluation of twice the rows

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "victor_hip.h"
#include "vk_host.h"
#include "vk_kernel_fit.h"
#include "vk_kernel_chain.h"
#include "vk_kernel_stretch.h"
#include "vk_kernel_temper.h"
#include "vk_kernel_autocorr.h"
#include "vk_kernel_predictive.h"
#include "vk_kernel_hessian.h"
#include "vk_kernel_fisher.h"
#include "vk_kernel_grid.h"
#include "vk_kernel_importance.h"
#include "vk_kernel_is_own.h"
#include "vk_kernel_is_predict.h"
#include "vk_kernel_is_tail.h"
#include "vk_kernel_nested.h"
#include "vk_kernel_blend.h"

using namespace vk;
using vkh::check_joint;
using vkh::check_opts;
using vkh::check_real_lds;
using vkh::enqueue_realisations;
using vkh::sync_knobs;

// ---- the shared core: a set of sampled-parameter problems on a context ---------------------------------------------------------
constexpr int kSampledMax = 65536;         // problems (chains) of one handle
constexpr int kSampledMaxP = vkfit::kMaxP;
static_assert(vkchain::kMaxP == kSampledMaxP && vkrow::kMaxP == kSampledMaxP, "best fits and chains sample the same columns");

struct Sampled {
  vk_ctx* ctx = nullptr;                   // of a joint fit: the lead block's (its stream carries the loop)
  std::vector<vk_ctx*> blocks;             // a joint fit's contexts in block order, blocks[0] == ctx (empty: a single fit)
  vk_joint_cov* cov = nullptr;             // ... under this covariance handle (NULL: block-diagonal)
  size_t rows_max = 0;                     // rows of the largest launch the handle makes
  vk_eval_opts opts{};
  int P = 0;                               // sampled parameters
  int col[kSampledMaxP] = {};
  int sets = 1;                            // row sets of d_base and d_rows: 1, or a set per block (the _blocks create calls)
  int pblock[kSampledMaxP] = {};           // ... and the set each sampled parameter is written to (-1: every set)
  double alpha = 1.0;
  bool real = false;
  int max_which = -1;
  long long cross = 0;                     // > 0: every pending row goes against all `cross` realisations (an importance handle)
  void* d_mem = nullptr;                   // one allocation holding every device array of the handle
  double *d_base = nullptr, *d_rows = nullptr, *d_th = nullptr;   // each problem's base row; the pending rows, their theory vectors
  int *d_which = nullptr, *d_row_which = nullptr;                 // realisation of each problem, of each pending row
  vkprior::Prior prior{};                  // the Gaussian prior the step kernels add to lnL (vk_fit_set_prior / vk_chain_set_prior)
  bool keep_theory = false;                // the data-vector route stores the rows' theory vectors in d_th (vk_chain_set_predictive)
  // Likelihood-level beta interpolation (VK_OPT_BETA_BLEND of the create call's opts; vk_kernel_blend.h, a single fit only): the
  // m pending rows are evaluated as 2 m rows - rows [0, m) at the lower, rows [m, 2 m) at the upper bracketing node of the data
  // vector's beta grid - and blended.  The doubled launch's arrays live in the handle's one allocation (blend_layout), d_th is
  // sized for twice rows_max (workspace_doubles); d_rows / d_row_which / the callers' d_lnl and d_chi stay what they were.
  struct Blend {
    bool on = false;
    int n_grid = 0;
    long long per_row = 1;                 // outputs of a pending row: n_real in cross mode (a handle's prepare sets it), else 1
    double *grid = nullptr, *rows = nullptr, *t = nullptr, *lnl = nullptr, *chi = nullptr;   // [n_grid], [2 rows_max][VK_NPAR], [rows_max], raw [2 rows_max][per_row] x 2
    int *which = nullptr, *fail = nullptr;                                                    // [2 rows_max], [rows_max]
  } blend;
  std::string err;

  // doubles between two row sets of d_rows (fixed per handle: a best fit's launches shrink, its sets stay where they are)
  long long par_stride() const { return sets > 1 ? (long long)rows_max * VK_NPAR : 0; }
  vkrow::Blocks row_sets(size_t n) const {
    vkrow::Blocks b{};
    b.n = sets;
    b.row_stride = par_stride();
    b.base_stride = sets > 1 ? (long long)n * VK_NPAR : 0;
    for (int j = 0; j < vkrow::kMaxP; ++j) b.param_block[j] = pblock[j];
    return b;
  }

  // the blend arrays, first in every handle's layout (nothing without the mode); the int arrays take an even count each, so
  // what follows stays aligned for doubles
  template <class C>
  void blend_layout(C& c) {
    if (!blend.on) return;
    const size_t n = rows_max, even = (n + 1) & ~(size_t)1;
    c.take(blend.grid, (size_t)blend.n_grid);
    c.take(blend.rows, 2 * n * VK_NPAR);
    c.take(blend.t, n);
    c.take(blend.lnl, 2 * n * (size_t)blend.per_row);
    c.take(blend.chi, 2 * n * (size_t)blend.per_row);
    c.take(blend.which, 2 * n);
    c.take(blend.fail, even);
  }

  // doubles of d_th: the theory vectors of rows_max rows; of a joint fit, the workspace of its evaluation of that many rows
  // (whose head is the rows' theory vectors, block by block).  Block-diagonal that is B rows_max (N_max + 2) in pairs mode - per
  // block lnl | chi2 | theory - and B rows_max (N_max + 2 cross) in cross mode, where a row has `cross` values of lnl and of chi2;
  // under a covariance the outputs are the handle's own arrays in either mode (vkh::joint_workspace_doubles).
  size_t workspace_doubles() const {
    return blocks.empty() ? rows_max * (blend.on ? 2 : 1) * ctx->N
                          : vkh::joint_workspace_doubles(cov, blocks.data(), (int)blocks.size(), (long long)rows_max, real, cross);
  }
};

// The typed arrays of a handle inside its one allocation: a handle's layout() names them once, in order of descending
// alignment - without a base to count the bytes, then over the allocation to hand the pointers out.
struct Carve {
  char* base = nullptr;
  size_t bytes = 0;
  template <class T>
  void take(T*& p, size_t count) {
    p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += count * sizeof(T);
  }
};

// Count a layout with a Carve, allocate that many bytes on `device`, hand the layout's pointers out over them.  False: nothing
// is allocated (`bytes` says what was asked for).
template <class Layout>
static bool carve_alloc(int device, void*& mem, size_t& bytes, Layout&& layout) {
  Carve count;
  layout(count);
  bytes = count.bytes;
  mem = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&mem, bytes) != hipSuccess) {
    (void)hipGetLastError();
    mem = nullptr;
    return false;
  }
  Carve carve{static_cast<char*>(mem)};
  layout(carve);
  return true;
}
static std::string cannot_allocate(size_t bytes) { return "cannot allocate " + std::to_string(bytes) + " bytes of device memory"; }

// a HIP call on behalf of a handle: the error text goes to the handle (vk_fit_last_error / vk_chain_last_error)
#define VK_SAMPLED_HIP(f, call)                                                        \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (f)->err = std::string(#call " failed: ") + hipGetErrorString(e_);               \
      return VK_E_HIP;                                                                 \
    }                                                                                  \
  } while (0)

// vk_fit_destroy / vk_chain_destroy, after whatever was in flight has been waited for
template <class H>
static void sampled_destroy(H* f) {
  if (f->d_mem) {
    (void)hipSetDevice(f->ctx->device);
    (void)hipFree(f->d_mem);
  }
  delete f;
}

// vk_fit_create / vk_chain_create and their _joint forms (`who`; a problem is a `noun` in its texts).  H is a Sampled with
// shape(n, lo, hi), which keeps the count, the box and what follows from P, and layout(Carve&) (hidden: no symbol of theirs
// leaves the library).  joint: ctxs are the n_ctx blocks of a joint fit, lead first, under cov (NULL: block-diagonal); otherwise
// ctxs is the one context.  param_block (the _blocks forms; NULL otherwise): the block each sampled parameter belongs to, or -1;
// base_rows then holds a set of n rows per block.
// prepare(f) runs on the new handle before shape(): a handle whose layout needs more than the count and the box (a grid's bins,
// pairs and chunk) takes it there.
template <class H, class Prepare>
static H* sampled_create(const char* who, const char* noun, vk_ctx* const* ctxs, int n_ctx, bool joint, vk_joint_cov* cov,
                         const vk_eval_opts* opts, int32_t n, int32_t n_params, const int32_t* columns, const int32_t* param_block,
                         const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which, char* err,
                         size_t errlen, Prepare prepare) {
  auto bail = [&](const std::string& msg) -> H* {
    if (err && errlen) {
      strncpy(err, msg.c_str(), errlen - 1);
      err[errlen - 1] = 0;
    }
    return nullptr;
  };
  const std::string me = std::string(who) + ": ";
  if (!ctxs || (!joint && !ctxs[0]) || !opts || !columns || !lo || !hi || !base_rows) return bail(me + "NULL argument");
  if (n_ctx < 1 || n_ctx > 32) return bail(me + "need 1 <= contexts <= 32");
  for (int q = 0; q < n_ctx; ++q)
    if (!ctxs[q]) return bail(me + "context " + std::to_string(q) + " is NULL");
  vk_ctx* ctx = ctxs[0];
  if (n < 1 || n > kSampledMax) return bail(me + "need 1 <= " + noun + "s <= 65536");
  if (n_params < 1 || n_params > kSampledMaxP)
    return bail(me + "need 1 <= parameters <= 10 (the row columns other than aperp / apar / epsilon, and epsilon)");
  for (int q = 0; q < n_ctx; ++q) {
    sync_knobs(ctxs[q]);
    if (check_opts(ctxs[q], opts) != VK_OK) return bail(ctxs[q]->err);
  }
  if (!joint && !ctx->d_data) return bail(me + "context was created without a data vector");
  const bool blend = (opts->reserved & VK_OPT_BETA_BLEND) != 0;
  if (blend && joint)
    return bail(me + "VK_OPT_BETA_BLEND (beta_interpolation 'likelihood') is refused for a joint fit: a blend per block under one "
                     "beta is a design of its own");
  if (blend && which && ctx->n_cuts > 0)          // (a handle over the data vector reads nothing the cuts changed)
    return bail(me + "VK_OPT_BETA_BLEND (beta_interpolation 'likelihood') is refused with scale cuts resident on the context "
                     "(vk_set_cuts)");
  if (blend && ctx->n_beta_d < 2)
    return bail(me + "VK_OPT_BETA_BLEND (beta_interpolation 'likelihood') needs a data vector gridded in beta: a fixed data vector "
                     "has no nodes to blend between");
  // a joint fit: one device, data vectors, the handle's lead and block sizes; against realisations, the same number of them on
  // every context and the LDS the realisation kernels need
  if (joint && check_joint(cov, ctxs, n_ctx, which != nullptr) != VK_OK) return bail(me + ctx->err);
  // a column (epsilon: slot VK_NPAR) is named once for all blocks, or once per block it belongs to
  bool shared[VK_NPAR + 1] = {};
  uint32_t owned[VK_NPAR + 1] = {};
  bool eps_twice = false;                  // (without param_block: reported after every parameter's own checks, as it always was)
  for (int j = 0; j < n_params; ++j) {
    const int c = columns[j], b = param_block ? param_block[j] : -1;
    if (c != VK_WALK_EPSILON && (c < 0 || c >= VK_NPAR || (c >= VK_P_APERP && c <= VK_P_EPSILON)))
      return bail(me + "a sampled parameter must name a row column other than aperp / apar / epsilon, or VK_WALK_EPSILON, once");
    if (b < -1 || b >= n_ctx)
      return bail(me + "param_block " + std::to_string(b) + " of parameter " + std::to_string(j) + " is outside -1.." +
                  std::to_string(n_ctx - 1));
    const int k = c == VK_WALK_EPSILON ? VK_NPAR : c;
    if (b < 0 ? owned[k] != 0 : shared[k])
      return bail(me + "parameter " + std::to_string(j) + ": a column is sampled for all blocks or per block, not both");
    if (b < 0 ? shared[k] : (owned[k] >> b & 1u) != 0) {
      if (param_block) return bail(me + "parameter " + std::to_string(j) + " names a (column, block) pair a second time");
      if (c != VK_WALK_EPSILON)
        return bail(me + "a sampled parameter must name a row column other than aperp / apar / epsilon, or VK_WALK_EPSILON, once");
      eps_twice = true;
    }
    if (b < 0) shared[k] = true;
    else owned[k] |= 1u << b;
    if (b >= 0 && c == VK_P_BETA && vkh::joint_cov_n_beta(cov) > 0)
      return bail(me + "beta cannot be sampled per block under a covariance gridded in beta (the joint chi-square brackets the "
                       "covariance with one beta per point)");
    if (!(hi[j] > lo[j])) return bail(me + "the prior box needs lo < hi");
  }
  if (eps_twice) return bail(me + "epsilon sampled twice");
  int max_which = -1;
  if (which)
    for (int i = 0; i < n; ++i) {
      if (which[i] < 0 || which[i] >= vkh::n_problems(ctx))
        return bail(me + "realisation index " + std::to_string(which[i]) + " of " + noun + " " + std::to_string(i) +
                    " is outside 0.." + std::to_string(vkh::n_problems(ctx) - 1));
      max_which = std::max(max_which, (int)which[i]);
    }
  H* f = new (std::nothrow) H();
  if (!f) return bail("out of memory");
  f->ctx = ctx;
  if (joint) f->blocks.assign(ctxs, ctxs + n_ctx);
  f->cov = cov;
  f->opts = *opts;
  f->opts.reserved &= ~VK_OPT_BETA_BLEND;    // (the handle's mode, not the evaluation's: the entry points it calls see the word without it)
  f->blend.on = blend;
  f->blend.n_grid = blend ? ctx->n_beta_d : 0;
  f->P = n_params;
  for (int j = 0; j < kSampledMaxP; ++j) f->pblock[j] = -1;
  for (int j = 0; j < n_params; ++j) {
    f->col[j] = columns[j];
    if (param_block) f->pblock[j] = param_block[j];
  }
  f->sets = param_block ? n_ctx : 1;
  f->alpha = alpha;
  f->real = which != nullptr;
  f->max_which = max_which;
  prepare(f);
  f->shape(n, lo, hi);
  size_t bytes = 0;
  if (!carve_alloc(ctx->device, f->d_mem, bytes, [&](Carve& c) { f->layout(c); })) {
    delete f;
    return bail(me + cannot_allocate(bytes));
  }
  bool ok = hipMemcpy(f->d_base, base_rows, (size_t)f->sets * n * VK_NPAR * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok && which) ok = hipMemcpy(f->d_which, which, (size_t)n * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  if (ok && blend)                         // the handle's own copy of the data vector's beta nodes, once
    ok = hipMemcpy(f->blend.grid, ctx->d_beta_d, (size_t)f->blend.n_grid * sizeof(double), hipMemcpyDeviceToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    sampled_destroy(f);
    return bail(me + "upload failed");
  }
  return f;
}

template <class H>
static H* sampled_create(const char* who, const char* noun, vk_ctx* const* ctxs, int n_ctx, bool joint, vk_joint_cov* cov,
                         const vk_eval_opts* opts, int32_t n, int32_t n_params, const int32_t* columns, const int32_t* param_block,
                         const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which, char* err,
                         size_t errlen) {
  return sampled_create<H>(who, noun, ctxs, n_ctx, joint, cov, opts, n, n_params, columns, param_block, lo, hi, base_rows, alpha,
                           which, err, errlen, [](H*) {});
}

// the _blocks create calls, whose param_block is not optional
static bool no_param_block(const char* who, const int32_t* param_block, char* err, size_t errlen) {
  if (!param_block && err && errlen) snprintf(err, errlen, "%s: NULL argument", who);
  return !param_block;
}

// a call refused before anything was enqueued: the text goes to the handle
static int refused(Sampled* f, const std::string& msg) {
  f->err = msg;
  return VK_E_ARG;
}

// vk_fit_set_prior / vk_chain_set_prior (`who`): mu [P] and the packed triangle [P (P + 1) / 2] of vk_prior.h, or NULL, NULL
static int sampled_set_prior(Sampled* f, const char* who, const double* mu, const double* pp) {
  if (!mu && !pp) {
    f->prior = vkprior::Prior{};
    f->err.clear();
    return VK_OK;
  }
  if (!mu || !pp) return refused(f, std::string(who) + ": mu and pp_packed are both given or both NULL");
  const int T = f->P * (f->P + 1) / 2;
  for (int j = 0; j < f->P; ++j)
    if (!__builtin_isfinite(mu[j])) return refused(f, std::string(who) + ": the mean of parameter " + std::to_string(j) + " is not finite");
  for (int i = 0; i < T; ++i)
    if (!__builtin_isfinite(pp[i])) return refused(f, std::string(who) + ": entry " + std::to_string(i) + " of the packed precision matrix is not finite");
  vkprior::Prior p{};
  p.on = 1;
  for (int j = 0; j < f->P; ++j) p.mu[j] = mu[j];
  for (int i = 0; i < T; ++i) p.pp[i] = pp[i];
  f->prior = p;
  f->err.clear();
  return VK_OK;
}

// May the handle use its context now?  What every call that touches the context checks first.  (vk_fit_run reports an LDS
// refusal in the context's words alone, the chain entry points under their own name: name_lds.)
static int sampled_ready(Sampled* f, const char* who, const char* noun, bool name_lds) {
  vk_ctx* ctx = f->ctx;
  auto refuse = [&](const std::string& msg) { return refused(f, std::string(who) + ": " + msg); };
  if (!f->blocks.empty()) {                // a joint fit: every block's context
    for (size_t q = 0; q < f->blocks.size(); ++q)
      if (f->blocks[q]->begun_n != 0)
        return refuse("a batch begun with vk_eval_batch_begin is awaiting vk_eval_batch_finish on context " + std::to_string(q));
    if (check_joint(f->cov, f->blocks.data(), (int)f->blocks.size(), f->real) != VK_OK) return refuse(ctx->err);
    if (f->real && f->max_which >= vkh::n_problems(ctx))
      return refuse("the contexts hold " + std::to_string(vkh::n_problems(ctx)) + " realisations, a " + noun + " asks for number " +
                    std::to_string(f->max_which));
    return VK_OK;
  }
  if (ctx->begun_n != 0) return refuse("a batch begun with vk_eval_batch_begin is awaiting vk_eval_batch_finish on the context");
  if (f->real) {
    if (ctx->n_real <= 0 || !ctx->d_real) return refuse("no realisations are set on the context (vk_set_realisations)");
    if (f->max_which >= vkh::n_problems(ctx))
      return refuse("the context holds " + std::to_string(vkh::n_problems(ctx)) + " realisations, a " + noun + " asks for number " +
                    std::to_string(f->max_which));
    if (check_real_lds(ctx) != VK_OK) return name_lds ? refuse(ctx->err) : refused(f, ctx->err);
  }
  return VK_OK;
}

// the evaluation of the first m pending rows into d_lnl / d_chi, on the context's stream: the fit's own data vector with lnL /
// chi2 in the theory launch (the fused tail applies), realisations in pairs mode - or, of a handle that keeps no d_row_which (an
// importance handle), in cross mode: every row against every realisation, outputs [m][n_real], single fit and joint fit alike
static int sampled_evaluate_blend(Sampled* f, long long m, double* d_lnl, double* d_chi);
static int sampled_evaluate(Sampled* f, long long m, double* d_lnl, double* d_chi) {
  int rc;
  if (f->blend.on) return sampled_evaluate_blend(f, m, d_lnl, d_chi);
  if (f->blocks.empty()) {
    // (with lnL requested the data-vector route treats d_th as scratch and its fused tail never stores the theory vector:
    // keep_theory asks for the stores - TheoryArgs::want_theory -, which change no bit of lnL; the realisation route writes d_th)
    f->ctx->theory_wanted = f->keep_theory && !f->real;
    rc = f->real ? enqueue_realisations(f->ctx, &f->opts, f->d_rows, m, f->d_th, d_lnl, d_chi, f->d_row_which)
                 : vk_eval_batch_device_async(f->ctx, &f->opts, f->d_rows, m, d_lnl, d_chi, f->d_th);
    f->ctx->theory_wanted = false;
  } else {
    // A joint fit: the launches of the joint entry points, enqueue only.  Stream order: the rows (and their realisation
    // indices) were written on the lead stream; every route first puts each block's stream behind an event of the lead stream
    // (fan_out), so the blocks' launches read finished rows, and ends on the lead stream behind an event of every block's
    // stream (the joint chi-square kernel, or the block-order sum) - so the step kernel that follows on the lead stream reads
    // finished results, and overwrites the rows only once no block reads them any more.
    vk_ctx* const* cs = f->blocks.data();
    const int nb = (int)f->blocks.size();
    const long long ps = f->par_stride();  // block q's rows: d_rows + q * ps (0: one row set)
    if (!f->real) {
      // (block-diagonal, each block's launch carries its own lnL: as above, keep_theory asks the fused tails for the stores)
      for (int q = 0; q < nb; ++q) cs[q]->theory_wanted = f->keep_theory && !f->cov;
      rc = f->cov ? vk_joint_cov_eval_blocks_device_async(f->cov, cs, nb, &f->opts, f->d_rows, ps, m, d_lnl, d_chi, f->d_th)
                  : vk_joint_eval_blocks_device_async(cs, nb, &f->opts, f->d_rows, ps, m, d_lnl, d_chi, f->d_th);
      for (int q = 0; q < nb; ++q) cs[q]->theory_wanted = false;
    }
    else if (f->cov)
      rc = vkh::enqueue_joint_cov_realisations(f->cov, cs, nb, &f->opts, f->d_rows, ps, m, f->d_row_which, d_lnl, d_chi,
                                               vkh::joint_real_carve(f->cov, f->d_th, (long long)f->rows_max));
    else
      rc = vkh::enqueue_joint_sum_realisations(cs, nb, &f->opts, f->d_rows, ps, m, f->d_row_which, d_lnl, d_chi, f->d_th);
  }
  if (rc) f->err = f->ctx->err;
  return rc;
}

// a kernel of `threads` threads (one per problem; of a kernel of one block per item, items x block) on the handle's stream
template <class Args>
static int sampled_launch(Sampled* f, void (*kern)(Args), long long threads, int block, const Args& a) {
  hipLaunchKernelGGL(kern, dim3((unsigned)((threads + block - 1) / block)), dim3(block), 0, f->ctx->stream, a);
  VK_SAMPLED_HIP(f, hipGetLastError());
  return VK_OK;
}

// sampled_evaluate of a handle in blend mode (a single fit: sampled_create): the split kernel writes the 2 m rows, the evaluation
// sampled_evaluate makes otherwise runs over them into the raw arrays - the data vector, realisations in pairs mode with the
// duplicated indices, or in cross mode [2 m][n_real] -, the merge kernel blends into the caller's arrays.  m <= rows_max.
static int sampled_evaluate_blend(Sampled* f, long long m, double* d_lnl, double* d_chi) {
  if (m <= 0) return VK_OK;
  if (f->real && f->ctx->n_cuts > 0) {
    f->err = "the handle blends the likelihood between two grid betas (VK_OPT_BETA_BLEND), which is refused with scale cuts resident "
             "on the context (vk_set_cuts)";
    return VK_E_ARG;
  }
  const Sampled::Blend& b = f->blend;
  const int* row_which = f->real ? f->d_row_which : nullptr;     // (NULL against realisations: cross mode)
  BlendArgs q{};
  q.grid = b.grid;
  q.n_grid = b.n_grid;
  q.m = m;
  q.per_row = f->real && !row_which ? b.per_row : 1;
  q.rows = f->d_rows;
  q.row_which = row_which;
  q.rows2 = b.rows;
  q.which2 = b.which;
  q.t = b.t;
  q.fail = b.fail;
  q.raw_lnl = b.lnl;
  q.raw_chi = b.chi;
  q.lnl = d_lnl;
  q.chi = d_chi;
  int rc = sampled_launch(f, vk_blend_split_kernel, m, kBlendBlock, q);
  if (rc) return rc;
  rc = f->real ? enqueue_realisations(f->ctx, &f->opts, b.rows, 2 * m, f->d_th, b.lnl, b.chi, row_which ? b.which : nullptr)
               : vk_eval_batch_device_async(f->ctx, &f->opts, b.rows, 2 * m, b.lnl, b.chi, f->d_th);
  if (rc) {
    f->err = f->ctx->err;
    return rc;
  }
  return sampled_launch(f, vk_blend_merge_kernel, m * q.per_row, kBlendBlock, q);
}

// Device arrays copied home, each if the caller gave it a destination: plain copies, complete on return, or (on_stream) enqueued
// on the handle's stream for the caller to wait for.
struct Home {
  void* dst;
  const void* src;
  size_t bytes;
};
static int sampled_home(Sampled* f, std::initializer_list<Home> arrays, bool on_stream = false) {
  for (const Home& a : arrays) {
    if (!a.dst || !a.bytes) continue;
    if (on_stream) VK_SAMPLED_HIP(f, hipMemcpyAsync(a.dst, a.src, a.bytes, hipMemcpyDeviceToHost, f->ctx->stream));
    else VK_SAMPLED_HIP(f, hipMemcpy(a.dst, a.src, a.bytes, hipMemcpyDeviceToHost));
  }
  return VK_OK;
}

// an error after something was enqueued (the handle holds its text): leave nothing in flight
static int sampled_abort(Sampled* f, int rc) {
  for (size_t q = 1; q < f->blocks.size(); ++q) (void)hipStreamSynchronize(f->blocks[q]->stream);   // (a joint fit's other blocks)
  (void)hipStreamSynchronize(f->ctx->stream);
  (void)hipGetLastError();
  return rc;
}

// ---- best fits: bounded Nelder-Mead, one simplex per problem, one launch per iteration (include/victor_hip.h, vk_kernel_fit.h) --
// An iteration enqueues, on the context's stream, the evaluation of the active problems' S rows each (sampled_evaluate) and the
// step kernel behind it - no host synchronisation and no graph inside an iteration.  Every kFitCheck iterations the host reads
// the status words, keeps the problems still running (in problem order) and lays their rows out again, so a finished problem
// stops costing evaluations and which rows share a launch does not depend on timing.
constexpr int kFitCheck = 8;

struct __attribute__((visibility("hidden"))) vk_fit : Sampled {
  int R = 0, S = 0;                        // problems, rows of a problem in a launch
  double lo[vkfit::kMaxP] = {}, hi[vkfit::kMaxP] = {};
  vkfit::State* d_state = nullptr;         // [R]
  double *d_x0 = nullptr, *d_lnl = nullptr, *d_chi = nullptr;
  int *d_active = nullptr, *d_status = nullptr;

  void shape(int n, const double* lo_, const double* hi_) {
    R = n;
    S = vkfit::slots(P);
    rows_max = (size_t)R * S;
    for (int j = 0; j < P; ++j) {
      lo[j] = lo_[j];
      hi[j] = hi_[j];
    }
  }
  void layout(Carve& c) {
    const size_t n = R, rows = n * S;
    blend_layout(c);
    c.take(d_state, n);
    c.take(d_base, sets * n * VK_NPAR);
    c.take(d_x0, n * P);
    c.take(d_rows, sets * rows * VK_NPAR);
    c.take(d_lnl, rows);
    c.take(d_chi, rows);
    c.take(d_th, workspace_doubles());
    c.take(d_active, n);
    c.take(d_row_which, rows);
    c.take(d_which, n);
    c.take(d_status, n);
  }
};

// the loop of vk_fit_run
static int fit_loop(vk_fit* f, const vkfit::Params& q, const double* x0, std::vector<vkfit::State>* out) {
  vk_ctx* ctx = f->ctx;
  const int R = f->R, S = f->S;
  VK_SAMPLED_HIP(f, hipSetDevice(ctx->device));
  std::vector<int> act(R), status(R);
  for (int p = 0; p < R; ++p) act[p] = p;
  VK_SAMPLED_HIP(f, hipMemcpyAsync(f->d_x0, x0, (size_t)R * f->P * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  VK_SAMPLED_HIP(f, hipMemcpyAsync(f->d_active, act.data(), (size_t)R * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  FitArgs a{};
  a.q = q;
  a.state = f->d_state;
  a.base = f->d_base;
  a.x0 = f->d_x0;
  a.active = f->d_active;
  a.n_active = R;
  a.lnl = f->d_lnl;
  a.chi2 = f->d_chi;
  a.rows = f->d_rows;
  a.row_which = f->real ? f->d_row_which : nullptr;
  a.which = f->real ? f->d_which : nullptr;
  a.status = f->d_status;
  for (int j = 0; j < vkfit::kMaxP; ++j) a.col[j] = f->col[j];
  a.alpha = f->alpha;
  a.blocks = f->row_sets((size_t)R);
  a.prior = f->prior;
  a.post = f->d_lnl;
  int rc = sampled_launch(f, vk_fit_init_kernel, R, kFitBlock, a);
  while (rc == VK_OK) {
    for (int t = 0; t < kFitCheck && rc == VK_OK; ++t) {
      rc = sampled_evaluate(f, (long long)a.n_active * S, f->d_lnl, f->d_chi);
      if (rc == VK_OK) rc = sampled_launch(f, vk_fit_step_kernel, a.n_active, kFitBlock, a);
    }
    if (rc) return rc;
    VK_SAMPLED_HIP(f, hipMemcpyAsync(status.data(), f->d_status, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    VK_SAMPLED_HIP(f, hipStreamSynchronize(ctx->stream));
    std::vector<int> next;
    for (int p : act)
      if (status[p] < 0) next.push_back(p);
    if (next.empty()) break;
    if ((int)next.size() < a.n_active) {
      act.swap(next);
      a.n_active = (int)act.size();
      VK_SAMPLED_HIP(f, hipMemcpyAsync(f->d_active, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
      rc = sampled_launch(f, vk_fit_emit_kernel, a.n_active, kFitBlock, a);
    }
  }
  if (rc) return rc;
  out->resize(R);
  VK_SAMPLED_HIP(f, hipMemcpy(out->data(), f->d_state, (size_t)R * sizeof(vkfit::State), hipMemcpyDeviceToHost));
  return VK_OK;
}

extern "C" {

vk_fit* vk_fit_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_problems, int32_t n_params, const int32_t* columns,
                      const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which, char* err,
                      size_t errlen) {
  return sampled_create<vk_fit>("vk_fit_create", "problem", &ctx, 1, false, nullptr, opts, n_problems, n_params, columns, nullptr,
                                lo, hi, base_rows, alpha, which, err, errlen);
}

vk_fit* vk_fit_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_problems,
                            int32_t n_params, const int32_t* columns, const double* lo, const double* hi, const double* base_rows,
                            double alpha, const int32_t* which, char* err, size_t errlen) {
  return sampled_create<vk_fit>("vk_fit_create_joint", "problem", ctxs, n_ctx, true, cov, opts, n_problems, n_params, columns,
                                nullptr, lo, hi, base_rows, alpha, which, err, errlen);
}

vk_fit* vk_fit_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                   int32_t n_problems, int32_t n_params, const int32_t* columns, const int32_t* param_block,
                                   const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which,
                                   char* err, size_t errlen) {
  if (no_param_block("vk_fit_create_joint_blocks", param_block, err, errlen)) return nullptr;
  return sampled_create<vk_fit>("vk_fit_create_joint_blocks", "problem", ctxs, n_ctx, true, cov, opts, n_problems, n_params, columns,
                                param_block, lo, hi, base_rows, alpha, which, err, errlen);
}

const char* vk_fit_last_error(const vk_fit* f) { return f ? f->err.c_str() : ""; }

int vk_fit_set_prior(vk_fit* f, const double* mu, const double* pp_packed) {
  if (!f) return VK_E_ARG;
  return sampled_set_prior(f, "vk_fit_set_prior", mu, pp_packed);       // (vk_fit_run is synchronous: nothing is ever in flight)
}

void vk_fit_destroy(vk_fit* f) {
  if (f) sampled_destroy(f);
}

int vk_fit_run(vk_fit* f, const double* x0, const double* step, const double* xtol, double ftol, int32_t max_iter, int32_t restarts,
               double* x, double* lnl, double* chi2, int32_t* status, int32_t* n_iter, int64_t* n_evals) {
  if (!f) return VK_E_ARG;
  if (!x0 || !step || !xtol || !x || !lnl || !chi2 || !status || !n_iter || !n_evals) return refused(f, "vk_fit_run: NULL argument");
  int rc = sampled_ready(f, "vk_fit_run", "problem", false);
  if (rc) return rc;
  if (max_iter < 1 || restarts < 0 || !(ftol >= 0)) return refused(f, "vk_fit_run: need max_iter >= 1, restarts >= 0, ftol >= 0");
  vkfit::Params q{};
  q.d = f->P;
  q.S = f->S;
  q.max_iter = max_iter;
  q.restarts = restarts;
  q.ftol = ftol;
  for (int j = 0; j < f->P; ++j) {
    if (!(step[j] > 0) || !(xtol[j] >= 0)) return refused(f, "vk_fit_run: parameter " + std::to_string(j) + " needs step > 0 and xtol >= 0");
    q.lo[j] = f->lo[j];
    q.hi[j] = f->hi[j];
    q.step[j] = step[j];
    q.xtol[j] = xtol[j];
  }
  for (int p = 0; p < f->R; ++p)
    if (!vkfit::in_box(q, x0 + (size_t)p * f->P)) return refused(f, "vk_fit_run: the start of problem " + std::to_string(p) + " is outside the box");
  std::vector<vkfit::State> st;
  rc = fit_loop(f, q, x0, &st);
  if (rc != VK_OK) return sampled_abort(f, rc);
  for (int p = 0; p < f->R; ++p) {
    const vkfit::State& s = st[p];
    for (int j = 0; j < f->P; ++j) x[(size_t)p * f->P + j] = s.v[0][j];
    lnl[p] = -s.f[0];
    chi2[p] = s.chi[0];
    status[p] = s.status;
    n_iter[p] = s.iter;
    n_evals[p] = s.n_evals;
  }
  f->err.clear();
  return VK_OK;
}

}  // extern "C"

// ---- Hessians at given points: one central-difference stencil per problem (include/victor_hip.h, vk_kernel_hessian.h) --------
// The R M stencil rows are evaluated in chunks of rows_max consecutive global rows - the pending-row buffers, the workspace and
// par_stride() stay what the search uses, chunk boundaries fall inside problems - each chunk a rows kernel, sampled_evaluate
// (the launches fit_loop makes) and two copies of its results into the call's own [R M] arrays; one assemble kernel follows.
// Everything the call needs beyond the handle lives in one allocation of the call.
struct HessMem {
  double *x = nullptr, *h = nullptr, *values = nullptr, *chis = nullptr, *a = nullptr, *hess = nullptr, *cov = nullptr;
  double *lnpost = nullptr, *chi2 = nullptr;
  int* status = nullptr;
  void layout(Carve& c, size_t R, size_t d, size_t M) {
    c.take(x, R * d);
    c.take(h, R * d);
    c.take(values, R * M);
    c.take(chis, R * M);
    c.take(a, R * d * d);
    c.take(hess, R * d * d);
    c.take(cov, R * d * d);
    c.take(lnpost, R);
    c.take(chi2, R);
    c.take(status, R);
  }
};

static int hessian_run(vk_fit* f, const HessMem& m, const double* x, const double* h, double* values, double* a, double* hess,
                       double* cov, double* lnpost, double* chi2, int32_t* status) {
  vk_ctx* ctx = f->ctx;
  const size_t R = f->R, d = f->P, M = (size_t)vkhess::n_points(f->P);
  VK_SAMPLED_HIP(f, hipMemcpyAsync(m.x, x, R * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  VK_SAMPLED_HIP(f, hipMemcpyAsync(m.h, h, R * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HessArgs q{};
  q.d = (int)d;
  q.M = (int)M;
  q.R = (int)R;
  for (size_t j = 0; j < d; ++j) {
    q.lo[j] = f->lo[j];
    q.hi[j] = f->hi[j];
  }
  q.x = m.x;
  q.h = m.h;
  q.base = f->d_base;
  q.rows = f->d_rows;
  q.row_which = f->real ? f->d_row_which : nullptr;
  q.which = f->real ? f->d_which : nullptr;
  for (int j = 0; j < vkhess::kMaxP; ++j) q.col[j] = f->col[j];
  q.alpha = f->alpha;
  q.blocks = f->row_sets(R);
  q.prior = f->prior;
  q.values = m.values;
  q.chis = m.chis;
  q.a = m.a;
  q.hess = m.hess;
  q.cov = m.cov;
  q.lnpost = m.lnpost;
  q.chi2 = m.chi2;
  q.status = m.status;
  const long long total = (long long)(R * M), chunk = (long long)f->rows_max;
  for (long long g0 = 0; g0 < total; g0 += chunk) {
    const long long n = std::min(chunk, total - g0);
    q.g0 = g0;
    q.n = n;
    int rc = sampled_launch(f, vk_hess_rows_kernel, (int)n, kHessBlock, q);
    if (rc == VK_OK) rc = sampled_evaluate(f, n, f->d_lnl, f->d_chi);
    if (rc) return rc;
    VK_SAMPLED_HIP(f, hipMemcpyAsync(m.values + g0, f->d_lnl, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    VK_SAMPLED_HIP(f, hipMemcpyAsync(m.chis + g0, f->d_chi, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  }
  int rc = sampled_launch(f, vk_hess_assemble_kernel, (long long)R * kHessBlock, kHessBlock, q);      // one wave per problem
  const size_t one = R * sizeof(double), mat = one * d * d;
  if (rc == VK_OK)
    rc = sampled_home(f, {{values, m.values, one * M}, {a, m.a, mat}, {hess, m.hess, mat}, {cov, m.cov, mat}, {lnpost, m.lnpost, one},
                          {chi2, m.chi2, one}, {status, m.status, R * sizeof(int)}}, true);
  if (rc) return rc;
  VK_SAMPLED_HIP(f, hipStreamSynchronize(ctx->stream));
  return VK_OK;
}

extern "C" {

int64_t vk_hessian_rows(int32_t n_params) {
  return n_params >= 1 && n_params <= kSampledMaxP ? (int64_t)vkhess::n_points(n_params) : 0;
}

int vk_fit_hessian(vk_fit* f, const double* x, const double* h, double* values, double* a, double* hess, double* cov, double* lnpost,
                   double* chi2, int32_t* status) {
  if (!f) return VK_E_ARG;
  if (!x || !h) return refused(f, "vk_fit_hessian: NULL argument");
  int rc = sampled_ready(f, "vk_fit_hessian", "problem", false);
  if (rc) return rc;
  const size_t R = f->R, d = f->P;
  for (size_t p = 0; p < R; ++p)
    for (size_t j = 0; j < d; ++j) {
      if (!__builtin_isfinite(x[p * d + j]))
        return refused(f, "vk_fit_hessian: the point of problem " + std::to_string(p) + " is not finite in parameter " + std::to_string(j));
      if (!(h[p * d + j] > 0) || !__builtin_isfinite(h[p * d + j]))
        return refused(f, "vk_fit_hessian: problem " + std::to_string(p) + ", parameter " + std::to_string(j) + " needs a finite step > 0");
    }
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  HessMem m;
  void* mem = nullptr;
  size_t bytes = 0;
  if (!carve_alloc(f->ctx->device, mem, bytes, [&](Carve& c) { m.layout(c, R, d, (size_t)vkhess::n_points(f->P)); })) {
    f->err = "vk_fit_hessian: " + cannot_allocate(bytes);
    return VK_E_HIP;
  }
  rc = hessian_run(f, m, x, h, values, a, hess, cov, lnpost, chi2, status);
  if (rc != VK_OK) rc = sampled_abort(f, rc);
  (void)hipFree(mem);
  if (rc == VK_OK) f->err.clear();
  return rc;
}

}  // extern "C"

// ---- Fisher matrices at given points: one Jacobian stencil of theory vectors per problem (include/victor_hip.h, vk_kernel_fisher.h)
// The R M stencil rows, M = 2 d + 1, go through in chunks of rows_max consecutive global rows as the Hessian's do (M may be
// smaller than a problem's S rows - d = 1 - or larger; chunk boundaries fall inside problems): a rows kernel, then a THEORY-ONLY
// evaluation (vk_eval_batch_device_async without lnl / chi2: no data vector and no realisation is read, the handle's pending
// results and workspace stay untouched) straight into the call's own [R M][N] allocation at the chunk's offset.  A joint fit
// makes one such evaluation per block context into that block's [R M][N_q] part, on the block's own stream between the two
// event hand-overs the joint entry points use: every block stream waits for the lead's (the rows are written there), the lead
// waits for every block's before it writes the next chunk's rows or assembles.  One assemble kernel follows on the lead stream.
// Nothing of the handle or its contexts is toggled: a handle that never calls this makes the launches it made before.
struct FisherMem {
  double *x = nullptr, *h = nullptr, *vec = nullptr, *fisher = nullptr, *a = nullptr, *cov = nullptr;
  int* status = nullptr;
  void layout(Carve& c, size_t R, size_t d, size_t M, size_t N) {
    c.take(x, R * d);
    c.take(h, R * d);
    c.take(vec, R * M * N);
    c.take(fisher, R * d * d);
    c.take(a, R * d * d);
    c.take(cov, R * d * d);
    c.take(status, R);
  }
};

// the entries of the handle's theory vector (a joint fit: of its blocks' vectors, concatenated)
static int fisher_entries(const vk_fit* f) {
  if (f->blocks.empty()) return f->ctx->N;
  int n = 0;
  for (const vk_ctx* c : f->blocks) n += c->N;
  return n;
}

// c of vk_fisher.h for the handle's likelihood form; false: the blocks of a block-diagonal joint fit disagree about it
static bool fisher_scale(const vk_fit* f, double* c) {
  const vk_eval_opts& o = f->opts;
  if (f->blocks.empty() || f->cov) {
    *c = vkfisher::form_scale(o.like_form, o.nmocks, o.nparams, (double)fisher_entries(f));
    return true;
  }
  *c = vkfisher::form_scale(o.like_form, o.nmocks, o.nparams, (double)f->blocks[0]->N);
  for (const vk_ctx* b : f->blocks)
    if (vkfisher::form_scale(o.like_form, o.nmocks, o.nparams, (double)b->N) != *c) return false;
  return true;
}

static int fisher_run(vk_fit* f, const FisherMem& m, double c, const double* x, const double* h, double* vectors, double* fisher,
                      double* a, double* cov, int32_t* status) {
  vk_ctx* ctx = f->ctx;
  const size_t R = f->R, d = f->P, M = (size_t)vkfisher::n_rows(f->P), N = (size_t)fisher_entries(f);
  const int nb = (int)f->blocks.size();
  VK_SAMPLED_HIP(f, hipMemcpyAsync(m.x, x, R * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  VK_SAMPLED_HIP(f, hipMemcpyAsync(m.h, h, R * d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  FisherArgs q{};
  q.d = (int)d;
  q.M = (int)M;
  q.R = (int)R;
  q.N = (int)N;
  for (size_t j = 0; j < d; ++j) {
    q.lo[j] = f->lo[j];
    q.hi[j] = f->hi[j];
  }
  q.x = m.x;
  q.h = m.h;
  q.base = f->d_base;
  q.rows = f->d_rows;
  // xi^r table sets resident on the context (vk_set_model_realisations) and a handle over realisations: problem p's stencil is
  // evaluated from table set which[p] - the rows kernel writes the rows' indices, the theory launch selects by them
  const bool paired = f->real && !nb && ctx->n_sets > 0;
  if (paired && ctx->n_sets != ctx->n_real) {
    f->err = "the context holds " + std::to_string(ctx->n_sets) + " model realisations (vk_set_model_realisations) and " +
             std::to_string(ctx->n_real) + " realisations of the data: the counts must agree";
    return VK_E_ARG;
  }
  q.row_which = paired ? f->d_row_which : nullptr;
  q.which = paired ? f->d_which : nullptr;
  for (int j = 0; j < vkhess::kMaxP; ++j) q.col[j] = f->col[j];
  q.alpha = f->alpha;
  q.blocks = f->row_sets(R);
  q.prior = f->prior;
  q.c = c;
  q.fisher = m.fisher;
  q.a = m.a;
  q.cov = m.cov;
  q.status = m.status;
  // the segments: block b's vectors at vec + R M off_b, against the precision its entries meet
  q.n_seg = nb ? nb : 1;
  int off = 0;
  for (int b = 0; b < q.n_seg; ++b) {
    const vk_ctx* bc = nb ? f->blocks[b] : ctx;
    FisherSeg& s = q.seg[b];
    s.theory = m.vec + R * M * (size_t)off;
    s.N = bc->N;
    s.off = off;
    if (f->cov) {                                  // one covariance across the blocks: its padded slices, beta of block 0's rows
      const vkh::JointCovView v = vkh::joint_cov_view(f->cov);
      s.prec = v.prec;
      s.beta_c = v.beta;
      s.n_beta_c = v.n_beta;
      s.ld = v.NTp;
      s.slice = (long long)v.NTp * v.NTp;
      s.prow0 = off;
      s.poff = 0;
      s.pn = v.NT;
      s.set = 0;
    } else {
      s.prec = bc->d_prec;
      s.beta_c = bc->n_beta_c > 0 ? bc->d_beta_c : nullptr;
      s.n_beta_c = bc->n_beta_c;
      s.ld = bc->N;
      s.slice = (long long)bc->N * bc->N;
      s.prow0 = 0;
      s.poff = off;
      s.pn = bc->N;
      s.set = f->sets > 1 ? b : 0;
    }
    off += bc->N;
  }
  const long long total = (long long)(R * M), chunk = (long long)f->rows_max, ps = f->par_stride();
  for (int b = 1; b < nb; ++b)
    if (!f->blocks[b]->ev_joint) VK_SAMPLED_HIP(f, hipEventCreateWithFlags(&f->blocks[b]->ev_joint, hipEventDisableTiming));
  if (nb && !ctx->ev_joint) VK_SAMPLED_HIP(f, hipEventCreateWithFlags(&ctx->ev_joint, hipEventDisableTiming));
  for (long long g0 = 0; g0 < total; g0 += chunk) {
    const long long n = std::min(chunk, total - g0);
    q.g0 = g0;
    q.n = n;
    int rc = sampled_launch(f, vk_fisher_rows_kernel, n, kFisherRowsBlock, q);
    if (rc) return rc;
    if (!nb) {
      ctx->row_set = paired ? f->d_row_which : nullptr;
      rc = vk_eval_batch_device_async(ctx, &f->opts, f->d_rows, n, nullptr, nullptr, m.vec + (size_t)g0 * N);
      ctx->row_set = nullptr;
      if (rc) f->err = ctx->err;
      if (rc) return rc;
      continue;
    }
    VK_SAMPLED_HIP(f, hipEventRecord(ctx->ev_joint, ctx->stream));
    for (int b = 0; b < nb; ++b) {
      vk_ctx* bc = f->blocks[b];
      if (b > 0) VK_SAMPLED_HIP(f, hipStreamWaitEvent(bc->stream, ctx->ev_joint, 0));
      rc = vk_eval_batch_device_async(bc, &f->opts, f->d_rows + b * ps, n, nullptr, nullptr,
                                      const_cast<double*>(q.seg[b].theory) + (size_t)g0 * bc->N);
      if (rc) f->err = bc->err;
      if (rc) return rc;
    }
    for (int b = 1; b < nb; ++b) {
      VK_SAMPLED_HIP(f, hipEventRecord(f->blocks[b]->ev_joint, f->blocks[b]->stream));
      VK_SAMPLED_HIP(f, hipStreamWaitEvent(ctx->stream, f->blocks[b]->ev_joint, 0));
    }
  }
  const size_t lds = fisher_lds_doubles((int)N, (int)d) * sizeof(double);
  if (lds > 64 * 1024) {                           // (the per-kernel opt-in of launch_on_stream, victor_hip.hip: sticky, asked for once)
    int& granted = ctx->lds_opt_in[reinterpret_cast<const void*>(vk_fisher_assemble_kernel)];
    if ((int)lds > granted) {
      VK_SAMPLED_HIP(f, hipFuncSetAttribute(reinterpret_cast<const void*>(vk_fisher_assemble_kernel),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      granted = (int)lds;
    }
  }
  hipLaunchKernelGGL(vk_fisher_assemble_kernel, dim3((unsigned)R), dim3(kFisherBlock), lds, ctx->stream, q);   // a workgroup per problem
  VK_SAMPLED_HIP(f, hipGetLastError());
  const size_t mat = R * d * d * sizeof(double);
  int rc = sampled_home(f, {{fisher, m.fisher, mat}, {a, m.a, mat}, {cov, m.cov, mat}, {status, m.status, R * sizeof(int)}}, true);
  if (rc) return rc;
  // the vectors, [R][M][N]: a joint fit's blocks side by side in every row
  if (vectors)
    for (int b = 0; b < q.n_seg; ++b)
      VK_SAMPLED_HIP(f, hipMemcpy2DAsync(vectors + q.seg[b].off, N * sizeof(double), q.seg[b].theory, (size_t)q.seg[b].N * sizeof(double),
                                         (size_t)q.seg[b].N * sizeof(double), R * M, hipMemcpyDeviceToHost, ctx->stream));
  VK_SAMPLED_HIP(f, hipStreamSynchronize(ctx->stream));
  return VK_OK;
}

extern "C" {

int64_t vk_fisher_rows(int32_t n_params) {
  return n_params >= 1 && n_params <= kSampledMaxP ? (int64_t)vkfisher::n_rows(n_params) : 0;
}

int vk_fit_fisher(vk_fit* f, const double* x, const double* h, double* vectors, double* fisher, double* a, double* cov, double* scale,
                  int32_t* status) {
  if (!f) return VK_E_ARG;
  if (!x || !h) return refused(f, "vk_fit_fisher: NULL argument");
  if (f->blend.on)
    return refused(f, "vk_fit_fisher: the handle blends the likelihood between two grid betas (VK_OPT_BETA_BLEND): a point has two "
                      "theory vectors and no one Jacobian");
  if (f->real && f->ctx->n_cuts > 0)           // (a handle over the data vector forecasts from the full precision, as ever)
    return refused(f, "vk_fit_fisher: scale cuts are resident on the context (vk_set_cuts): the forecast forms J^T P J from the "
                      "context's full precision, not from a cut's");
  int rc = sampled_ready(f, "vk_fit_fisher", "problem", false);
  if (rc) return rc;
  const size_t R = f->R, d = f->P;
  for (size_t p = 0; p < R; ++p)
    for (size_t j = 0; j < d; ++j) {
      if (!__builtin_isfinite(x[p * d + j]))
        return refused(f, "vk_fit_fisher: the point of problem " + std::to_string(p) + " is not finite in parameter " + std::to_string(j));
      if (!(h[p * d + j] > 0) || !__builtin_isfinite(h[p * d + j]))
        return refused(f, "vk_fit_fisher: problem " + std::to_string(p) + ", parameter " + std::to_string(j) + " needs a finite step > 0");
    }
  const int N = fisher_entries(f);
  if (fisher_lds_doubles(N, (int)d) > (size_t)kFisherLdsDoubles)
    return refused(f, "vk_fit_fisher: a theory vector of " + std::to_string(N) + " entries with " + std::to_string(d) +
                          " parameters needs more than 160 KiB of LDS (entries x parameters <= " +
                          std::to_string((kFisherLdsDoubles - 3 * vkhess::kMaxP * vkhess::kMaxP) / 2) + ")");
  double c = 1.0;
  if (!fisher_scale(f, &c))
    return refused(f, "vk_fit_fisher: the blocks of a block-diagonal joint fit have different lengths, and this likelihood form "
                      "scales each block's chi-square by a factor of its own: there is no one scale");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  FisherMem m;
  void* mem = nullptr;
  size_t bytes = 0;
  if (!carve_alloc(f->ctx->device, mem, bytes, [&](Carve& cv) { m.layout(cv, R, d, (size_t)vkfisher::n_rows(f->P), (size_t)N); })) {
    f->err = "vk_fit_fisher: " + cannot_allocate(bytes);
    return VK_E_HIP;
  }
  rc = fisher_run(f, m, c, x, h, vectors, fisher, a, cov, status);
  if (rc != VK_OK) rc = sampled_abort(f, rc);
  (void)hipFree(mem);
  if (rc == VK_OK) {
    if (scale) *scale = c;
    f->err.clear();
  }
  return rc;
}

}  // extern "C"

// ---- Metropolis chains: one chain per thread, one launch per step (include/victor_hip.h, vk_kernel_chain.h) ------------------
// A step enqueues, on the context's stream, the evaluation of the C chains' rows (sampled_evaluate: the launches fit_loop makes)
// and the step kernel behind it, which decides and writes the next rows.  No host synchronisation and no graph inside a block of
// up to 64 steps: vk_chain_begin uploads the block's random numbers and enqueues all of it, vk_chain_finish waits and brings the
// block's kept steps home, and the host draws the next block's numbers in between.

// Device memory a chain handle owns beside its one allocation, for state that is asked for after the create call (hidden, as
// the handles: no symbol of its leaves the library).
struct __attribute__((visibility("hidden"))) DevBlock {
  void* p = nullptr;
  size_t bytes = 0;
  // Allocate what `layout` counts and hand its pointers out; zeroed on the handle's stream (idle now: the kernels that write
  // the block run there) and waited for.  On failure nothing is held and the handle has the text, under the caller's name.
  template <class Layout>
  int make(Sampled* f, const std::string& me, Layout&& layout) {
    if (!carve_alloc(f->ctx->device, p, bytes, layout)) {
      f->err = me + cannot_allocate(bytes);
      bytes = 0;
      return VK_E_HIP;
    }
    if (zero(f) != hipSuccess || hipStreamSynchronize(f->ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      drop(f);
      f->err = me + "hipMemsetAsync failed";
      return VK_E_HIP;
    }
    return VK_OK;
  }
  hipError_t zero(Sampled* f) const { return hipMemsetAsync(p, 0, bytes, f->ctx->stream); }      // in stream order
  void drop(Sampled* f) {
    if (p) {
      (void)hipSetDevice(f->ctx->device);
      (void)hipFree(p);
    }
    p = nullptr;
    bytes = 0;
  }
};

struct __attribute__((visibility("hidden"))) vk_chain : Sampled {
  int C = 0, T = 0;                        // chains, entries of a packed second-moment triangle
  vkchain::Box box{};
  bool started = false;
  int in_flight = 0;                       // steps of the block begun and not finished
  int block_kept = 0;                      // history slots the block in flight fills (0 without a history)
  double *d_x = nullptr, *d_lnl = nullptr, *d_chi = nullptr, *d_pivot = nullptr, *d_sum1 = nullptr, *d_sum2 = nullptr;
  double *d_x0 = nullptr, *d_res_lnl = nullptr, *d_res_chi = nullptr;
  double *d_dz = nullptr, *d_logu = nullptr, *d_hx = nullptr, *d_hl = nullptr, *d_hc = nullptr;
  long long *d_acc = nullptr, *d_steps = nullptr, *d_kept = nullptr;
  std::vector<int> h_which;                // the chains' realisation indices, read back for chain_one_realisation
  // What a handle may hold beside its one allocation: a DevBlock each, and the words the kernels take (whose pointers lie in it).
  // a stretch block's numbers [64][2][C / 2] and the proposals of a half-step [P][C / 2], made by the first vk_chain_begin_stretch
  DevBlock stretch;
  double *d_sz = nullptr, *d_slz = nullptr, *d_slogu = nullptr, *d_prop = nullptr;
  int* d_partner = nullptr;
  // the marginal histograms h1 | h2 of vk_marginals.h (vk_chain_set_marginals)
  DevBlock marg_mem;
  vkmarg::Marginals marg{};
  // the series state pivot | total | head | ring | acc of vk_autocorr.h (vk_chain_set_autocorr); ac.n counts the kept steps
  // enqueued since vk_chain_start
  DevBlock ac_mem;
  vkac::Autocorr ac{};
  // replica exchange (vk_kernel_temper.h): betas [K] | pivot_e, e1, e2 [C] | a block of swap levels [64][C] | n_e, n_swap_try,
  // n_swap_acc [C] (vk_chain_set_tempering); temper.K == 0: none
  DevBlock temper_mem;
  TemperArgs temper{};
  double* d_logs = nullptr;
  // the posterior-predictive state of vk_predictive.h, pivot_t | sum_t | sum_tt [R][N] | held [C][N] | dev [R][6] | n, n_skipped
  // [R] | seen [C]: (C + 3 R) N + 6 R doubles and C + 2 R counters (vk_chain_set_predictive)
  DevBlock pred_mem;
  vkpred::Predictive pred{};

  size_t series() const { return (size_t)(C / ac.group) * P; }          // C / group problems x P parameters

  // the layouts of those blocks, from the words' own counts (m.group, m.n_bins, ...)
  void marginals_layout(Carve& c, vkmarg::Marginals& m) const {
    const size_t problems = (size_t)(C / m.group);
    c.take(m.h1, problems * P * ((size_t)m.n_bins + 2));
    c.take(m.h2, problems * m.n_pairs * ((size_t)m.n_bins2 * m.n_bins2));
  }

  void autocorr_layout(Carve& c, vkac::Autocorr& a) const {
    const size_t n = (size_t)(C / a.group) * P, lags = n * (size_t)a.max_lag;
    c.take(a.pivot, n);
    c.take(a.total, n);
    c.take(a.head, lags);
    c.take(a.ring, lags);
    c.take(a.acc, lags);
  }

  void predictive_layout(Carve& c, vkpred::Predictive& p) const {
    const size_t n = C, R = n / p.group, N = p.N;
    c.take(p.pivot_t, R * N);
    c.take(p.sum_t, R * N);
    c.take(p.sum_tt, R * N);
    c.take(p.held, n * N);
    c.take(p.dev, R * vkpred::kDeviance);
    c.take(p.n, R);
    c.take(p.n_skipped, R);
    c.take(p.seen, n);
  }

  void temper_layout(Carve& c, TemperArgs& t, double*& logs, int K) const {
    const size_t n = C;
    double* betas = nullptr;
    c.take(betas, (size_t)K);
    t.betas = betas;
    c.take(t.pivot_e, n);                    // (pivot_e .. e2 and n_e .. n_swap_acc are contiguous: zeroed in two calls)
    c.take(t.e1, n);
    c.take(t.e2, n);
    c.take(logs, (size_t)vkchain::kBlock * n);
    c.take(t.n_e, n);
    c.take(t.n_swap_try, n);
    c.take(t.n_swap_acc, n);
  }

  void stretch_layout(Carve& c) {
    const size_t block = (size_t)vkchain::kBlock * C;         // 64 sweeps x 2 halves x C / 2
    c.take(d_sz, block);
    c.take(d_slz, block);
    c.take(d_slogu, block);
    c.take(d_prop, (size_t)P * (C / 2));
    c.take(d_partner, block);
  }

  void shape(int n, const double* lo, const double* hi) {
    C = n;
    T = vkchain::n_tri(P);
    rows_max = (size_t)C;
    box.d = P;
    for (int j = 0; j < P; ++j) {
      box.lo[j] = lo[j];
      box.hi[j] = hi[j];
    }
  }
  // state | base, x0, rows, results, theory workspace | one block of random numbers | one block of history | counters | indices
  void layout(Carve& c) {
    const size_t n = C, block = vkchain::kBlock * n;
    blend_layout(c);
    c.take(d_x, n * P);
    c.take(d_lnl, n);
    c.take(d_chi, n);
    c.take(d_pivot, n * P);
    c.take(d_sum1, n * P);
    c.take(d_sum2, n * T);
    c.take(d_base, sets * n * VK_NPAR);
    c.take(d_x0, n * P);
    c.take(d_rows, sets * n * VK_NPAR);
    c.take(d_res_lnl, n);
    c.take(d_res_chi, n);
    c.take(d_th, workspace_doubles());
    c.take(d_dz, block * P);
    c.take(d_logu, block);
    c.take(d_hx, block * P);
    c.take(d_hl, block);
    c.take(d_hc, block);
    c.take(d_acc, n);
    c.take(d_steps, n);
    c.take(d_kept, n);
    c.take(d_which, n);
    c.take(d_row_which, n);
  }
};

static ChainArgs chain_args(const vk_chain* f) {
  ChainArgs a{};
  a.box = f->box;
  a.C = f->C;
  a.x = f->d_x;
  a.lnl = f->d_lnl;
  a.chi2 = f->d_chi;
  a.pivot = f->d_pivot;
  a.sum1 = f->d_sum1;
  a.sum2 = f->d_sum2;
  a.n_accept = f->d_acc;
  a.n_steps = f->d_steps;
  a.n_kept = f->d_kept;
  a.base = f->d_base;
  a.which = f->real ? f->d_which : nullptr;
  a.x0 = f->d_x0;
  a.res_lnl = f->d_res_lnl;
  a.res_chi2 = f->d_res_chi;
  a.rows = f->d_rows;
  a.row_which = f->real ? f->d_row_which : nullptr;
  for (int j = 0; j < vkchain::kMaxP; ++j) a.col[j] = f->col[j];
  a.alpha = f->alpha;
  a.blocks = f->row_sets((size_t)f->C);
  a.prior = f->prior;
  a.marg = f->marg;
  return a;
}

// What a setter's clearing form does, and a setter that replaces state first: no such state any more - the words the kernels
// take read "off", and the handle makes the launches it made before it had any.
template <class Words>
static int chain_drop(vk_chain* f, DevBlock& mem, Words& words) {
  mem.drop(f);
  words = Words{};
  f->err.clear();
  return VK_OK;
}

// what a getter ends with: the arrays the caller asked for, complete on return
static int chain_home(vk_chain* f, std::initializer_list<Home> arrays) {
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const int rc = sampled_home(f, arrays);
  if (rc == VK_OK) f->err.clear();
  return rc;
}

// the refusals several entry points share (`me`: "vk_chain_...: ")
static int refused_in_flight(vk_chain* f, const std::string& me) {
  return refused(f, me + "a block begun with vk_chain_begin is awaiting vk_chain_finish");
}
static int refused_groups(vk_chain* f, const std::string& me, const std::string& groups) {
  return refused(f, me + std::to_string(f->C) + " chains are not a whole number of " + groups);
}

// The chains of a group (`size` consecutive ones) move along or exchange each other's positions, so they share a data vector:
// one realisation per group, that of its first chain (`first`: what the texts call it).  The indices are read back once.
static int chain_one_realisation(vk_chain* f, const std::string& me, int size, const char* first) {
  if (!f->real) return VK_OK;
  if (f->h_which.empty()) {
    std::vector<int> which(f->C);
    VK_SAMPLED_HIP(f, hipMemcpy(which.data(), f->d_which, (size_t)f->C * sizeof(int), hipMemcpyDeviceToHost));
    f->h_which.swap(which);
  }
  for (int c = 0; c < f->C; ++c)
    if (f->h_which[c] != f->h_which[c - c % size])
      return refused(f, me + "chain " + std::to_string(c) + " is not of the realisation of " + first);
  return VK_OK;
}

// the hold behind the step kernel of a launch of M rows (half == 0: a Metropolis launch), before the next evaluation overwrites
// d_th: one wave per row
static int chain_hold(vk_chain* f, int M, int half, int side, bool all) {
  HoldArgs h{};
  h.p = f->pred;
  h.th = f->d_th;
  h.n_accept = f->d_acc;
  h.M = M;
  h.half = half;
  h.side = side;
  h.all = all ? 1 : 0;
  return sampled_launch(f, vk_chain_hold_kernel, (long long)M * kChainBlock, kChainBlock, h);
}

// the predict kernel behind the hold of a kept step (a kept sweep's second half), or behind the start's hold: the pivots
static int chain_predict(vk_chain* f, bool start) {
  PredictArgs q{};
  q.p = f->pred;
  q.chi2 = f->d_chi;
  q.lnl = f->d_lnl;
  q.R = f->C / f->pred.group;
  q.start = start ? 1 : 0;
  const long long per = (f->pred.N + kChainBlock - 1) / kChainBlock;       // blocks of a problem
  return sampled_launch(f, vk_chain_predict_kernel, q.R * per * kChainBlock, kChainBlock, q);
}

// fresh energy sums and swap counters, in stream order
static hipError_t chain_zero_tempering(vk_chain* f) {
  const size_t n = f->C;
  hipError_t e = hipMemsetAsync(f->temper.pivot_e, 0, 3 * n * sizeof(double), f->ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(f->temper.n_e, 0, 3 * n * sizeof(long long), f->ctx->stream);
  return e;
}

// the series kernel behind the step kernel of a kept step (a kept sweep's second half): one wave per (problem, parameter)
static int chain_series(vk_chain* f) {
  SeriesArgs s{};
  s.ac = f->ac;
  s.x = f->d_x;
  s.C = f->C;
  s.d = f->P;
  const int rc = sampled_launch(f, vk_chain_series_kernel, (long long)f->series() * kChainBlock, kChainBlock, s);
  if (rc == VK_OK) f->ac.n += 1;
  return rc;
}

// ---- what vk_chain_begin, vk_chain_begin_stretch and vk_chain_begin_tempered share (`who`: the entry point, a block of `noun`) --
// the refusals between an entry point's NULL arguments (`null_arg`) and its own checks
static int begin_check(vk_chain* f, const char* who, const char* noun, bool null_arg, int32_t n_steps, int64_t first_step,
                       int64_t burn, int64_t thin) {
  const std::string me = std::string(who) + ": ";
  if (null_arg) return refused(f, me + "NULL argument");
  if (!f->started) return refused(f, me + "the chains have no start (vk_chain_start)");
  if (f->in_flight) return refused(f, me + "the previous block has not been finished (vk_chain_finish)");
  if (n_steps < 1 || n_steps > vkchain::kBlock) return refused(f, me + "need 1 <= " + noun + " <= 64 in a block");
  if (first_step < 0 || burn < 0 || thin < 1) return refused(f, me + "need first_step >= 0, burn >= 0, thin >= 1");
  return VK_OK;
}

// ... and behind them: may the handle use its context now?
static int begin_ready(vk_chain* f, const char* who) {
  const int rc = sampled_ready(f, who, "chain", true);
  if (rc) return rc;
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  return VK_OK;
}

// a step's (a sweep's) place in the pattern: is it kept, and the history slot of `a` it then fills, the block's slot-th
static bool begin_slot(const vk_chain* f, ChainArgs& a, int64_t step, int64_t burn, int64_t thin, bool want_history, int& slot) {
  const bool kept = vkchain::is_kept(step, burn, thin), hist = kept && want_history;
  const size_t C = f->C;
  a.kept = kept ? 1 : 0;
  a.hist_x = hist ? f->d_hx + (size_t)slot * C * f->P : nullptr;
  a.hist_lnl = hist ? f->d_hl + (size_t)slot * C : nullptr;
  a.hist_chi2 = hist ? f->d_hc + (size_t)slot * C : nullptr;
  if (hist) ++slot;
  return kept;
}

// everything is enqueued, or rc says what failed (the handle holds its text)
static int begin_done(vk_chain* f, int rc, int32_t n_steps, int slot, int32_t* n_kept) {
  if (rc) return sampled_abort(f, rc);
  f->in_flight = n_steps;
  f->block_kept = slot;
  if (n_kept) *n_kept = slot;
  f->err.clear();
  return VK_OK;
}

extern "C" {

vk_chain* vk_chain_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_chains, int32_t n_params, const int32_t* columns,
                          const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which, char* err,
                          size_t errlen) {
  return sampled_create<vk_chain>("vk_chain_create", "chain", &ctx, 1, false, nullptr, opts, n_chains, n_params, columns, nullptr,
                                  lo, hi, base_rows, alpha, which, err, errlen);
}

vk_chain* vk_chain_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_chains,
                                int32_t n_params, const int32_t* columns, const double* lo, const double* hi, const double* base_rows,
                                double alpha, const int32_t* which, char* err, size_t errlen) {
  return sampled_create<vk_chain>("vk_chain_create_joint", "chain", ctxs, n_ctx, true, cov, opts, n_chains, n_params, columns,
                                  nullptr, lo, hi, base_rows, alpha, which, err, errlen);
}

vk_chain* vk_chain_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                       int32_t n_chains, int32_t n_params, const int32_t* columns, const int32_t* param_block,
                                       const double* lo, const double* hi, const double* base_rows, double alpha,
                                       const int32_t* which, char* err, size_t errlen) {
  if (no_param_block("vk_chain_create_joint_blocks", param_block, err, errlen)) return nullptr;
  return sampled_create<vk_chain>("vk_chain_create_joint_blocks", "chain", ctxs, n_ctx, true, cov, opts, n_chains, n_params, columns,
                                  param_block, lo, hi, base_rows, alpha, which, err, errlen);
}

const char* vk_chain_last_error(const vk_chain* f) { return f ? f->err.c_str() : ""; }

int vk_chain_set_prior(vk_chain* f, const double* mu, const double* pp_packed) {
  if (!f) return VK_E_ARG;
  if (f->in_flight) return refused_in_flight(f, "vk_chain_set_prior: ");
  return sampled_set_prior(f, "vk_chain_set_prior", mu, pp_packed);
}

// The marginal histograms of the kept positions (vk_marginals.h).  Everything the kernels index with is checked here: the
// group, the bin counts and the pair list fix the size of the buffers the slots address.
int vk_chain_set_marginals(vk_chain* f, int32_t group, int32_t n_bins, const double* lo, const double* hi, int32_t n_pairs,
                           const int32_t* pairs, int32_t n_bins2) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_chain_set_marginals: ";
  if (f->in_flight) return refused_in_flight(f, me);
  if (n_bins == 0 && !lo && !hi) return chain_drop(f, f->marg_mem, f->marg);
  if (n_bins < 1 || n_bins > vkmarg::kMaxBins) return refused(f, me + "need 1 <= n_bins <= 1024 (0 with NULL ranges clears)");
  if (!lo || !hi) return refused(f, me + "NULL argument");
  if (group < 1 || f->C % group) return refused_groups(f, me, "groups of " + std::to_string(group));
  if (n_pairs < 0 || n_pairs > vkmarg::kMaxPairs) return refused(f, me + "need 0 <= n_pairs <= 45");
  if (n_pairs > 0 && !pairs) return refused(f, me + "NULL argument");
  if (n_pairs > 0 && (n_bins2 < 1 || n_bins2 > vkmarg::kMaxBins2)) return refused(f, me + "need 1 <= n_bins2 <= 128");
  for (int j = 0; j < f->P; ++j)
    if (!__builtin_isfinite(lo[j]) || !__builtin_isfinite(hi[j]) || !(lo[j] < hi[j]) || !__builtin_isfinite(hi[j] - lo[j]))
      return refused(f, me + "the range of parameter " + std::to_string(j) + " is not finite with lo < hi");
  vkmarg::Marginals m{};
  for (int p = 0; p < n_pairs; ++p) {
    const int j = pairs[2 * p], k = pairs[2 * p + 1];
    if (j < 0 || k >= f->P || j >= k)
      return refused(f, me + "pair " + std::to_string(p) + " (" + std::to_string(j) + ", " + std::to_string(k) + ") needs 0 <= j < k < " +
                            std::to_string(f->P));
    for (int q = 0; q < p; ++q)
      if (m.pair[q][0] == j && m.pair[q][1] == k) return refused(f, me + "pair " + std::to_string(p) + " repeats pair " + std::to_string(q));
    m.pair[p][0] = j;
    m.pair[p][1] = k;
  }
  m.on = 1;
  m.group = group;
  m.n_bins = n_bins;
  m.n_pairs = n_pairs;
  m.n_bins2 = n_pairs > 0 ? n_bins2 : 1;
  for (int j = 0; j < f->P; ++j) {
    m.a[j] = lo[j];
    m.b[j] = hi[j];
    m.inv[j] = vkmarg::inverse_width(m.n_bins, lo[j], hi[j]);
    m.inv2[j] = vkmarg::inverse_width(m.n_bins2, lo[j], hi[j]);
  }
  chain_drop(f, f->marg_mem, f->marg);     // (a failed allocation leaves the handle without marginals)
  const int rc = f->marg_mem.make(f, me, [&](Carve& c) { f->marginals_layout(c, m); });
  if (rc) return rc;
  f->marg = m;
  f->err.clear();
  return VK_OK;
}

int vk_chain_marginals(vk_chain* f, int64_t* h1, int64_t* h2) {
  if (!f) return VK_E_ARG;
  if (f->in_flight) return refused_in_flight(f, "vk_chain_marginals: ");
  if (!f->marg.on) return refused(f, "vk_chain_marginals: the handle has no marginals (vk_chain_set_marginals)");
  const size_t first = (size_t)(f->marg.h2 - f->marg.h1) * sizeof(int64_t);         // h1 | h2 fill the block
  return chain_home(f, {{h1, f->marg.h1, first}, {h2, f->marg.h2, f->marg_mem.bytes - first}});
}

// The running autocorrelation of the ensemble series (vk_autocorr.h).  Everything the series kernel indexes with is checked
// here: the group and the lag count fix the size of the state it addresses.
int vk_chain_set_autocorr(vk_chain* f, int32_t group, int32_t max_lag) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_chain_set_autocorr: ";
  if (f->in_flight) return refused_in_flight(f, me);
  if (max_lag == 0) return chain_drop(f, f->ac_mem, f->ac);
  if (max_lag < 1 || max_lag > vkac::kMaxLag) return refused(f, me + "need 1 <= max_lag <= 1024 (0 clears)");
  if (group < 1 || f->C % group) return refused_groups(f, me, "groups of " + std::to_string(group));
  vkac::Autocorr a{};
  a.on = 1;
  a.group = group;
  a.max_lag = max_lag;
  a.n = 0;
  chain_drop(f, f->ac_mem, f->ac);         // (a failed allocation leaves the handle without autocorrelation)
  const int rc = f->ac_mem.make(f, me, [&](Carve& c) { f->autocorr_layout(c, a); });
  if (rc) return rc;
  f->ac = a;
  f->err.clear();
  return VK_OK;
}

int vk_chain_autocorr(vk_chain* f, double* pivot, double* total, double* head, double* ring, double* acc, int64_t* n) {
  if (!f) return VK_E_ARG;
  if (f->in_flight) return refused_in_flight(f, "vk_chain_autocorr: ");
  if (!f->ac.on) return refused(f, "vk_chain_autocorr: the handle has no autocorrelation (vk_chain_set_autocorr)");
  const size_t one = f->series() * sizeof(double), lags = one * (size_t)f->ac.max_lag;
  const vkac::Autocorr& a = f->ac;
  const int rc = chain_home(f, {{pivot, a.pivot, one}, {total, a.total, one}, {head, a.head, lags}, {ring, a.ring, lags}, {acc, a.acc, lags}});
  if (rc == VK_OK && n) *n = (int64_t)a.n;
  return rc;
}

// The posterior-predictive sums (vk_predictive.h).  Everything the two kernels index with is checked here: the group and the
// context's N fix the size of the state they address.
int vk_chain_set_predictive(vk_chain* f, int32_t group) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_chain_set_predictive: ";
  if (f->in_flight) return refused_in_flight(f, me);
  if (group == 0) {
    f->keep_theory = false;
    return chain_drop(f, f->pred_mem, f->pred);
  }
  if (!f->blocks.empty())
    return refused(f, me + "a joint handle (vk_chain_create_joint) is refused: its theory workspace is laid out by the route that "
                           "evaluates it, not as one vector per row");
  if (f->blend.on)
    return refused(f, me + "the handle blends the likelihood between two grid betas (VK_OPT_BETA_BLEND): a point has two theory "
                           "vectors, and the sums are of one");
  if (f->temper.K)
    return refused(f, me + "the handle is tempered (vk_chain_set_tempering): a swap moves states without touching the accept "
                           "counters the held vectors follow");
  if (f->real && f->ctx->n_cuts > 0)
    return refused(f, me + "scale cuts are resident on the context (vk_set_cuts): the predictive sums and the DIC are of the full "
                           "data vector");
  if (group < 1 || f->C % group) return refused_groups(f, me, "groups of " + std::to_string(group));
  vkpred::Predictive p{};
  p.on = 1;
  p.group = group;
  p.N = f->ctx->N;
  DevBlock mem;
  const int rc = mem.make(f, me, [&](Carve& c) { f->predictive_layout(c, p); });
  if (rc) return rc;                       // (the handle keeps the sums it had, as after a refusal)
  f->pred_mem.drop(f);
  f->pred_mem = mem;
  f->pred = p;
  f->keep_theory = true;
  f->started = false;                      // the held vectors are taken at the start: chains already running need a new one
  f->err.clear();
  return VK_OK;
}

int vk_chain_predictive(vk_chain* f, double* pivot_t, double* sum_t, double* sum_tt, double* deviance, int64_t* n, int64_t* n_skipped,
                        double* held) {
  if (!f) return VK_E_ARG;
  if (f->in_flight) return refused_in_flight(f, "vk_chain_predictive: ");
  if (!f->pred.on) return refused(f, "vk_chain_predictive: the handle has no predictive sums (vk_chain_set_predictive)");
  const vkpred::Predictive& p = f->pred;
  const size_t R = (size_t)f->C / p.group, one = R * sizeof(double), vec = one * p.N;
  return chain_home(f, {{pivot_t, p.pivot_t, vec}, {sum_t, p.sum_t, vec}, {sum_tt, p.sum_tt, vec}, {deviance, p.dev, one * vkpred::kDeviance},
                        {n, p.n, R * sizeof(int64_t)}, {n_skipped, p.n_skipped, R * sizeof(int64_t)},
                        {held, p.held, (size_t)f->C * p.N * sizeof(double)}});
}

void vk_chain_destroy(vk_chain* f) {
  if (!f) return;
  if (f->in_flight) (void)hipStreamSynchronize(f->ctx->stream);
  for (DevBlock* mem : {&f->marg_mem, &f->ac_mem, &f->temper_mem, &f->pred_mem, &f->stretch}) mem->drop(f);
  sampled_destroy(f);
}

int vk_chain_start(vk_chain* f, const double* x0) {
  if (!f) return VK_E_ARG;
  vk_ctx* ctx = f->ctx;
  if (!x0) return refused(f, "vk_chain_start: NULL argument");
  if (f->in_flight) return refused_in_flight(f, "vk_chain_start: ");
  int rc = sampled_ready(f, "vk_chain_start", "chain", true);
  if (rc) return rc;
  for (int c = 0; c < f->C; ++c)
    if (!vkchain::in_box(f->box, x0 + (size_t)c * f->P))
      return refused(f, "vk_chain_start: the start of chain " + std::to_string(c) + " is outside the box");
  VK_SAMPLED_HIP(f, hipSetDevice(ctx->device));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_x0, x0, (size_t)f->C * f->P * sizeof(double), hipMemcpyHostToDevice));
  // fresh chains: fresh histograms, series and predictive sums, as the counters and the moment sums (in stream order) ...
  for (DevBlock* mem : {&f->marg_mem, &f->ac_mem, &f->pred_mem})
    if (mem->p) VK_SAMPLED_HIP(f, mem->zero(f));
  f->ac.n = 0;
  if (f->temper.K) VK_SAMPLED_HIP(f, chain_zero_tempering(f));          // ... and fresh energy sums and swap counters
  ChainArgs a = chain_args(f);
  rc = sampled_launch(f, vk_chain_init_kernel, a.C, kChainBlock, a);
  if (rc == VK_OK) rc = sampled_evaluate(f, f->C, f->d_res_lnl, f->d_res_chi);
  a.adopt = 1;
  if (rc == VK_OK) rc = sampled_launch(f, vk_chain_step_kernel, a.C, kChainBlock, a);
  if (rc == VK_OK && f->pred.on) rc = chain_hold(f, f->C, 0, 0, true);   // every chain holds its start's theory vector ...
  if (rc == VK_OK && f->pred.on) rc = chain_predict(f, true);            // ... and the pivots are taken from it
  if (rc) return sampled_abort(f, rc);
  VK_SAMPLED_HIP(f, hipStreamSynchronize(ctx->stream));
  f->started = true;
  f->err.clear();
  return VK_OK;
}

int vk_chain_begin(vk_chain* f, int32_t n_steps, const double* dz, const double* logu, int64_t first_step, int64_t burn, int64_t thin,
                   int32_t want_history, int32_t* n_kept) {
  if (!f) return VK_E_ARG;
  int rc = begin_check(f, "vk_chain_begin", "steps", !dz || !logu, n_steps, first_step, burn, thin);
  if (rc == VK_OK) rc = begin_ready(f, "vk_chain_begin");
  if (rc) return rc;
  const size_t C = f->C, P = f->P;
  // the stream is idle (the block before was finished): plain copies, complete on return
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_dz, dz, (size_t)n_steps * C * P * sizeof(double), hipMemcpyHostToDevice));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_logu, logu, (size_t)n_steps * C * sizeof(double), hipMemcpyHostToDevice));
  ChainArgs a = chain_args(f);
  a.dz = f->d_dz;
  rc = sampled_launch(f, vk_chain_propose_kernel, a.C, kChainBlock, a);
  int slot = 0;
  for (int t = 0; t < n_steps && rc == VK_OK; ++t) {
    rc = sampled_evaluate(f, f->C, f->d_res_lnl, f->d_res_chi);
    if (rc) break;
    const bool kept = begin_slot(f, a, first_step + t, burn, thin, want_history != 0, slot);
    a.dz = f->d_dz + (size_t)t * C * P;
    a.logu = f->d_logu + (size_t)t * C;
    a.dz_next = t + 1 < n_steps ? a.dz + C * P : nullptr;
    rc = sampled_launch(f, vk_chain_step_kernel, a.C, kChainBlock, a);
    if (rc == VK_OK && kept && f->ac.on) rc = chain_series(f);
    if (rc == VK_OK && f->pred.on) rc = chain_hold(f, f->C, 0, 0, false);      // (every step: accepts happen on steps not kept)
    if (rc == VK_OK && kept && f->pred.on) rc = chain_predict(f, false);
  }
  return begin_done(f, rc, n_steps, slot, n_kept);
}

// A block of stretch-move sweeps on the chains of a handle read as C / walkers ensembles (vk_kernel_stretch.h).  Per half-step:
// the propose kernel, the evaluation of the C / 2 rows (sampled_evaluate: of a joint fit, forked onto the blocks' streams and
// joined back onto the lead stream) and the step kernel - plain launches on the handle's stream, no host synchronisation and no
// graph inside the block.  Everything the kernels index with is checked here first.
int vk_chain_begin_stretch(vk_chain* f, int32_t n_steps, int32_t walkers, const double* z, const double* lz, const double* logu,
                           const int32_t* partner, int64_t first_step, int64_t burn, int64_t thin, int32_t want_history,
                           int32_t* n_kept) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_chain_begin_stretch: ";
  int rc = begin_check(f, "vk_chain_begin_stretch", "sweeps", !z || !lz || !logu || !partner, n_steps, first_step, burn, thin);
  if (rc) return rc;
  if (walkers < 2 || walkers % 2) return refused(f, me + "an ensemble needs an even number of walkers, at least 2");
  if (f->C % walkers) return refused_groups(f, me, "ensembles of " + std::to_string(walkers));
  const int half = walkers / 2;
  const size_t M = (size_t)f->C / 2, n = (size_t)n_steps * 2 * M;
  for (size_t i = 0; i < n; ++i)
    if (partner[i] < 0 || partner[i] >= half)
      return refused(f, me + "partner index " + std::to_string(partner[i]) + " (entry " + std::to_string(i) + ") is outside 0.." +
                            std::to_string(half - 1));
  rc = begin_ready(f, "vk_chain_begin_stretch");
  if (rc == VK_OK) rc = chain_one_realisation(f, me, walkers, "its ensemble's first walker");     // (partners share a data vector)
  if (rc) return rc;
  // (the buffers are written before they are read: not zeroed)
  if (!f->stretch.p && !carve_alloc(f->ctx->device, f->stretch.p, f->stretch.bytes, [&](Carve& c) { f->stretch_layout(c); })) {
    f->err = me + cannot_allocate(f->stretch.bytes);
    return VK_E_HIP;
  }
  // the stream is idle (the block before was finished): plain copies, complete on return
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_sz, z, n * sizeof(double), hipMemcpyHostToDevice));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_slz, lz, n * sizeof(double), hipMemcpyHostToDevice));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_slogu, logu, n * sizeof(double), hipMemcpyHostToDevice));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_partner, partner, n * sizeof(int), hipMemcpyHostToDevice));
  StretchArgs a{};
  a.c = chain_args(f);
  a.half = half;
  a.M = (int)M;
  a.prop = f->d_prop;
  int slot = 0;
  for (int t = 0; t < n_steps && rc == VK_OK; ++t) {
    const bool kept = begin_slot(f, a.c, first_step + t, burn, thin, want_history != 0, slot);
    for (int side = 0; side < 2 && rc == VK_OK; ++side) {
      const size_t at = ((size_t)t * 2 + side) * M;
      a.side = side;
      a.z = f->d_sz + at;
      a.lz = f->d_slz + at;
      a.logu = f->d_slogu + at;
      a.partner = f->d_partner + at;
      rc = sampled_launch(f, vk_stretch_propose_kernel, a.M, kChainBlock, a);
      if (rc == VK_OK) rc = sampled_evaluate(f, (long long)M, f->d_res_lnl, f->d_res_chi);
      if (rc == VK_OK) rc = sampled_launch(f, vk_stretch_step_kernel, a.M, kChainBlock, a);
      if (rc == VK_OK && f->pred.on) rc = chain_hold(f, (int)M, half, side, false);
    }
    if (rc == VK_OK && kept && f->ac.on) rc = chain_series(f);     // (behind the second half: all W walkers as the sweep leaves them)
    if (rc == VK_OK && kept && f->pred.on) rc = chain_predict(f, false);
  }
  return begin_done(f, rc, n_steps, slot, n_kept);
}

// Replica exchange on the chains of a handle read as C / (rungs walkers) problems of `rungs` temperatures and `walkers` ladders
// each (vk_kernel_temper.h).  Everything the two kernels index with is checked here: rungs and walkers fix the pairs the swap
// kernel addresses and the size of the arrays the step kernel adds to.
int vk_chain_set_tempering(vk_chain* f, int32_t rungs, int32_t walkers, const double* betas) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_chain_set_tempering: ";
  if (f->in_flight) return refused_in_flight(f, me);
  if (rungs == 0) {
    f->d_logs = nullptr;
    return chain_drop(f, f->temper_mem, f->temper);
  }
  if (rungs < 1 || walkers < 1) return refused(f, me + "need rungs >= 1 and walkers >= 1 (rungs == 0 clears)");
  if (f->pred.on)
    return refused(f, me + "the handle keeps predictive sums (vk_chain_set_predictive), which follow the accept counters: a swap "
                           "moves states without touching them");
  if (!betas) return refused(f, me + "NULL argument");
  const long long ladder = (long long)rungs * walkers;
  if (ladder > f->C || f->C % ladder)
    return refused_groups(f, me, "problems of " + std::to_string(rungs) + " rungs x " + std::to_string(walkers) + " walkers");
  for (int k = 0; k < rungs; ++k)
    if (!__builtin_isfinite(betas[k]) || betas[k] < 0.0)
      return refused(f, me + "the inverse temperature of rung " + std::to_string(k) + " is not finite and >= 0");
  if (betas[0] != 1.0) return refused(f, me + "rung 0 is the posterior itself: betas[0] must be 1");
  for (int k = 1; k < rungs; ++k)
    if (!(betas[k] < betas[k - 1])) return refused(f, me + "the inverse temperatures must decrease strictly from rung to rung");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  int rc = chain_one_realisation(f, me, (int)ladder, "its problem's first chain");      // (the rungs of a ladder exchange positions)
  if (rc) return rc;
  f->d_logs = nullptr;
  chain_drop(f, f->temper_mem, f->temper);   // (a failed allocation leaves the handle without tempering)
  TemperArgs t{};
  double* logs = nullptr;
  rc = f->temper_mem.make(f, me, [&](Carve& c) { f->temper_layout(c, t, logs, rungs); });
  if (rc) return rc;
  if (hipMemcpy(const_cast<double*>(t.betas), betas, (size_t)rungs * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    f->temper_mem.drop(f);
    f->err = me + "upload failed";
    return VK_E_HIP;
  }
  t.K = rungs;
  t.W = walkers;
  f->temper = t;
  f->d_logs = logs;
  f->err.clear();
  return VK_OK;
}

int vk_chain_tempering(vk_chain* f, double* pivot_e, double* e1, double* e2, int64_t* n_e, int64_t* n_swap_try, int64_t* n_swap_acc) {
  if (!f) return VK_E_ARG;
  if (f->in_flight) return refused_in_flight(f, "vk_chain_tempering: ");
  if (!f->temper.K) return refused(f, "vk_chain_tempering: the handle has no tempering (vk_chain_set_tempering)");
  const TemperArgs& t = f->temper;
  const size_t one = (size_t)f->C * sizeof(double);                      // (sums and counters alike: [C] words of 8 bytes)
  return chain_home(f, {{pivot_e, t.pivot_e, one}, {e1, t.e1, one}, {e2, t.e2, one}, {n_e, t.n_e, one}, {n_swap_try, t.n_swap_try, one},
                        {n_swap_acc, t.n_swap_acc, one}});
}

// A block of tempered steps (vk_kernel_temper.h).  Per step: the evaluation of the C rows and the tempered step kernel, which
// writes the next rows itself - unless a swap event follows the step: then the step kernel writes none, the swap kernel exchanges
// the states of the event's pairs and the propose kernel forms the next rows from what the swap left.  Plain launches on the
// handle's stream, no host synchronisation and no graph inside the block.
int vk_chain_begin_tempered(vk_chain* f, int32_t n_steps, const double* dz, const double* logu, const double* logs, int64_t swap_every,
                            int64_t first_step, int64_t burn, int64_t thin, int32_t want_history, int32_t* n_kept) {
  if (!f) return VK_E_ARG;
  const char* who = "vk_chain_begin_tempered";
  if (!f->temper.K) return refused(f, std::string(who) + ": the handle has no tempering (vk_chain_set_tempering)");
  int rc = begin_check(f, who, "steps", !dz || !logu || (swap_every > 0 && !logs), n_steps, first_step, burn, thin);
  if (rc) return rc;
  if (swap_every < 0) return refused(f, std::string(who) + ": need swap_every >= 0 (0: never)");
  rc = begin_ready(f, who);
  if (rc) return rc;
  const size_t C = f->C, P = f->P;
  // the stream is idle (the block before was finished): plain copies, complete on return
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_dz, dz, (size_t)n_steps * C * P * sizeof(double), hipMemcpyHostToDevice));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_logu, logu, (size_t)n_steps * C * sizeof(double), hipMemcpyHostToDevice));
  if (swap_every > 0) VK_SAMPLED_HIP(f, hipMemcpy(f->d_logs, logs, (size_t)n_steps * C * sizeof(double), hipMemcpyHostToDevice));
  TemperStepArgs g{};
  g.c = chain_args(f);
  g.t = f->temper;
  ChainArgs& a = g.c;
  SwapArgs w{};
  w.C = f->C;
  w.d = f->P;
  w.x = f->d_x;
  w.lnl = f->d_lnl;
  w.chi2 = f->d_chi;
  w.t = f->temper;
  const int problems = f->C / (f->temper.K * f->temper.W);
  a.dz = f->d_dz;
  rc = sampled_launch(f, vk_chain_propose_kernel, a.C, kChainBlock, a);
  int slot = 0;
  for (int t = 0; t < n_steps && rc == VK_OK; ++t) {
    rc = sampled_evaluate(f, f->C, f->d_res_lnl, f->d_res_chi);
    if (rc) break;
    const bool kept = begin_slot(f, a, first_step + t, burn, thin, want_history != 0, slot);
    // a swap event with no pair (one rung; two rungs at odd parity) is no event: the step kernel keeps writing the next rows
    const int parity = vktemper::is_swap(first_step + t, swap_every) ? vktemper::swap_parity(first_step + t, swap_every) : 0;
    const int pairs = vktemper::is_swap(first_step + t, swap_every) ? vktemper::pairs_of(f->temper.K, parity) : 0;
    a.dz = f->d_dz + (size_t)t * C * P;
    a.logu = f->d_logu + (size_t)t * C;
    const double* next = t + 1 < n_steps ? a.dz + C * P : nullptr;
    a.dz_next = pairs ? nullptr : next;
    rc = sampled_launch(f, vk_chain_step_tempered_kernel, a.C, kChainBlock, g);
    if (rc == VK_OK && kept && f->ac.on) rc = chain_series(f);      // (the positions the sums have just taken: before the swap)
    if (rc == VK_OK && pairs) {
      w.logs = f->d_logs + (size_t)t * C;
      w.parity = parity;
      w.pairs = pairs;
      w.n = problems * pairs * f->temper.W;
      rc = sampled_launch(f, vk_chain_swap_kernel, w.n, kChainBlock, w);
      if (rc == VK_OK && next) {
        ChainArgs p = a;
        p.dz = next;
        rc = sampled_launch(f, vk_chain_propose_kernel, p.C, kChainBlock, p);
      }
    }
  }
  return begin_done(f, rc, n_steps, slot, n_kept);
}

int vk_chain_finish(vk_chain* f, double* x, double* lnl, double* chi2) {
  if (!f) return VK_E_ARG;
  vk_ctx* ctx = f->ctx;
  if (!f->in_flight) return refused(f, "vk_chain_finish: nothing was begun");
  if (f->block_kept > 0 && (!x || !lnl || !chi2)) {
    f->in_flight = f->block_kept = 0;
    f->err = "vk_chain_finish: the block keeps a history: NULL argument";
    return sampled_abort(f, VK_E_ARG);
  }
  const size_t n = (size_t)f->block_kept * f->C;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess && n) e = hipMemcpyAsync(x, f->d_hx, n * f->P * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(lnl, f->d_hl, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(chi2, f->d_hc, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  f->in_flight = 0;
  f->block_kept = 0;
  if (e != hipSuccess) {
    (void)hipGetLastError();
    f->err = std::string("vk_chain_finish: ") + hipGetErrorString(e);
    return VK_E_HIP;
  }
  f->err.clear();
  return VK_OK;
}

int vk_chain_state(vk_chain* f, double* x, double* lnl, double* chi2, int64_t* n_accept, int64_t* n_steps, int64_t* n_kept,
                   double* pivot, double* sum1, double* sum2) {
  if (!f) return VK_E_ARG;
  vk_ctx* ctx = f->ctx;
  if (!f->started || f->in_flight)
    return refused(f, f->started ? "vk_chain_state: a block begun with vk_chain_begin is awaiting vk_chain_finish"
                                 : "vk_chain_state: the chains have no start (vk_chain_start)");
  const size_t C = f->C, P = f->P, T = f->T;
  VK_SAMPLED_HIP(f, hipSetDevice(ctx->device));
  // the state block x | lnl | chi2 | pivot | sum1 | sum2 and the three counters are contiguous
  std::vector<double> h(C * (3 * P + 2 + T));
  std::vector<long long> n(3 * C);
  VK_SAMPLED_HIP(f, hipMemcpy(h.data(), f->d_x, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  VK_SAMPLED_HIP(f, hipMemcpy(n.data(), f->d_acc, n.size() * sizeof(long long), hipMemcpyDeviceToHost));
  const double *hx = h.data(), *hl = hx + C * P, *hc = hl + C, *hp = hc + C, *h1 = hp + C * P, *h2 = h1 + C * P;
  for (size_t c = 0; c < C; ++c) {
    for (size_t j = 0; j < P; ++j) {
      if (x) x[c * P + j] = hx[j * C + c];
      if (pivot) pivot[c * P + j] = hp[j * C + c];
      if (sum1) sum1[c * P + j] = h1[j * C + c];
      if (sum2)
        for (size_t k = j; k < P; ++k) {           // the packed triangle, mirrored into a full symmetric matrix
          const double v = h2[(size_t)vkchain::tri((int)P, (int)j, (int)k) * C + c];
          sum2[(c * P + j) * P + k] = v;
          sum2[(c * P + k) * P + j] = v;
        }
    }
    if (lnl) lnl[c] = hl[c];
    if (chi2) chi2[c] = hc[c];
    if (n_accept) n_accept[c] = n[c];
    if (n_steps) n_steps[c] = n[C + c];
    if (n_kept) n_kept[c] = n[2 * C + c];
  }
  f->err.clear();
  return VK_OK;
}

}  // extern "C"

// ---- grid posteriors: marginals, profiles and the evidence of every problem over one shared grid (include/victor_hip.h, -------
// vk_kernel_grid.h; the definition: victor_amd/grid.py, the index rules and the step: vk_grid.h) -------------------------------
// A grid handle is a Sampled with ONE base row whose pending rows are a chunk of the grid: per chunk a rows kernel, sampled_evaluate
// (the data-vector route with lnL, or enqueue_realisations in cross mode - d_row_which stays NULL, every row against every
// realisation, [n][R]), then the max, weight and accumulate kernels, all on the context's stream with no host synchronisation
// between chunks; vk_grid_run waits once at its end.  One allocation holds rows, workspace, the chunk's values and the accumulators.
struct __attribute__((visibility("hidden"))) vk_grid : Sampled {
  vkgrid::Shape g{};
  int R = 1, chunk = 0, n1 = 0, n2 = 0, n_pairs = 0, n_eps = 0;
  int axis_off[vkgrid::kMaxP] = {}, pair[vkgrid::kMaxPairs][2] = {}, pair_off[vkgrid::kMaxPairs] = {};
  long long done = 0;                      // flat indices [0, done) are in the accumulators
  vkgrid::Running* d_run = nullptr;        // [R + 1]: the problems', the prior's own
  double *d_nodes = nullptr, *d_eps = nullptr, *d_lnprior = nullptr, *d_lnl = nullptr, *d_chi = nullptr, *d_wp = nullptr;
  double *d_total = nullptr, *d_m1 = nullptr, *d_p1 = nullptr, *d_m2 = nullptr, *d_p2 = nullptr;

  void shape(int, const double*, const double*) { rows_max = (size_t)chunk; }
  void layout(Carve& c) {
    const size_t n = (size_t)chunk, r = (size_t)R;
    blend_layout(c);
    c.take(d_run, r + 1);
    c.take(d_base, VK_NPAR);
    c.take(d_rows, n * VK_NPAR);
    c.take(d_nodes, (size_t)n1);
    c.take(d_eps, (size_t)std::max(n_eps, 1));
    c.take(d_lnprior, n);
    c.take(d_lnl, n * r);
    c.take(d_chi, n * r);                  // the evaluation's chi-squares, then the chunk's weights (vk_grid_weight_kernel)
    c.take(d_wp, n);
    c.take(d_th, workspace_doubles());
    c.take(d_total, r + 1);
    c.take(d_m1, r * n1);
    c.take(d_p1, r * n1);
    c.take(d_m2, r * n2);
    c.take(d_p2, r * n2);
  }
  int Rp() const { return prior.on ? R + 1 : R; }
  long long cells() const { return 1 + (long long)n1 + n2; }
};

static GridArgs grid_args(const vk_grid* f) {
  GridArgs a{};
  a.shape = f->g;
  a.R = f->R;
  a.Rp = f->Rp();
  a.nodes = f->d_nodes;
  a.eps_pow = f->n_eps ? f->d_eps : nullptr;
  a.base = f->d_base;
  a.rows = f->d_rows;
  for (int j = 0; j < vkgrid::kMaxP; ++j) {
    a.col[j] = f->col[j];
    a.axis_off[j] = f->axis_off[j];
  }
  a.alpha = f->alpha;
  a.prior = f->prior;
  a.lnprior = f->d_lnprior;
  a.lnl = f->d_lnl;
  a.w = f->d_chi;
  a.wp = f->d_wp;
  a.run = f->d_run;
  a.total = f->d_total;
  a.m1 = f->d_m1;
  a.p1 = f->d_p1;
  a.m2 = f->d_m2;
  a.p2 = f->d_p2;
  a.n1 = f->n1;
  a.n2 = f->n2;
  a.n_pairs = f->n_pairs;
  a.pr = 1;
  while (a.pr < 64 && a.pr < a.Rp) a.pr *= 2;
  for (int q = 0; q < f->n_pairs; ++q) {
    a.pair[q][0] = f->pair[q][0];
    a.pair[q][1] = f->pair[q][1];
    a.pair_off[q] = f->pair_off[q];
  }
  return a;
}

// may the handle run now: the context, and of the realisation route that the set on the context is the one it was made for
static int grid_ready(vk_grid* f, const char* who) {
  int rc = sampled_ready(f, who, "grid", true);
  if (rc) return rc;
  if (f->real && vkh::n_problems(f->ctx) != f->R)
    return refused(f, std::string(who) + ": the context holds " + std::to_string(vkh::n_problems(f->ctx)) + " realisations, the grid was made for " +
                          std::to_string(f->R));
  if (f->real && f->ctx->n_sets > 0)
    return refused(f, std::string(who) + ": model realisations are set on the context (vk_set_model_realisations): a point has one "
                          "theory vector per realisation, and a grid evaluates every point once");
  return VK_OK;
}

// the launches of flat indices [first, end), chunk by chunk
static int grid_chunks(vk_grid* f, long long first, long long end) {
  GridArgs a = grid_args(f);
  int rc = VK_OK;
  if (first == 0) {
    const long long most = std::max<long long>({a.Rp, (long long)a.R * a.n1, (long long)a.R * a.n2});
    rc = sampled_launch(f, vk_grid_init_kernel, most, kGridBlock, a);
  }
  for (long long g0 = first; g0 < end && rc == VK_OK; g0 += f->chunk) {
    a.g0 = g0;
    a.n = (int)std::min<long long>(f->chunk, end - g0);
    rc = sampled_launch(f, vk_grid_rows_kernel, a.n, kGridBlock, a);
    if (rc == VK_OK) rc = sampled_evaluate(f, a.n, f->d_lnl, f->d_chi);
    if (rc == VK_OK) rc = sampled_launch(f, vk_grid_max_kernel, (long long)((a.Rp + a.pr - 1) / a.pr) * kGridBlock, kGridBlock, a);
    if (rc == VK_OK) rc = sampled_launch(f, vk_grid_weight_kernel, (long long)a.n * a.Rp, kGridBlock, a);
    if (rc == VK_OK) rc = sampled_launch(f, vk_grid_accumulate_kernel, f->cells() * a.Rp, kGridBlock, a);
  }
  if (rc) return rc;
  VK_SAMPLED_HIP(f, hipStreamSynchronize(f->ctx->stream));
  return VK_OK;
}

extern "C" {

vk_grid* vk_grid_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_axes, const int32_t* columns, const int32_t* bins,
                        const double* nodes, const double* eps_pow, const double* base_row, double alpha, int32_t every_realisation,
                        int32_t n_pairs, const int32_t* pairs, int32_t chunk, char* err, size_t errlen) {
  auto bail = [&](const std::string& msg) -> vk_grid* {
    if (err && errlen) snprintf(err, errlen, "vk_grid_create: %s", msg.c_str());
    return nullptr;
  };
  if (!ctx || !opts || !columns || !bins || !nodes || !base_row || (n_pairs > 0 && !pairs)) return bail("NULL argument");
  if (n_axes < 1 || n_axes > vkgrid::kMaxP) return bail("need 1 <= axes <= 10");
  if (chunk < 1 || chunk > vkgrid::kMaxChunk) return bail("need 1 <= chunk <= 65536");
  if (n_pairs < 0 || n_pairs > vkgrid::kMaxPairs) return bail("need 0 <= pairs <= 45");
  long long G = 1, n1 = 0;
  int eps_axis = -1;
  for (int j = 0; j < n_axes; ++j) {
    if (bins[j] < 1 || bins[j] > vkgrid::kMaxBins) return bail("axis " + std::to_string(j) + " needs 1 <= bins <= 1024");
    G *= bins[j];                          // (at most 2^40 x 2^10 before the check: 64 bits hold it)
    if (G > vkgrid::kMaxPoints) return bail("the grid has more than 2^40 points");
    for (int k = 0; k < bins[j]; ++k)
      if (!__builtin_isfinite(nodes[n1 + k])) return bail("node " + std::to_string(k) + " of axis " + std::to_string(j) + " is not finite");
    n1 += bins[j];
    if (columns[j] == VK_WALK_EPSILON) eps_axis = j;
  }
  if (eps_axis >= 0 && !eps_pow) return bail("an epsilon axis needs eps_pow, the host's eps^(-2/3) of every node");
  long long n2 = 0;
  for (int q = 0; q < n_pairs; ++q) {
    const int ja = pairs[2 * q], jb = pairs[2 * q + 1];
    if (ja < 0 || jb >= n_axes || ja >= jb) return bail("pair " + std::to_string(q) + " needs two axes 0 <= a < b < axes");
    if (bins[ja] > vkgrid::kMaxBins2 || bins[jb] > vkgrid::kMaxBins2) return bail("an axis of a pair has at most 128 bins");
    n2 += (long long)bins[ja] * bins[jb];
  }
  int R = 1;
  if (every_realisation) {
    if (ctx->n_real <= 0 || !ctx->d_real) return bail("no realisations are set on the context (vk_set_realisations)");
    if (ctx->n_sets > 0)
      return bail("model realisations are set on the context (vk_set_model_realisations): a point has one theory vector per "
                  "realisation, and a grid evaluates every point once");
    if (check_real_lds(ctx) != VK_OK) return bail(ctx->err);
    R = vkh::n_problems(ctx);
  }
  if ((1 + n1 + n2) * (long long)(R + 1) > (1LL << 31) * (kGridBlock / 2))
    return bail("too many accumulators for one launch (cells x problems)");
  const double inf = __builtin_inf();
  double lo[vkgrid::kMaxP], hi[vkgrid::kMaxP];                 // (a grid has nodes, not a box)
  for (int j = 0; j < vkgrid::kMaxP; ++j) lo[j] = -inf, hi[j] = inf;
  vk_grid* f = sampled_create<vk_grid>("vk_grid_create", "grid", &ctx, 1, false, nullptr, opts, 1, n_axes, columns, nullptr, lo, hi,
                                       base_row, alpha, nullptr, err, errlen, [&](vk_grid* h) {
    h->g = vkgrid::make_shape(n_axes, bins);
    h->R = R;
    h->real = every_realisation != 0;
    h->blend.per_row = R;                  // (cross mode: every grid point against every realisation)
    h->max_which = h->real ? R - 1 : -1;
    h->chunk = chunk;
    h->n1 = (int)n1;
    h->n2 = (int)n2;
    h->n_pairs = n_pairs;
    h->n_eps = eps_axis >= 0 ? bins[eps_axis] : 0;
    int off = 0;
    for (int j = 0; j < n_axes; ++j) {
      h->axis_off[j] = off;
      off += bins[j];
    }
    off = 0;
    for (int q = 0; q < n_pairs; ++q) {
      h->pair[q][0] = pairs[2 * q];
      h->pair[q][1] = pairs[2 * q + 1];
      h->pair_off[q] = off;
      off += bins[pairs[2 * q]] * bins[pairs[2 * q + 1]];
    }
  });
  if (!f) return nullptr;
  bool ok = hipMemcpy(f->d_nodes, nodes, (size_t)n1 * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (ok && f->n_eps) ok = hipMemcpy(f->d_eps, eps_pow, (size_t)f->n_eps * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    sampled_destroy(f);
    return bail("upload failed");
  }
  return f;
}

const char* vk_grid_last_error(const vk_grid* f) { return f ? f->err.c_str() : ""; }

int vk_grid_set_prior(vk_grid* f, const double* mu, const double* pp_packed) {
  if (!f) return VK_E_ARG;
  const int rc = sampled_set_prior(f, "vk_grid_set_prior", mu, pp_packed);      // (vk_grid_run is synchronous: nothing is in flight)
  if (rc == VK_OK) f->done = 0;            // the accumulators hold another posterior: the next run starts at 0
  return rc;
}

void vk_grid_destroy(vk_grid* f) {
  if (f) sampled_destroy(f);
}

int vk_grid_run(vk_grid* f, int64_t first, int64_t count) {
  if (!f) return VK_E_ARG;
  int rc = grid_ready(f, "vk_grid_run");
  if (rc) return rc;
  const long long G = f->g.G;
  if (first < 0 || first >= G || count < 1) return refused(f, "vk_grid_run: need 0 <= first < points and count >= 1");
  if (first % f->chunk) return refused(f, "vk_grid_run: first must be a multiple of the chunk (" + std::to_string(f->chunk) + ")");
  if (first != 0 && first != f->done)
    return refused(f, "vk_grid_run: the chunks go in order: first must be 0 (a new run) or " + std::to_string(f->done) +
                          " (where the last call ended)");
  const long long end = count > G - first ? G : first + count;
  if (end != G && count % f->chunk) return refused(f, "vk_grid_run: count must be whole chunks, or reach the end of the grid");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  f->done = 0;
  rc = grid_chunks(f, first, end);
  if (rc != VK_OK) return sampled_abort(f, rc);
  f->done = end;
  f->err.clear();
  return VK_OK;
}

int vk_grid_rows(vk_grid* f, int64_t first, int32_t count, double* rows) {
  if (!f) return VK_E_ARG;
  if (!rows) return refused(f, "vk_grid_rows: NULL argument");
  int rc = grid_ready(f, "vk_grid_rows");
  if (rc) return rc;
  if (first < 0 || count < 1 || count > f->chunk || first > f->g.G - count)
    return refused(f, "vk_grid_rows: need 1 <= count <= chunk and 0 <= first <= points - count");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  GridArgs a = grid_args(f);
  a.g0 = first;
  a.n = count;
  rc = sampled_launch(f, vk_grid_rows_kernel, a.n, kGridBlock, a);
  if (rc == VK_OK) rc = sampled_home(f, {{rows, f->d_rows, (size_t)count * VK_NPAR * sizeof(double)}}, true);
  if (rc != VK_OK) return sampled_abort(f, rc);
  VK_SAMPLED_HIP(f, hipStreamSynchronize(f->ctx->stream));
  f->err.clear();
  return VK_OK;
}

int vk_grid_result(vk_grid* f, double* ln_max, int64_t* arg_max, double* total, int64_t* n_finite, double* m1, double* p1, double* m2,
                   double* p2, double* prior_ln_max, double* prior_total) {
  if (!f) return VK_E_ARG;
  if (f->done != f->g.G) return refused(f, "vk_grid_result: the run has reached " + std::to_string(f->done) + " of " + std::to_string(f->g.G) + " points");
  const size_t R = (size_t)f->R, Rp = (size_t)f->Rp();
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  std::vector<vkgrid::Running> run(Rp);
  std::vector<double> tot(Rp);
  const size_t one = R * sizeof(double);
  int rc = sampled_home(f, {{run.data(), f->d_run, Rp * sizeof(vkgrid::Running)}, {tot.data(), f->d_total, Rp * sizeof(double)},
                            {m1, f->d_m1, one * f->n1}, {p1, f->d_p1, one * f->n1}, {m2, f->d_m2, one * f->n2}, {p2, f->d_p2, one * f->n2}});
  if (rc) return rc;
  for (size_t r = 0; r < R; ++r) {
    if (ln_max) ln_max[r] = run[r].m;
    if (arg_max) arg_max[r] = run[r].arg;
    if (total) total[r] = tot[r];
    if (n_finite) n_finite[r] = run[r].n_finite;
  }
  if (prior_ln_max) *prior_ln_max = f->prior.on ? run[R].m : 0.0;
  if (prior_total) *prior_total = f->prior.on ? tot[R] : 0.0;
  f->err.clear();
  return VK_OK;
}

}  // extern "C"

// ---- importance-sampled posteriors: the evidence, effective sample size, moments and marginal histograms of every problem from --
// one shared sample (include/victor_hip.h, vk_kernel_importance.h; the definition: victor_amd/importance.py, the index rules, the
// list walk and the terms: vk_importance.h) --------------------------------------------------------------------------------------
// An importance handle is a Sampled with ONE base row whose pending rows are a chunk of the uploaded sample: per chunk a rows
// kernel, sampled_evaluate (the data-vector route with lnL, or enqueue_realisations in cross mode, [n][R]), then the max, weight
// and accumulate kernels, all on the context's stream with no host synchronisation between chunks; vk_is_run waits once at its
// end.  One allocation holds the sample, its lists and offsets, rows, workspace, the chunk's values and the accumulators.
// Of a joint fit (vk_is_create_joint): the same handle over the blocks' contexts - sampled_evaluate's joint routes, against the
// joint data vector or every joint realisation (cross mode) - with one base row and one set of pending rows, or
// (vk_is_create_joint_blocks) one of each per block.
struct __attribute__((visibility("hidden"))) vk_is : Sampled {
  int R = 1, chunk = 0, n_lists = 0, n_cells = 0, n_acc = 0, n1 = 0, n2 = 0;
  bool eps = false, own = false;           // epsilon is sampled; the prior's own problem rides along
  bool each = false;                       // a proposal per problem (vk_is_create_own): R samples of G points, pairs mode
  long long G = 0, n_chunks = 0;
  int cell_off[vkis::kMaxLists + 1] = {};
  long long done = 0;                      // points [0, done) are in the accumulators
  vkgrid::Running* d_run = nullptr;        // [R + 1]: the problems', the prior's own
  double *d_x = nullptr, *d_y = nullptr, *d_eps = nullptr, *d_lno = nullptr, *d_lnop = nullptr, *d_lnl = nullptr, *d_chi = nullptr;
  double *d_wp = nullptr, *d_acc = nullptr;
  int *d_list = nullptr, *d_off = nullptr;
  // the posterior-predictive state of vk_is_predict.h, beside the one allocation (vk_is_set_predictive; pred_N == 0: none):
  // pivot_t [N] | pt, ptt [N][R] | pivots [2][R] | dev [4][R] | the chunk's weights [chunk][R], which then leave d_chi alone
  DevBlock pred_mem;
  int pred_N = 0;                          // entries of a theory vector (of a joint handle: of the joint vector)
  double *p_pivot_t = nullptr, *p_pt = nullptr, *p_ptt = nullptr, *p_pivots = nullptr, *p_dev = nullptr, *p_w = nullptr;

  // the tail state of vk_is_tail.h, beside the one allocation (vk_is_set_tail; tail_K == 0: none): threshold [R] | the held
  // values, two buffers [R][K] | their points, two buffers [R][K] | the chunk's candidate rows [R][chunk] | the slices' candidate
  // counts [kMaxSlices][R] | count, side [R]
  DevBlock tail_mem;
  int tail_K = 0;                          // entries held per problem
  double *t_threshold = nullptr, *t_val[2] = {nullptr, nullptr};
  int *t_idx[2] = {nullptr, nullptr}, *t_cand = nullptr, *t_count = nullptr, *t_side = nullptr, *t_n_cand = nullptr;

  void tail_layout(Carve& c, size_t K) {
    const size_t r = (size_t)R;
    c.take(t_threshold, r);
    c.take(t_val[0], r * K);
    c.take(t_val[1], r * K);
    c.take(t_idx[0], r * K);
    c.take(t_idx[1], r * K);
    c.take(t_cand, r * (size_t)chunk);
    c.take(t_n_cand, r * (size_t)vkist::kMaxSlices);
    c.take(t_count, r);
    c.take(t_side, r);
  }

  void predictive_layout(Carve& c, size_t N) {
    const size_t r = (size_t)R;
    c.take(p_pivot_t, N);
    c.take(p_pt, N * r);
    c.take(p_ptt, N * r);
    c.take(p_pivots, 2 * r);
    c.take(p_dev, (size_t)vkisp::kDeviance * r);
    c.take(p_w, (size_t)chunk * r);
  }

  void shape(int, const double*, const double*) { rows_max = (size_t)chunk * (each ? (size_t)R : 1); }
  long long offsets_per_chunk() const { return (long long)n_cells + n_lists; }
  // a proposal per problem: every per-point array holds R values per point ([G][R]...), a chunk has chunk R rows, every problem
  // has a prior problem of its own (2 R running states and accumulator columns) and the rows carry their realisation
  void layout(Carve& c) {
    const size_t r = (size_t)R, m = each ? r : 1, n = (size_t)chunk * m, g = (size_t)G * m;
    blend_layout(c);
    if (each) return layout_each(c, r, n, g);
    c.take(d_run, r + 1);
    c.take(d_base, (size_t)sets * VK_NPAR);          // (a base row and a set of pending rows per block: vk_is_create_joint_blocks)
    c.take(d_rows, (size_t)sets * n * VK_NPAR);
    c.take(d_x, g * P);
    c.take(d_y, g * P);
    c.take(d_eps, eps ? g : 1);
    c.take(d_lno, g);
    c.take(d_lnop, own ? g : 1);
    c.take(d_lnl, n * r);
    c.take(d_chi, n * r);                  // the evaluation's chi-squares, then the chunk's weights (vk_is_weight_kernel)
    c.take(d_wp, n);
    c.take(d_th, workspace_doubles());
    c.take(d_acc, (size_t)n_acc * (r + 1));
    c.take(d_list, (size_t)n_lists * g);
    c.take(d_off, (size_t)(n_chunks * offsets_per_chunk()));
  }
  void layout_each(Carve& c, size_t r, size_t n, size_t g) {
    c.take(d_run, 2 * r);
    c.take(d_base, VK_NPAR);
    c.take(d_rows, n * VK_NPAR);
    c.take(d_x, g * P);
    c.take(d_y, g * P);
    c.take(d_eps, eps ? g : 1);
    c.take(d_lno, g);
    c.take(d_lnop, own ? g : 1);
    c.take(d_lnl, n);
    c.take(d_chi, n);                      // the evaluation's chi-squares, then the chunk's weights [chunk][R]
    c.take(d_wp, n);                       // ... of the prior problems
    c.take(d_th, workspace_doubles());
    c.take(d_acc, (size_t)n_acc * 2 * r);
    c.take(d_list, (size_t)n_lists * g);
    c.take(d_off, (size_t)(n_chunks * offsets_per_chunk()) * r);
    c.take(d_which, r);
    c.take(d_row_which, n);
  }
  int Rp() const { return own ? (each ? 2 * R : R + 1) : R; }
};

static IsArgs is_args(const vk_is* f) {
  IsArgs a{};
  a.d = f->P;
  a.R = f->R;
  a.Rp = f->Rp();
  a.own = f->each ? f->R : 0;
  a.G = f->G;
  a.x = f->d_x;
  a.eps_pow = f->eps ? f->d_eps : nullptr;
  a.base = f->d_base;
  a.rows = f->d_rows;
  a.blocks = f->row_sets(1);
  for (int j = 0; j < vkis::kMaxP; ++j) a.col[j] = f->col[j];
  a.alpha = f->alpha;
  a.y = f->d_y;
  a.lno = f->d_lno;
  a.lnop = f->own ? f->d_lnop : nullptr;
  a.lnl = f->d_lnl;
  a.w = f->pred_N ? f->p_w : f->d_chi;    // (with predictive sums the chi-squares survive to vk_is_predict_kernel)
  a.wp = f->d_wp;
  a.run = f->d_run;
  a.acc = f->d_acc;
  a.n_acc = f->n_acc;
  a.whole = vkis::whole(f->P);
  a.n_lists = f->n_lists;
  a.pr = 1;
  while (a.pr < 64 && a.pr < a.Rp) a.pr *= 2;
  a.list = f->d_list;
  for (int l = 0; l <= f->n_lists; ++l) a.cell_off[l] = f->cell_off[l];
  return a;
}

// may the handle run now: the context, and of the realisation route that the set on the context is the one it was made for - of
// a joint handle every block's context (sampled_ready has been through check_joint: the counts agree between the blocks, no
// block holds model realisations, the realisation kernels have their LDS)
static int is_ready(vk_is* f, const char* who) {
  int rc = sampled_ready(f, who, "sample", true);
  if (rc || !f->real) return rc;
  if (f->each) {                           // pairs mode: the indices were checked (max_which); model realisations count as the data's
    if (f->ctx->n_sets > 0 && f->ctx->n_sets != f->ctx->n_real)
      return refused(f, std::string(who) + ": the context holds " + std::to_string(f->ctx->n_sets) + " model realisations and " +
                            std::to_string(f->ctx->n_real) + " realisations of the data: the counts must agree");
    return VK_OK;
  }
  const size_t nb = f->blocks.empty() ? 1 : f->blocks.size();
  for (size_t q = 0; q < nb; ++q) {
    const vk_ctx* c = f->blocks.empty() ? f->ctx : f->blocks[q];
    const std::string ctx_q = f->blocks.empty() ? "the context" : "context " + std::to_string(q);
    if (vkh::n_problems(c) != f->R)
      return refused(f, std::string(who) + ": " + ctx_q + " holds " + std::to_string(vkh::n_problems(c)) + " realisations, the sample was made for " +
                            std::to_string(f->R));
    if (c->n_sets > 0)
      return refused(f, std::string(who) + ": model realisations are set on " + ctx_q + " (vk_set_model_realisations): a point has one "
                            "theory vector per realisation, and a shared sample evaluates every point once");
  }
  return VK_OK;
}

// The predictive sums of the chunk just accumulated (n rows from kept point g0): one launch of vk_is_predict_kernel - of a joint
// handle one per block segment, which the block's vectors were left in by the route that evaluated the chunk
// (vkh::joint_theory_segment).  On the lead stream, which every route has put behind the blocks' streams.
static int is_predict(vk_is* f, long long g0, int n) {
  IsPredictArgs q{};
  q.n = n;
  q.R = f->R;
  q.pr = vkisp::problems_per_wave(f->R);
  q.first = g0 == 0 ? 1 : 0;
  q.w = f->p_w;
  q.chi2 = f->d_chi;
  q.lnl = f->d_lnl;
  q.run = f->d_run;
  q.pivots = f->p_pivots;
  q.dev = f->p_dev;
  const int nb = (int)f->blocks.size();
  size_t off = 0;
  for (int b = 0; b < (nb ? nb : 1); ++b) {
    q.N = nb ? f->blocks[b]->N : f->ctx->N;
    q.th = nb ? vkh::joint_theory_segment(f->cov, f->blocks.data(), nb, b, n, f->real, f->cross, f->d_th) : f->d_th;
    q.deviance = b == 0 ? 1 : 0;
    q.pivot_t = f->p_pivot_t + off;
    q.pt = f->p_pt + off * (size_t)f->R;
    q.ptt = f->p_ptt + off * (size_t)f->R;
    const dim3 grid((unsigned)vkisp::problem_tiles(q.R, q.pr), (unsigned)(vkisp::entry_tiles(q.N, q.pr) + q.deviance));
    if (q.pr == vkisp::kWave) hipLaunchKernelGGL(vk_is_predict_kernel<true>, grid, dim3(vkisp::kBlock), 0, f->ctx->stream, q);
    else hipLaunchKernelGGL(vk_is_predict_kernel<false>, grid, dim3(vkisp::kBlock), 0, f->ctx->stream, q);
    VK_SAMPLED_HIP(f, hipGetLastError());
    off += (size_t)q.N;
  }
  return VK_OK;
}

// the tail's words for the chunk of `a` (vk_is_set_tail has sized what they point to for R, K and the handle's chunk)
static IsTailArgs is_tail_args(const vk_is* f, const IsArgs& a) {
  IsTailArgs q{};
  q.n = a.n;
  q.R = f->R;
  q.K = f->tail_K;
  q.cap = f->chunk;
  q.pr = vkist::problems_per_block(f->R);
  q.gy = vkist::row_blocks(a.n, q.pr);
  q.g0 = a.g0;
  q.lnl = f->d_lnl;
  q.lno = f->d_lno;
  q.own = a.own;
  q.threshold = f->t_threshold;
  q.count = f->t_count;
  q.side = f->t_side;
  q.n_cand = f->t_n_cand;
  q.cand = f->t_cand;
  for (int s = 0; s < 2; ++s) q.val[s] = f->t_val[s], q.idx[s] = f->t_idx[s];
  return q;
}

// The tail of the chunk just evaluated: the filter kernel over [n][R] - tiles of pr problems times gy blocks of rows -, then a
// merge workgroup per problem.
static int is_tail_chunk(vk_is* f, const IsArgs& a) {
  const IsTailArgs q = is_tail_args(f, a);
  const dim3 grid((unsigned)((q.R + q.pr - 1) / q.pr), (unsigned)q.gy);
  hipLaunchKernelGGL(vk_is_tail_filter_kernel, grid, dim3(vkist::kBlock), 0, f->ctx->stream, q);
  VK_SAMPLED_HIP(f, hipGetLastError());
  return sampled_launch(f, vk_is_tail_merge_kernel, (long long)q.R * vkist::kBlock, vkist::kBlock, q);
}

// a proposal per problem: the words of vk_kernel_is_own.h for the chunk of `a`
static IsOwnArgs is_own_args(const vk_is* f, const IsArgs& a) {
  IsOwnArgs q{};
  q.is = a;
  q.which = f->d_which;
  q.row_which = f->d_row_which;
  q.per_chunk = f->offsets_per_chunk();
  return q;
}

// ... and its chunk: the rows [n][R], their evaluation in pairs mode, then the shared sample's max, tail and weight kernels over
// the [n][R] values and the accumulate kernel that walks every problem's own lists
static int is_own_chunk(vk_is* f, const IsArgs& a) {
  const IsOwnArgs q = is_own_args(f, a);
  const long long rows = (long long)a.n * a.R;
  int rc = sampled_launch(f, vk_is_own_rows_kernel, rows, kIsBlock, q);
  if (rc == VK_OK) rc = sampled_evaluate(f, rows, f->d_lnl, f->d_chi);
  if (rc == VK_OK) rc = sampled_launch(f, vk_is_max_kernel, (long long)((a.Rp + a.pr - 1) / a.pr) * kIsBlock, kIsBlock, a);
  if (rc == VK_OK && f->tail_K) rc = is_tail_chunk(f, a);
  if (rc == VK_OK) rc = sampled_launch(f, vk_is_weight_kernel, (long long)a.n * a.Rp, kIsBlock, a);
  if (rc == VK_OK) rc = sampled_launch(f, vk_is_own_accumulate_kernel, (long long)a.n_acc * a.Rp, kIsBlock, q);
  return rc;
}

// the launches of points [first, end), chunk by chunk
static int is_chunks(vk_is* f, long long first, long long end) {
  IsArgs a = is_args(f);
  int rc = VK_OK;
  if (first == 0) rc = sampled_launch(f, vk_is_init_kernel, (long long)a.n_acc * a.Rp, kIsBlock, a);
  if (first == 0 && rc == VK_OK && f->tail_K) rc = sampled_launch(f, vk_is_tail_init_kernel, f->R, vkist::kBlock, is_tail_args(f, a));
  for (long long g0 = first; g0 < end && rc == VK_OK; g0 += f->chunk) {
    a.g0 = g0;
    a.n = (int)std::min<long long>(f->chunk, end - g0);
    a.off = f->d_off + (g0 / f->chunk) * f->offsets_per_chunk() * (f->each ? f->R : 1);   // (vkis::own_offsets(c, 0, R, per chunk))
    if (f->each) {
      rc = is_own_chunk(f, a);
      continue;
    }
    rc = sampled_launch(f, vk_is_rows_kernel, a.n, kIsBlock, a);
    if (rc == VK_OK) rc = sampled_evaluate(f, a.n, f->d_lnl, f->d_chi);
    if (rc == VK_OK) rc = sampled_launch(f, vk_is_max_kernel, (long long)((a.Rp + a.pr - 1) / a.pr) * kIsBlock, kIsBlock, a);
    if (rc == VK_OK && f->tail_K) rc = is_tail_chunk(f, a);
    if (rc == VK_OK) rc = sampled_launch(f, vk_is_weight_kernel, (long long)a.n * a.Rp, kIsBlock, a);
    if (rc == VK_OK) rc = sampled_launch(f, vk_is_accumulate_kernel, (long long)a.n_acc * a.Rp, kIsBlock, a);
    if (rc == VK_OK && f->pred_N) rc = is_predict(f, g0, a.n);
  }
  if (rc) return rc;
  VK_SAMPLED_HIP(f, hipStreamSynchronize(f->ctx->stream));
  return VK_OK;
}

// vk_is_create and its _joint forms (`who`): the one place where a sample's shape, bins, offsets, lists and values are checked,
// the handle is made (sampled_create) and the sample goes up.  joint: ctxs are the n_ctx blocks of a joint fit, lead first, under
// cov (NULL: block-diagonal); otherwise ctxs is the one context.  param_block (the _blocks form; NULL otherwise): the block each
// axis belongs to, or -1; base_rows then holds one row per block.  which (vk_is_create_own; NULL otherwise): n_problems
// realisation indices - every per-point array then holds a value per point and problem, the lists and offsets a set per problem
// (vk_importance.h), and the handle evaluates in pairs mode.
static vk_is* is_create(const char* who, vk_ctx* const* ctxs, int n_ctx, bool joint, vk_joint_cov* cov, const vk_eval_opts* opts,
                        int32_t n_axes, const int32_t* columns, const int32_t* param_block, int64_t n_points, const double* x,
                        const double* y, const double* eps_pow, const double* lno, const double* lno_prior, const int32_t* n_bins,
                        int32_t n_pairs, const int32_t* pair_bins, const int32_t* lists, const int32_t* offsets, const double* base_rows,
                        double alpha, int32_t every_realisation, int32_t chunk, char* err, size_t errlen, int32_t n_problems = 1,
                        const int32_t* which = nullptr) {
  auto bail = [&](const std::string& msg) -> vk_is* {
    if (err && errlen) snprintf(err, errlen, "%s: %s", who, msg.c_str());
    return nullptr;
  };
  if (!ctxs || (!joint && !ctxs[0]) || !opts || !columns || !x || !y || !lno || !n_bins || !lists || !offsets || !base_rows ||
      (n_pairs > 0 && !pair_bins))
    return bail("NULL argument");
  if (n_ctx < 1 || n_ctx > 32) return bail("need 1 <= contexts <= 32");
  for (int q = 0; q < n_ctx; ++q)
    if (!ctxs[q]) return bail("context " + std::to_string(q) + " is NULL");
  vk_ctx* ctx = ctxs[0];
  if (n_axes < 1 || n_axes > vkis::kMaxP) return bail("need 1 <= axes <= 10");
  if (n_points < 1 || n_points > vkis::kMaxPoints) return bail("need 1 <= points <= 2^24");
  if (chunk < 1 || chunk > vkis::kMaxChunk) return bail("need 1 <= chunk <= 65536");
  if (n_pairs < 0 || n_pairs > vkis::kMaxPairs) return bail("need 0 <= pairs <= 45");
  const bool each = which != nullptr;
  const long long RR = each ? n_problems : 1;                  // samples: one, or one per problem
  if (each) {
    if (n_problems < 1 || n_problems > vkis::kMaxChunk) return bail("need 1 <= problems <= 65536");
    if (n_points * RR > vkis::kMaxPoints) return bail("need points x problems <= 2^24");
    if ((long long)chunk * RR > vkis::kMaxChunk) return bail("need chunk x problems <= 65536 (the rows of one launch)");
    if (ctx->n_real <= 0 || !ctx->d_real) return bail("no realisations are set on the context (vk_set_realisations)");
    for (long long r = 0; r < RR; ++r)
      if (which[r] < 0 || which[r] >= vkh::n_problems(ctx))
        return bail("realisation index " + std::to_string(which[r]) + " of problem " + std::to_string(r) + " is outside 0.." +
                    std::to_string(vkh::n_problems(ctx) - 1));
    if (ctx->n_sets > 0 && ctx->n_sets != ctx->n_real)
      return bail(std::to_string(ctx->n_sets) + " model realisations (vk_set_model_realisations) against " + std::to_string(ctx->n_real) +
                  " realisations of the data (vk_set_realisations): the counts must agree");
    if (check_real_lds(ctx) != VK_OK) return bail(ctx->err);
  }
  const long long G = n_points, n_chunks = (G + chunk - 1) / chunk;
  const int n_lists = n_axes + n_pairs;
  int cell_off[vkis::kMaxLists + 1] = {};
  long long cells = 0, n1 = 0;
  bool eps = false;
  for (int j = 0; j < n_axes; ++j) {
    if (n_bins[j] < 1 || n_bins[j] > vkis::kMaxBins) return bail("axis " + std::to_string(j) + " needs 1 <= bins <= 1024");
    cell_off[j] = (int)cells;
    cells += n_bins[j] + 2;                // below, the bins, above
    if (columns[j] == VK_WALK_EPSILON) {
      eps = true;
      // (eps_pow holds one power per point: two blocks' epsilons of a point would read the same one)
      if (param_block && param_block[j] >= 0) return bail("epsilon cannot be sampled per block (eps_pow holds one eps^(-2/3) per point)");
    }
  }
  n1 = cells;
  for (int q = 0; q < n_pairs; ++q) {
    if (pair_bins[q] < 1 || pair_bins[q] > vkis::kMaxBins2) return bail("pair " + std::to_string(q) + " needs 1 <= bins <= 128 per axis");
    cell_off[n_axes + q] = (int)cells;
    cells += (long long)pair_bins[q] * pair_bins[q];
  }
  cell_off[n_lists] = (int)cells;
  if (eps && !eps_pow) return bail("a sampled epsilon needs eps_pow, the host's eps^(-2/3) of every point");
  const long long per_chunk = cells + n_lists;
  if (n_chunks * per_chunk * RR > vkis::kMaxOffsets) return bail("too many cell offsets (chunks x cells): at most 2^27, take a larger chunk or fewer cells");
  // (with a sample per problem flat index g R + r: point g of problem r)
  const std::string of_problem = each ? " (point x problems + problem)" : "";
  for (long long g = 0; g < G * RR; ++g) {
    for (int j = 0; j < n_axes; ++j)
      if (!__builtin_isfinite(x[g * n_axes + j]) || !__builtin_isfinite(y[g * n_axes + j]))
        return bail("point " + std::to_string(g) + of_problem + " is not finite in axis " + std::to_string(j));
    if (__builtin_isnan(lno[g]) || (lno_prior && __builtin_isnan(lno_prior[g])))
      return bail("lno of point " + std::to_string(g) + of_problem + " is NaN");
  }
  // every index a kernel forms: a list entry inside its chunk, a cell's end inside the chunk's count, offsets that never decrease
  for (long long c = 0; c < n_chunks; ++c) {
    const long long g0 = c * chunk;
    const int n = (int)std::min<long long>(chunk, G - g0);
    for (int r = 0; r < (int)RR; ++r)
      for (int l = 0; l < n_lists; ++l) {
        long long where = 0;
        const int* seg = each ? lists + vkis::own_list(r, l, n_lists, G) + g0 : lists + (size_t)l * G + g0;
        const int* off = offsets + (each ? vkis::own_offsets(c, r, (int)RR, per_chunk) : c * per_chunk) + cell_off[l] + l;
        const int bad = vkis::check_list(seg, off, cell_off[l + 1] - cell_off[l], n, &where);
        const std::string in = " in chunk " + std::to_string(c) + (each ? " of problem " + std::to_string(r) : "");
        if (bad == 1)
          return bail("offset " + std::to_string(where) + " of list " + std::to_string(l) + in +
                      " is wrong: the offsets start at 0, never decrease and end inside the chunk's " + std::to_string(n) + " points");
        if (bad == 2)
          return bail("entry " + std::to_string(where) + " of list " + std::to_string(l) + in +
                      " is outside its chunk of " + std::to_string(n) + " points, or not after the entry before it in its cell");
      }
  }
  int R = 1;
  if (each) {
    R = n_problems;
  } else if (every_realisation && joint) {
    // every block: realisations set, the same number of them as the lead's, no model realisations (no cross mode), the LDS the
    // realisation kernels need
    if (check_joint(cov, ctxs, n_ctx, true) != VK_OK) return bail(ctx->err);
    R = vkh::n_problems(ctx);
  } else if (every_realisation) {
    if (ctx->n_real <= 0 || !ctx->d_real) return bail("no realisations are set on the context (vk_set_realisations)");
    if (ctx->n_sets > 0)
      return bail("model realisations are set on the context (vk_set_model_realisations): a point has one theory vector per "
                  "realisation, and a shared sample evaluates every point once");
    if (check_real_lds(ctx) != VK_OK) return bail(ctx->err);
    R = vkh::n_problems(ctx);
  }
  const long long n_acc = vkis::whole(n_axes) + cells;
  if (n_acc * (long long)(each ? 2 * R : R + 1) > (1LL << 31) * (kIsBlock / 2)) return bail("too many accumulators for one launch (accumulators x problems)");
  const double inf = __builtin_inf();
  double lo[vkis::kMaxP], hi[vkis::kMaxP];                     // (a sample has points, not a box)
  for (int j = 0; j < vkis::kMaxP; ++j) lo[j] = -inf, hi[j] = inf;
  vk_is* f = sampled_create<vk_is>(who, "sample", ctxs, n_ctx, joint, cov, opts, 1, n_axes, columns, param_block, lo, hi, base_rows,
                                   alpha, nullptr, err, errlen, [&](vk_is* h) {
    h->R = R;
    h->each = each;
    h->real = each || every_realisation != 0;
    h->cross = h->real && !each ? R : 0;
    h->blend.per_row = each ? 1 : R;
    h->max_which = h->real ? R - 1 : -1;
    if (each) h->max_which = *std::max_element(which, which + R);
    h->chunk = chunk;
    h->G = G;
    h->n_chunks = n_chunks;
    h->n_lists = n_lists;
    h->n_cells = (int)cells;
    h->n1 = (int)n1;
    h->n2 = (int)(cells - n1);
    h->n_acc = (int)n_acc;
    h->eps = eps;
    h->own = lno_prior != nullptr;
    for (int l = 0; l <= n_lists; ++l) h->cell_off[l] = cell_off[l];
  });
  if (!f) return nullptr;
  auto up = [&](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
  const size_t g = (size_t)(G * RR);
  bool ok = up(f->d_x, x, g * n_axes * sizeof(double)) && up(f->d_y, y, g * n_axes * sizeof(double)) && up(f->d_lno, lno, g * sizeof(double));
  if (ok && eps) ok = up(f->d_eps, eps_pow, g * sizeof(double));
  if (ok && lno_prior) ok = up(f->d_lnop, lno_prior, g * sizeof(double));
  if (ok) ok = up(f->d_list, lists, (size_t)n_lists * g * sizeof(int)) && up(f->d_off, offsets, (size_t)(n_chunks * per_chunk * RR) * sizeof(int));
  if (ok && each) ok = up(f->d_which, which, (size_t)R * sizeof(int));
  if (!ok) {
    (void)hipGetLastError();
    sampled_destroy(f);
    return bail("upload failed");
  }
  return f;
}

extern "C" {

vk_is* vk_is_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_axes, const int32_t* columns, int64_t n_points, const double* x,
                    const double* y, const double* eps_pow, const double* lno, const double* lno_prior, const int32_t* n_bins,
                    int32_t n_pairs, const int32_t* pair_bins, const int32_t* lists, const int32_t* offsets, const double* base_row,
                    double alpha, int32_t every_realisation, int32_t chunk, char* err, size_t errlen) {
  return is_create("vk_is_create", &ctx, 1, false, nullptr, opts, n_axes, columns, nullptr, n_points, x, y, eps_pow, lno, lno_prior, n_bins,
                   n_pairs, pair_bins, lists, offsets, base_row, alpha, every_realisation, chunk, err, errlen);
}

vk_is* vk_is_create_own(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_axes, const int32_t* columns, int64_t n_points,
                        int32_t n_problems, const int32_t* which, const double* x, const double* y, const double* eps_pow,
                        const double* lno, const double* lno_prior, const int32_t* n_bins, int32_t n_pairs, const int32_t* pair_bins,
                        const int32_t* lists, const int32_t* offsets, const double* base_row, double alpha, int32_t chunk, char* err,
                        size_t errlen) {
  if (!which || !ctx) {
    if (err && errlen) snprintf(err, errlen, "vk_is_create_own: NULL argument");
    return nullptr;
  }
  return is_create("vk_is_create_own", &ctx, 1, false, nullptr, opts, n_axes, columns, nullptr, n_points, x, y, eps_pow, lno, lno_prior,
                   n_bins, n_pairs, pair_bins, lists, offsets, base_row, alpha, 1, chunk, err, errlen, n_problems, which);
}

vk_is* vk_is_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_axes,
                          const int32_t* columns, int64_t n_points, const double* x, const double* y, const double* eps_pow,
                          const double* lno, const double* lno_prior, const int32_t* n_bins, int32_t n_pairs, const int32_t* pair_bins,
                          const int32_t* lists, const int32_t* offsets, const double* base_row, double alpha, int32_t every_realisation,
                          int32_t chunk, char* err, size_t errlen) {
  return is_create("vk_is_create_joint", ctxs, n_ctx, true, cov, opts, n_axes, columns, nullptr, n_points, x, y, eps_pow, lno, lno_prior,
                   n_bins, n_pairs, pair_bins, lists, offsets, base_row, alpha, every_realisation, chunk, err, errlen);
}

vk_is* vk_is_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_axes,
                                 const int32_t* columns, const int32_t* param_block, int64_t n_points, const double* x, const double* y,
                                 const double* eps_pow, const double* lno, const double* lno_prior, const int32_t* n_bins,
                                 int32_t n_pairs, const int32_t* pair_bins, const int32_t* lists, const int32_t* offsets,
                                 const double* base_rows, double alpha, int32_t every_realisation, int32_t chunk, char* err,
                                 size_t errlen) {
  if (no_param_block("vk_is_create_joint_blocks", param_block, err, errlen)) return nullptr;
  return is_create("vk_is_create_joint_blocks", ctxs, n_ctx, true, cov, opts, n_axes, columns, param_block, n_points, x, y, eps_pow, lno,
                   lno_prior, n_bins, n_pairs, pair_bins, lists, offsets, base_rows, alpha, every_realisation, chunk, err, errlen);
}

const char* vk_is_last_error(const vk_is* f) { return f ? f->err.c_str() : ""; }

void vk_is_destroy(vk_is* f) {
  if (!f) return;
  f->pred_mem.drop(f);
  f->tail_mem.drop(f);
  sampled_destroy(f);
}

// The posterior-predictive sums (vk_is_predict.h).  Everything vk_is_predict_kernel indexes with is fixed here: R, the chunk and
// the entries of the theory vectors - of a joint handle the blocks' N, in block order - size the state it addresses.
int vk_is_set_predictive(vk_is* f, int32_t on) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_is_set_predictive: ";
  if (f->each) return refused(f, me + "a handle with a proposal per problem (vk_is_create_own) keeps no predictive sums");
  if (on && f->blend.on)
    return refused(f, me + "the handle blends the likelihood between two grid betas (VK_OPT_BETA_BLEND): a point has two theory "
                           "vectors, and the sums are of one");
  if (f->done != 0 && f->done != f->G) return refused(f, me + "a run is under way (call it before the first vk_is_run)");
  if (on && f->real && f->ctx->n_cuts > 0)
    return refused(f, me + "scale cuts are resident on the context (vk_set_cuts): the predictive sums and the DIC are of the full "
                           "data vector");
  f->pred_mem.drop(f);
  f->pred_N = 0;
  f->keep_theory = false;
  f->done = 0;                             // (the sums belong to a whole run: the next one starts at point 0)
  f->err.clear();
  if (!on) return VK_OK;
  long long N = 0;
  if (f->blocks.empty()) N = f->ctx->N;
  for (const vk_ctx* b : f->blocks) N += b->N;
  for (size_t b = 0; b < (f->blocks.empty() ? 1 : f->blocks.size()); ++b)
    if ((f->blocks.empty() ? f->ctx : f->blocks[b])->N > vkisp::kMaxEntries)
      return refused(f, me + "a theory vector of more than 2^17 entries");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const int rc = f->pred_mem.make(f, me, [&](Carve& c) { f->predictive_layout(c, (size_t)N); });
  if (rc) return rc;
  f->pred_N = (int)N;
  f->keep_theory = true;
  return VK_OK;
}

int vk_is_predictive(vk_is* f, double* pivot_t, double* sum_t, double* sum_tt, double* pivots, double* deviance) {
  if (!f) return VK_E_ARG;
  if (!f->pred_N) return refused(f, "vk_is_predictive: the handle has no predictive sums (vk_is_set_predictive)");
  if (f->done != f->G) return refused(f, "vk_is_predictive: the run has reached " + std::to_string(f->done) + " of " + std::to_string(f->G) + " points");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const size_t one = (size_t)f->R * sizeof(double), vec = (size_t)f->pred_N * sizeof(double);
  const int rc = sampled_home(f, {{pivot_t, f->p_pivot_t, vec}, {sum_t, f->p_pt, vec * f->R}, {sum_tt, f->p_ptt, vec * f->R},
                                  {pivots, f->p_pivots, 2 * one}, {deviance, f->p_dev, vkisp::kDeviance * one}});
  if (rc == VK_OK) f->err.clear();
  return rc;
}

// The tail (vk_is_tail.h).  Everything the tail kernels index with is fixed here and by the launch: R and the chunk - the
// candidate slots of a problem, which no chunk can exceed - and K size the state they address.
int vk_is_set_tail(vk_is* f, int32_t K) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_is_set_tail: ";
  if (f->done != 0 && f->done != f->G) return refused(f, me + "a run is under way (call it before the first vk_is_run)");
  if (K != 0 && (K < 2 || K > vkist::kMaxK || K > f->G))
    return refused(f, me + "need 2 <= K <= min(4096, points) entries per problem, or 0 for none (K = " + std::to_string(K) + ", " +
                          std::to_string(f->G) + " points)");
  f->tail_mem.drop(f);
  f->tail_K = 0;
  f->done = 0;                             // (the tail belongs to a whole run: the next one starts at point 0)
  f->err.clear();
  if (!K) return VK_OK;
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const int rc = f->tail_mem.make(f, me, [&](Carve& c) { f->tail_layout(c, (size_t)K); });
  if (rc) return rc;
  f->tail_K = K;
  return VK_OK;
}

int vk_is_tail(vk_is* f, double* lnpost, int64_t* index, int64_t* count) {
  if (!f) return VK_E_ARG;
  if (!f->tail_K) return refused(f, "vk_is_tail: the handle keeps no tail (vk_is_set_tail)");
  if (f->done != f->G) return refused(f, "vk_is_tail: the run has reached " + std::to_string(f->done) + " of " + std::to_string(f->G) + " points");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const size_t R = (size_t)f->R, K = (size_t)f->tail_K;
  std::vector<double> val[2];
  std::vector<int> idx[2], held(R), side(R);
  for (int s = 0; s < 2; ++s) val[s].resize(R * K), idx[s].resize(R * K);
  const int rc = sampled_home(f, {{val[0].data(), f->t_val[0], R * K * sizeof(double)}, {val[1].data(), f->t_val[1], R * K * sizeof(double)},
                                  {idx[0].data(), f->t_idx[0], R * K * sizeof(int)}, {idx[1].data(), f->t_idx[1], R * K * sizeof(int)},
                                  {held.data(), f->t_count, R * sizeof(int)}, {side.data(), f->t_side, R * sizeof(int)}});
  if (rc) return rc;
  for (size_t r = 0; r < R; ++r) {
    const size_t n = (size_t)std::min<long long>(std::max(held[r], 0), (long long)K);
    const int s = side[r] & 1;
    if (count) count[r] = (int64_t)n;
    for (size_t k = 0; k < K; ++k) {
      if (lnpost) lnpost[r * K + k] = k < n ? val[s][r * K + k] : -__builtin_inf();
      if (index) index[r * K + k] = k < n ? (int64_t)idx[s][r * K + k] : -1;
    }
  }
  f->err.clear();
  return VK_OK;
}

int vk_is_run(vk_is* f, int64_t first, int64_t count) {
  if (!f) return VK_E_ARG;
  int rc = is_ready(f, "vk_is_run");
  if (rc) return rc;
  const long long G = f->G;
  if (first < 0 || first >= G || count < 1) return refused(f, "vk_is_run: need 0 <= first < points and count >= 1");
  if (first % f->chunk) return refused(f, "vk_is_run: first must be a multiple of the chunk (" + std::to_string(f->chunk) + ")");
  if (first != 0 && first != f->done)
    return refused(f, "vk_is_run: the chunks go in order: first must be 0 (a new run) or " + std::to_string(f->done) +
                          " (where the last call ended)");
  const long long end = count > G - first ? G : first + count;
  if (end != G && count % f->chunk) return refused(f, "vk_is_run: count must be whole chunks, or reach the end of the sample");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  f->done = 0;
  rc = is_chunks(f, first, end);
  if (rc != VK_OK) return sampled_abort(f, rc);
  f->done = end;
  f->err.clear();
  return VK_OK;
}

int vk_is_rows(vk_is* f, int64_t first, int32_t count, double* rows) {
  if (!f) return VK_E_ARG;
  if (!rows) return refused(f, "vk_is_rows: NULL argument");
  int rc = is_ready(f, "vk_is_rows");
  if (rc) return rc;
  if (first < 0 || count < 1 || count > f->chunk || first > f->G - count)
    return refused(f, "vk_is_rows: need 1 <= count <= chunk and 0 <= first <= points - count");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  IsArgs a = is_args(f);
  a.g0 = first;
  a.n = count;
  if (f->each) {                           // count x R rows, row i R + r: point first + i of problem r
    rc = sampled_launch(f, vk_is_own_rows_kernel, (long long)a.n * a.R, kIsBlock, is_own_args(f, a));
    if (rc == VK_OK) rc = sampled_home(f, {{rows, f->d_rows, (size_t)count * f->R * VK_NPAR * sizeof(double)}}, true);
    if (rc != VK_OK) return sampled_abort(f, rc);
    VK_SAMPLED_HIP(f, hipStreamSynchronize(f->ctx->stream));
    f->err.clear();
    return VK_OK;
  }
  rc = sampled_launch(f, vk_is_rows_kernel, a.n, kIsBlock, a);
  // rows [sets][count][VK_NPAR]: one set, or (vk_is_create_joint_blocks) block q's rows from its set at d_rows + q par_stride
  const size_t set_doubles = (size_t)count * VK_NPAR;
  for (int q = 0; q < f->sets && rc == VK_OK; ++q)
    rc = sampled_home(f, {{rows + q * set_doubles, f->d_rows + q * f->par_stride(), set_doubles * sizeof(double)}}, true);
  if (rc != VK_OK) return sampled_abort(f, rc);
  VK_SAMPLED_HIP(f, hipStreamSynchronize(f->ctx->stream));
  f->err.clear();
  return VK_OK;
}

int vk_is_result(vk_is* f, double* ln_max, int64_t* arg_max, int64_t* n_finite, double* total, double* sq, double* s1, double* s2,
                 double* h1, double* h2, double* prior_ln_max, double* prior_total) {
  if (!f) return VK_E_ARG;
  if (f->done != f->G) return refused(f, "vk_is_result: the run has reached " + std::to_string(f->done) + " of " + std::to_string(f->G) + " points");
  const size_t R = (size_t)f->R, Rp = (size_t)f->Rp(), A = (size_t)f->n_acc;
  const int d = f->P, T = d * (d + 1) / 2, W = vkis::whole(d);
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  std::vector<vkgrid::Running> run(Rp);
  std::vector<double> acc(A * Rp);
  int rc = sampled_home(f, {{run.data(), f->d_run, Rp * sizeof(vkgrid::Running)}, {acc.data(), f->d_acc, A * Rp * sizeof(double)}});
  if (rc) return rc;
  auto at = [&](size_t a, size_t r) { return acc[a * Rp + r]; };
  for (size_t r = 0; r < R; ++r) {
    if (ln_max) ln_max[r] = run[r].m;
    if (arg_max) arg_max[r] = run[r].arg;
    if (n_finite) n_finite[r] = run[r].n_finite;
    if (total) total[r] = at(vkis::kTotal, r);
    if (sq) sq[r] = at(vkis::kSq, r);
    if (s1)
      for (int j = 0; j < d; ++j) s1[r * d + j] = at(vkis::first(j), r);
    if (s2)
      for (int t = 0; t < T; ++t) s2[r * T + t] = at(vkis::kFirst + d + t, r);
    if (h1)
      for (int c = 0; c < f->n1; ++c) h1[r * f->n1 + c] = at(W + c, r);
    if (h2)
      for (int c = 0; c < f->n2; ++c) h2[r * f->n2 + c] = at(W + f->n1 + c, r);
  }
  // (a proposal per problem: R values each, problem r's prior problem is problem R + r)
  for (size_t r = 0; r < (f->each ? R : 1); ++r) {
    if (prior_ln_max) prior_ln_max[r] = f->own ? run[R + r].m : 0.0;
    if (prior_total) prior_total[r] = f->own ? at(vkis::kTotal, R + r) : 0.0;
  }
  f->err.clear();
  return VK_OK;
}

}  // extern "C"

// ---- nested sampling: R problems of L live points, K replaced per iteration by S constrained steps (include/victor_hip.h, --------
// vk_kernel_nested.h; the definition: victor_amd/nested.py, the rules: vk_nested_step.h) ----------------------------------------
// A nested handle is a Sampled of R K rows: row r K + k is walker k of problem r in every launch it makes.  An iteration enqueues
// the select kernel, S times (sampled_evaluate, the step kernel) and the commit kernel on the context's stream; a block of up
// to 8 iterations runs without host synchronisation between vk_nested_begin, which uploads the block's random numbers, and
// vk_nested_finish, which waits and brings the block's dead record and the live lnL home.
struct __attribute__((visibility("hidden"))) vk_nested : Sampled {
  int R = 0, L = 0, K = 0, S = 0, RK = 0;
  double scale = 0.0;
  vkchain::Box box{};
  bool started = false;
  int in_flight = 0;                       // iterations of the block begun and not finished
  long long done = 0;                      // iterations finished since vk_nested_start
  int last_n = 0;                          // iterations of the block finished last (vk_nprior_record)
  double *d_lx = nullptr, *d_llnl = nullptr, *d_lchi = nullptr, *d_wx = nullptr, *d_wlnl = nullptr, *d_wchi = nullptr;
  double *d_lstar = nullptr, *d_range = nullptr, *d_x0 = nullptr, *d_res_lnl = nullptr, *d_res_chi = nullptr;
  double *d_pick = nullptr, *d_dz = nullptr, *d_dlnl = nullptr, *d_dchi = nullptr, *d_dx = nullptr;
  double *d_llp = nullptr, *d_wlp = nullptr, *d_dlp = nullptr;     // ln prior of the live points, the walkers, a block's dead record
  long long *d_acc = nullptr, *d_steps = nullptr, *d_stuck = nullptr;
  int *d_wslot = nullptr, *d_wmoved = nullptr;

  void shape(int n, const double* lo, const double* hi) {
    RK = n;
    R = n / K;
    rows_max = (size_t)n;
    box.d = P;
    for (int j = 0; j < P; ++j) {
      box.lo[j] = lo[j];
      box.hi[j] = hi[j];
    }
  }
  // live points | walkers | L*, ranges | base, start, rows, results, theory workspace | one block of random numbers | one block of
  // dead record | ln prior of live points, walkers and the block's dead record (vk_nprior_set may come any time before a start)
  // | counters | indices
  void layout(Carve& c) {
    const size_t n = RK, live = (size_t)R * L, block = (size_t)vknest::kBlock * n;
    blend_layout(c);
    c.take(d_lx, live * P);
    c.take(d_llnl, live);
    c.take(d_lchi, live);
    c.take(d_wx, n * P);
    c.take(d_wlnl, n);
    c.take(d_wchi, n);
    c.take(d_lstar, (size_t)R);
    c.take(d_range, (size_t)R * P);
    c.take(d_base, sets * n * VK_NPAR);
    c.take(d_x0, live * P);
    c.take(d_rows, sets * n * VK_NPAR);
    c.take(d_res_lnl, n);
    c.take(d_res_chi, n);
    c.take(d_th, workspace_doubles());
    c.take(d_pick, block);
    c.take(d_dz, block * S * P);
    c.take(d_dlnl, block);
    c.take(d_dchi, block);
    c.take(d_dx, block * P);
    c.take(d_llp, live);
    c.take(d_wlp, n);
    c.take(d_dlp, block);
    c.take(d_acc, n);
    c.take(d_steps, n);
    c.take(d_stuck, n);
    c.take(d_which, n);
    c.take(d_row_which, n);
    c.take(d_wslot, n);
    c.take(d_wmoved, n);
  }
};

static NestedArgs nested_args(const vk_nested* f) {
  NestedArgs a{};
  a.box = f->box;
  a.R = f->R;
  a.L = f->L;
  a.K = f->K;
  a.scale = f->scale;
  a.lx = f->d_lx;
  a.llnl = f->d_llnl;
  a.lchi = f->d_lchi;
  a.wx = f->d_wx;
  a.wlnl = f->d_wlnl;
  a.wchi = f->d_wchi;
  a.wslot = f->d_wslot;
  a.wmoved = f->d_wmoved;
  a.n_accept = f->d_acc;
  a.n_steps = f->d_steps;
  a.n_stuck = f->d_stuck;
  a.lstar = f->d_lstar;
  a.range = f->d_range;
  a.base = f->d_base;
  a.which = f->real ? f->d_which : nullptr;
  a.rows = f->d_rows;
  a.row_which = f->real ? f->d_row_which : nullptr;
  a.res_lnl = f->d_res_lnl;
  a.res_chi2 = f->d_res_chi;
  a.x0 = f->d_x0;
  for (int j = 0; j < vknest::kMaxP; ++j) a.col[j] = f->col[j];
  a.alpha = f->alpha;
  a.blocks = f->row_sets((size_t)f->RK);
  return a;
}

static NestedPriorArgs nested_prior_args(const vk_nested* f) {
  NestedPriorArgs a{};
  static_cast<NestedArgs&>(a) = nested_args(f);
  a.prior = f->prior;
  a.llp = f->d_llp;
  a.wlp = f->d_wlp;
  return a;
}

// the L / K passes of vk_nested_start, enqueued (Args: NestedArgs, or NestedPriorArgs of a handle under a prior)
template <class Args>
static int nested_enqueue_start(vk_nested* f, Args a) {
  int rc = VK_OK;
  for (int p = 0; p < f->L / f->K && rc == VK_OK; ++p) {
    a.pass = p;
    rc = sampled_launch(f, vk_nested_load_kernel, f->RK, kNestedBlock, a);
    if (rc == VK_OK) rc = sampled_evaluate(f, f->RK, f->d_res_lnl, f->d_res_chi);
    if (rc == VK_OK) rc = sampled_launch(f, vk_nested_adopt_kernel, f->RK, kNestedBlock, a);
  }
  return rc;
}

// the n_iter iterations of vk_nested_begin, enqueued; dead_lp(a, t): where iteration t's ln prior record goes (a prior's Args)
template <class Args, class DeadLp>
static int nested_enqueue_block(vk_nested* f, Args a, int n_iter, int keep_dead, DeadLp dead_lp) {
  const size_t n = f->RK, P = f->P, S = f->S;
  int rc = VK_OK;
  for (int t = 0; t < n_iter && rc == VK_OK; ++t) {
    const double* dz_t = f->d_dz + (size_t)t * S * n * P;
    a.pick = f->d_pick + (size_t)t * n;
    a.dz = dz_t;
    a.dz_next = nullptr;
    a.dead_lnl = f->d_dlnl + (size_t)t * n;
    a.dead_chi2 = f->d_dchi + (size_t)t * n;
    a.dead_x = keep_dead ? f->d_dx + (size_t)t * n * P : nullptr;
    dead_lp(a, t);
    rc = sampled_launch(f, vk_nested_select_kernel, (long long)f->R * kNestedSelect, kNestedSelect, a);
    for (size_t s = 0; s < S && rc == VK_OK; ++s) {
      rc = sampled_evaluate(f, f->RK, f->d_res_lnl, f->d_res_chi);
      if (rc) break;
      a.dz = dz_t + s * n * P;
      a.dz_next = s + 1 < S ? a.dz + n * P : nullptr;
      rc = sampled_launch(f, vk_nested_step_kernel, f->RK, kNestedBlock, a);
    }
    if (rc == VK_OK) rc = sampled_launch(f, vk_nested_commit_kernel, f->RK, kNestedBlock, a);
  }
  return rc;
}

// vk_nested_create and its joint forms: the shape is checked before the shared create call, which lays the handle out from it
template <class Make>
static vk_nested* nested_create(const char* who, int32_t n_rows, int32_t n_live, int32_t batch, int32_t steps, double scale, char* err,
                                size_t errlen, Make make) {
  auto bail = [&](const std::string& msg) -> vk_nested* {
    if (err && errlen) snprintf(err, errlen, "%s: %s", who, msg.c_str());
    return nullptr;
  };
  if (n_live < 2 || n_live > vknest::kMaxLive) return bail("need 2 <= live points <= 4096");
  if (batch < 1 || n_live % batch || batch > n_live / 2)
    return bail("the batch must divide the live points and be at most half of them");
  if (steps < 1 || steps > 1024) return bail("need 1 <= steps <= 1024");
  if (!(scale > 0) || !__builtin_isfinite(scale)) return bail("need a finite scale > 0");
  if (n_rows < 1 || n_rows > kSampledMax) return bail("need 1 <= rows <= 65536");
  if (n_rows % batch) return bail(std::to_string(n_rows) + " rows are not a whole number of problems of " + std::to_string(batch));
  return make([=](vk_nested* h) {
    h->L = n_live;
    h->K = batch;
    h->S = steps;
    h->scale = scale;
  });
}

extern "C" {

vk_nested* vk_nested_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_rows, int32_t n_live, int32_t batch, int32_t steps,
                            double scale, int32_t n_params, const int32_t* columns, const double* lo, const double* hi,
                            const double* base_rows, double alpha, const int32_t* which, char* err, size_t errlen) {
  return nested_create("vk_nested_create", n_rows, n_live, batch, steps, scale, err, errlen, [&](auto prepare) {
    return sampled_create<vk_nested>("vk_nested_create", "row", &ctx, 1, false, nullptr, opts, n_rows, n_params, columns, nullptr, lo,
                                     hi, base_rows, alpha, which, err, errlen, prepare);
  });
}

vk_nested* vk_nested_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_rows,
                                  int32_t n_live, int32_t batch, int32_t steps, double scale, int32_t n_params,
                                  const int32_t* columns, const double* lo, const double* hi, const double* base_rows, double alpha,
                                  const int32_t* which, char* err, size_t errlen) {
  return nested_create("vk_nested_create_joint", n_rows, n_live, batch, steps, scale, err, errlen, [&](auto prepare) {
    return sampled_create<vk_nested>("vk_nested_create_joint", "row", ctxs, n_ctx, true, cov, opts, n_rows, n_params, columns, nullptr,
                                     lo, hi, base_rows, alpha, which, err, errlen, prepare);
  });
}

vk_nested* vk_nested_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                         int32_t n_rows, int32_t n_live, int32_t batch, int32_t steps, double scale,
                                         int32_t n_params, const int32_t* columns, const int32_t* param_block, const double* lo,
                                         const double* hi, const double* base_rows, double alpha, const int32_t* which, char* err,
                                         size_t errlen) {
  if (no_param_block("vk_nested_create_joint_blocks", param_block, err, errlen)) return nullptr;
  return nested_create("vk_nested_create_joint_blocks", n_rows, n_live, batch, steps, scale, err, errlen, [&](auto prepare) {
    return sampled_create<vk_nested>("vk_nested_create_joint_blocks", "row", ctxs, n_ctx, true, cov, opts, n_rows, n_params, columns,
                                     param_block, lo, hi, base_rows, alpha, which, err, errlen, prepare);
  });
}

const char* vk_nested_last_error(const vk_nested* f) { return f ? f->err.c_str() : ""; }

void vk_nested_destroy(vk_nested* f) {
  if (!f) return;
  if (f->in_flight) (void)hipStreamSynchronize(f->ctx->stream);
  sampled_destroy(f);
}

// x0 [R][L][d]: the live points, inside the box.  L / K launches of R K rows each evaluate them: row r K + k of pass p is live
// point p K + k of problem r.
int vk_nested_start(vk_nested* f, const double* x0) {
  if (!f) return VK_E_ARG;
  if (!x0) return refused(f, "vk_nested_start: NULL argument");
  if (f->in_flight) return refused(f, "vk_nested_start: a block begun with vk_nested_begin is awaiting vk_nested_finish");
  int rc = sampled_ready(f, "vk_nested_start", "row", true);
  if (rc) return rc;
  const size_t live = (size_t)f->R * f->L;
  for (size_t i = 0; i < live; ++i)
    if (!vkchain::in_box(f->box, x0 + i * f->P))
      return refused(f, "vk_nested_start: live point " + std::to_string(i % f->L) + " of problem " + std::to_string(i / f->L) +
                            " is outside the box");
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_x0, x0, live * f->P * sizeof(double), hipMemcpyHostToDevice));
  f->started = false;
  rc = f->prior.on ? nested_enqueue_start(f, nested_prior_args(f)) : nested_enqueue_start(f, nested_args(f));
  if (rc) return sampled_abort(f, rc);
  VK_SAMPLED_HIP(f, hipStreamSynchronize(f->ctx->stream));
  f->started = true;
  f->done = 0;
  f->last_n = 0;
  f->err.clear();
  return VK_OK;
}

// pick [n_iter][R K], dz [n_iter][S][R K][d]: the block's random numbers; first_iter: the life-long index of its first iteration
int vk_nested_begin(vk_nested* f, int32_t n_iter, const double* pick, const double* dz, int64_t first_iter, int32_t keep_dead) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_nested_begin: ";
  if (!pick || !dz) return refused(f, me + "NULL argument");
  if (!f->started) return refused(f, me + "the live points have no start (vk_nested_start)");
  if (f->in_flight) return refused(f, me + "the previous block has not been finished (vk_nested_finish)");
  if (n_iter < 1 || n_iter > vknest::kBlock) return refused(f, me + "need 1 <= iterations <= 8 in a block");
  if (first_iter != f->done)
    return refused(f, me + "the iterations go in order: first_iter must be " + std::to_string(f->done) + " (where the last block ended)");
  int rc = sampled_ready(f, "vk_nested_begin", "row", true);
  if (rc) return rc;
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const size_t n = f->RK, P = f->P, S = f->S;
  // the stream is idle (the block before was finished): plain copies, complete on return
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_pick, pick, (size_t)n_iter * n * sizeof(double), hipMemcpyHostToDevice));
  VK_SAMPLED_HIP(f, hipMemcpy(f->d_dz, dz, (size_t)n_iter * S * n * P * sizeof(double), hipMemcpyHostToDevice));
  rc = f->prior.on ? nested_enqueue_block(f, nested_prior_args(f), n_iter, keep_dead,
                                          [&](NestedPriorArgs& a, int t) { a.dead_lp = f->d_dlp + (size_t)t * n; })
                   : nested_enqueue_block(f, nested_args(f), n_iter, keep_dead, [](NestedArgs&, int) {});
  if (rc) return sampled_abort(f, rc);
  f->in_flight = n_iter;
  f->err.clear();
  return VK_OK;
}

// dead_lnl, dead_chi2 [n_iter][R][K] and dead_x [n_iter][R][K][d] (NULL: not wanted) of the block, live_lnl [R][L] behind it
int vk_nested_finish(vk_nested* f, double* dead_lnl, double* dead_chi2, double* dead_x, double* live_lnl) {
  if (!f) return VK_E_ARG;
  if (!f->in_flight) return refused(f, "vk_nested_finish: nothing was begun");
  const size_t n = (size_t)f->in_flight * f->RK, one = sizeof(double);
  int rc = hipSetDevice(f->ctx->device) == hipSuccess ? VK_OK : VK_E_HIP;
  if (rc == VK_OK)
    rc = sampled_home(f, {{dead_lnl, f->d_dlnl, n * one}, {dead_chi2, f->d_dchi, n * one}, {dead_x, f->d_dx, n * f->P * one},
                          {live_lnl, f->d_llnl, (size_t)f->R * f->L * one}}, true);
  hipError_t e = hipStreamSynchronize(f->ctx->stream);
  f->done += f->in_flight;
  f->last_n = f->in_flight;
  f->in_flight = 0;
  if (rc != VK_OK || e != hipSuccess) {
    (void)hipGetLastError();
    if (rc == VK_OK) f->err = std::string("vk_nested_finish: ") + hipGetErrorString(e);
    return VK_E_HIP;
  }
  f->err.clear();
  return VK_OK;
}

// x [R][L][d], lnl, chi2 [R][L]: the live points; n_accept, n_steps, n_stuck [R]: per problem, summed over its walkers
int vk_nested_state(vk_nested* f, double* x, double* lnl, double* chi2, int64_t* n_accept, int64_t* n_steps, int64_t* n_stuck) {
  if (!f) return VK_E_ARG;
  if (!f->started || f->in_flight)
    return refused(f, f->started ? "vk_nested_state: a block begun with vk_nested_begin is awaiting vk_nested_finish"
                                 : "vk_nested_state: the live points have no start (vk_nested_start)");
  const size_t live = (size_t)f->R * f->L, P = f->P, n = f->RK;
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  std::vector<double> h(x ? live * P : 0);
  std::vector<long long> cnt(3 * n);                       // n_accept | n_steps | n_stuck are contiguous
  int rc = sampled_home(f, {{h.data(), f->d_lx, h.size() * sizeof(double)}, {lnl, f->d_llnl, live * sizeof(double)},
                            {chi2, f->d_lchi, live * sizeof(double)}, {cnt.data(), f->d_acc, cnt.size() * sizeof(long long)}});
  if (rc) return rc;
  if (x)
    for (size_t i = 0; i < live; ++i)
      for (size_t j = 0; j < P; ++j) x[i * P + j] = h[j * live + i];
  int64_t* out[3] = {n_accept, n_steps, n_stuck};
  for (int q = 0; q < 3; ++q) {
    if (!out[q]) continue;
    for (int r = 0; r < f->R; ++r) {
      long long sum = 0;
      for (int k = 0; k < f->K; ++k) sum += cnt[(size_t)q * n + (size_t)r * f->K + k];
      out[q][r] = sum;
    }
  }
  f->err.clear();
  return VK_OK;
}

// A Gaussian prior (vk_prior.h) on a nested handle of any of the three create calls: mu [d], pp [d (d + 1) / 2] as
// vk_chain_set_prior takes them; NULL, NULL clears it.  The live points of a start carry the ln prior of the prior they were
// started under, so a change of prior ends the start: the next call is vk_nested_start.
int vk_nprior_set(vk_nested* f, const double* mu, const double* pp) {
  if (!f) return VK_E_ARG;
  if (f->in_flight) return refused(f, "vk_nprior_set: a block begun with vk_nested_begin is awaiting vk_nested_finish");
  const int rc = sampled_set_prior(f, "vk_nprior_set", mu, pp);
  if (rc == VK_OK) {
    f->started = false;
    f->last_n = 0;
  }
  return rc;
}

// dead_lnprior [n_iter][R][K] of the block finished last (n_iter: its length) and live_lnprior [R][L] behind it; either may be NULL
int vk_nprior_record(vk_nested* f, int32_t n_iter, double* dead_lnprior, double* live_lnprior) {
  if (!f) return VK_E_ARG;
  const std::string me = "vk_nprior_record: ";
  if (!f->prior.on) return refused(f, me + "the handle has no prior (vk_nprior_set)");
  if (f->in_flight) return refused(f, me + "a block begun with vk_nested_begin is awaiting vk_nested_finish");
  if (!f->started) return refused(f, me + "the live points have no start (vk_nested_start)");
  if (dead_lnprior && n_iter != f->last_n)
    return refused(f, me + "the block finished last had " + std::to_string(f->last_n) + " iterations, not " + std::to_string(n_iter));
  VK_SAMPLED_HIP(f, hipSetDevice(f->ctx->device));
  const int rc = sampled_home(f, {{dead_lnprior, f->d_dlp, (size_t)f->last_n * f->RK * sizeof(double)},
                                  {live_lnprior, f->d_llp, (size_t)f->R * f->L * sizeof(double)}});
  if (rc) return rc;
  f->err.clear();
  return VK_OK;
}

}  // extern "C"

// ---- the kernels of vk_kernel_blend.h alone, on host buffers (include/victor_hip.h: vk_blend_split / vk_blend_merge) ----------
// One allocation per call, the kernels on the device's null stream, the results copied home: what sampled_evaluate_blend
// launches around its evaluation, with nothing between them.
namespace {
struct BlendMem {
  double *grid = nullptr, *rows = nullptr, *rows2 = nullptr, *t = nullptr, *raw_lnl = nullptr, *raw_chi = nullptr, *lnl = nullptr,
         *chi = nullptr;
  int *which = nullptr, *which2 = nullptr, *fail = nullptr;
};

template <class Layout, class Body>
int blend_call(int device, Layout&& layout, Body&& body) {
  void* mem = nullptr;
  size_t bytes = 0;
  if (!carve_alloc(device, mem, bytes, layout)) return VK_E_HIP;
  const bool ok = body();
  const bool clean = hipDeviceSynchronize() == hipSuccess;
  (void)hipGetLastError();
  (void)hipFree(mem);
  return ok && clean ? VK_OK : VK_E_HIP;
}
}  // namespace

extern "C" {

int vk_blend_split(int device, const double* grid, int32_t n_grid, const double* rows, const int32_t* which, int64_t m, double* rows2,
                   int32_t* which2, double* t, int32_t* fail) {
  if (!grid || !rows || !rows2 || !t || !fail || (which && !which2) || m < 1 || m > (1LL << 30) || n_grid < 2) return VK_E_ARG;
  const size_t n = (size_t)m;
  BlendMem b;
  return blend_call(device, [&](Carve& c) {
    c.take(b.grid, (size_t)n_grid);
    c.take(b.rows, n * VK_NPAR);
    c.take(b.rows2, 2 * n * VK_NPAR);
    c.take(b.t, n);
    c.take(b.which, n);
    c.take(b.which2, 2 * n);
    c.take(b.fail, n);
  }, [&]() {
    auto up = [](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
    auto home = [](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    if (!up(b.grid, grid, (size_t)n_grid * sizeof(double)) || !up(b.rows, rows, n * VK_NPAR * sizeof(double))) return false;
    if (which && !up(b.which, which, n * sizeof(int))) return false;
    BlendArgs q{};
    q.grid = b.grid;
    q.n_grid = n_grid;
    q.m = m;
    q.per_row = 1;
    q.rows = b.rows;
    q.row_which = which ? b.which : nullptr;
    q.rows2 = b.rows2;
    q.which2 = b.which2;
    q.t = b.t;
    q.fail = b.fail;
    hipLaunchKernelGGL(vk_blend_split_kernel, dim3((unsigned)((m + kBlendBlock - 1) / kBlendBlock)), dim3(kBlendBlock), 0, nullptr, q);
    if (hipGetLastError() != hipSuccess) return false;
    return home(rows2, b.rows2, 2 * n * VK_NPAR * sizeof(double)) && home(t, b.t, n * sizeof(double)) &&
           home(fail, b.fail, n * sizeof(int)) && (!which || home(which2, b.which2, 2 * n * sizeof(int)));
  });
}

int vk_blend_merge(int device, const double* t, const int32_t* fail, int64_t m, int64_t per_row, const double* raw_lnl,
                   const double* raw_chi, double* lnl, double* chi) {
  if (!t || !fail || !raw_lnl || !raw_chi || !lnl || !chi || m < 1 || per_row < 1 || m > (1LL << 30) / per_row) return VK_E_ARG;
  const size_t n = (size_t)m, out = n * (size_t)per_row;
  BlendMem b;
  return blend_call(device, [&](Carve& c) {
    c.take(b.t, n);
    c.take(b.raw_lnl, 2 * out);
    c.take(b.raw_chi, 2 * out);
    c.take(b.lnl, out);
    c.take(b.chi, out);
    c.take(b.fail, n);
  }, [&]() {
    auto up = [](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
    auto home = [](void* dst, const void* src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    if (!up(b.t, t, n * sizeof(double)) || !up(b.fail, fail, n * sizeof(int)) || !up(b.raw_lnl, raw_lnl, 2 * out * sizeof(double)) ||
        !up(b.raw_chi, raw_chi, 2 * out * sizeof(double)))
      return false;
    BlendArgs q{};
    q.m = m;
    q.per_row = per_row;
    q.t = b.t;
    q.fail = b.fail;
    q.raw_lnl = b.raw_lnl;
    q.raw_chi = b.raw_chi;
    q.lnl = b.lnl;
    q.chi = b.chi;
    hipLaunchKernelGGL(vk_blend_merge_kernel, dim3((unsigned)(((long long)out + kBlendBlock - 1) / kBlendBlock)), dim3(kBlendBlock), 0,
                       nullptr, q);
    if (hipGetLastError() != hipSuccess) return false;
    return home(lnl, b.lnl, out * sizeof(double)) && home(chi, b.chi, out * sizeof(double));
  });
}

}  // extern "C"
