/*
 * victor_hip.h - C ABI of libvictor_hip.so, the MI355X (gfx950) implementation of
 * victor's per-step likelihood hot path.
 *
 * The reference (seshnadathur/victor, pure Python) has no native boundary of its
 * own; the replaceable interface is its Python class API.  Each entry point below
 * names the reference method whose work it performs for a whole BATCH of parameter
 * points (paths relative to the reference root):
 *
 *   vk_eval_batch        CCFFit.log_likelihood        victor/ccf_fit.py:356-483
 *                        CCFFit.chi_squared           victor/ccf_fit.py:325-354
 *                        CCFModel.theory_multipole_vector  victor/ccf_model.py:829-860
 *   vk_theory_batch      CCFModel.theory_multipoles   victor/ccf_model.py:791-827
 *                        (+ utils.multipoles_from_fn  victor/utils.py:9-58)
 *   vk_xi_smu_batch      CCFModel.theory_xi           victor/ccf_model.py:538-789
 *   vk_eval_realisations CCFFit.log_likelihood against every simulation realisation of the
 *                        data file (simulation_number, victor/ccf_fit.py:59-61,93-100)
 *   vk_set_cuts          ... under many scale cuts (s ranges, multipole sets) at once, a use of the reference that
 *                        slices the data and covariance files by hand, once per cut
 *   vk_set_model_realisations  ... each with the model of its own real-space CCF
 *                        (realspace_ccf.simulation_number, victor/ccf_model.py:127-162)
 *   vk_joint_cov_eval_realisations  the same for a joint fit under one covariance: realisation m
 *                        of every block's own file (victor/ccf_fit.py:59-61,93-100,325-483)
 *   vk_fit_create_joint, vk_chain_create_joint   a host optimiser / cobaya (victor/likelihoods/
 *                        CCFLikelihood.py:32) around that joint likelihood, data vectors or every
 *                        joint realisation: the loops of vk_fit_run / vk_chain_begin over a joint fit
 *   vk_create            CCFModel.__init__ / CCFFit.__init__ table set-up
 *                        victor/ccf_model.py:33-97, victor/ccf_fit.py:15-42
 *                        (the host has already turned every spline into explicit
 *                        piecewise-cubic coefficient tables; vk_create uploads them)
 *
 * Conventions
 *   - plain C, no C++/torch types; all arrays are contiguous row-major doubles
 *   - the caller owns every host buffer; the context owns device memory and one
 *     HIP stream; a context is bound to one device and is not thread-safe
 *   - return value 0 = success, negative = VK_E_* code; vk_last_error() gives text
 *   - calls are synchronous unless the name ends in _async (then use vk_sync)
 *   - there is no CPU fallback anywhere in the library
 */
#ifndef VICTOR_HIP_H
#define VICTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_ABI_VERSION 22

/* error codes */
#define VK_OK 0
#define VK_E_ARG (-1)      /* bad argument / unsupported option combination */
#define VK_E_HIP (-2)      /* a HIP runtime call failed */
#define VK_E_NODEVICE (-3) /* no usable GPU */
#define VK_E_RCCL (-4)     /* an RCCL call failed */
#define VK_E_NOMEM (-5)    /* a host allocation failed */

/* one row of the parameter batch: VK_NPAR doubles (ccf_model.py:583-613,638,695-696) */
#define VK_NPAR 12
#define VK_P_FSIGMA8 0 /* params['fsigma8']                                   */
#define VK_P_SIGMAV 1  /* params.get('sigma_v', 380)                          */
#define VK_P_APERP 2   /* alpha_perp  (from aperp, or epsilon*apar)           */
#define VK_P_APAR 3    /* alpha_par   (from apar, or alpha*epsilon^(-2/3))    */
#define VK_P_EPSILON 4 /* epsilon     (given, or aperp/apar)                  */
#define VK_P_BETA 5    /* reconstruction beta (0.40 dummy when irrelevant)    */
#define VK_P_ASTAR 6   /* params.get('astar', 1)                              */
#define VK_P_M 7       /* Kaiser nuisance M (default 1)                       */
#define VK_P_Q 8       /* Kaiser nuisance Q (default 1)                       */
#define VK_P_BIAS 9    /* params.get('bias', model['bias']) - linear_bias matter model (ccf_model.py:359,430) */
#define VK_P_AV 10     /* params.get('Av', 0) - empirical velocity correction (ccf_model.py:453) */
#define VK_P_SPARE 11

/* vk_eval_opts.rsd_model (ccf_model.py:646-787) */
#define VK_RSD_STREAMING 0
#define VK_RSD_DISPERSION 1
#define VK_RSD_KAISER 2
#define VK_RSD_EUCLID 3

/* vk_tables.matter_model (ccf_model.py:71,358-372) */
#define VK_MATTER_TEMPLATE 0
#define VK_MATTER_LINEAR_BIAS 1
#define VK_MATTER_VELOCITY_TEMPLATE 2 /* velocity_pdf.mean.model == 'template' (ccf_model.py:439-443,483-490): the
                                         tables hold the template v_r(r) itself, amplitude = fsigma8 * vt_amp */

/* vk_eval_opts.like_form (ccf_fit.py:455-473) */
#define VK_LIKE_GAUSSIAN 0
#define VK_LIKE_SELLENTIN 1
#define VK_LIKE_HARTLAP 2
#define VK_LIKE_PERCIVAL 3

/*
 * A clamped piecewise-cubic table  f(u) = sum_p coef[i][p] * (u - knot_i)^p  on interval i.
 * Evaluation clamps u to [knots[0], knots[n_int]] first (FITPACK ext=3 / box clamp).
 * Interval search: the first `lead` intervals are irregular, the rest start at knots[lead].
 * inv_h > 0: those knots are exactly uniform with spacing 1/inv_h; inv_h < 0: nearly uniform (every knot within
 * 0.4 spacings of the uniform position, mean spacing 1/|inv_h|; the estimate is corrected against the knots);
 * inv_h == 0: arbitrary knots, binary search.
 */
typedef struct vk_pp {
  int32_t n_int;        /* number of intervals; knots has n_int+1 entries      */
  int32_t lead;         /* 0 or 1 leading irregular interval                   */
  double inv_h;         /* see above                                           */
  const double* knots;  /* [n_int+1]                                           */
  const double* coef;   /* [n_var][n_int][4]; n_var is table specific          */
} vk_pp;

typedef struct vk_tables {
  /* ---- redshift-space grid of the data vector and its projection ---------- */
  int32_t n_s;          /* s bins of the data vector (ccf_fit.py:90)           */
  int32_t n_mu;         /* mu nodes, 100 (ccf_model.py:819,822)                */
  int32_t n_x;          /* velocity nodes, 50 (ccf_model.py:570)               */
  int32_t n_ell;        /* multipoles in the data vector (ccf_fit.py:92)       */
  const double* s;      /* [n_s]                                               */
  const double* mu;     /* [n_mu]                                              */
  const double* w_ell;  /* [n_ell][n_mu] projection weights (utils.py:45-56 composed with
                           the cubic interp2d of ccf_model.py:824)             */
  const double* x;      /* [n_x] v/sigma_v nodes, linspace(-6,6,n_x)           */
  const double* w_x;    /* [n_x] Simpson weights * dx / sqrt(2 pi) (ccf_model.py:690).  For the reference's 50 (even) nodes
                           the caller chooses which SciPy's default `simps` rule the weights restate: SciPy >= 1.11
                           (1/3,4/3,2/3,...,4/3 - 1/12, 1/3 + 2/3, 5/12) or SciPy < 1.11, even='avg'
                           (5/12, 13/12, 1, ..., 1, 13/12, 5/12); victor_amd.tables.simpson_weights builds both */

  /* ---- real-space CCF multipoles xi^r_l(r) (ccf_model.py:615-621) ---------- */
  int32_t n_ell_r;      /* real-space multipoles available: 1..3 (l = 0,2,4)   */
  int32_t n_beta_r;     /* 0: tables fixed; else nodes of the reconstruction-beta grid */
  const double* beta_r; /* [n_beta_r]                                          */
  vk_pp xi;             /* fixed: coef[n_ell_r][n_int][4]
                           beta-dependent: coef[n_ell_r][n_beta_r-1][n_int][4][4], the last
                           index being the power of (beta - beta_r[k]) (PCHIP in beta,
                           ccf_model.py:323-326, composed with the not-a-knot spline in r) */

  /* ---- matter profile -> velocity profile (ccf_model.py:421-459,625-636) --- */
  int32_t matter_model; /* VK_MATTER_TEMPLATE or VK_MATTER_LINEAR_BIAS: selects the per-point amplitude
                           (growth term and powers of 1/bias, ccf_model.py:426-435)                */
  int32_t vr_beta_dep;  /* 0: velocity tables fixed; 1: they depend on the reconstruction beta through
                           xi^r_0 (linear_bias with reconstruction): PCHIP-in-beta form on beta_r  */
  vk_pp vr;             /* splined on r_ext = [0.01, r...]:
                           fixed:  coef[5][n_int][4] = V1 = r*Delta, Da = delta - 2 Delta/3,
                                   V2 = r*Delta*delta, Ge1, Ge2 (numerical-gradient tables of the
                                   empirical_corr branch, ccf_model.py:455-459; /3 folded in)
                           beta-dependent: coef[2][n_beta_r-1][n_int][4][4] = V1, Da              */
  const double* vr_emp; /* beta-dependent tables only, may be NULL (then empirical_corr is refused):
                           [3][n_beta_r-1][vr.n_int][4][7] = V2, Ge1, Ge2 as polynomials of degree 6 in
                           (beta - beta_r[k]) - V2 and Ge2 are products of two PCHIP cubics              */
  double vt_amp;        /* VK_MATTER_VELOCITY_TEMPLATE only: template_hubble_ratio * (1+z_sim)/(1+z_eff) /
                           template_fsigma8 (ccf_model.py:442-443); apar cancels against aH_true       */
  /* ---- velocity dispersion template (ccf_model.py:654-655) ----------------- */
  vk_pp sv;             /* isotropic template: coef[1][n_int][4], normalised sigma_v(r) shape;
                           anisotropic template: knots = r_for_sv only (coef unused, see sv2d)          */
  int32_t sv_n_mu;      /* 0: isotropic.  else number of mu nodes of the sigma_v(r, mu) template        */
  double sv_mu_inv_h;   /* 1/spacing of the mu nodes if uniform, else 0                                 */
  const double* sv_mu;  /* [sv_n_mu] mu nodes                                                           */
  const double* sv2d;   /* [sv.n_int][sv_n_mu-1][4][4] bicubic patches: coefficient of du^p dmu^q of the
                           tensor-product not-a-knot spline (RectBivariateSpline, ccf_model.py:654)     */

  /* ---- optional unified grid: one interval index for sigma_v, V1 and every xi^r_l -------------------- */
  /* When the r grid and the sigma_v grid are uniform and commensurate, the host re-expresses all tables on
   * their common refinement (u0 + q/inv_h, q < uni_n) in interval units; the fast theory kernels need it.
   * The grid starts at or below the first knot of vr (u = 0.01): refined intervals below a table's first knot hold
   * its boundary value, the interval that contains 0.01 holds the leading V cubic (the kernels never evaluate
   * below u = 0.01: V is clamped there, ccf_model.py:625 with ext=3, and every other table is constant).       */
  int32_t uni_n;        /* 0: not available (only the generic theory kernel is used)                    */
  double uni_u0;        /* left end of the refined grid, <= vr.knots[0]                                  */
  double uni_inv_h;     /* 1/spacing of the refined grid                                                 */
  const double* uni_sv_v; /* [uni_n][2][4]: sigma_v shape and V1 = r*Delta, coefficients of tau^p        */
  const double* uni_xi; /* fixed: [n_ell_r][uni_n][4]; beta-dependent: [n_ell_r][n_beta_r-1][uni_n][4][4]
                           (last index = power of beta - beta_r[k])                                       */
  const double* uni_xic;/* same shape, the Legendre sum regrouped in powers of m = mu_r^2 (n_ell_r >= 2 only):
                           sum_l xi_l P_l(mu_r) = A + m B + m^2 C with A = xi_0 - xi_2/2 + 3 xi_4/8,
                           B = 3 xi_2/2 - 15 xi_4/4, C = 35 xi_4/8; used when the anisotropic sum is asked for  */
  const double* uni_vb; /* vr_beta_dep only (else NULL): V1 on the unified grid as beta polynomials,
                           [n_beta_r-1][uni_n][4][4]; the V half of uni_sv_v is then rebuilt per point            */
  const double* uni_v2; /* fixed velocity tables only (else NULL): V2 = r*Delta*delta on the unified grid, [uni_n][4];
                           with empirical_corr the V half of the records becomes V1 + Av V2 per point            */
  const double* uni_da; /* fixed velocity tables only (else NULL): Da = delta - 2 Delta/3 on the unified grid,
                           [uni_n][4]; lets the dispersion model run on the fast kernels                        */
  const double* uni_ge; /* fixed velocity tables only (else NULL): the numerical-gradient tables Ge1, Ge2 of the
                           empirical_corr branch on the unified grid, [2][uni_n][4]: the dispersion model then uses
                           Ge1 + Av Ge2 in place of Da (ccf_model.py:455-459)                                    */
  const double* uni_dab;/* vr_beta_dep only (else NULL): Da on the unified grid as beta polynomials,
                           [n_beta_r-1][uni_n][4][4]: the dispersion model on the fast kernels with linear_bias on a
                           reconstructed real-space ccf (ccf_model.py:358-370, 658-671)                           */
  const double* uni_empb;/* vr_beta_dep only (else NULL): V2, Ge1, Ge2 of the empirical_corr branch on the unified grid,
                           degree 6 in beta (vr_emp refined): [3][n_beta_r-1][uni_n][4][7]                        */
  /* Union-grid form of the same tables for knots that are not uniform or not commensurate: uni_n intervals between
   * the sorted distinct knots uni_knots[0..uni_n] of vr (uni_knots[0] = vr.knots[0] = 0.01), xi and sv; the
   * coefficient arrays above are then in units of each interval's own width.  A uniform look-up table of
   * uni_lut_n - 1 cells over [0, uni_knots[uni_n]) plus one guard cell locates the interval: every cell holds at most
   * TWO interior knots and uni_lut[c] is the interval that contains the cell's left edge (guard cell: the last
   * interval); the kernels add (u >= next knot) + (u >= the one after).  uni_u0 / uni_inv_h are unused here.     */
  int32_t uni_lut_n;      /* 0: uniform-lattice form.  > 0: union-grid form, entries of the table (<= 4097)     */
  double uni_lut_inv_g;   /* cells per unit length: (uni_lut_n - 1) / uni_knots[uni_n]                          */
  const uint16_t* uni_lut;/* [uni_lut_n]                                                                        */
  const double* uni_knots;/* [uni_n + 1]                                                                        */

  double iaH;           /* (1+z)/(100 E(z)) (ccf_model.py:43-45)               */
  double template_sigma8; /* ccf_model.py:432-435                              */

  /* ---- data vector (ccf_fit.py:166-193,306-323) ---------------------------- */
  int32_t n_beta_d;     /* 0: fixed data vector; else beta nodes               */
  const double* beta_d; /* [n_beta_d]                                          */
  const double* data;   /* fixed: [N]; else PCHIP pieces [n_beta_d-1][N][4], N = n_ell*n_s */

  /* ---- covariance / precision (ccf_fit.py:195-260, 445-453) ---------------- */
  int32_t n_beta_c;     /* 0: fixed; else beta nodes of the covariance stack   */
  const double* beta_c; /* [n_beta_c]                                          */
  const double* prec;   /* fixed: [N][N]; else [n_beta_c][N][N] (inverse of each slice) */
  const double* logdet; /* [n_beta_c] log det of each covariance slice (NULL if fixed) */
  const double* eig;    /* [n_beta_c][N] generalised eigenvalues of (cov[last], cov[k]) so that
                           logdet((1-t) cov[k] + t cov[last]) = logdet[k] + sum log(1-t+t*eig) */
} vk_tables;

typedef struct vk_eval_opts {
  int32_t rsd_model;         /* VK_RSD_*                                        */
  int32_t assume_isotropic;  /* use xi^r_0 only (ccf_model.py:681-687)          */
  int32_t rescale_from_ap;   /* 0: c = astar; 1: c = AP integral (ccf_model.py:606-611) */
  int32_t like_form;         /* VK_LIKE_*                                       */
  double nmocks;             /* ccf_fit.py:456                                  */
  double nparams;            /* ccf_fit.py:465                                  */
  int32_t kaiser_approx;     /* ccf_model.py:730-738                            */
  int32_t kaiser_coord_shift;/* ccf_model.py:698-707                            */
  int32_t niter;             /* fixed-point iterations (ccf_model.py:661,701), default 5 */
  int32_t from_data;         /* realspace_ccf_from_data: xi^r evaluated at fiducial coordinates, un-rescaled
                                abscissae (ccf_model.py:618-619,675-679); growth term beta*bias for linear_bias */
  int32_t empirical_corr;    /* velocity multiplied by (1 + Av delta(r)) (ccf_model.py:451-459)          */
  int32_t reserved;          /* flag word: VK_OPT_* below, read by the create calls of the sampled handles alone; 0 otherwise */
} vk_eval_opts;

/* ---- likelihood-level beta interpolation in the device loops (ccf_fit.py:383-440) ---------------------------------------------
 * The reference's `beta_interpolation: likelihood` evaluates a point at the two nodes of the data vector's beta grid that
 * bracket its beta - lo the last node with g < beta, hi the first with g >= beta (ccf_fit.py:386-390; a beta on a node gives
 * hi = that node and t = 1) - and blends lnL and chi-square linearly with t = (beta - g[lo]) / (g[hi] - g[lo]); an end that is
 * not finite fails both (ccf_fit.py:402-410).
 *
 * VK_OPT_BETA_BLEND in opts->reserved of vk_fit_create / vk_chain_create / vk_nested_create / vk_grid_create / vk_is_create /
 * vk_is_create_own puts the new handle in that mode: every evaluation of its m pending rows becomes a split kernel (2 m rows:
 * [0, m) at g[lo], [m, 2 m) at g[hi], realisation indices duplicated), the unchanged evaluation of the 2 m rows - the data
 * vector, realisations in pairs mode, realisations in cross mode - and a merge kernel that forms (1 - t) lo + t hi with separate
 * roundings, the host expression's bits.  A row without a bracket (beta <= g[0], beta > g[last], NaN: where the reference
 * raises IndexError) reports (-inf, +inf), so a sampler rejects it.  g is the context's beta_d, copied once per handle; the
 * handle's pending-row copies, realisation indices, theory workspace and raw results are sized for twice its largest launch,
 * inside its one allocation (a create call that cannot allocate says how many bytes it asked for).
 * Refused by the create call, before any device call (VK_E_ARG words in `err`): the _joint and _joint_blocks forms (a blend per
 * block under one beta is a design of its own) and a context whose data vector is not gridded in beta.  On a handle in this
 * mode vk_fit_fisher, vk_chain_set_predictive and vk_is_set_predictive are refused: a blended point has two theory vectors.
 * The evaluation entry points (vk_eval_batch and its kin) never read the word; the handle clears the flag in its own copy.
 *
 * vk_blend_split / vk_blend_merge run the two kernels alone on host buffers (device `device`, synchronous; for tests):
 *   split: grid [n_grid] increasing, rows [m][VK_NPAR], which [m] or NULL -> rows2 [2 m][VK_NPAR], which2 [2 m] (untouched
 *          without which), t [m], fail [m].
 *   merge: t [m], fail [m], raw_lnl / raw_chi [2 m][per_row] -> lnl / chi [m][per_row] (per_row: 1, or n_real in cross mode).
 * Both return VK_OK, VK_E_ARG (a NULL array, m < 1, n_grid < 2, per_row < 1) or VK_E_HIP. */
#define VK_OPT_BETA_BLEND 1
int vk_blend_split(int device, const double* grid, int32_t n_grid, const double* rows, const int32_t* which, int64_t m, double* rows2,
                   int32_t* which2, double* t, int32_t* fail);
int vk_blend_merge(int device, const double* t, const int32_t* fail, int64_t m, int64_t per_row, const double* raw_lnl,
                   const double* raw_chi, double* lnl, double* chi);

typedef struct vk_ctx vk_ctx;

int vk_abi_version(void);
int vk_device_count(void);
/* The VICTOR_HIP_* tuning / A-B environment knobs are read when a context is created, not per launch; call this after
 * changing one in a running process and every context re-reads them at its next entry point. */
void vk_knobs_refresh(void);

/* ---- the polling hand-off's launch rule (pure functions: no context, no GPU) -----------------------------------------------
 * Launches of at most 8 points whose (mu, v) planes are split over workgroups - one point per call, the reference's calling
 * convention (CCFLikelihood.py:32-39), the mailbox server's launches, the half-ensembles of victor_amd/sampler.py - may hand
 * their partial sums over by POLLING: the workgroup of a point's last work item waits, resident, for the other workgroups'
 * sums.  Waiting workgroups are harmless as long as they can never hold ALL workgroup slots of an XCD while the workgroups
 * they wait for are not placed yet.  The rule that guarantees it:
 *   - a launch polls only if at least two of its workgroups fit on a CU, so an XCD (32 CUs) offers 64 slots at least, if it
 *     fits on the chip at once, and if its context holds a reservation for its points (one waiter per point);
 *   - a context reserves on demand, up to 8 waiters, out of a budget of 32 per PROCESS (enforced here; a context's launches
 *     are stream-ordered, so its reservation bounds what it has resident); without reservation the launch hands over through
 *     completion counters - the same sums in the same order, bit-identical results, ~1.2 us slower;
 *   - across processes the reservations of one GPU must stay below 64 in all - one process with the full budget (the GPU
 *     owner, victor_amd/broker.py: 4 contexts x 8 requests) plus up to 31 processes that evaluate one point per call in one
 *     context, or up to 63 such processes (vk_poll_budget returns 1: the number of full-budget processes per device).  The
 *     processes of one user on one host enforce it among themselves through a ledger in /dev/shm, one file per GPU
 *     (victor_hip_poll2_<uid>_<PCI bus id>, 5 KB: a slot per owner, written by that owner only).  An owner is {pid, start time
 *     of that pid, inode of its pid namespace, library instance} - a recycled pid does not inherit a dead process's
 *     reservation, two copies of the library in one process keep a slot each; slots of owners that are gone (dead, a zombie,
 *     the pid now another process) are ignored and reused; a slot written in ANOTHER pid namespace (containers sharing
 *     /dev/shm) cannot be judged from here and counts as living, for good: the bound errs towards the counters.  The file is
 *     opened without following symbolic links and must be a regular file of this user, closed to group and others, of the
 *     expected size and version: otherwise the process does not poll at all.  Without /dev/shm (nothing to create the file
 *     in) the process budget alone applies.  A process beyond the bound gets no reservation and hands over through the
 *     counters; a launch asks for a reservation only if it would poll with it, and after a refusal only once the ledger has
 *     changed.  Processes that do not share that file (other users, other /dev/shm mounts) are the operator's to keep within
 *     the bound.
 * Failure mode if the rule is broken (or a launch is lost): a waiting workgroup gives up after 5 s of wall clock, the call -
 * or, for enqueued work, the next call / vk_sync on that context - returns VK_E_HIP ("waited ... for partial sums that never
 * arrived") and the context stays unusable: destroy it and create a new one.  No result of such a launch is delivered.
 * vk_poll_rule: 1 when a launch of `n_points` points, `parts` workgroups per plane and `workgroups` workgroups in all, of
 * which `workgroups_per_cu` fit on a CU of a device with `n_cu` CUs, polls under a context reservation of `reserved` waiters.
 * vk_poll_grant: how many MORE waiters a context holding `ctx_reserved` is granted when it wants `want`, the process has
 * `process_reserved` reserved in all and the other living processes of the ledger `others_reserved` (0 or want - ctx_reserved:
 * all or nothing).  vk_poll_device_reserved: what the ledger of `ctx`'s GPU holds for the other processes and for this one
 * (VK_E_ARG, *others = -1, when no ledger could be mapped). */
int32_t vk_poll_rule(int64_t n_points, int32_t parts, int64_t workgroups, int32_t workgroups_per_cu, int32_t n_cu, int32_t reserved);
int32_t vk_poll_grant(int32_t others_reserved, int32_t process_reserved, int32_t ctx_reserved, int32_t want);
int32_t vk_poll_budget(int32_t* per_process, int32_t* xcd_slots);
int32_t vk_poll_device_reserved(const vk_ctx* ctx, int32_t* others, int32_t* mine);

/* ---- the ledger's operations on a file of the caller's choosing, for an owner of the caller's making ------------------------
 * DEVELOPMENT entry points (tests/test_ledger.py drives them without a GPU): like every development switch of the library they
 * answer only with VICTOR_HIP_DEV=1 in the environment (otherwise: NULL / -1 / 0, nothing is touched).
 * vk_ledger_open_at: opens (creates) the ledger file at `path` and claims a slot for the owner {pid, start, ns, lib}; pid <= 0:
 *   the calling process itself (lib != 0 then stands for another copy of the library in it).  *status: 0 opened, 1 unavailable
 *   (cannot be created), 2 untrusted (a symbolic link, another owner or mode, wrong size / magic / version, a lock nobody
 *   releases), 3 full.  vk_ledger_close(led, keep_slot): keep_slot != 0 leaves the slot behind as a killed process would.
 * vk_ledger_others: waiters reserved by the other owners that are living or cannot be judged.  vk_ledger_grant / _release:
 *   the library's own grant / release protocol with *process_reserved standing for the owner's process-wide count.
 * vk_ledger_self(what, pid): 0 pid, 1 start time, 2 pid-namespace inode, 3 library instance of the caller; 4 start time of
 *   process `pid` (0: gone), 5: 1 if process `pid` is there (not gone, not a zombie).
 * vk_ledger_layout: bytes of the file's header and of a slot {int64 pid, uint64 start, uint64 ns, uint64 lib, int32 reserved,
 *   int32 pad}, number of slots, format version (header: uint32 magic "VKPL", uint32 version, uint32 generation, uint32 pad). */
void vk_ledger_layout(int32_t* header_bytes, int32_t* slot_bytes, int32_t* slots, int32_t* version);
uint64_t vk_ledger_self(int32_t what, int64_t pid);
void* vk_ledger_open_at(const char* path, int64_t pid, uint64_t start, uint64_t ns, uint64_t lib, int32_t* status);
int32_t vk_ledger_slot(const void* led);
int32_t vk_ledger_others(const void* led);
uint32_t vk_ledger_generation(const void* led);
int32_t vk_ledger_grant(void* led, int32_t* process_reserved, int32_t ctx_reserved, int32_t want);
void vk_ledger_release(void* led, int32_t* process_reserved, int32_t n);
void vk_ledger_close(void* led, int32_t keep_slot);

/* Copies every table to `device`.  On failure returns NULL and writes a message to err. */
vk_ctx* vk_create(const vk_tables* tables, int device, char* err, size_t errlen);
void vk_destroy(vk_ctx* ctx);
const char* vk_last_error(const vk_ctx* ctx);
/* name of the theory-kernel variant the most recent evaluation launched (diagnostics / benchmarks) */
const char* vk_last_kernel(const vk_ctx* ctx);
/* the exact instantiation of that launch and the chi-square kernel that ran with it, "cells<3,2,1,dispersion,0>+fused",
 * "fast<1,1,0,from_data,0>+like_tiled<8>", "generic<kaiser,2,3>+like", "cells<1,1,0,streaming,0>+none" (theory only),
 * "xi<euclid,1>" (K1x), "cells<3,2,1,streaming,0>+joint_chi2" (the lead context of vk_joint_cov_eval_device_async: the
 * lead block's theory launch and the joint chi-square kernel; "+joint_real_chi2" after vk_joint_cov_eval_realisations);
 * valid until the next call on ctx */
const char* vk_last_instance(const vk_ctx* ctx);
/* 1 when that launch also took the chi-square / log-likelihood (fused tail), 0 when K2 ran as its own launch */
int vk_last_fused(const vk_ctx* ctx);
/* 1 when that launch handed the partial sums of its split planes over by polling (vk_poll_rule below), 0 otherwise */
int vk_last_polled(const vk_ctx* ctx);
void vk_default_opts(vk_eval_opts* opts);

/* Full likelihood for n parameter rows (host buffers).  Any of lnl/chi2/theory may be NULL.
 * lnl[i] = -inf, chi2[i] = +inf where the reference returns (-inf, inf) (ccf_fit.py:447-450,477-481).
 * theory is [n][n_ell*n_s].  Synchronous for the caller: the results are in lnl / chi2 on return.  (Calls of a few
 * hundred points that do not ask for `theory` return as soon as the results have arrived in pinned host memory, with
 * the launch still retiring on the context's stream; every later call, vk_sync and vk_destroy are ordered behind it.) */
int vk_eval_batch(vk_ctx* ctx, const vk_eval_opts* opts, const double* params, int64_t n,
                  double* lnl, double* chi2, double* theory);

/* The same call in two halves for callers that have host work to overlap with the launch (the walker ensembles of
 * victor_amd/sampler.py advance one half of their walkers while the other half is on the GPU): vk_eval_batch_begin copies the
 * rows and enqueues the launch (1 <= n <= 4096), vk_eval_batch_finish waits for lnl / chi2 (either may be NULL).  One batch
 * per context at a time - several contexts may each have one in flight; nothing else may be called on a context between
 * its begin and its finish. */
int vk_eval_batch_begin(vk_ctx* ctx, const vk_eval_opts* opts, const double* params, int64_t n);
int vk_eval_batch_finish(vk_ctx* ctx, double* lnl, double* chi2);

/* ---- lock-step Metropolis walkers, advanced natively --------------------------------------------------------------------
 * The reference is sampled by cobaya, one likelihood per call (victor/likelihoods/CCFLikelihood.py:32-39);
 * victor_amd/sampler.py: EnsembleMetropolis advances W random-walk Metropolis chains together, one likelihood batch per step,
 * from the priors / proposal widths of the same `params:` block (config/boss_cobaya_config.yaml:50-97 of the reference).
 * vk_walk_run is that sampler's step loop in the library: the ensemble as two halves on two contexts (vk_eval_batch_begin /
 * _finish: half A of step t + 1 is on the GPU while half B of step t is accepted / rejected), rows formed as
 * CCFModel._param_rows forms them (one routine for the Alcock-Paczynski factors: vk_epsilon_to_ap), the caller's pre-drawn
 * random numbers - without `speculate` the same launches as the Python loop, hence the same chain bit for bit
 * (tests/test_gpu_workloads.py), without the host's ~20 NumPy calls per step.
 *   columns[j]   row column (VK_P_*) the j-th sampled parameter is written to, or VK_WALK_EPSILON: the parameter is epsilon and
 *                the columns APERP, APAR, EPSILON follow from it (apar = alpha eps^(-2/3), aperp = eps apar, ccf_model.py:589-592)
 *   lo, hi       uniform prior box; a proposal outside it is evaluated at the walker's position, discarded, and reads -inf
 *   base_rows    [n_walkers][VK_NPAR]: the fixed parameters and defaults of every row
 *   speculate    != 0: TWO steps per launch.  The proposal of step t + 1 starts from the proposal of step t (accepted) or from
 *                the old position (rejected) - both are known when step t is proposed, so a walker's three points travel in one
 *                launch and both decisions are taken when the results arrive: two steps per round trip host -> GPU -> host
 *                (what bounds a small ensemble: the GPU is far from full) for three evaluations instead of two.  The same
 *                proposals, the same acceptance levels as the step-by-step loop; n_evals counts the evaluations that loop
 *                would have made.  PARITY WITH THE STEP-BY-STEP LOOP IS TO ROUNDING, NOT BIT FOR BIT: a launch of three rows
 *                per walker takes another work split than one of one row, so the log-likelihoods agree to ~1e-13 relative
 *                and an acceptance `logu < lnL' - lnL` decided within that margin may fall the other way; positions and
 *                decisions were identical over every chain compared so far (thousands of steps), the stored lnL differ in
 *                their last bits.  A caller who needs the step-by-step chain bit for bit passes speculate = 0.  What does NOT
 *                vary: the chain for a given `speculate` is independent of how a run is cut into vk_walk_run calls - a left-
 *                over single step travels in a launch of the same shape (its two candidate rows idle).  Worth it while three
 *                times the ensemble still fits the idle part of the GPU (victor_amd/sampler.py chooses; ignored when a launch
 *                would exceed 4096 rows)
 * vk_walk_run: x [W][P] and lnl [W] are the ensemble's state (in / out); dz [n_steps][W][P] the proposal increments, logu
 * [n_steps][W] the log acceptance levels; chain [n_steps][W][P] and lnl_hist [n_steps][W] receive the state after every step
 * (either may be NULL); *n_accept and *n_evals are incremented.  One or two contexts holding the same tables (two: the halves
 * overlap); nothing else may use those contexts during a run.  On error the code is returned, vk_walk_last_error gives the
 * text, no batch stays begun on the contexts and x / lnl hold the state after the last completed half-step. */
#define VK_WALK_EPSILON (-1)
typedef struct vk_walk vk_walk;
vk_walk* vk_walk_create(vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts, int32_t n_walkers, int32_t n_params,
                        const int32_t* columns, const double* lo, const double* hi, const double* base_rows, double alpha,
                        int32_t speculate, char* err, size_t errlen);
int vk_walk_run(vk_walk* w, int64_t n_steps, double* x, double* lnl, const double* dz, const double* logu, double* chain,
                double* lnl_hist, int64_t* n_accept, int64_t* n_evals);
const char* vk_walk_last_error(const vk_walk* w);
void vk_walk_destroy(vk_walk* w);
/* apar[i] = alpha * eps[i]^(-2/3) (alpha == 1: no multiply), aperp[i] = eps[i] * apar[i] with libm's pow, as the reference
 * evaluates them on Python floats (ccf_model.py:589-592): the one routine behind every row the package forms from an epsilon.
 * Pure host arithmetic: no context, no GPU. */
void vk_epsilon_to_ap(const double* eps, int64_t n, double alpha, double* aperp, double* apar);

/* ---- one parameter batch against many simulation realisations of the data vector ---------------------------------------
 * The reference reads ONE realisation of a stacked data file, the one `simulation_number` names (victor/ccf_fit.py:59-61,
 * 93-100); validating a model on mocks evaluates the same points against every realisation.  The theory vector of a point does
 * not depend on the realisation: it is computed once, then compared with each data vector under the context's covariance
 * (victor/ccf_fit.py:349-354 for chi2, :166-193 for the data vector at beta, :195-260 and :444-481 for the precision, the log
 * determinant, the likelihood forms and the (-inf, inf) guards - the same arithmetic as vk_eval_batch, summed in another order).
 * vk_set_realisations: n_real blocks back to back, each with exactly the layout of vk_tables.data ([N] for a fixed data vector,
 *   the PCHIP pieces [n_beta_d-1][N][4] otherwise); copied to the device, resident until replaced or vk_destroy (n_real = 0
 *   releases them).  The context must have been created with a data vector.
 * vk_eval_realisations: which == NULL - every point against every realisation, lnl / chi2 [n][n_real]; otherwise which[i] is
 *   the realisation (0 .. n_real-1) of point i and lnl / chi2 are [n].  Both modes return the same bits for the same (point,
 *   realisation).  Either output may be NULL.  VK_E_ARG when no realisations are set or an index is out of range.  Synchronous;
 *   large batches are cut into launches whose outputs stay below 256 MB. */
int vk_set_realisations(vk_ctx* ctx, const double* data, int32_t n_real);
int vk_eval_realisations(vk_ctx* ctx, const vk_eval_opts* opts, const double* params, int64_t n, const int32_t* which,
                         double* lnl, double* chi2);

/* ---- scale cuts: every realisation under many s ranges and multipole sets, from one theory vector ------------------------
 * A cut k keeps n_k of the context's N data-vector entries, index_k[0 .. n_k-1] strictly increasing (layout of the data vector:
 * multipole-major).  Its chi2 is r^T inv(C[idx, idx]) r over the kept entries - the inverse of the SUB-covariance, not a
 * sub-block of the context's precision -, its log determinant is the sub-covariance's and the likelihood forms (Hartlap,
 * Percival) count n_k data points.  The theory vector of a point does not depend on the cut.
 * vk_set_cuts: n_cuts cuts next to the realisations already set (vk_set_realisations comes first).  With S = max(n_beta_c, 1)
 *   covariance slices:  n_keep [n_cuts];  index [n_cuts][N] (row k: its first n_keep[k] entries are read);  prec [n_cuts][S][N*N]
 *   (slot (k, j) starts at (k S + j) N N and holds inv(C_j[idx_k, idx_k]) compact, row stride n_keep[k]);  logdet [n_cuts][n_beta_c]
 *   and eig [n_cuts][n_beta_c][N] (row (k, j): its first n_keep[k] entries) as vk_tables.logdet / eig of the sub-covariances -
 *   both NULL for a fixed covariance.  Copied to the device; resident until replaced, until n_cuts = 0, until the next
 *   vk_set_realisations (cuts belong to the realisations they were set next to) or vk_destroy.
 * While cuts are resident a PROBLEM is the flat index v = k * n_real + m (cut-major): vk_eval_realisations returns [n][n_cuts *
 *   n_real] in cross mode and takes which[i] = v in pairs mode (the same bits in both modes), and every handle over realisations
 *   (vk_fit_*, vk_chain_*, vk_nested_*, vk_grid_*, vk_is_*) sees n_cuts * n_real realisations.  Without cuts nothing changes.
 * VK_E_ARG: no realisations set; model realisations resident (vk_set_model_realisations - a row's table set is its realisation,
 *   not the flat index; that call is refused in turn while cuts are resident); n_keep outside 1..N; indices not strictly
 *   increasing within 0..N-1; a needed pointer NULL.  Refused while cuts are resident, each with VK_E_ARG and a text, the handle
 *   or context staying usable, ON WHAT ADDRESSES REALISATIONS: joint evaluations and joint handles against the blocks'
 *   realisations, and of a handle created with `which` (or over every realisation) vk_fit_fisher (J^T P J is formed from the full
 *   precision), vk_chain_set_predictive / vk_is_set_predictive and VK_OPT_BETA_BLEND.  Everything over the context's own data
 *   vector - vk_eval_batch*, handles created with which == NULL with their Fisher, predictive and blend calls, joint evaluations
 *   against the data vectors - reads nothing the cuts changed and does what it did before, cuts resident or not. */
int vk_set_cuts(vk_ctx* ctx, int32_t n_cuts, const int32_t* n_keep, const int32_t* index, const double* prec, const double* logdet,
                const double* eig);

/* ---- every realisation with its own real-space CCF: xi^r table sets selected per row ------------------------------------
 * The reference picks the real-space multipoles xi^r_l(r) - with reconstruction xi^r_l(beta, r) - of ONE simulation out of a
 * stacked model file, the one `realspace_ccf.simulation_number` names (victor/ccf_model.py:127-162), as it picks the data vector;
 * a mock test fits mock m's redshift-space multipoles with the model built from mock m's own real-space CCF.
 * vk_set_model_realisations: n_sets table sets back to back, each with exactly the layout and length of vk_tables.xi.coef,
 *   vk_tables.uni_xi and vk_tables.uni_xic of the context (set m of xi_coef at xi_coef + m * length, and so on).  A pointer whose
 *   array the context was created without (a context without unified tables reads neither uni_xi nor uni_xic) may be NULL; the
 *   others must be given.  Copied to the device, resident until replaced or vk_destroy; n_sets = 0 releases them, after which
 *   the context does exactly what it did before.  VK_E_ARG: n_sets < 0; a needed pointer is NULL; velocity tables that depend on
 *   the real-space CCF (vk_tables.vr_beta_dep, or matter_model linear_bias, whose profile is derived from xi^r_0) - those would
 *   need sets of their own.
 * While sets are resident: the pairs mode of vk_eval_realisations (which != NULL) and every fit, chain, stretch, tempered,
 *   Hessian, Fisher and predictive launch of a handle created with `which` evaluate row i from table set which[i] - everything
 *   else of the arithmetic is unchanged, so a row's bits are those of a context created from set which[i]'s tables at the same
 *   batch size.  These launches need n_sets == n_real (VK_E_ARG otherwise).  Cross mode (which == NULL) of vk_eval_realisations
 *   is refused with VK_E_ARG - a point no longer has one theory vector; expand it into pairs.  Every entry point without
 *   realisation indices (vk_eval_batch*, vk_theory_batch, vk_xi_smu_batch, the walkers, the mailbox server, handles created with
 *   which == NULL) keeps using the context's own tables, bit for bit.  Joint evaluations (vk_joint_*, joint handles) over a
 *   context with sets resident are refused with VK_E_ARG. */
int vk_set_model_realisations(vk_ctx* ctx, const double* xi_coef, const double* uni_xi, const double* uni_xic, int32_t n_sets);

/* ---- best-fit points: bounded Nelder-Mead on the device, one simplex per problem ----------------------------------------
 * The reference has no optimiser: a user maximises CCFFit.log_likelihood (victor/ccf_fit.py:356-483) with a host optimiser,
 * one call per point.  A PROBLEM is one maximisation of that lnL - the likelihood form, and for a beta-dependent covariance
 * the log-determinant term (:444-481), included: with uniform priors the MAP point - over the d sampled parameters inside
 * their prior box, against the context's data vector or against one simulation realisation (vk_set_realisations).  The
 * chi-square reported is the chi-square AT that point (:325-354), not a separate chi-square minimum.
 * Every problem runs textbook Nelder-Mead (Lagarias et al. 1998, the rules of scipy.optimize's 'Nelder-Mead'; DESIGN.md
 * section 7a) with the four candidates of an iteration evaluated in one launch: a problem owns S = max(4, d + 1) rows per
 * launch, all problems advance together, one launch per iteration, no host round trip per iteration.
 *   columns[j]  row column (VK_P_*) of the j-th sampled parameter, or VK_WALK_EPSILON (the columns APERP, APAR, EPSILON follow
 *               from it and `alpha` as vk_epsilon_to_ap forms them); each column once, 1 <= n_params <= 10
 *   lo, hi      [n_params] the box; a candidate outside it reads f = +inf and is not evaluated
 *   base_rows   [n_problems][VK_NPAR]: the fixed parameters and defaults of each problem's rows
 *   which       [n_problems] realisation (0 .. n_real - 1 of the context's set) of each problem; NULL: the data vector
 * vk_fit_run: x0 [n_problems][n_params] starts (inside the box), step [n_params] initial steps (> 0: vertex j of the start
 *   simplex is x0 + step_j e_j, else x0 - step_j e_j, else clamped to the box), xtol [n_params] and ftol (in lnL) the
 *   convergence test (every parameter's spread over the simplex <= xtol_j, and the spread of -lnL <= ftol), max_iter the
 *   iteration limit (launches of the problem: init, candidate and shrink launches), restarts the number of times a converged
 *   simplex is rebuilt around its best vertex before the problem is done.  Out, per problem: x [n_problems][n_params] the best
 *   vertex, lnl / chi2 there, status VK_FIT_*, n_iter, n_evals (rows whose value the search used: what a one-point-at-a-time
 *   Nelder-Mead would have evaluated; the GPU evaluates S rows per iteration).  VK_FIT_NO_FINITE_START: every start vertex
 *   read -inf; then x = x0, lnl = -inf, chi2 = inf.  Synchronous.  A run owns its context: nothing else may use it until the
 *   run returns.  On error the code is returned, vk_fit_last_error gives the text and nothing stays in flight.
 *   Refused (VK_E_ARG): a batch begun with vk_eval_batch_begin, realisation mode without (enough) realisations set, a start
 *   outside the box, a step <= 0. */
#define VK_FIT_CONVERGED 0
#define VK_FIT_MAX_ITER 1
#define VK_FIT_NO_FINITE_START 2
typedef struct vk_fit vk_fit;
vk_fit* vk_fit_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_problems, int32_t n_params, const int32_t* columns,
                      const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which,
                      char* err, size_t errlen);
int vk_fit_run(vk_fit* f, const double* x0, const double* step, const double* xtol, double ftol, int32_t max_iter,
               int32_t restarts, double* x, double* lnl, double* chi2, int32_t* status, int32_t* n_iter, int64_t* n_evals);
const char* vk_fit_last_error(const vk_fit* f);
void vk_fit_destroy(vk_fit* f);

/* ---- Metropolis chains of the data vector or one realisation each, stepped on the device ---------------------------------
 * The reference is sampled by cobaya, one likelihood per call (victor/likelihoods/CCFLikelihood.py:32), one data vector at a
 * time; under MPI it runs independent chains, one process each (README.md:30).  Here C independent random-walk Metropolis
 * chains of that lnL (victor/ccf_fit.py:356-483) - against the context's data vector, or chain c against realisation which[c]
 * (vk_set_realisations) - advance in lock step with the step loop on the device: per step one evaluation of C rows and one
 * small kernel that decides and writes the next rows.  Random numbers are the caller's: the chain is
 * defined by a host loop (victor_amd/chains.py) and the device reproduces it.
 *   columns, lo, hi, base_rows, alpha, which   as vk_fit_create, per CHAIN ([n_chains][VK_NPAR] base rows, [n_chains] indices);
 *               1 <= n_chains <= 65536, 1 <= n_params <= 10.  Device memory is bounded by one block of 64 steps.
 * One step of one chain: prop = x + dz; a proposal outside the box is evaluated at the chain's current position, discarded, and
 *   reads lnL = -inf (every launch has n_chains rows); accept when logu < lnL' - lnL (IEEE: a NaN difference rejects); on accept
 *   x, lnL, chi2 are replaced.  The decisions use additions and comparisons only; with the same rows in the same launches the
 *   log-likelihoods are the bits vk_eval_batch / vk_eval_realisations (pairs mode) return for them.  When epsilon is sampled the
 *   Alcock-Paczynski factors of a row are formed with the device's pow, the host's (vk_epsilon_to_ap) with libm's: rows, and so
 *   log-likelihoods, then agree with a host-driven chain to rounding, not bit for bit.
 * vk_chain_start: x0 [n_chains][n_params], inside the box; evaluates the starts.  Resets counters and moment sums; the pivot
 *   of a chain's moment sums is its start.  Synchronous.
 * vk_chain_begin: enqueues n_steps (1 .. 64) steps: dz [n_steps][n_chains][n_params] proposal increments, logu
 *   [n_steps][n_chains] log acceptance levels.  Step t of the block is step first_step + t of the chains' life; it is KEPT when
 *   it is >= burn and (step - burn) % thin == 0.  A kept step enters the chain's moment sums and, with want_history, the
 *   block's history; *n_kept (may be NULL) receives the number of history slots the block fills.  Returns with the work
 *   enqueued and the inputs consumed: the caller draws the next block meanwhile.
 * vk_chain_finish: waits for the block and copies its history: x [n_kept][n_chains][n_params], lnl, chi2 [n_kept][n_chains]
 *   (state after each kept step; NULL allowed when the block keeps none).
 * vk_chain_state (between blocks): x [n_chains][n_params], lnl, chi2 [n_chains], the counters n_accept, n_steps, n_kept
 *   [n_chains], pivot, sum1 [n_chains][n_params] (sum over kept steps of x_j - pivot_j), sum2 [n_chains][n_params][n_params]
 *   (sum of (x_j - pivot_j)(x_k - pivot_k), symmetric), plain double sums in step order.  Any output may be NULL.
 * A chain handle owns its context from vk_chain_begin to vk_chain_finish.  On error the code is returned, vk_chain_last_error
 *   gives the text and nothing stays in flight.  Refused (VK_E_ARG): a batch begun with vk_eval_batch_begin, realisation mode
 *   without (enough) realisations set, a start outside the box, begin without start or before the previous finish. */
typedef struct vk_chain vk_chain;
vk_chain* vk_chain_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_chains, int32_t n_params, const int32_t* columns,
                          const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which,
                          char* err, size_t errlen);
int vk_chain_start(vk_chain* f, const double* x0);
int vk_chain_begin(vk_chain* f, int32_t n_steps, const double* dz, const double* logu, int64_t first_step, int64_t burn,
                   int64_t thin, int32_t want_history, int32_t* n_kept);
int vk_chain_finish(vk_chain* f, double* x, double* lnl, double* chi2);
int vk_chain_state(vk_chain* f, double* x, double* lnl, double* chi2, int64_t* n_accept, int64_t* n_steps, int64_t* n_kept,
                   double* pivot, double* sum1, double* sum2);
const char* vk_chain_last_error(const vk_chain* f);
void vk_chain_destroy(vk_chain* f);

/* ---- Stretch-move ensembles on the same handles ------------------------------------------------------------------------------
 * vk_chain_begin_stretch reads the n_chains chains of a handle made by vk_chain_create / vk_chain_create_joint as
 * n_chains / walkers ensembles of `walkers` walkers each (walker c = r walkers + w) and enqueues n_steps (1 .. 64) SWEEPS of the
 * affine-invariant stretch move (Goodman & Weare 2010) in its two-half parallel form: half 0 of every ensemble (w < walkers / 2)
 * moves against partners drawn from half 1, then half 1 against the updated half 0.  Start, finish, state and destroy are the
 * entry points above; blocks of vk_chain_begin and of vk_chain_begin_stretch may follow each other on one handle.  The extra
 * device buffers of a block are allocated by the first call.
 *   z, lz, logu [n_steps][2][n_chains / 2], partner (int32, same shape): entry [t][h][i] belongs to sweep t, half-step h and
 *               moving walker i % (walkers / 2) of ensemble i / (walkers / 2): its stretch factor, lz = (n_params - 1) log z
 *               (formed by the caller), its log acceptance level, and its partner's index within the OTHER half, in
 *               [0, walkers / 2).
 * One half-step of one walker at x with partner p: prop = p + z (x - p), a multiplication and an addition, each rounded (no
 *   fused multiply-add); a proposal outside the box is evaluated at the walker's current position, discarded, and reads
 *   lnL = -inf (every launch has n_chains / 2 rows); accept when logu < (lz + lnL') - lnL (IEEE: a NaN rejects).  Per half-step the
 *   library enqueues a kernel that forms the proposals and their rows, the evaluation of those rows and a kernel that decides -
 *   three launches in stream order, because a half's proposals read what the other half's decisions have just written.
 * first_step, burn, thin, want_history, n_kept as vk_chain_begin, counting sweeps: a kept sweep enters the moment sums and the
 *   history with all n_chains walkers as they stand after its second half.  n_steps of vk_chain_state counts a walker's own
 *   half-steps, one per sweep.
 * Refused (VK_E_ARG) before anything is enqueued, the handle staying usable: a NULL argument, no start or a block in flight,
 *   walkers odd or < 2, n_chains not a multiple of walkers, a partner index outside [0, walkers / 2), realisation indices that
 *   differ within one ensemble, and what vk_chain_begin refuses. */
int vk_chain_begin_stretch(vk_chain* f, int32_t n_steps, int32_t walkers, const double* z, const double* lz, const double* logu,
                           const int32_t* partner, int64_t first_step, int64_t burn, int64_t thin, int32_t want_history,
                           int32_t* n_kept);

/* ---- A Gaussian prior on the sampled parameters of a best-fit or chain handle ------------------------------------------------
 * The handles above know the uniform box.  vk_fit_set_prior / vk_chain_set_prior multiply a Gaussian onto it, on any handle of
 * the create calls (single fit, joint, joint with a row set per block): ln prior = -1/2 (x - mu)^T P (x - mu), no normalisation
 * constant (a constant changes no decision and no maximum).  The device evaluates it, because the accept / reject decision and
 * the Nelder-Mead comparison run on the device between launches.
 *   mu         [n_params] the mean, in the order of the handle's sampled parameters (0 for a parameter without a prior)
 *   pp_packed  [n_params (n_params + 1) / 2] the upper triangle of the precision matrix P of the sampled parameters (zero rows
 *              for parameters without a prior), row by row - (j, k), j <= k, at j n - j (j - 1) / 2 + (k - j) - with every
 *              OFF-DIAGONAL entry doubled.  The arithmetic order is fixed (vk_prior.h): q = sum over j, then k >= j, of
 *              (pp[jk] * (x_j - mu_j)) * (x_k - mu_k), each product and each sum rounded (no fused multiply-add);
 *              ln prior = -0.5 q.
 * Both copy their inputs; NULL, NULL clears the prior, and a handle without one takes the code path, makes the launches and
 * returns the bytes it always did.  The prior holds for every later vk_fit_run / block of vk_chain_begin or
 * vk_chain_begin_stretch.
 *   best fits  the search maximises lnL + ln prior: the value of a live row is lnL + ln prior at its point.  vk_fit_run then
 *              returns that sum in `lnl`; chi2 stays the chi-square of the row.
 *   Metropolis accept when logu < (lnL' + lp') - (lnL + lp): lp' the prior at the proposal, lp recomputed at the current position.
 *   stretch    accept when logu < (lz + (lnL' + lp')) - (lnL + lp): lp' the prior at the stored proposal.
 *              Outside the box lnL' = -inf as before, and -inf plus a finite lp' is -inf; a NaN lnL' rejects.  The chains' state
 *              and history keep the log-LIKELIHOOD.
 * Refused (VK_E_ARG, the handle's last_error gives the text): one of the two NULL, a value that is not finite, and
 * vk_chain_set_prior while a block begun with vk_chain_begin / vk_chain_begin_stretch awaits vk_chain_finish. */
int vk_fit_set_prior(vk_fit* f, const double* mu, const double* pp_packed);
int vk_chain_set_prior(vk_chain* f, const double* mu, const double* pp_packed);

/* ---- Marginal histograms of a chain handle's kept positions ------------------------------------------------------------------
 * With keep-nothing runs (want_history = 0) the moment sums are all a handle returns of its posterior.  vk_chain_set_marginals
 * makes the step kernels of vk_chain_begin and vk_chain_begin_stretch count, on any handle of the create calls, every position
 * that enters the moment sums - a kept step; a kept sweep, in the walker's own moving half-step - in 64-bit histograms on the
 * device: one of every sampled parameter and one of each of n_pairs pairs of them.  Integer adds commute, so the counts do not
 * depend on the order the chains arrive in.
 *   group      chains per problem: the histograms are pooled, chain c adds to problem c / group (n_chains / group problems)
 *   n_bins     bins of a 1-D histogram, 1..1024; lo, hi [n_params]: the range [a_j, b_j] of each sampled parameter, in the order
 *              of the handle's sampled parameters (any finite lo < hi: it need not be the box)
 *   pairs      [n_pairs][2] parameter indices (j, k), j < k, each pair once, n_pairs in 0..45 (NULL for 0); n_bins2: bins per axis
 *              of a 2-D histogram, 1..128 (not read when n_pairs == 0)
 * The slot rule (vk_marginals.h), with inv_j = n_bins / (b_j - a_j), one IEEE division made once on the host: a value v < a_j
 * goes to slot 0 ("below"), v > b_j to slot n_bins + 1 ("above"), any other to slot 1 + min(n_bins - 1, (int)((v - a_j) * inv_j))
 * - one subtraction, one multiplication, one truncating conversion, nothing to fuse; v == b_j lands in the last bin.  A sample
 * enters the histogram of pair (j, k) only when it lies inside both ranges, in cell (bin_j, bin_k) by the same rule with n_bins2.
 * vk_chain_marginals copies the counts out, between blocks; either pointer may be NULL:
 *   h1         [n_chains / group][n_params][n_bins + 2]
 *   h2         [n_chains / group][n_pairs][n_bins2][n_bins2], row bin_j
 * The handle owns the buffers: made and zeroed by vk_chain_set_marginals (a second call replaces them), zeroed again by
 * vk_chain_start - which resets the counters and the moment sums too -, kept across blocks, freed by vk_chain_destroy.
 * n_bins == 0 with lo == hi == NULL clears the marginals and frees the buffers; a handle that never had them, or had them
 * cleared, makes the launches and returns the bytes it always did.
 * Refused (VK_E_ARG, vk_chain_last_error gives the text, the handle stays usable and keeps the marginals it had): a block begun
 * and not finished; group < 1 or n_chains % group != 0; n_bins outside 1..1024; n_pairs outside 0..45; with pairs, n_bins2
 * outside 1..128; a pair with j >= k or an index outside 0..n_params - 1, or a repeated pair; a range that is not finite or
 * without lo < hi; vk_chain_marginals on a handle without marginals.  Device memory that cannot be had is reported as
 * vk_chain_create reports it (VK_E_HIP, "cannot allocate ... bytes of device memory"); the handle then has no marginals. */
int vk_chain_set_marginals(vk_chain* f, int32_t group, int32_t n_bins, const double* lo, const double* hi, int32_t n_pairs,
                           const int32_t* pairs, int32_t n_bins2);
int vk_chain_marginals(vk_chain* f, int64_t* h1, int64_t* h2);

/* ---- Autocorrelation of a chain handle's ensemble series ---------------------------------------------------------------------
 * How many independent samples stand behind the moment sums and the histograms of a run without a history?  vk_chain_set_autocorr
 * makes vk_chain_begin and vk_chain_begin_stretch keep, on any handle of the create calls, one series per problem and sampled
 * parameter - the per-step SUM over the problem's `group` chains (walkers), one value per kept step (per kept sweep, after its
 * second half) - and that series' lagged products up to lag max_lag - 1 (vk_autocorr.h states the update):
 *   series value   lane l of 64 starts from +0.0 and adds the chains w = l, l + 64, ... in increasing w; a 64-lane xor butterfly
 *                  (offsets 32 .. 1, v = v + v_partner) follows.  No division by `group`.
 *   a_n            0 at the first kept step, whose series value becomes the pivot; s - pivot afterwards
 *   kept step n    acc[k] += a_n a_{n - k} for 0 <= k <= min(n, L - 1), product and sum each rounded; total += a_n;
 *                  head[n] = a_n while n < L; ring[n mod L] = a_n
 * in a small launch of its own behind the step kernel of every kept step (the second half's, of a kept sweep) on the handle's
 * stream: no host synchronisation, no atomics.  Series (problem r, parameter j) is number r n_params + j.
 * vk_chain_autocorr copies the state out, between blocks; any pointer may be NULL:
 *   pivot, total   [n_chains / group][n_params]
 *   head, ring, acc  [n_chains / group][n_params][max_lag]
 *   n              kept steps the series hold (the same for every series; the host counts them)
 * With mu = total / n, H_k the sum of the first k head values and Z_k the sum of the last k ring values, the centred lagged sum
 * is  n c_k = acc[k] - mu (2 total - H_k - Z_k) + (n - k) mu^2  and rho_k = c_k / c_0 (victor_amd/autocorr.py reads it in extended
 * precision and applies Sokal's window).
 * The handle owns the state, (3 max_lag + 2) doubles per series: made and zeroed by vk_chain_set_autocorr (a second call replaces
 * it), zeroed again by vk_chain_start together with n, kept across blocks, freed by vk_chain_destroy.  max_lag == 0 clears it; a
 * handle that never had it, or had it cleared, makes the launches and returns the bytes it always did.
 * Refused (VK_E_ARG, vk_chain_last_error gives the text, the handle stays usable and keeps the state it had): a block begun and
 * not finished; group < 1 or n_chains % group != 0; max_lag outside 1..1024; vk_chain_autocorr on a handle without it.  Device
 * memory that cannot be had is reported as vk_chain_create reports it (VK_E_HIP); the handle then has no autocorrelation. */
int vk_chain_set_autocorr(vk_chain* f, int32_t group, int32_t max_lag);
int vk_chain_autocorr(vk_chain* f, double* pivot, double* total, double* head, double* ring, double* acc, int64_t* n);

/* ---- Replica exchange on a chain handle: tempered chains and the sums of thermodynamic integration ---------------------------
 * vk_chain_set_tempering reads the n_chains chains of any handle of the three chain create calls as n_chains / (rungs walkers)
 * problems of `rungs` inverse temperatures 1 = betas[0] > betas[1] > ... > betas[rungs - 1] >= 0 and `walkers` ladders each: chain
 * c = (r rungs + k) walkers + w is problem r, rung k, walker w.  A `group` of `walkers` (vk_chain_set_marginals,
 * vk_chain_set_autocorr) then sees every (r, k) as a problem.  vk_chain_begin_tempered is vk_chain_begin with three changes
 * (vk_temper_step.h states them, victor_amd/tempering.py is the definition):
 *   the step       a chain of rung k decides on  post = betas[k] * lnL (+ ln prior), product and sum each rounded:
 *                  accept <=> the proposal is inside the box and logu < post' - post (a NaN rejects).  At beta = 1 this is the
 *                  decision of vk_chain_begin bit for bit.  0 * -inf is NaN: at beta = 0 a proposal whose row failed is rejected,
 *                  and a chain whose stored lnL is -inf never moves by a step.  State, history and chi2 keep the log-likelihood.
 *   the energy     at every kept step, after the decision and before any swap, a chain whose stored lnL is finite adds it to its
 *                  sums: n_e += 1; the first such value becomes pivot_e; a = lnL - pivot_e; e1 += a; e2 += a * a (the product
 *                  rounded before the sum).  ln Z = the integral over beta of the rungs' mean lnL follows on the host.
 *   the swap       with swap_every > 0 a swap event follows the step with index s (first_step + its place in the block) when
 *                  (s + 1) % swap_every == 0; event e = (s + 1) / swap_every - 1 pairs rung k with rung k + 1, walker for walker
 *                  inside a problem, for every k = e % 2, e % 2 + 2, ... with k + 1 < rungs:
 *                  accept <=> logs < (betas[k] - betas[k + 1]) * (lnL_(k+1) - lnL_k), one subtraction each, one product, a NaN
 *                  rejects; logs is the entry of the lower rung's chain in the step's row of `logs`.  On accept the sampled
 *                  values, lnL and chi2 are exchanged; base rows, temperatures, pivots, moment sums, energy sums, histograms
 *                  and counters stay with the rung.  The lower chain counts n_swap_try and n_swap_acc.
 * logs is [n_steps][n_chains] like logu (the rows of steps without an event are not read; NULL is allowed with swap_every == 0);
 * everything else - up to 64 steps, asynchronous, first_step, burn, thin, want_history, n_kept, vk_chain_finish - is the contract
 * of vk_chain_begin.  A history slot holds the state after the decision and before the swap.  Launches: per step the evaluation
 * and the tempered step kernel; on a swap step that kernel writes no next rows, the swap kernel (one thread per candidate pair, no
 * atomics) and the propose kernel follow it.  vk_chain_tempering copies the sums out, between blocks; any pointer may be NULL;
 * every output is [n_chains].
 * The handle owns the arrays: made and zeroed by vk_chain_set_tempering (a second call replaces them), zeroed again by
 * vk_chain_start, kept across blocks, freed by vk_chain_destroy.  rungs == 0 clears the tempering; a handle that never had it, or
 * had it cleared, makes the launches and returns the bytes it always did.  vk_chain_begin on a handle with tempering steps every
 * chain at beta = 1 and swaps nothing.
 * Refused (VK_E_ARG, vk_chain_last_error gives the text, the handle stays usable and keeps what it had): a block begun and not
 * finished; rungs < 0, walkers < 1 or n_chains % (rungs walkers) != 0; betas[0] != 1; betas not strictly decreasing; a beta below
 * 0 or not finite; chains of one problem on different realisations; swap_every < 0; vk_chain_begin_tempered or
 * vk_chain_tempering on a handle without tempering.  Device memory that cannot be had is reported as vk_chain_create reports it
 * (VK_E_HIP); the handle then has no tempering. */
int vk_chain_set_tempering(vk_chain* f, int32_t rungs, int32_t walkers, const double* betas);
int vk_chain_begin_tempered(vk_chain* f, int32_t n_steps, const double* dz, const double* logu, const double* logs, int64_t swap_every,
                            int64_t first_step, int64_t burn, int64_t thin, int32_t want_history, int32_t* n_kept);
int vk_chain_tempering(vk_chain* f, double* pivot_e, double* e1, double* e2, int64_t* n_e, int64_t* n_swap_try, int64_t* n_swap_acc);

/* ---- Posterior-predictive sums of a chain handle: the model vector's band, mean chi-square and DIC ---------------------------
 * The runs above return everything about the parameters and nothing about the MODEL VECTOR: the posterior band of xi_0 / xi_2 /
 * xi_4 drawn through the data needs the theory vector at every kept position, which a run without a history no longer has and a
 * run with one would have to evaluate a second time.  The theory vector of every proposal is in device memory when its step is
 * decided; vk_chain_set_predictive makes vk_chain_begin and vk_chain_begin_stretch, on a handle of vk_chain_create, keep each
 * chain's current one and sum it at the kept steps (vk_predictive.h states the rules, victor_amd/predictive.py is the
 * definition).  Problem r owns the `group` chains c = r group + w; N is the length of the context's data vector.
 *   hold           held[c] is the theory vector at chain c's current position, seen[c] the chain's accept count when it was taken.
 *                  After vk_chain_start's evaluation every chain takes its row; after every decision - kept or not - a chain whose
 *                  accept count differs from seen[c] takes its row of the launch just decided (row c; in a stretch half-step the
 *                  row of the moving walker).  A rejected proposal and one outside the box leave held[c] alone.  The step
 *                  kernels are untouched: the accept counter is the hand-off.
 *   pivot          at vk_chain_start pivot_t[r][k] = held[r group][k] if finite, else 0; pivot_chi2 and pivot_lnl likewise from the
 *                  start of chain r group.
 *   kept step      (a kept sweep, after its second half) for w = 0 .. group - 1 in that order: if chi2[c] and lnL[c] are both
 *                  finite, v = held[c][k] - pivot_t[r][k], sum_t[r][k] += v, sum_tt[r][k] += v v for every k, chi2 and lnL likewise
 *                  into s_chi2, s_chi2sq, s_lnl, s_lnlsq about their pivots, n[r] += 1; otherwise n_skipped[r] += 1.  Plain double
 *                  sums in (step, walker) order - independent of how a run is cut into blocks; a product may be contracted into
 *                  an fma.
 * Launches: behind every step kernel (each half's, of a sweep) a hold kernel of one wave per row, before the next evaluation
 * overwrites the theory vectors; behind the hold of every kept step (a kept sweep's second half) a kernel of one thread per
 * (problem, entry).  No host synchronisation, no atomics.  On the data-vector route the evaluation is asked to store the theory
 * vectors its fused chi-square would not otherwise write: stores only, lnL keeps its bits.
 * vk_chain_predictive copies the state out, between blocks; any pointer may be NULL:
 *   pivot_t, sum_t, sum_tt   [n_chains / group][N]
 *   deviance       [n_chains / group][6]: pivot_chi2, pivot_lnl, s_chi2, s_chi2sq, s_lnl, s_lnlsq
 *   n, n_skipped   [n_chains / group]
 *   held           [n_chains][N]
 * The handle owns the state, (n_chains + 3 n_chains / group) N doubles and a few per problem and chain: made and zeroed by
 * vk_chain_set_predictive (a second call replaces it), after which the chains need a (new) vk_chain_start - the held vectors are
 * taken there; zeroed again by vk_chain_start, kept across blocks, freed by vk_chain_destroy.  group == 0 clears it; a handle that
 * never had it, or had it cleared, makes the launches and returns the bytes it always did.
 * Refused (VK_E_ARG, vk_chain_last_error gives the text, the handle stays usable and keeps the state it had): a block begun and
 * not finished; a handle of vk_chain_create_joint / _joint_blocks (its theory workspace is laid out by the route that evaluates
 * it); a handle with tempering, and vk_chain_set_tempering on a handle with predictive sums (a swap moves states without touching
 * the accept counters); group < 1 or n_chains % group != 0; vk_chain_predictive on a handle without it.  Device memory that cannot
 * be had is reported as vk_chain_create reports it (VK_E_HIP); the handle keeps the sums it had. */
int vk_chain_set_predictive(vk_chain* f, int32_t group);
int vk_chain_predictive(vk_chain* f, double* pivot_t, double* sum_t, double* sum_tt, double* deviance, int64_t* n, int64_t* n_skipped,
                        double* held);

/* ---- Hessians of lnL + ln prior at given points of a best-fit handle: Laplace covariances -----------------------------------
 * vk_fit_run returns a point per problem and nothing about its uncertainty.  vk_fit_hessian evaluates, on any handle of the
 * three vk_fit_create calls (before or after vk_fit_run; with the prior of vk_fit_set_prior, if any), one central-difference
 * stencil per problem - M = vk_hessian_rows(n_params) = 2 n_params^2 + 1 rows - around the point x_p with the steps h_p, and
 * from its values the Hessian of lnL + ln prior there and its negative inverse, the covariance of the local Gaussian
 * approximation of the posterior (vk_hessian.h states the stencil and every rounding; victor_amd/laplace.py restates it in
 * NumPy, bit for bit):
 *   point m     0: x;  1 + 2 j + s: x +- h_j e_j (s = 0: +);  1 + 2 d + 4 q + c: x_j and x_k displaced, q the pair j < k in the
 *               order (0,1), (0,2), .., (1,2), .., c = 0..3 the signs (+,+), (+,-), (-,+), (-,-); a displaced coordinate is the
 *               rounded sum.  Rows are formed on the device as the search forms them (epsilon -> aperp, apar; row sets).
 *   a           A = -H o (h h^T):  A_jj = ((v0 + v0) - v(+j)) - v(-j),  A_jk = 0.25 ((v(+-) - v(++)) + (v(-+) - v(--)))
 *   hess, cov   hess_jk = -A_jk / (h_j h_k);  cov_jk = (h_j h_k) B_jk with B = A^-1 through the Cholesky factor of A
 *   status      VK_HESS_AT_BOUND: some x_j - h_j < lo_j or x_j + h_j > hi_j, or x outside the box - the problem's rows are all
 *               evaluated at x (the launch shape never depends on the data) and a, hess, cov are NaN;  VK_HESS_NOT_FINITE: a
 *               value of the stencil is not finite (a, hess, cov NaN);  VK_HESS_NOT_POSDEF: a Cholesky pivot fails > 0 (a and
 *               hess given, cov NaN);  VK_HESS_OK otherwise - in this precedence.  The caller chooses the steps: the device
 *               only flags.
 *   x, h        [n_problems][n_params] each: the points and per-problem steps (> 0)
 *   values      [n_problems][M] the value of every stencil point: lnL of its row, plus ln prior at the point under a prior
 *   a, hess, cov  [n_problems][n_params][n_params], symmetric;  lnpost, chi2 [n_problems]: value and chi-square of the centre;
 *               status [n_problems].  Any output may be NULL.
 * The R M rows are evaluated in chunks of the handle's largest launch (n_problems S rows, S = max(4, n_params + 1): at most
 * ceil(M / S) <= 19 evaluations, chunk boundaries inside problems), with the launches vk_fit_run makes for as many rows; the
 * values and outputs live in an allocation of the call, freed before it returns.  Synchronous; the call owns the context as
 * vk_fit_run does.  On error the code is returned, vk_fit_last_error gives the text and nothing stays in flight.  Refused
 * (VK_E_ARG): what vk_fit_run refuses of the context, a NULL x or h, a point that is not finite, a step that is not finite
 * or <= 0.  A handle that never calls it makes the launches it made before and returns the bytes it returned. */
#define VK_HESS_OK 0
#define VK_HESS_AT_BOUND 1
#define VK_HESS_NOT_FINITE 2
#define VK_HESS_NOT_POSDEF 3
int64_t vk_hessian_rows(int32_t n_params);
int vk_fit_hessian(vk_fit* f, const double* x, const double* h, double* values, double* a, double* hess, double* cov,
                   double* lnpost, double* chi2, int32_t* status);

/* ---- Fisher matrices from model-vector Jacobians at given points of a best-fit handle: forecasts ----------------------------
 * vk_fit_hessian differentiates lnL twice against a data vector.  vk_fit_fisher answers the question asked before the data
 * exist: on any handle of the three vk_fit_create calls it evaluates one central-difference stencil of THEORY VECTORS per
 * problem - M = vk_fisher_rows(n_params) = 2 n_params + 1 rows, the first 2 n_params + 1 points of the Hessian's stencil -
 * around the point x_p with the steps h_p, and forms F = J^T P J with J = d(theory vector)/d(theta) and P the precision the
 * handle's chi-square uses at the centre's beta (vk_fisher.h states every order and rounding; victor_amd/fisher.py restates it
 * in NumPy, bit for bit).  No data vector and no realisation is read: a handle made against realisations only supplies
 * n_problems.
 *   vector      N entries: the context's; of a joint handle the blocks' vectors concatenated in block order
 *   D           D_ak = t_a(x + h_k e_k) - t_a(x - h_k e_k); the division by 2 h is folded into the scaling of the matrices
 *   P           a fixed covariance: its slice; a beta-gridded one: slice lo where the bracket's weight t is 0, else
 *               (1 - t) P_lo + t P_last, at the beta of the centre's row (a joint covariance: block 0's row; a block-diagonal
 *               joint fit: block-diagonal, each block bracketed at the beta of its own row)
 *   S           S_jk = sum_a D_aj (sum_b P_ab D_bk)
 *   scale       c = -2 dlnL/dchi2 at chi2 = 0 of the handle's likelihood form: gaussian 1, hartlap (nm - N - 2) / (nm - 1),
 *               sellentin nm / (nm - 1), percival m / (nm - 1) - exact where data = model
 *   fisher, a, cov   fisher_jk = (c / 4) S_jk / (h_j h_k): the likelihood's information;  A_jk = (c / 4) S_jk + Lambda_jk h_j h_k
 *               with Lambda the precision of the prior of vk_fit_set_prior (absent without one);  cov_jk = (h_j h_k) B_jk with
 *               B = A^-1 through the Cholesky factor of A
 *   status      the codes of vk_fit_hessian, in this precedence: VK_HESS_AT_BOUND (the stencil leaves the box or x is outside
 *               it: every row of the problem is formed at x; fisher, a, cov NaN), VK_HESS_NOT_FINITE (an entry of the M vectors
 *               is not finite; fisher, a, cov NaN), VK_HESS_NOT_POSDEF (a Cholesky pivot fails > 0 - a parameter the theory does
 *               not depend on gives S_jj = 0 exactly -: fisher and a given, cov NaN), VK_HESS_OK
 *   x, h        [n_problems][n_params]: the points and per-problem steps (> 0)
 *   vectors     [n_problems][M][N] the theory vector of every stencil row, or NULL: not downloaded
 *   fisher, a, cov   [n_problems][n_params][n_params], symmetric;  scale: one double;  status [n_problems].  Any output may be NULL.
 * The R M rows are evaluated theory-only, in chunks of the handle's largest launch (n_problems S rows, S = max(4, n_params + 1);
 * chunk boundaries inside problems), into an allocation of the call, [R M][N]; a joint handle makes one theory launch per block
 * and chunk on the block's stream, ordered against the lead's as the joint entry points order theirs.  One assemble kernel, a
 * workgroup per problem, holds 2 N n_params doubles in LDS: N n_params <= 10026, more is refused.  Synchronous; the call owns
 * the contexts as vk_fit_run does.  On error the code is returned, vk_fit_last_error gives the text and nothing stays in
 * flight.  Refused (VK_E_ARG): what vk_fit_hessian refuses (of the context, a NULL x or h, a point that is not finite, a step
 * that is not finite or <= 0), a vector too long for the LDS, and a block-diagonal joint handle whose blocks would take
 * different scales (hartlap / percival with blocks of different lengths).  A handle that never calls it makes the launches it
 * made before and returns the bytes it returned; the call changes nothing on the handle or its contexts. */
int64_t vk_fisher_rows(int32_t n_params);
int vk_fit_fisher(vk_fit* f, const double* x, const double* h, double* vectors, double* fisher, double* a, double* cov, double* scale,
                  int32_t* status);

/* ---- Grid posteriors: marginals, profile likelihoods and the evidence of every problem over one shared grid -----------------
 * The fits have two to four sampled parameters: a grid gives exact marginals, profiles and the evidence where chains, histograms,
 * Laplace and thermodynamic integration estimate them.  The reference has nothing of the kind (a user would loop
 * CCFFit.log_likelihood, victor/ccf_fit.py:356-483, over the nodes on the host).  A grid handle evaluates that lnL at the nodes of
 * a regular grid over d sampled parameters - against the context's data vector (one problem) or against EVERY realisation set on
 * the context (vk_set_realisations: R = n_real problems, each grid point's theory vector computed once for all of them, the cross
 * mode of vk_eval_realisations) - and reduces the values where they are produced; (G, R) values never travel to the host.
 * victor_amd/grid.py states the definition in NumPy, vk_grid.h the index rules and the step, DESIGN.md section 7c the mapping.
 *   columns[j]  row column (VK_P_*) of axis j, or VK_WALK_EPSILON, each once, 1 <= n_axes <= 10 (as vk_fit_create)
 *   bins[j]     nodes of axis j, 1 .. 1024; G = prod bins[j] <= 2^40.  Flat index g is ROW-MAJOR: the last axis varies fastest
 *   nodes       the node values of all axes, concatenated (sum bins[j] doubles, finite).  The caller's arrays are the definition:
 *               the device looks nodes up and never recomputes one
 *   eps_pow     [bins of the epsilon axis] the caller's own eps^(-2/3) of every node of an epsilon axis (NULL without one): the
 *               row kernel forms apar = alpha eps_pow, aperp = eps apar from it, so a device row equals the row the host forms
 *               (vk_epsilon_to_ap, CCFFit._fit_rows) BIT FOR BIT WITH EPSILON AS AN AXIS - unlike the best fits and chains above,
 *               whose rows use the device's pow.  A node whose eps_pow is NaN (eps < 0) gives a row that fails: lnL = -inf
 *   base_row    [VK_NPAR] the fixed parameters and defaults;  alpha as vk_fit_create
 *   every_realisation   0: the context's data vector, R = 1;  else every realisation set on the context, R = n_real (a context
 *               with model realisations, vk_set_model_realisations, is refused: a point has one theory vector there per realisation)
 *   pairs       [n_pairs][2] axis pairs (a < b) for the two-dimensional products, at most 45, each axis of a pair at most 128 bins
 *   chunk       grid points per launch, 1 .. 65536: the handle's one device allocation holds rows, workspace and two [chunk][R]
 *               arrays
 * lnpost[g][r] = lnL[g][r], plus ln prior at the point under vk_grid_set_prior (mu, pp_packed as vk_fit_set_prior; one rounded
 * addition); a value that is not finite counts as -inf.  The chunks [c chunk, min((c + 1) chunk, G)) go in order; per chunk and
 * problem, with M the running maximum (-inf at the start):
 *   M' = max(M, max_g lnpost[g]); arg_max moves on a strict increase only, to the smallest such g; M' = -inf: nothing else happens
 *   M' > M: total, m1, m2 of the problem are multiplied by exp(M - M') (exp(-inf) = 0), then M = M'
 *   every accumulator adds exp(lnpost[g] - M) for its g of the chunk, ONE AT A TIME IN INCREASING g from its own value - no
 *   pairwise or tree sums, no floating-point atomics -; p1, p2 take the maximum of lnpost; n_finite counts
 * so maxima, arg max and counts do not depend on the chunk, sums depend on it through rounding only, and for a given chunk the
 * bytes depend neither on how vk_grid_run calls cut the run nor on anything timed.
 * vk_grid_run(h, first, count) enqueues the whole chunks of flat indices [first, min(first + count, G)) on the context's stream -
 *   per chunk a rows kernel, the evaluation (the launches vk_eval_batch / vk_eval_realisations make for as many rows), and the
 *   max, weight and accumulate kernels, no host synchronisation between chunks - and waits once at its end.  first is a multiple
 *   of chunk: 0 starts a new run (the accumulators are reset), otherwise where the last call ended; count is whole chunks or
 *   reaches G.  Resumable: a long grid reports progress between calls.
 * vk_grid_rows(h, first, count, rows) forms the rows of flat indices first .. first + count - 1 (count <= chunk) as vk_grid_run
 *   forms them and copies them home, [count][VK_NPAR]; nothing is evaluated.
 * vk_grid_result, after a run has reached G, per problem r: ln_max [R] the largest lnpost (-inf: no node was finite), arg_max [R]
 *   the smallest flat index attaining it (-1), total [R] = sum_g exp(lnpost_g - ln_max), n_finite [R], m1 / p1 [R][sum bins] the
 *   weight sum and the lnpost maximum over the cells of every node of every axis (axis j at sum_{i<j} bins[i]), m2 / p2
 *   [R][sum_pairs bins_a bins_b] the same per pair, [ka][kb];  prior_ln_max, prior_total: under a prior the same two numbers of
 *   lnpost = ln prior alone - the Gaussian's own midpoint sum over the grid, accumulated by the same kernels as one more problem -
 *   else 0.  Any output may be NULL.
 * Synchronous calls that own the context while they run.  On error the code is returned, vk_grid_last_error gives the text and
 * nothing stays in flight.  Refused (VK_E_ARG): what vk_fit_run refuses of the context, another number of realisations on the
 * context than at vk_grid_create, a first that is not where the run stands, a result before the run is complete;
 * vk_grid_set_prior moves the run back to its start. */
typedef struct vk_grid vk_grid;
vk_grid* vk_grid_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_axes, const int32_t* columns, const int32_t* bins,
                        const double* nodes, const double* eps_pow, const double* base_row, double alpha,
                        int32_t every_realisation, int32_t n_pairs, const int32_t* pairs, int32_t chunk, char* err, size_t errlen);
int vk_grid_set_prior(vk_grid* h, const double* mu, const double* pp_packed);
int vk_grid_run(vk_grid* h, int64_t first, int64_t count);
int vk_grid_rows(vk_grid* h, int64_t first, int32_t count, double* rows);
int vk_grid_result(vk_grid* h, double* ln_max, int64_t* arg_max, double* total, int64_t* n_finite, double* m1, double* p1,
                   double* m2, double* p2, double* prior_ln_max, double* prior_total);
const char* vk_grid_last_error(const vk_grid* h);
void vk_grid_destroy(vk_grid* h);

/* ---- Importance-sampled posteriors: the evidence, the effective sample size, moments and marginal histograms of every problem --
 * from ONE shared sample.  G points drawn once from a proposal that covers every problem's posterior are evaluated once - against
 * the context's data vector (one problem) or against EVERY realisation set on the context (R = n_real problems, the cross mode of
 * vk_eval_realisations) - and reduced where the values are produced; (G, R) values never travel to the host.  The reduction is
 * the grid's step (vk_grid_run above) generalised from lattice nodes to scattered points: what the lattice gave for free - the
 * cells' run patterns, nodes looked up by index, no proposal density - the caller states.  victor_amd/importance.py states the
 * definition in NumPy, vk_importance.h the accumulator index rules, the list walk and the terms, DESIGN.md section 7e the mapping.
 *   columns[j]  row column (VK_P_*) of axis j, or VK_WALK_EPSILON, each once, 1 <= n_axes <= 10 (as vk_fit_create)
 *   n_points    G, 1 .. 2^24: the points kept, in the order they were drawn
 *   x, y        [G][n_axes] the points and their centred coordinates y = x - centre the moments use (finite)
 *   eps_pow     [G] the caller's own eps^(-2/3) of every point when epsilon is sampled (NULL otherwise): a device row equals the
 *               row the host forms (CCFFit._fit_rows) bit for bit, as with vk_grid_create
 *   lno         [G] ln prior(x_g) - ln q(x_g), added to lnL once;  lno_prior [G] or NULL: lnpost of the prior's own problem,
 *               which rides along as problem R and keeps a total alone
 *   n_bins[j]   bins of axis j's histogram, 1 .. 1024: n_bins[j] + 2 cells (below the range, the bins, above it)
 *   pair_bins[q]  bins per axis of pair q's two-dimensional histogram, 1 .. 128: pair_bins[q]^2 cells; at most 45 pairs
 *   lists       [n_axes + n_pairs][G]: per list (the axes, then the pairs) and chunk c the chunk's segment starts at c chunk; it
 *               names the chunk's points (g - c chunk) cell by cell, increasing inside a cell.  A point outside either range of a
 *               pair is in none of the pair's cells
 *   offsets     [chunks][cells + lists]: per chunk, list after list, one offset more than the list has cells: cell k of the list
 *               holds entries off[k] .. off[k + 1] - 1 of the chunk's segment.  vk_is_create checks every index a kernel will
 *               form: offsets that start at 0, never decrease and end inside the chunk's points, entries inside the chunk that
 *               increase inside a cell
 *   base_row, alpha, every_realisation, chunk: as vk_grid_create
 * lnpost[g][r] = lnL[g][r] + lno[g], one rounded addition; a value that is not finite counts as -inf.  The chunks go in order and
 * per chunk and problem the step is vk_grid_run's - the running maximum M, arg_max on a strict increase to the smallest g, every
 * accumulator multiplied by exp(M - M') when M rises (the sum of squares twice, each product rounded), w = exp(lnpost - M) - with
 * the additions ONE AT A TIME IN INCREASING g:  total += w;  sq += w w;  s1[j] += w y_j;  s2[j][k] += (w y_j) y_k, j <= k;  every
 * histogram and pair cell += w over its list.  No pairwise or tree sums, no floating-point atomics: maxima, arg max and counts do
 * not depend on the chunk, sums depend on it through rounding only, and two runs give the same bytes.
 * vk_is_run(h, first, count), vk_is_rows(h, first, count, rows): as vk_grid_run and vk_grid_rows, over points for flat indices.
 * vk_is_result, after a run has reached G, per problem r: ln_max, arg_max, n_finite, total, sq [R]; s1 [R][d]; s2
 *   [R][d (d + 1) / 2], the packed upper triangle row by row; h1 [R][sum (n_bins[j] + 2)], axis after axis; h2
 *   [R][sum pair_bins[q]^2];  prior_ln_max, prior_total: the two numbers of the prior's own problem, else 0.  Any may be NULL.
 * Synchronous calls that own the context while they run.  On error the code is returned, vk_is_last_error gives the text,
 * nothing stays in flight and the handle stays usable.  Refused (VK_E_ARG): what vk_grid_run refuses. */
typedef struct vk_is vk_is;
vk_is* vk_is_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_axes, const int32_t* columns, int64_t n_points, const double* x,
                    const double* y, const double* eps_pow, const double* lno, const double* lno_prior, const int32_t* n_bins,
                    int32_t n_pairs, const int32_t* pair_bins, const int32_t* lists, const int32_t* offsets, const double* base_row,
                    double alpha, int32_t every_realisation, int32_t chunk, char* err, size_t errlen);
int vk_is_run(vk_is* h, int64_t first, int64_t count);
int vk_is_rows(vk_is* h, int64_t first, int32_t count, double* rows);
int vk_is_result(vk_is* h, double* ln_max, int64_t* arg_max, int64_t* n_finite, double* total, double* sq, double* s1, double* s2,
                 double* h1, double* h2, double* prior_ln_max, double* prior_total);
const char* vk_is_last_error(const vk_is* h);
void vk_is_destroy(vk_is* h);
/* Posterior-predictive sums of the sample (victor_amd/csrc/vk_is_predict.h; the definition: victor_amd/importance.py): per problem
 * the weighted first and second sums of the points' THEORY VECTORS and of their chi2 and lnL, taken from what every chunk leaves
 * on the device - one more launch per chunk (of a joint handle one per block), no further theory evaluation.
 * vk_is_set_predictive(h, on): before the first vk_is_run (a completed run's results are dropped: the next run starts at point
 *   0); on != 0 allocates the state beside the handle's allocation - (1 + 2 R) N + 6 R + chunk R doubles, N the entries of a
 *   theory vector, of a joint handle the sum of the blocks' - and makes the evaluation keep the points' vectors, which changes no
 *   bit of lnL, of chi2 or of anything vk_is_result returns; on == 0 releases it, and the handle allocates and launches what it
 *   did before.  Refused: a run under way; a block whose theory vector has more than 2^17 entries.
 * The rules, per chunk: pivot_t = the theory vector of point 0 where finite, else 0 (one vector for all problems; of a joint
 *   handle the blocks' vectors in block order); pivot_chi2[r], pivot_lnl[r] = chi2 and lnL of point 0 for problem r where finite,
 *   else 0.  Every sum is multiplied ONCE by the chunk's factor exp(M - M'); then every point with w > 0 adds, with v = T - pivot_t,
 *   a = chi2 - pivot_chi2[r], b = lnl - pivot_lnl[r]:  w v and (w v) v per entry;  w a, (w a) a, w b, (w b) b.  A point of weight 0
 *   adds nothing.  Each difference and product is rounded on its own; the additions run in a fixed order of the kernel's (four
 *   slices of the chunk, combined in slice order), so two runs give the same bytes, and the sums agree with the definition's
 *   (increasing g) to rounding.  The prior's own problem keeps no such sums.
 * vk_is_predictive, after a run has reached G: pivot_t [N]; sum_t, sum_tt [N][R] - entry k of problem r at k R + r -; pivots
 *   [2][R]: pivot_chi2 | pivot_lnl; deviance [4][R]: sum w a | sum (w a) a | sum w b | sum (w b) b.  Any may be NULL.  The sums are
 *   in units of the weights of vk_is_result: divide by total[r]. */
int vk_is_set_predictive(vk_is* h, int32_t on);
int vk_is_predictive(vk_is* h, double* pivot_t, double* sum_t, double* sum_tt, double* pivots, double* deviance);
/* The tail of the sample (victor_amd/csrc/vk_is_tail.h; the definition: victor_amd/importance.py, rule 7): per problem the K
 * largest finite lnpost[g][r] of the WHOLE sample with their points g - what a Pareto fit to the largest weights and the smoothed
 * estimates built on it need (PSIS), selected while the chunks stream by: two more launches per chunk behind the max kernel, no
 * host synchronisation, and (G, R) values still never travel.  lnpost is the value above (one addition; not finite: never held).
 * The order is total - the larger lnpost first, between equal values the smaller g first - so the held entries and their order
 * are unique: they depend neither on the chunk nor on anything timed, and two runs give the same bytes.  The prior's own problem
 * keeps no tail.
 * vk_is_set_tail(h, K): before the first vk_is_run (a completed run's results are dropped: the next run starts at point 0);
 *   2 <= K <= min(4096, G) allocates the state beside the handle's allocation - per problem 2 K + 1 doubles and 2 K + chunk +
 *   258 32-bit words - and changes no bit of anything vk_is_result or vk_is_predictive returns; K == 0 releases it, and
 *   the handle allocates and launches what it did before.  Refused: a run under way; any other K.
 * vk_is_tail, after a run has reached G: count [R] = min(K, n_finite[r]); lnpost [R][K] the held values in order, -inf behind
 *   the count; index [R][K] their points, -1 behind the count.  Any may be NULL.  Refused: a handle without the state, a run
 *   that is not complete. */
int vk_is_set_tail(vk_is* h, int32_t K);
int vk_is_tail(vk_is* h, double* lnpost, int64_t* index, int64_t* count);
/* A proposal per problem (victor_amd/csrc/vk_kernel_is_own.h; the definition: victor_amd/importance.py, rule 8): R problems, each
 * with G points of its OWN - drawn from its own proposal, a best fit with its Laplace covariance, say - and evaluated against
 * realisation which[r] alone: point g of problem r is row g R + r of a pairs-mode evaluation, so a run costs G R theory
 * evaluations.  A context with model realisations set (vk_set_model_realisations) is accepted, as vk_nested_create and
 * vk_chain_create accept it: row g R + r is then evaluated with the model of realisation which[r].
 * Arguments as vk_is_create, with the problem the fastest-varying index of everything that was one value per point:
 *   n_points    G, the points of EVERY problem;  n_problems R;  which [R], each in 0 .. n_real - 1
 *   x, y        [G][R][n_axes];   eps_pow, lno, lno_prior [G][R].  lno may be -inf: a point the caller drew outside the prior
 *               box, whose x the caller has replaced by a point inside (it is evaluated, weighs nothing and is in no list)
 *   lists       [R][n_axes + n_pairs][G]: problem r's lists, each as vk_is_create's
 *   offsets     [chunks][R][cells + lists]: per chunk, problem after problem; chunks x R x (cells + lists) <= 2^27
 *   chunk       points of every problem per launch: chunk x R <= 65536 rows;  G x R <= 2^24
 * Every index a kernel will form is checked as vk_is_create checks it, per problem; refused with text in err besides: an index of
 * which outside the context's realisations; G x R or chunk x R above their limits; model realisations whose number differs from
 * the data realisations'.  With lno_prior problem r has a prior problem of its own (lnpost = lno_prior[g][r], a total alone).
 * vk_is_run, _result, _set_tail, _tail, _last_error and _destroy serve the handle as they serve vk_is_create's, per problem r over
 * its own points; vk_is_rows(first, count) returns count x R rows, row i R + r point first + i of problem r; vk_is_result writes
 * R values to prior_ln_max and to prior_total; vk_is_set_predictive is refused (VK_E_ARG). */
vk_is* vk_is_create_own(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_axes, const int32_t* columns, int64_t n_points,
                        int32_t n_problems, const int32_t* which, const double* x, const double* y, const double* eps_pow,
                        const double* lno, const double* lno_prior, const int32_t* n_bins, int32_t n_pairs, const int32_t* pair_bins,
                        const int32_t* lists, const int32_t* offsets, const double* base_row, double alpha, int32_t chunk, char* err,
                        size_t errlen);

/* ---- nested sampling: the evidence and a posterior sample of the data vector or of every realisation ---------------------------
 * R problems of L live points each inside the box [lo, hi]; per iteration the K lowest live points of every problem die and K
 * walkers, each started at a surviving live point, take S constrained random-walk steps and replace them.  The handle is one of
 * R K rows: row r K + k of EVERY launch it makes is walker k of problem r (base_rows, which: one entry per row, as
 * vk_chain_create; the K rows of a problem name one realisation).  victor_amd/nested.py states the loop in NumPy - that is the
 * definition, reproduced bit for bit with epsilon fixed -, vk_nested_step.h the rules, DESIGN.md section 7d the mapping.
 *   n_rows      R K, at most 65536;  n_live L, 2 .. 4096;  batch K, a divisor of L with K <= L / 2;  steps S, 1 .. 1024
 *   scale       the proposal of a step is  y_j + (scale range_j) dz_j,  range_j = max - min of parameter j over the problem's L
 *               live points at the start of the iteration; each product and the sum rounded on its own
 *   n_params, columns, lo, hi, base_rows, alpha, which (and ctxs, cov, param_block of the joint forms): as vk_chain_create
 * vk_nested_start(h, x0): x0 [R][L][d], inside the box.  L / K launches evaluate the points: row r K + k of pass p is live point
 *   p K + k of problem r.  A NaN lnL is stored as -inf.  Fresh counters.  Synchronous.
 * vk_nested_begin(h, n_iter, pick, dz, first_iter, keep_dead) enqueues 1 <= n_iter <= 8 iterations, first_iter the number of
 *   iterations finished since the start: pick [n_iter][R K] in [0, 1), dz [n_iter][S][R K][d].  Per iteration and problem: the K
 *   live points smallest in (lnL, index) are dead points 0 .. K - 1 in that order (ties go to the smaller index), L* the lnL of
 *   the last; walker k starts at survivor min(floor(pick (L - K)), L - K - 1) of the L - K others in increasing index; a step is
 *   accepted when its proposal lies inside the box and lnL' > L* (strict; a NaN rejects), a proposal outside the box is
 *   evaluated at the walker's position and discarded; after step S walker k takes the slot of dead point k.  No host
 *   synchronisation inside the block.
 * vk_nested_finish(h, dead_lnl, dead_chi2, dead_x, live_lnl) waits and copies home the block's dead record [n_iter][R][K]
 *   (dead_x [n_iter][R][K][d]: what keep_dead asked for, else unspecified) and the live lnL [R][L] behind it.  Any may be NULL.
 * vk_nested_state(h, x, lnl, chi2, n_accept, n_steps, n_stuck): the live points [R][L][d], [R][L] and per problem [R] the
 *   accepted steps, the steps and the walkers that never moved in their iteration (they leave a duplicate).  Any may be NULL.
 * On error the code is returned, vk_nested_last_error gives the text and nothing stays in flight.  Refused (VK_E_ARG): what
 * vk_chain_begin refuses of the context, a block out of order, a start outside the box, a second begin before the finish. */
typedef struct vk_nested vk_nested;
vk_nested* vk_nested_create(vk_ctx* ctx, const vk_eval_opts* opts, int32_t n_rows, int32_t n_live, int32_t batch, int32_t steps,
                            double scale, int32_t n_params, const int32_t* columns, const double* lo, const double* hi,
                            const double* base_rows, double alpha, const int32_t* which, char* err, size_t errlen);
int vk_nested_start(vk_nested* h, const double* x0);
int vk_nested_begin(vk_nested* h, int32_t n_iter, const double* pick, const double* dz, int64_t first_iter, int32_t keep_dead);
int vk_nested_finish(vk_nested* h, double* dead_lnl, double* dead_chi2, double* dead_x, double* live_lnl);
int vk_nested_state(vk_nested* h, double* x, double* lnl, double* chi2, int64_t* n_accept, int64_t* n_steps, int64_t* n_stuck);
const char* vk_nested_last_error(const vk_nested* h);
void vk_nested_destroy(vk_nested* h);

/* A Gaussian prior on a nested handle (of any of its three create calls): ln prior = -1/2 (x - mu)^T P (x - mu) of vk_prior.h,
 * multiplied onto the box.  The run still samples the uniform box; it orders, kills and constrains on lnpost = lnL + ln prior
 * (one rounded addition): the dead points are the K smallest in (lnpost, index), L* is the lnpost of the last, and a step is
 * accepted when its proposal lies inside the box and lnL' + lnprior(proposal) > L*.  dead_lnl and live_lnl keep holding lnL.
 * vk_nprior_set(h, mu, pp): mu [d], pp [d (d + 1) / 2] as vk_chain_set_prior takes them; (NULL, NULL) clears the prior.  The
 *   live points of a start carry the ln prior they were started under, so an accepted call ends the start: the next call is the
 *   start of a run, and a begin before it is refused.  Refused (VK_E_ARG, the handle usable and unchanged): a block in flight,
 *   one pointer NULL, a value that is not finite.
 * vk_nprior_record(h, n_iter, dead_lnprior, live_lnprior): after the finish of a block of n_iter iterations and before the next
 *   begin, the block's ln prior record [n_iter][R][K] and the live points' [R][L].  Either may be NULL.  Refused: a handle
 *   without a prior or without a start, a block in flight, an n_iter that is not the finished block's. */
int vk_nprior_set(vk_nested* h, const double* mu, const double* pp);
int vk_nprior_record(vk_nested* h, int32_t n_iter, double* dead_lnprior, double* live_lnprior);

/* Theory multipoles on a caller-supplied s grid: out[n][n_ell][n_s] with the caller's own
 * projection weights w_ell[n_ell][n_mu] on mu[n_mu] (host buffers). */
int vk_theory_batch(vk_ctx* ctx, const vk_eval_opts* opts, const double* params, int64_t n,
                    const double* s, int32_t n_s, const double* mu, int32_t n_mu,
                    const double* w_ell, int32_t n_ell, double* out);

/* xi^s(mu_i, s_j) for every point: out[n][n_mu][n_s] (host buffers). */
int vk_xi_smu_batch(vk_ctx* ctx, const vk_eval_opts* opts, const double* params, int64_t n,
                    const double* s, int32_t n_s, const double* mu, int32_t n_mu, double* out);

/* ---- device-resident variants (inputs/outputs already in HBM) ----------------------- */
void* vk_device_alloc(vk_ctx* ctx, size_t bytes);
void vk_device_free(vk_ctx* ctx, void* ptr);
int vk_memcpy_h2d(vk_ctx* ctx, void* dst, const void* src, size_t bytes);
int vk_memcpy_d2h(vk_ctx* ctx, void* dst, const void* src, size_t bytes);
/* enqueue on the context's stream; d_theory_ws is a device workspace of n*N doubles.  With d_lnl or d_chi2 given it is SCRATCH:
 * its contents after the call are unspecified (a launch that takes the chi-square inside the theory kernel never writes the
 * theory vectors to HBM).  With d_lnl = d_chi2 = NULL the theory vectors [n][N] are the result and are left in d_theory_ws. */
int vk_eval_batch_device_async(vk_ctx* ctx, const vk_eval_opts* opts, const double* d_params,
                               int64_t n, double* d_lnl, double* d_chi2, double* d_theory_ws);
int vk_sync(vk_ctx* ctx);

/* ---- joint fit of several data vectors sharing one parameter batch (block-diagonal covariance) ----------------------
 * BASELINE config 5 (density-split quantiles: five CCFFit-equivalents, N = 5 x 120): the reference has no joint class
 * (density-split centres are only mentioned, victor/ccf_model.py:28-30); with a block-diagonal covariance chi2 and lnL of
 * the blocks add.  One context per block, all on one device; ONE parameter upload, every block's two kernels enqueued on its
 * own stream behind the lead context's stream (the launches overlap on the GPU), lnL and chi2 summed on the device in block
 * order; a block that fails its guards (-inf, inf) fails the point.  Enqueued; vk_sync(ctxs[0]) waits for the result.
 * d_ws: vk_joint_workspace_doubles(...) doubles of device memory. */
size_t vk_joint_workspace_doubles(vk_ctx* const* ctxs, int32_t n_ctx, int64_t n);
int vk_joint_eval_device_async(vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts, const double* d_params,
                               int64_t n, double* d_lnl, double* d_chi2, double* d_ws);
/* The same with a row set per block (per-block nuisance parameters: a sigma_v of each quantile's own): d_params holds n_ctx sets
 * of n rows and block q's launches read d_params + q * par_stride (par_stride in doubles, 0 or >= n * VK_NPAR).  par_stride == 0
 * is the call above - it IS that call: the same launches on the same rows.  Block-diagonal, every block reads every column,
 * beta included, from its own rows. */
int vk_joint_eval_blocks_device_async(vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts, const double* d_params,
                                      int64_t par_stride, int64_t n, double* d_lnl, double* d_chi2, double* d_ws);

/* ---- joint fit under ONE covariance matrix across the data vectors ---------------------------------------------------
 * The quantiles of a density-split analysis share their galaxies and voids: their data vectors are correlated and the
 * covariance estimated from mocks is one dense (NT x NT) matrix, NT = sum of the blocks' N.  The joint vector is the blocks'
 * data vectors concatenated in block order; with it the evaluation is CCFFit's (victor/ccf_fit.py:325-483) on that vector:
 * r = concat_q (t_q - d_q(beta)), chi2 = r^T Psi(beta) r, the covariance bracket of ccf_fit.py:213-228 across the slices, -1/2
 * log det C(beta) for a beta-dependent covariance (the generalised-eigenvalue scheme of vk_tables.logdet / eig) and the
 * likelihood form with p = NT.  The blocks' own covariances (vk_tables.prec ...) are not used.
 *
 * vk_joint_cov_tables: n_blocks (<= 32) block sizes in block order; n_beta = 0 for one fixed precision matrix prec [NT][NT],
 *   else the strictly increasing grid beta [n_beta], the precision slices prec [n_beta][NT][NT], logdet [n_beta] (NaN where
 *   the slice's determinant is not positive) and eig [n_beta][NT] (the factors of vk_tables.eig; a NaN row fails every
 *   blended evaluation that starts from its slice).
 * vk_joint_cov_create copies the tables to lead's device and returns the handle in *out; errors (VK_E_ARG, VK_E_HIP, VK_E_NOMEM)
 *   are reported through vk_last_error(lead).  vk_joint_cov_destroy waits for the evaluations that read the handle, not for
 *   other work on the device.  The handle may be used with any contexts on that device whose N match the block sizes, lead first.
 * vk_joint_cov_eval_device_async: every block's theory launch (theory only) on its own stream behind the lead stream, then the
 *   joint chi-square kernel on the lead stream; lnl / chi2 [n] (either may be NULL, not both).  Enqueued; vk_sync(ctxs[0])
 *   waits for it.  d_ws: vk_joint_cov_workspace_doubles(...) doubles of device memory. */
typedef struct vk_joint_cov_tables {
  int32_t n_blocks;
  const int32_t* block_n;    /* [n_blocks] */
  int32_t n_beta;            /* 0: fixed covariance */
  const double* beta;        /* [n_beta] */
  const double* prec;        /* [max(n_beta, 1)][NT][NT] */
  const double* logdet;      /* [n_beta] */
  const double* eig;         /* [n_beta][NT] */
} vk_joint_cov_tables;

typedef struct vk_joint_cov vk_joint_cov;

int vk_joint_cov_create(vk_ctx* lead, const vk_joint_cov_tables* tables, vk_joint_cov** out);
void vk_joint_cov_destroy(vk_joint_cov* h);
size_t vk_joint_cov_workspace_doubles(const vk_joint_cov* h, int64_t n);
int vk_joint_cov_eval_device_async(vk_joint_cov* h, vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts,
                                   const double* d_params, int64_t n, double* d_lnl, double* d_chi2, double* d_ws);
/* The same with a row set per block, as vk_joint_eval_blocks_device_async takes them: block q's theory launch reads d_params +
 * q * par_stride; par_stride == 0 is the call above.  UNDER A JOINT COVARIANCE BETA OF A POINT IS READ FROM BLOCK 0'S ROW: the
 * joint chi-square kernel brackets the covariance slices, takes -1/2 log det C(beta) and interpolates every block's data vector
 * with that one beta.  A block's own beta column reaches its theory launch only; callers that grid the covariance in beta keep
 * beta the same in every block's row. */
int vk_joint_cov_eval_blocks_device_async(vk_joint_cov* h, vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts,
                                          const double* d_params, int64_t par_stride, int64_t n, double* d_lnl, double* d_chi2,
                                          double* d_ws);

/* ---- joint fit under ONE covariance against many simulation realisations of every block --------------------------------
 * Validating a density-split pipeline on the mocks its joint covariance was estimated from: joint realisation m is realisation
 * m of EVERY block, each read from that block's own stacked file as simulation_number reads it (victor/ccf_fit.py:59-61,93-100),
 * and the joint vector is evaluated as vk_joint_cov_eval_device_async evaluates it (victor/ccf_fit.py:325-483 on the
 * concatenation: the bracket rule of :213-228, -1/2 log det C(beta) of :444-451, the likelihood forms of :455-473 with p = NT,
 * the (-inf, inf) guards of :448-450, 477-481).  The theory vectors do not depend on the realisation: each chunk of points runs
 * every block's theory launch once (theory only, on its own stream), then one chi-square kernel over the (point, realisation)
 * pairs; -1/2 log det is taken once per point.
 * vk_joint_cov_eval_realisations: the realisations of block q are those set on ctxs[q] with vk_set_realisations; every context
 *   must hold the same n_real.  which == NULL - every point against every realisation, lnl / chi2 [n][n_real]; otherwise
 *   which[i] is the realisation (0 .. n_real-1) of point i and lnl / chi2 are [n].  Both modes return the same bits for the same
 *   (point, realisation).  Either output may be NULL.  Host buffers, synchronous; large batches are cut into launches whose
 *   outputs stay below 256 MB.  VK_E_ARG for the checks of vk_joint_cov_eval_device_async, a context without realisations,
 *   contexts with different n_real and an index of which out of range. */
int vk_joint_cov_eval_realisations(vk_joint_cov* h, vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts,
                                   const double* params, int64_t n, const int32_t* which, double* lnl, double* chi2);
/* The same with a row set per block: params [n_ctx][n][VK_NPAR] (host), block q's rows at params + q * n * VK_NPAR.  The points
 * are cut into the chunks of the call above (at most 65536 points) and each block's slice of a chunk is uploaded for that block's
 * theory launch; beta of a point is block 0's (vk_joint_cov_eval_blocks_device_async).  With the same rows in every set it
 * returns the bits of the call above. */
int vk_joint_cov_eval_realisations_blocks(vk_joint_cov* h, vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts,
                                          const double* params, int64_t n, const int32_t* which, double* lnl, double* chi2);

/* ---- best fits and Metropolis chains of a joint fit: the data vectors, or every joint realisation ------------------------
 * The handles of the two sections above over a joint fit instead of one context: a problem (a chain) samples ONE parameter row
 * for all blocks - or, made by the _blocks forms below, a row per block - and every other call of those sections (run, start,
 * begin, begin_stretch, finish, state, last_error, destroy) serves the handle unchanged.  ctxs [n_ctx]: the blocks' contexts, lead first, all on one device, each with a data vector.
 *   cov == NULL   block-diagonal: lnL and chi2 of the blocks add in block order and a failed block fails the row, the rule of
 *                 vk_joint_eval_device_async;
 *   otherwise     the joint vector under the handle's covariance, ctxs[0] the context it was created with and the blocks'
 *                 sizes the handle's, as vk_joint_cov_eval_device_async checks them.
 *   which == NULL the blocks' own data vectors; otherwise problem i runs against joint realisation which[i] - realisation
 *                 which[i] of EVERY block (vk_set_realisations on each context, the same n_real on all of them).
 * The other arguments and every check are those of the single-context forms, applied to every context.  An evaluation makes
 * the launches of the joint entry points - block-diagonal against realisations: each block's theory and realisation chi-square
 * launches on its own stream (pairs mode) and the block-order sum behind them; under a covariance: the launches of
 * vk_joint_cov_eval_realisations in pairs mode - enqueued on the blocks' streams with the loop on the lead's: no host
 * synchronisation and no graph inside an iteration or a block of steps, and the same bits as those entry points return for
 * the same rows in the same launches.  Block-diagonal against realisations no host entry point makes these launches: each
 * block's pair is that of vk_eval_realisations in pairs mode, and the device's block-order sum returns the bits of the same sum
 * of those results in IEEE doubles on the host (0 + a_0 + a_1 + ...; a non-finite lnL reads -inf, inf).
 * Refused with NULL and the text in err: a NULL entry of ctxs, contexts on different devices, a context without a data vector,
 * a block count or size that differs from the handle's, (with which) a context without realisations or with another n_real, an
 * index out of range, a joint vector that needs more than 160 KiB of LDS. */
vk_fit* vk_fit_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                            int32_t n_problems, int32_t n_params, const int32_t* columns, const double* lo, const double* hi,
                            const double* base_rows, double alpha, const int32_t* which, char* err, size_t errlen);
vk_chain* vk_chain_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                int32_t n_chains, int32_t n_params, const int32_t* columns, const double* lo, const double* hi,
                                const double* base_rows, double alpha, const int32_t* which, char* err, size_t errlen);
/* Per-block nuisance parameters.  The quantiles of a density split share fsigma8, beta and epsilon; each has a velocity
 * dispersion (a bias, an Av) of its own.  The _blocks forms keep a ROW PER BLOCK for every problem (chain):
 *   param_block [n_params]  -1: sampled parameter j is written to every block's row; q (0 .. n_ctx - 1): to block q's row alone.
 *                A (column, block) pair is named once, and a column is either shared or per block, not both; VK_WALK_EPSILON
 *                counts as a column (an epsilon per block sets that block's aperp / apar / epsilon).
 *   base_rows    [n_ctx][n][VK_NPAR]: the fixed parameters and defaults of block q's rows at base_rows + q * n * VK_NPAR (a
 *                parameter fixed at a value per block differs between the sets).
 * Everything else is the call above, and 1 <= n_params <= 10 still counts every sampled value: five quantiles with one
 * nuisance parameter each, fsigma8 and epsilon are 7.  The rows are formed on the device by the one routine the other handles
 * use (vk_sampled_row.h over the selection rule of vk_row_select.h) and evaluated through
 * vk_joint_eval_blocks_device_async / vk_joint_cov_eval_blocks_device_async and their twins against realisations, so the bits are
 * those entry points' for the same rows in the same launches; with every param_block -1 and the same base rows in every set they
 * are the bits of a handle of vk_*_create_joint.  Under a covariance handle beta of a row is block 0's.
 * Refused in addition: param_block NULL or outside -1 .. n_ctx - 1, a (column, block) pair named twice, a column both shared and
 * per block, and VK_P_BETA per block under a handle gridded in beta (n_beta > 0).
 * Not offered: more than 10 sampled values, a beta per block under a covariance gridded in beta, blocks that cannot share one
 * option block. */
vk_fit* vk_fit_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                   int32_t n_problems, int32_t n_params, const int32_t* columns, const int32_t* param_block,
                                   const double* lo, const double* hi, const double* base_rows, double alpha, const int32_t* which,
                                   char* err, size_t errlen);
vk_chain* vk_chain_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                       int32_t n_chains, int32_t n_params, const int32_t* columns, const int32_t* param_block,
                                       const double* lo, const double* hi, const double* base_rows, double alpha,
                                       const int32_t* which, char* err, size_t errlen);
/* Nested sampling (vk_nested_create above) of a joint fit: the same handle over the joint entry points, one row for all blocks
 * or (_blocks) a row per block; which[i]: joint realisation of row i.  Arguments as vk_chain_create_joint /
 * vk_chain_create_joint_blocks with the shape of vk_nested_create behind n_rows. */
vk_nested* vk_nested_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_rows,
                                  int32_t n_live, int32_t batch, int32_t steps, double scale, int32_t n_params,
                                  const int32_t* columns, const double* lo, const double* hi, const double* base_rows,
                                  double alpha, const int32_t* which, char* err, size_t errlen);
vk_nested* vk_nested_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts,
                                         int32_t n_rows, int32_t n_live, int32_t batch, int32_t steps, double scale,
                                         int32_t n_params, const int32_t* columns, const int32_t* param_block, const double* lo,
                                         const double* hi, const double* base_rows, double alpha, const int32_t* which, char* err,
                                         size_t errlen);
/* Importance-sampled posteriors (vk_is_create above) of a joint fit: the same handle over the joint entry points, block-diagonal
 * (cov NULL) or under the covariance handle, fixed or gridded in beta.  Arguments as vk_is_create behind ctxs, n_ctx and cov;
 * every_realisation: problem r is JOINT realisation r - realisation r of every block - and every point's theory vectors are
 * computed once per block and compared with all of them (the cross mode of vk_joint_cov_eval_realisations; block-diagonal each
 * block's cross-mode chi-squares, summed in block order by the rule of vk_joint_eval_device_async: start at 0, add block after
 * block, a sum that is not finite becomes (-inf, +inf)).  The _blocks form keeps a row per block as vk_fit_create_joint_blocks
 * does: param_block [n_axes] and base_rows [n_ctx][VK_NPAR]; vk_is_rows then returns [n_ctx][count][VK_NPAR].  vk_is_run, _rows,
 * _result, _last_error and _destroy serve these handles as they serve vk_is_create's.
 * Refused in addition to what vk_is_create and vk_fit_create_joint[_blocks] refuse: with every_realisation, blocks that hold
 * different numbers of realisations or none, a block with model realisations (vk_set_model_realisations: no cross mode), a block
 * whose realisation kernel lacks LDS - at create time and again at every run -; VK_WALK_EPSILON per block (eps_pow holds one
 * power per point). */
vk_is* vk_is_create_joint(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_axes,
                          const int32_t* columns, int64_t n_points, const double* x, const double* y, const double* eps_pow,
                          const double* lno, const double* lno_prior, const int32_t* n_bins, int32_t n_pairs, const int32_t* pair_bins,
                          const int32_t* lists, const int32_t* offsets, const double* base_row, double alpha, int32_t every_realisation,
                          int32_t chunk, char* err, size_t errlen);
vk_is* vk_is_create_joint_blocks(vk_ctx* const* ctxs, int32_t n_ctx, vk_joint_cov* cov, const vk_eval_opts* opts, int32_t n_axes,
                                 const int32_t* columns, const int32_t* param_block, int64_t n_points, const double* x, const double* y,
                                 const double* eps_pow, const double* lno, const double* lno_prior, const int32_t* n_bins,
                                 int32_t n_pairs, const int32_t* pair_bins, const int32_t* lists, const int32_t* offsets,
                                 const double* base_rows, double alpha, int32_t every_realisation, int32_t chunk, char* err,
                                 size_t errlen);

/* ---- many one-point callers sharing one GPU: mailboxes in shared memory -----------------------------------------------
 * The reference is sampled by cobaya, which asks for ONE likelihood per call (victor/likelihoods/CCFLikelihood.py:32-39); more
 * throughput comes from several chains, one process each, under mpirun (README.md:30).  P processes with a context each
 * serialise P small launches on the GPU.  Instead ONE owner process holds the context and serves an array of mailboxes that
 * lives in memory shared with the chains (a file in /dev/shm, victor_amd/broker.py): a chain writes its parameter row and
 * bumps `req_seq`; the owner evaluates everything that is pending as ONE launch and answers each mailbox by
 * writing lnl / chi2 / status and then `resp_seq = req_seq`.  The chains never touch the GPU (or this library).
 *
 * Protocol of one mailbox (all fields naturally aligned; release / acquire accesses on the two sequence words - this library's
 * side uses them on every architecture; the Python client of victor_amd/broker.py writes plain stores and relies on x86-64's
 * total store order: on another architecture use a native client):
 *   client   state = VK_BOX_ATTACHED once, with its pid;  per call: row[] <- parameters, then req_seq <- req_seq + 1 (release);
 *            wait until resp_seq == req_seq (acquire), then read lnl, chi2, status.  One call in flight per mailbox.
 *   server   sees req_seq != resp_seq (acquire), copies row[], evaluates, writes lnl, chi2, status, then resp_seq <- the
 *            req_seq it served (release).
 * status is the VK_* code of the batch the request was part of (0: lnl / chi2 valid, failed rows report -inf / +inf as
 * vk_eval_batch does). */
#define VK_BOX_FREE 0
#define VK_BOX_ATTACHED 1
typedef struct vk_mailbox {          /* 256 bytes: the client's and the server's words on different cache lines */
  volatile uint64_t req_seq;         /* client -> server                                                      */
  volatile uint32_t state;           /* VK_BOX_*; written by the client (attach / detach) and by vk_serve_mailboxes, which frees
                                        the boxes of dead clients at the start of a call (no launch of its own in flight then) */
  uint32_t reserved0;
  volatile int64_t client_pid;
  uint64_t reserved1[5];
  double row[VK_NPAR];               /* 96 bytes, the parameter row in the column order above                 */
  uint64_t reserved2[4];
  volatile uint64_t resp_seq;        /* server -> client                                                      */
  double lnl, chi2;
  int32_t status;
  uint32_t reserved3;
  uint64_t reserved4[4];
} vk_mailbox;

typedef struct vk_serve_stats {      /* accumulated over calls until the caller zeroes it */
  uint64_t batches, evals, max_batch, windows_timed_out;
  double busy_seconds;               /* inside vk_eval_batch */
} vk_serve_stats;

/* Serve `n_boxes` mailboxes until *stop != 0 or `max_seconds` have passed (then returns VK_OK once nothing is in flight; call
 * it again - the owner looks after its clients between calls).  `ctxs`: 1..8 contexts holding the SAME tables on one device
 * (the owner creates them from one vk_tables): one launch per context may be in flight, so a round's requests start at once
 * on a free context while earlier rounds are still on the GPU - the launches overlap there like those of separate processes -
 * and requests that arrive together share a launch.  `gather_window_us`: after the first pending request of a round the
 * server waits up to this long for the requests of the other attached clients that are not being served already (chains in
 * lock-step then share one launch instead of splitting into ever smaller ones; 0: launch at once).  When nothing is pending
 * or in flight it polls for ~0.2 ms, then naps in steps of 50 us (1 ms after 50 ms of silence).  n_boxes <= 1024.  Returns a
 * VK_E_* code only for bad arguments: an evaluation error is reported to the requesting mailboxes (status) and the loop goes
 * on.  A launch carries at most `max_batch` requests (1..32; 0 = 32: smaller launches finish sooner and leave the other contexts
 * something to overlap with), and every request is evaluated with the work split of a single-point
 * vk_eval_batch call whatever shares its launch: lnl / chi2 of a row are bit-identical to vk_eval_batch(ctx, opts, row, 1, ...)
 * and do not depend on what the other clients were doing. */
int vk_serve_mailboxes(vk_ctx* const* ctxs, int32_t n_ctx, const vk_eval_opts* opts, vk_mailbox* boxes, int32_t n_boxes,
                       const volatile uint32_t* stop, double gather_window_us, int32_t max_batch, double max_seconds,
                       vk_serve_stats* stats);

/* ---- timing on the context's stream (HIP events) ------------------------------------ */
/* Marks: 0 = before theory kernel, 1 = between kernels, 2 = after likelihood kernel, recorded by
 * the next vk_eval_batch_device_async when enabled.  Times accumulate until reset. */
int vk_timing_enable(vk_ctx* ctx, int on);
int vk_timing_read(vk_ctx* ctx, double* theory_ms, double* like_ms, int64_t* launches, int reset);

/* ---- multi-GPU gather of log-likelihoods over RCCL/xGMI ------------------------------ */
#define VK_COMM_ID_BYTES 128
int vk_comm_unique_id(char* id_out /* [VK_COMM_ID_BYTES] */);
int vk_comm_init(vk_ctx* ctx, const char* id, int rank, int nranks);
/* all ranks contribute count doubles at d_send, every rank receives nranks*count at d_recv */
int vk_comm_allgather_async(vk_ctx* ctx, const double* d_send, double* d_recv, int64_t count);
int vk_comm_destroy(vk_ctx* ctx);
/* PCI bus id of the context's GPU ("0000:c1:00.0"): ranks compare these (with their host names) before building a
 * communicator - RCCL needs one device per rank, and a launcher may give two ranks the same GPU under different ordinals. */
int vk_device_bus_id(const vk_ctx* ctx, char* buf, size_t len);
/* One process driving several GPUs (one context per device, any host thread): communicators for all n contexts at once
 * (ncclCommInitAll - no unique id, no rendezvous), context i being rank i.  Fails with VK_E_RCCL when two contexts share a
 * device (RCCL refuses that; callers then gather through the host). */
int vk_comm_init_all(vk_ctx* const* ctxs, int32_t n);
/* An all-gather of HOST data that is collected later (one process per GPU; after vk_comm_init): `send` (count doubles) is copied
 * to pinned memory; upload, ncclAllGather and download are enqueued on the context's stream and nothing waits.
 * vk_comm_allgather_host_finish waits for the download and writes recv[nranks][count], rank-major.  One gather per context at a
 * time.  For monitoring traffic that must not sit in a caller's step: victor_amd/sampler.py exchanges the walkers'
 * log-likelihoods of a block of steps this way, collecting one block late, on a context of the gather's own (an all-gather
 * enqueued on a stream the walkers launch on would hold their launches back until the slowest rank has arrived). */
int vk_comm_allgather_host_begin(vk_ctx* ctx, const double* send, int64_t count);
int vk_comm_allgather_host_finish(vk_ctx* ctx, double* recv);

/* The all-gather of such a group in one call: ncclGroupStart, one ncclAllGather per context on that context's stream
 * (d_send[i]: count doubles on device i, d_recv[i]: n*count doubles on device i), ncclGroupEnd.  Enqueued. */
int vk_comm_allgather_group_async(vk_ctx* const* ctxs, int32_t n, const double* const* d_send, double* const* d_recv,
                                  int64_t count);
/* Writes a JSON object naming the HIP runtime this process mapped (path, runtime/driver version, the HIP version the
 * library was built with) and the RCCL that vk_comm_* uses (path, ncclGetVersion).  RCCL is looked up next to the mapped
 * HIP runtime first, so both come from one ROCm install (PyTorch's bundled pair when torch was imported before this
 * library, /opt/rocm's otherwise); VICTOR_HIP_RCCL_LIB names another one in development runs only (VICTOR_HIP_DEV=1).  Returns VK_E_RCCL (buffer still filled) if no RCCL
 * could be loaded. */
int vk_comm_info(char* buf, size_t len);
/* What the LIVE communicator of `ctx` says about itself: ncclCommCount, ncclCommUserRank, ncclCommCuDevice (each -1 when the
 * loaded library does not export the call or it fails).  VK_E_RCCL without a communicator.  A multi-GPU record carries these per
 * rank (bench.py: config.rccl.ranks) next to the PCI bus ids the ranks compared before building it. */
int vk_comm_rank_info(const vk_ctx* ctx, int32_t* count, int32_t* user_rank, int32_t* device);

#ifdef __cplusplus
}
#endif
#endif /* VICTOR_HIP_H */
