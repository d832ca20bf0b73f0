"""Derived bounds for comparing two CORRECT evaluations of the same likelihood that differ in the order of their arithmetic
(another kernel mapping, another work split, a sub-batch on its own) - not a parity tolerance: parity against the oracle and
the reference's goldens is asserted with the contract's own numbers in the parity tests.

Why not a bare ``1e-12``: two mappings produce theory vectors that differ by a few rounding errors of their projection sums,
``|dt_k| <= u tau_k`` with ``tau_k = sum_i |W_l[i]| max(1 + xi)`` the magnitude of what is summed for entry k, and the
chi-square amplifies that by its conditioning.  With r = t - d and P the precision matrix,

    |d chi2|  <=  2 u  sum_jk |P_jk| |r_j| tau_k   +   u_s  sum_jk |P_jk| |r_j| |r_k|        (first order)

where the second term is the re-association of the quadratic form itself.  Both sums are computed here from the fit's own
arrays, per point, so the bound follows the point: a parameter set whose chi-square is a small difference of large terms is
allowed the error it must have, a well-conditioned one is held to a few 1e-14.  ``ulps`` is the number of unit roundoffs
(2^-53) the entries of the theory vector may differ by, relative to tau: 64 for two mappings of the same arithmetic (sums of
5000 terms in another order: ~sqrt(5000) u typical; an integrand whose exponent moved by one rounding: y^2 u <= 18 u), 1024
between the fast kernels and the generic one (library sqrt / exp / division against the refined hardware forms, each within
2 ulp - vk_devmath.h - over a chain of ~10 operations).

Every comparison appends its worst margin (observed difference / bound) to ``gpurun_out/tolerance_margins.txt`` when that
directory exists, so that a bound sitting close to what is observed is visible after a GPU run.
"""

import os

import numpy as np

U = 2.0 ** -53
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(what, margin):
    d = os.path.join(_ROOT, "gpurun_out")
    if os.path.isdir(d):
        try:
            with open(os.path.join(d, "tolerance_margins.txt"), "a") as fh:
                fh.write(f"{margin:.3e}  {what}\n")
        except OSError:
            pass


def _tau(fit):
    """Magnitude of the sums behind each entry of the theory vector: sum_i |W_l[i]| * 2 (1 + xi^r stays below 2)."""
    from victor_amd import tables as T
    poles = np.atleast_1d(fit.poles_s)
    w = T.projection_weights(T.mu_nodes_for(poles), poles)               # (n_ell, n_mu)
    return np.repeat(2.0 * np.abs(w).sum(axis=1), len(fit.s))            # (N,)


def chi2_bound(fit, params, ulps=64, **kwargs):
    """Per-point bound on |chi2_a - chi2_b| for two evaluation orders (see the module docstring).  ``params`` as for
    ``log_likelihood_batch``; ``kwargs`` are the model options of the call being compared.  Needs the GPU (theory vectors)."""
    from victor_amd import _native as N
    model = fit._merged(kwargs)
    rows = fit._fit_rows(params, model)
    t = fit.theory_vector_batch(rows, **kwargs)
    n, nd = t.shape
    beta = rows[:, N.P_BETA]
    if fit.fixed_data:
        d = np.broadcast_to(fit.multipole_datavector(), (n, nd))
    else:
        d = np.array([fit.multipole_datavector(b) for b in beta])
    absr = np.abs(t - d)
    v = absr + 2.0 * _tau(fit)[None, :]
    if fit.fixed_covmat:
        amp = np.einsum("ij,jk,ik->i", absr, np.abs(fit.icov), v)
    else:
        absP = np.abs(fit.icov)
        amp = np.empty(n)
        for i in range(n):
            lo, w = fit._bracket(beta[i]) if np.isfinite(beta[i]) else (0, 0.0)
            P = absP[lo] if w == 0.0 else (1 - w) * absP[lo] + w * absP[-1]
            amp[i] = absr[i] @ P @ v[i]
    return ulps * U * amp


def generic_chi2_bound(chi2, n_data, ulps=64):
    """Bound without the fit's arrays: ``ulps * u * n_data * 16`` relative - a conditioning budget of 16 (the entries of a
    chi-square of n_data terms, theory sums a few times the size of the residuals)."""
    return ulps * U * n_data * 16.0 * np.abs(np.asarray(chi2, float))


def assert_same_chi2(got, want, bound=None, n_data=None, what="", ulps=64):
    """chi-squares of two evaluation orders agree to ``bound`` (per point, from :func:`chi2_bound`; sliced by the caller for a
    sub-batch) or, without it, to :func:`generic_chi2_bound`.  Rows that failed in both (+inf) count as equal.  Returns the
    bound it used."""
    got, want = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(want, float))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore"):
        diff = np.where(both_inf, 0.0, np.abs(got - want))
    if bound is None:
        assert n_data, "assert_same_chi2 needs a bound or n_data"
        bound = generic_chi2_bound(np.maximum(np.abs(want), np.abs(got)), n_data, ulps)
    bound = np.broadcast_to(np.asarray(bound, float), diff.shape)
    bound = np.where(np.isfinite(bound), bound, 0.0)
    safe = np.where(bound > 0, bound, 1.0)
    ratio = np.where(bound > 0, diff / safe, np.where(diff > 0, np.inf, 0.0))
    margin = float(np.max(ratio)) if diff.size else 0.0
    _record(f"chi2 {what}", margin)
    assert margin <= 1.0, (what, "worst margin %.3g at index %d" % (margin, int(np.argmax(ratio))), float(np.max(diff)))
    return bound


def assert_same_lnl(got, want, chi2_bounds, what="", offset_scale=1000.0):
    """log-likelihoods of two evaluation orders: every likelihood form is a function of chi2 with |d lnL / d chi2| <= 0.51
    (gaussian -1/2; hartlap / percival rescale by a factor below one; sellentin -n/2(n-1) / (1 + chi2/(n-1))), plus a
    beta-dependent log-determinant of magnitude <= ``offset_scale`` that carries a few roundings of its own.  ABSOLUTE bound:
    lnL passes through zero where the log-determinant term cancels the chi-square term."""
    got, want = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(want, float))
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore"):
        diff = np.where(both_inf, 0.0, np.abs(got - want))
    bound = 0.51 * np.atleast_1d(np.asarray(chi2_bounds, float)) + 16 * U * (np.abs(want) + offset_scale)
    bound = np.where(np.isfinite(bound), bound, 0.0)
    margin = float(np.max(diff / np.where(bound > 0, bound, 1.0))) if diff.size else 0.0
    _record(f"lnl  {what}", margin)
    assert np.all(diff <= bound), (what, "worst margin %.3g" % margin, float(diff.max()))


def assert_same_theory(got, want, what="", ulps=512, tau=2.0):
    """Theory vectors / multipoles of two evaluation orders: entries differ by at most ``ulps`` unit roundoffs of the summed
    magnitude tau * sum|W| (see the module docstring); W-sums of the shipped grids are below 4."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = ulps * U * tau * 4.0 * max(1.0, float(np.max(np.abs(want))) if want.size else 1.0)
    diff = float(np.max(np.abs(got - want))) if got.size else 0.0
    _record(f"theory {what}", diff / bound)
    assert diff <= bound, (what, diff, bound)


# ------------------------------------------------------------------------------------------------------------------------
# Bounds against an exact value: |gpu - xp|, xp the table contract in extended precision (tests/xp_reference.py)
# ------------------------------------------------------------------------------------------------------------------------
# The bounds above hold two FP64 evaluations to each other, so an error both share is invisible to them.  The ones below
# hold ONE kernel to tests/xp_reference.py, which evaluates the same discrete operation on the same tables in longdouble
# (its own error is ~1e-19 relative, and tests/test_xp_reference.py checks it against mpmath): what remains is the kernel's
# error alone, and it is bounded to first order from the relative errors its operations are documented to have
# (vk_devmath.h; tests/test_gpu_devmath.py asserts each of them on the hardware), with ULP = 2^-52 (an ulp of a double in
# [1, 2), the unit in which those are quoted) and u = 2^-53:
#
#   exp_gauss      1.5e-13 (EXPT 0, degree 3, 256 entries: every shipped kernel)    exp_nonpos, sqrt_rsqrt, rsqrt3: <= 2.5 ULP
#   rsqrt_nr, rsqrt_nr_x2: 22 ULP (one Newton step)                                  recip (third order): 1 ULP
#   recip_nr: 4e-15 (one Newton step)                                                the refined uni_* tables: XP_TABLE_ULPS
#
# For theory entry k (l, s_j), with the magnitude tau_k = sum_i |W_l[i]| (sum_v |w_v f_iv| + 1) of what the kernel sums and the
# sensitivities of xp_reference.Theory (each summed over the same terms with |W_l[i]| |w_v|):
#
#   |dt_k| <= (eps_F + (K_sum + K_f) u) tau_k                 every integrand term carries the exp's relative error eps_F,
#                                                             K_f u of its own products, K_sum u of the two summations
#           + c_ir s_ir_k                                     relative error of 1/r (moves r and mu_r = r_par / r together)
#           + c_u s_u_k                                       relative error of u = r / c: 1/c, the product, the AP integral
#           + K_rp u s_rp_k                                   r_par = s a_par mu - x B rounded relative to |s_par| + |x B|
#           + c_z s_z_k                                       relative error of z = (A V mu_r + x) / sigma: df/f = z dz
#           + c_fp s_fp_k                                     relative rounding of one pass of the fixed-point iteration,
#                                                             times its gain (xp: sum_{k<=niter} rho^k over the passes)
#
# K_sum = n_mu + n_x + 16: no kernel accumulates a longer serial chain than one node loop plus one mu loop plus the tree
# reductions (64 lanes: 6 levels, 4 waves, partial sums of up to 8 workgroups) - the generic kernel's per-lane chains are
# n_mu n_x / 64 = 78 terms long, the cells kernel's n_x then n_mu.  K_f = 16: the integrand's own products and sums (about
# ten roundings behind the exponential, xi^r's Horner form whose error is relative to 1 + |xi| since tau reads 1 + xi as
# 1 + |xi|).  K_rp = 4: s a_par, that times mu, x B and the difference.  Each family's eps_F / c_* are in XP_FAMILIES.
ULP = 2.0 ** -52
XP_TABLE_ULPS = 16          # refined tables against the vk_pp cubics, relative to the local magnitude (tests/test_xp_reference.py)
_TAB = XP_TABLE_ULPS * ULP
XP_FAMILIES = {
    # generic theory kernel and K1x: library-grade forms throughout (sqrt_rsqrt, recip, exp_nonpos), the vk_pp tables xp reads
    "generic": dict(eps=2.5 * ULP, c_ir=2.5 * ULP, c_u=2 * ULP, c_z=ULP + 16 * U, c_fp=4 * ULP),
    # point-major and cells streaming (EXPT 0): exp_gauss 1.5e-13, rsqrt_nr(_x2) 22 ULP on 1/r (and the interval coordinate
    # r / (c h) formed from it), recip_nr 4e-15 on 1/sigma, the refined tables' coefficients
    "fast": dict(eps=1.5e-13 + _TAB, c_ir=22 * ULP, c_u=4 * ULP, c_z=4e-15 + 16 * U + _TAB, c_fp=0.0),
    "cells": dict(eps=1.5e-13 + _TAB, c_ir=22 * ULP, c_u=4 * ULP, c_z=4e-15 + 16 * U + _TAB, c_fp=0.0),
    # dispersion on the fast kernels: second-order passes (rsqrt_nr_x2 22 ULP on 1/r, recip_nr 4e-15 = 18 ULP on 1/(1 + q)),
    # third-order last pass and final evaluation (rsqrt3_x2, recip), exp_gauss<0> on the node's Gaussian
    "dispersion": dict(eps=1.5e-13 + _TAB, c_ir=2.5 * ULP, c_u=4 * ULP, c_z=ULP + 16 * U + _TAB, c_fp=40 * ULP),
    # kaiser / euclid_special on the cells kernel: second-order passes (rsqrt_nr, recip_nr), rsqrt3 / recip at the end, no exp
    "kaiser": dict(eps=_TAB, c_ir=2.5 * ULP, c_u=4 * ULP, c_z=0.0, c_fp=40 * ULP),
}
XP_AP_ULPS = 64             # the 50-node AP trapezoid (49 additions, sqrt_rsqrt 2 ULP) when c is rescaled from AP


def _xp_ratio(diff, bound, ok):
    """diff / bound where ``ok``; a difference against a bound that is zero, negative or not finite is an infinite ratio (a
    bound that could not be formed never lets a difference pass), no difference is 0."""
    bound = np.asarray(bound, float)
    usable = np.isfinite(bound) & (bound > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(usable, diff / np.where(usable, bound, 1.0), np.where(diff > 0, np.inf, 0.0))
    return np.where(ok, r, 0.0)


def theory_xp_bound(th, family, n_mu, n_x, rescale_from_ap=True):
    """Per-entry bound (n, N) on |gpu - xp| for theory vectors of a kernel family (see above); ``th`` an
    xp_reference.Theory with sensitivities."""
    F = XP_FAMILIES[family]
    k_sum = n_mu + n_x + 16
    c_u = F["c_u"] + (XP_AP_ULPS * ULP if rescale_from_ap else 0.0)
    f = lambda a: np.asarray(a, dtype=float)         # noqa: E731
    return ((F["eps"] + (k_sum + 16) * U) * f(th.mag) + F["c_ir"] * f(th.s_ir) + c_u * f(th.s_u) + 4 * U * f(th.s_rp)
            + F["c_z"] * f(th.s_z) + F["c_fp"] * f(th.s_fp))


def assert_theory_xp(got, th, bound, what=""):
    """Theory vectors (n, N) of a kernel against xp (``th.t``) at the per-entry ``bound``; a NaN row must be NaN in both."""
    got = np.asarray(got, float)
    want = np.asarray(th.t, dtype=np.longdouble)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_x = np.isnan(want.astype(float))
    assert np.array_equal(np.isnan(got), nan_x), (what, "NaN pattern differs", np.argwhere(np.isnan(got) != nan_x)[:4])
    ok = ~nan_x
    diff = np.abs((got.astype(np.longdouble) - want)).astype(float)
    ratio = _xp_ratio(diff, bound, ok)
    margin = float(np.max(ratio)) if ratio.size else 0.0
    _record(f"xp theory {what}", margin)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else None
    assert margin <= 1.0, (what, "worst margin %.3g at %s" % (margin, i), float(diff[i]), float(bound[i]))
    return margin


def _blend_abs(stack, lo, t):
    """Magnitude of the blended precision (1 - t) P_lo + t P_last as its roundings see it: (1 - t) |P_lo| + t |P_last|
    (entrywise; larger than |blend| where the two slices cancel)."""
    a = np.abs(np.asarray(stack[lo], float))
    if t == 0:
        return a
    t = float(t)
    return (1 - t) * a + t * np.abs(np.asarray(stack[-1], float))


def _data_rounding(xp, beta):
    """Bound on the FP64 Horner evaluation of the data vector at beta: 8 u sum_p |c_jp| |db|^p per entry (0 if fixed)."""
    if not xp.n_beta_d:
        return np.zeros(xp.N)
    k, db = xp.beta_piece(xp.beta_d, beta)
    return 8 * U * (np.abs(np.asarray(xp.data[k], float)) @ (abs(float(db)) ** np.arange(4)))


def _quadratic_bound(r, absP, dd):
    return (2 * len(r) + 5) * U * (r @ absP @ r) + 2 * (absP @ r) @ dd


def chi2_xp_bound(xp, theory, rows, consumed_bound=None):
    """Per-point bound on |chi2_gpu - chi2_xp| when the chi-square kernel consumed ``theory`` (the vector xp is handed; n, N),
    xp an xp_reference.XP.  With r = t - d and |P| = (1 - t) |P_lo| + t |P_last| the magnitude of the (blended) precision,

        (2 N + 5) u sum_jk |r_j| |P_jk| |r_k|       the quadratic form: a sum of N^2 products (any order: gamma_{2N}), the
                                                    blend (1 - t) P_lo + t P_last (two roundings per entry), the fold of
                                                    P_jk + P_kj onto one triangle, the residual's subtraction
      + 2 sum_j |(|P| |r|)_j| dd_j                  the data at beta: Horner in FP64, dd_j = 8 u sum_p |c_jp| |db|^p

    plus ``consumed_bound`` (per point) where the theory the chi-square kernel consumed is not the vector that was downloaded
    (another launch: :func:`chi2_bound` at 64 ulps).  Rows that must fail (a theory entry not finite, or a NaN beta where data or
    precision depend on it) get 0: :func:`assert_chi2_xp` requires them to fail in both."""
    from victor_amd import _native as N
    theory = np.atleast_2d(np.asarray(theory, float))
    rows = np.atleast_2d(np.asarray(rows, float))
    out = np.zeros(len(rows))
    for n, row in enumerate(rows):
        beta = row[N.P_BETA]
        if not np.all(np.isfinite(theory[n])) or (not np.isfinite(beta) and (xp.n_beta_d or xp.n_beta_c)):
            continue
        r = np.abs(theory[n] - np.asarray(xp.data_at(beta), float))
        lo, t = xp.bracket(beta) if xp.n_beta_c else (0, 0)
        out[n] = _quadratic_bound(r, _blend_abs(xp.prec, lo, t), _data_rounding(xp, beta))
    if consumed_bound is not None:
        out = out + np.asarray(consumed_bound, float)
    return out


def joint_chi2_xp_bound(joint, xps, theory, rows, ulps=64):
    """:func:`chi2_xp_bound` for a JointFit under one covariance (``xps``: an xp_reference.XP per block): the blocks' data
    concatenated under the joint precision, plus the blocks' theory launches against the joint kernel's own (``ulps`` unit
    roundoffs of tau, as :func:`chi2_bound`: ulps u |r|^T |P| (|r| + 2 tau))."""
    from victor_amd import _native as N
    from tests.xp_reference import bracket
    theory = np.atleast_2d(np.asarray(theory, float))
    rows = np.atleast_2d(np.asarray(rows, float))
    stack = np.asarray(joint.icov, float)
    stack = stack[None] if joint.fixed_covmat else stack
    tau = np.concatenate([_tau(x.fit) for x in xps])
    out = np.zeros(len(rows))
    for n, row in enumerate(rows):
        beta = row[N.P_BETA]
        beta_used = not joint.fixed_covmat or any(x.n_beta_d for x in xps)
        if not np.all(np.isfinite(theory[n])) or (not np.isfinite(beta) and beta_used):
            continue
        d = np.concatenate([np.asarray(x.data_at(beta), float) for x in xps])
        r = np.abs(theory[n] - d)
        lo, t = (0, 0) if joint.fixed_covmat else bracket(np.asarray(joint.beta_covmat, float), beta)
        absP = _blend_abs(stack, lo, t)
        dd = np.concatenate([_data_rounding(x, beta) for x in xps])
        out[n] = _quadratic_bound(r, absP, dd) + ulps * U * (r @ absP @ (r + 2 * tau))
    return out


def assert_chi2_xp(got_lnl, got_chi2, want_lnl, want_chi2, bound, what="", offset_scale=1000.0):
    """chi2 and lnL of a chi-square kernel against xp_reference.chi2_from_theory: chi2 at ``bound``
    (:func:`chi2_xp_bound`), lnL as in :func:`assert_same_lnl`; failed rows (-inf, inf) must fail in both."""
    got_chi2 = np.atleast_1d(np.asarray(got_chi2, float))
    got_lnl = np.atleast_1d(np.asarray(got_lnl, float))
    want_chi2 = np.atleast_1d(np.asarray(want_chi2, dtype=np.longdouble))
    want_lnl = np.atleast_1d(np.asarray(want_lnl, dtype=np.longdouble))
    fail_x = np.isinf(want_chi2)
    assert np.array_equal(np.isinf(got_chi2), fail_x), (what, "failed rows differ", got_chi2, want_chi2.astype(float))
    assert np.array_equal(np.isinf(got_lnl), fail_x), (what, "failed rows differ (lnL)", got_lnl)
    ok = ~fail_x
    bound = np.broadcast_to(np.asarray(bound, float), got_chi2.shape)
    diff = np.where(ok, np.abs(got_chi2.astype(np.longdouble) - want_chi2).astype(float), 0.0)
    ratio = _xp_ratio(diff, bound, ok)
    margin = float(np.max(ratio)) if ratio.size else 0.0
    _record(f"xp chi2 {what}", margin)
    assert margin <= 1.0, (what, "worst margin %.3g at %d" % (margin, int(np.argmax(ratio))), float(np.max(diff)))
    lb = 0.51 * bound + 16 * U * (np.abs(want_lnl.astype(float)) + offset_scale)
    dl = np.where(ok, np.abs(got_lnl.astype(np.longdouble) - want_lnl).astype(float), 0.0)
    lm = float(np.max(_xp_ratio(dl, lb, ok))) if dl.size else 0.0
    _record(f"xp lnl  {what}", lm)
    assert lm <= 1.0, (what, "lnL worst margin %.3g" % lm)
    return margin
