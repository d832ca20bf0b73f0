"""Derived bounds for comparing two CORRECT Fisher matrices whose theory vectors come from two evaluation orders (another
launch shape, another route) or from the oracle - the companion of tests/tolerances.py for tests/test_gpu_fisher.py.

With ``dt`` the per-entry bound two theory vectors are granted, a difference ``D_ak = t_a(+) - t_a(-)`` moves by
``|dD| <= 2 dt``.  ``S_jk = sum_ab D_aj P_ab D_bk`` is bilinear in D, so to first order

    |dS_jk|  <=  sum_ab (|dD_aj| |P_ab| |D_bk| + |D_aj| |P_ab| |dD_bk|)  +  (2 N + 5) u sum_ab |D_aj| |P_ab| |D_bk|

where the last term is the rounding of the double sum itself (N^2 products in any order: gamma_{2N}; the blend of two
precision slices and the subtraction behind D: the "+ 5", as tests/tolerances._quadratic_bound counts them).  ``fisher`` is
``(c / 4) S / (h_j h_k)``: the bound scales the same way (the scaling's own three roundings are inside the "+ 5").
"""

import numpy as np

from tests.tolerances import U


def same_theory_delta(want, ulps=512, tau=2.0):
    """The per-entry bound ``tests.tolerances.assert_same_theory`` grants two evaluation orders of the vectors ``want``."""
    want = np.asarray(want, dtype=float)
    return ulps * U * tau * 4.0 * max(1.0, float(np.max(np.abs(want))) if want.size else 1.0)


def fisher_bound(D, P, h, scale, dt):
    """``(d, d)`` bound on ``|fisher_a - fisher_b|`` of one problem: ``D`` (N, d) the differences of either route, ``P`` (N, N)
    the precision (dense; block-diagonal for a block-diagonal joint fit), ``h`` (d,) the steps, ``scale`` the c of the
    likelihood form, ``dt`` the per-entry bound on the theory vectors (a scalar or (N,))."""
    D, P, h = np.abs(np.asarray(D, dtype=float)), np.abs(np.asarray(P, dtype=float)), np.asarray(h, dtype=float)
    N, d = D.shape
    dD = 2.0 * np.broadcast_to(np.asarray(dt, dtype=float), (N,))
    left = dD @ P @ D                  # sum_ab |dD_a| |P_ab| |D_bk|, per k
    right = (P @ dD) @ D               # sum_ab |D_aj| |P_ab| |dD_b|, per j
    T = D.T @ P @ D
    dS = right[:, None] + left[None, :] + (2 * N + 5) * U * T
    low = np.tril(np.ones((d, d), dtype=bool))
    dS = np.where(low, dS, dS.T)       # (entry (k, j), k < j, holds S_jk)
    return 0.25 * abs(float(scale)) * dS / np.outer(h, h)


def dense_precision(blocks, r, N, R, slices=None):
    """The (N, N) precision of problem ``r`` of R from a list of :class:`victor_amd.fisher.Block` (``slices``: the blocks'
    ``precision(R)``, formed once by a caller that loops over the problems)."""
    P = np.zeros((N, N))
    for i, b in enumerate(blocks):
        P[b.off:b.off + b.n, b.off:b.off + b.n] = (b.precision(R) if slices is None else slices[i])[r]
    return P


def assert_same_fisher(got, want, D, blocks, h, scale, dt, what=""):
    """``fisher`` (R, d, d) of two routes at :func:`fisher_bound`, problem by problem; records the worst margin."""
    from tests.tolerances import _record
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    slices = [b.precision(len(got)) for b in blocks]
    for r in range(len(got)):
        bound = fisher_bound(D[r], dense_precision(blocks, r, D.shape[1], len(got), slices), h[r], scale, dt)
        diff = np.abs(got[r] - want[r])
        assert np.all(np.isfinite(diff)), (what, r, "not finite")
        margin = float(np.max(diff / bound))
        worst = max(worst, margin)
        assert margin <= 1.0, (what, "problem %d: worst margin %.3g" % (r, margin), float(diff.max()), float(bound.min()))
    _record(f"fisher {what}", worst)
    return worst
