"""Likelihood-level beta interpolation on the device (``beta_interpolation='likelihood'`` on a beta-dependent data vector:
``VK_OPT_BETA_BLEND``, ``victor_amd/csrc/vk_kernel_blend.h``, ``sampled_evaluate_blend``).  The fits here carry
the option in their data block; every call below takes the mode from them.

1. The split and merge kernels alone (``vk_blend_split`` / ``vk_blend_merge``) against the NumPy expression of
   ``CCFFit._run_likelihood_interp``: rows, ``t`` and failure marks exactly, blended values bit for bit (a NaN for a NaN).
2. Every device loop in this mode against what it already answers to, with the comparison its own GPU tests use.  Epsilon is fixed
   throughout, so both routes put the same 2 m rows - the m rows at their lower nodes, then at their upper nodes - into launches of
   the same size through the same entry points, and everything is compared as BYTES (tests/test_gpu_fit_definition.py,
   tests/test_gpu_chains.py, tests/test_gpu_nested.py make the same argument for m rows); sums over chunks at the derived bounds
   of tests/test_grid.py and tests/test_importance.py.

The definition routes go through ``log_likelihood_batch`` / ``log_likelihood_pairs`` / ``Realisations.log_likelihood``, whose
host blend raises ``IndexError`` outside the beta grid, as the reference does.  Where a test puts points outside the grid on
purpose (the grid posterior) the definition route runs over an ``evaluate`` callable that moves those points' beta inside -
the launch keeps its size - and reports them as (-inf): the rule of the device.
"""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases
from tests import fit_definition as FD
from tests import test_grid as TG
from tests import test_importance as TI
from tests.test_chains import same_bytes
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
LIKE = dict(beta_interpolation="likelihood")
D2 = {"epsilon": 1.0, "sigma_v": 380.0}                   # d = 2: fsigma8 and beta
D1 = dict(D2, fsigma8=0.47)                               # d = 1: beta (the stretch move needs 2 (d + 1) <= 4 walkers)
EPS1 = {"epsilon": 1.0}
WIDE = dict(PARAMS, beta=dict(PARAMS["beta"], prior={"dist": "uniform", "min": 0.1, "max": 0.7}))     # wider than the grid
P_BETA = 5


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def like_fit(options):
    """The fit of ``options`` with ``beta_interpolation: likelihood`` in its data block, as a YAML configures it: the mode of a
    device loop is the fit's own (a per-call override into it stays refused; tests/test_beta_blend.py)."""
    import victor_amd
    model, data = options
    fit = victor_amd.CCFFit(model, dict(data, beta_interpolation="likelihood"))
    assert fit.fit_options["beta_interpolation"] == "likelihood" and not fit.fixed_data
    return fit


@pytest.fixture(scope="module")
def boss():
    fit = like_fit(cases.boss_options("config"))
    assert len(fit.beta_ccf) == 31 and not fit.fixed_covmat
    return fit


@pytest.fixture(scope="module")
def stack():
    return like_fit(stack_options())


@pytest.fixture(scope="module")
def rs3(stack):
    return stack.realisations([0, 1, 2])


# ------------------------------------------------------------------ 1. the kernels alone ----------------------------------------
def lib():
    from victor_amd import _native as N
    return N.load()


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def split(g, rows, which=None):
    m = len(rows)
    rows2, t, fail = np.full((2 * m, 12), -7.0), np.full(m, -7.0), np.full(m, -7, dtype=np.int32)
    which2 = np.full(2 * m, -7, dtype=np.int32)
    rc = lib().vk_blend_split(0, dp(g), len(g), dp(rows), None if which is None else ip(which), m, dp(rows2), ip(which2), dp(t), ip(fail))
    assert rc == 0
    return rows2, which2, t, fail


def merge(t, fail, per_row, raw_lnl, raw_chi):
    m = len(t)
    lnl, chi = np.full(m * per_row, -7.0), np.full(m * per_row, -7.0)
    assert lib().vk_blend_merge(0, dp(t), ip(fail), m, per_row, dp(raw_lnl), dp(raw_chi), dp(lnl), dp(chi)) == 0
    return lnl, chi


def host_split(g, rows):
    """``_run_likelihood_interp`` row by row; without a bracket (its IndexError) the failure mark, t = 0 and g[0] at both ends."""
    m = len(rows)
    both = np.concatenate([rows, rows])
    t, fail = np.zeros(m), np.zeros(m, dtype=np.int32)
    for i, b in enumerate(rows[:, P_BETA]):
        try:
            lo, hi = np.where(g < b)[0][-1], np.where(g >= b)[0][0]
        except IndexError:
            fail[i] = 1
            both[i, P_BETA] = both[m + i, P_BETA] = g[0]
            continue
        t[i] = (b - g[lo]) / (g[hi] - g[lo])
        both[i, P_BETA], both[m + i, P_BETA] = g[lo], g[hi]
    return both, t, fail


def special_betas(g):
    up, down = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    return np.array([g[1], g[-1], up(g[7]), down(g[7]), g[0], down(g[0]), up(g[0]), 0.05, up(g[-1]), 0.9, np.nan, np.inf, -np.inf,
                     g[15], down(g[-1]), 0.5 * (g[3] + g[4])])


def rows_with(beta, rng):
    rows = rng.standard_normal((len(beta), 12)) * 100.0
    rows[:, P_BETA] = beta
    return np.ascontiguousarray(rows)


@pytest.mark.parametrize("m", [1, 63, 257])
def test_split_kernel_against_the_numpy_expression(boss, m):
    """2 m = 2, 126, 514: below, across and past two workgroups of 256.  m = 1 takes every special value in turn."""
    g = np.ascontiguousarray(boss.beta_ccf)
    rng = np.random.default_rng(m)
    special = special_betas(g)
    outside_rule = lambda b: ~((b > g[0]) & (b <= g[-1]))                        # noqa: E731  (NaN: outside)
    for turn in range(len(special) if m == 1 else 1):
        beta = np.concatenate([np.roll(special, -turn), rng.uniform(0.1, 0.7, max(m - len(special), 0))])[:m]
        rows = rows_with(beta, rng)
        which = rng.integers(0, 5, m).astype(np.int32)
        want, want_t, want_fail = host_split(g, rows)
        assert np.array_equal(want_fail == 1, outside_rule(beta))
        rows2, which2, t, fail = split(g, rows, which)
        assert np.array_equal(fail, want_fail), (m, turn, beta[fail != want_fail])
        assert same_bytes(t, want_t), (m, turn, np.argwhere(t != want_t)[:4])
        assert same_bytes(rows2, want), (m, turn, np.argwhere(rows2 != want)[:4])
        assert np.array_equal(which2, np.concatenate([which, which]))
        _, untouched, t2, _ = split(g, rows)                                     # without realisation indices
        assert np.all(untouched == -7) and same_bytes(t2, want_t)
    if m > 16:
        ok = want_fail == 0
        assert np.any(want_t == 1.0) and np.any(ok & (want_t > 0) & (want_t < 1e-12)) and 6 <= (~ok).sum() < m // 2


def planted(n, free, rng):
    """lnl and chi2 [2 n] with every kind of value at either end - +-inf, NaN, zeros of either sign - one per output of ``free``
    (outputs of rows with a bracket and t < 1), in lnl first; finite everywhere else."""
    lnl, chi = -rng.uniform(1.0, 900.0, 2 * n), rng.uniform(1.0, 1800.0, 2 * n)
    slots = iter(free)
    for arr in (lnl, chi):
        for end in (0, n):
            for v in (np.inf, -np.inf, np.nan, 0.0, -0.0):
                k = next(slots, None)
                if k is not None:
                    arr[end + k] = v
    return lnl, chi


@pytest.mark.parametrize("m", [1, 63, 257])
@pytest.mark.parametrize("per_row", [1, 3])
def test_merge_kernel_bit_for_bit(boss, m, per_row):
    """``(1 - t) lo + t hi`` with NumPy's separate roundings; cross mode (n_real = 3): the row's t for its three outputs."""
    g = np.ascontiguousarray(boss.beta_ccf)
    rng = np.random.default_rng(100 * m + per_row)
    beta = np.concatenate([special_betas(g)[3 * (m == 1):], rng.uniform(0.1, 0.7, m)])[:m]
    _, t, fail = host_split(g, rows_with(beta, rng))
    n = m * per_row
    tt, ff = np.repeat(t, per_row), np.repeat(fail, per_row) != 0
    raw_lnl, raw_chi = planted(n, np.flatnonzero(~ff & (tt < 1.0)), rng)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(raw_lnl[:n]) | ~np.isfinite(raw_lnl[n:]) | ff
        want_l = (1 - tt) * raw_lnl[:n] + tt * raw_lnl[n:]
        want_c = (1 - tt) * raw_chi[:n] + tt * raw_chi[n:]
    want_l[bad], want_c[bad] = -np.inf, np.inf
    lnl, chi = merge(t, fail, per_row, raw_lnl, raw_chi)
    for got, want, name in ((lnl, want_l, "lnl"), (chi, want_c, "chi2")):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (name, m, per_row)
        assert same_bytes(got[~nan], want[~nan]), (name, m, per_row, np.argwhere(got[~nan] != want[~nan])[:4])
    assert not np.any(np.isnan(lnl)) and np.all(chi[bad] == np.inf) and np.all(lnl[bad] == -np.inf)
    if m > 16:
        assert bad.sum() > ff.sum() > 0 and np.any(np.isnan(want_c)) and np.any(~bad & (tt == 1.0))


# ------------------------------------------------------------------ 2. best fits and their Hessians ----------------------------
def both_fits(target, params, **kw):
    from tests.test_gpu_fit_definition import figures, same_fit
    ref = FD.best_fit(target, params, **kw)
    dev = target.best_fit(params, **kw)
    assert dev.names == ref.names
    figures(ref, "blend")
    same_fit(dev, ref, "blend")
    return ref, dev


def test_best_fit_of_the_data_vector_d2(boss):
    ref, dev = both_fits(boss, PARAMS, fixed=D2, restarts=1)
    assert ref.names == ["fsigma8", "beta"] and np.all(ref.status == FD.ST_CONVERGED) and np.all(np.isfinite(dev.lnl))
    plain = boss.best_fit(PARAMS, fixed=D2, restarts=1, beta_interpolation="datavector")       # (out of the mode, per call)
    assert not same_bytes(plain.lnl, dev.lnl)                                   # another posterior than the datavector mode's
    l, c = boss.log_likelihood_batch(dict(D2, fsigma8=dev.x[:, 0], beta=dev.x[:, 1]))
    g = boss.beta_ccf
    pts = lambda k: dict(D2, fsigma8=dev.x[:, 0], beta=g[k])                     # noqa: E731
    lo, hi = np.where(g < dev.x[0, 1])[0][-1], np.where(g >= dev.x[0, 1])[0][0]
    bound = np.maximum(chi2_bound(boss, pts([lo])), chi2_bound(boss, pts([hi])))
    assert_same_chi2(dev.chi2, c, bound, what="blend: best fit vs log_likelihood_batch")
    assert_same_lnl(dev.lnl, l, bound, what="blend: best fit vs log_likelihood_batch")


def test_best_fit_of_three_mocks(rs3):
    ref, dev = both_fits(rs3, PARAMS, fixed=D2, restarts=1)
    assert ref.x.shape == (3, 2) and np.all(ref.status == FD.ST_CONVERGED) and len(set(dev.lnl)) == 3


def test_laplace_inside_a_beta_cell(boss, rs3):
    """Between two nodes the blend is LINEAR in beta (both ends are evaluated at the nodes), so a fitted beta ends on a node and
    the Hessian has no curvature along it inside a cell: the covariance that exists there is the one of the other parameters at
    a beta held inside a cell - a blend of two negative-definite Hessians."""
    g = boss.beta_ccf
    beta = 0.5 * (g[12] + g[13]) + 0.001
    fixed = {"epsilon": 1.0, "beta": beta}
    for target, R in ((boss, 1), (rs3, 3)):
        bf = target.best_fit(PARAMS, fixed=fixed, covariance=True)
        assert bf.names == ["fsigma8", "sigma_v"] and bf.cov.shape == (R, 2, 2) and np.all(bf.status == bf.CONVERGED)
        assert np.all(np.isfinite(bf.cov)) and np.all(np.linalg.eigvalsh(bf.cov) > 0), bf.cov
        assert np.all(bf.laplace.status == 0), bf.laplace.status
        lap = target.laplace(PARAMS, bf, fixed=fixed)                   # a handle of its own
        assert np.all(np.isfinite(lap.cov)) and np.all(np.linalg.eigvalsh(lap.cov) > 0)
        np.testing.assert_allclose(lap.cov, bf.cov, rtol=1e-6)


# ------------------------------------------------------------------ 3. chains --------------------------------------------------
RUN = dict(walkers=4, seed=2)


def same_chains(dev, ref, what):
    from tests.test_gpu_chains import same_walk
    same_walk(dev, ref, what)
    for a in ("lnl_chain", "chi2_chain", "lnl", "chi2"):
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)
    assert 0.02 < ref.acceptance.mean() < 0.98, (what, ref.acceptance)


def final_state_is_the_likelihoods(fit, ch, fixed, what, exact=False):
    """The final lnl / chi2 of every walker against ``log_likelihood_batch`` in the same mode at its final x.  ``exact``: the
    launch that decided the walkers' last step held the same number of rows as this one call (Metropolis: all 4 walkers, 8 rows
    after the split), so the values are the same bits; a stretch half-step (2 walkers) and a tempered step (16 chains) were other
    launch sizes, which may be served by another kernel: held to the larger chi2_bound of the two bracketing evaluations, as
    tests/test_gpu_realisations.py holds the host blend."""
    x = ch.x.reshape(-1, len(ch.names))
    pts = dict(fixed, **{n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(ch.names)})
    lnl, chi2 = fit.log_likelihood_batch(pts)
    g = fit.beta_ccf
    beta = pts["beta"]
    assert np.all((beta > g[0]) & (beta <= g[-1]))
    lo = np.array([np.where(g < b)[0][-1] for b in beta])
    hi = np.array([np.where(g >= b)[0][0] for b in beta])
    bound = np.maximum(chi2_bound(fit, dict(pts, beta=g[lo])), chi2_bound(fit, dict(pts, beta=g[hi])))
    print(what, "final lnl equal as bytes:", same_bytes(ch.lnl.ravel(), lnl), "max |d lnl|", float(np.max(np.abs(ch.lnl.ravel() - lnl))))
    assert_same_chi2(ch.chi2.ravel(), chi2, bound, what=f"blend: final state vs log_likelihood_batch, {what}")
    assert_same_lnl(ch.lnl.ravel(), lnl, bound, what=f"blend: final state vs log_likelihood_batch, {what}")
    if exact:
        assert same_bytes(ch.lnl.ravel(), lnl) and same_bytes(ch.chi2.ravel(), chi2), what


def test_metropolis_chains(boss, rs3):
    kw = dict(fixed=D2, **RUN)
    ref = boss.sample_chains(PARAMS, 64, device=False, **kw)
    dev = boss.sample_chains(PARAMS, 64, **kw)
    assert dev.names == ["fsigma8", "beta"] and dev.chain.shape == (64, 1, 4, 2)
    same_chains(dev, ref, "blend: Metropolis, data vector")
    final_state_is_the_likelihoods(boss, dev, D2, "Metropolis", exact=True)
    ref = rs3.sample_chains(PARAMS, 64, device=False, **kw)                      # pairs mode: the realisation indices duplicated
    dev = rs3.sample_chains(PARAMS, 64, **kw)
    assert dev.chain.shape == (64, 3, 4, 2) and not same_bytes(dev.lnl[0], dev.lnl[1])
    same_chains(dev, ref, "blend: Metropolis, three mocks")


def test_stretch_ensemble(boss):
    from tests.test_gpu_stretch import BYTES
    kw = dict(fixed=D1, move="stretch", **RUN)
    ref = boss.sample_chains(PARAMS, 64, device=False, **kw)
    dev = boss.sample_chains(PARAMS, 64, **kw)
    assert dev.names == ["beta"] and dev.chain.shape == (64, 1, 4, 1) and 0.02 < ref.acceptance.mean() < 0.98
    for a in BYTES:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), ("blend: stretch", a)
    final_state_is_the_likelihoods(boss, dev, D1, "stretch")


def test_tempered_chains(boss):
    from tests.test_gpu_tempering import same_tempered
    kw = dict(fixed=D2, temper={"rungs": 4}, **RUN)
    ref = boss.sample_chains(PARAMS, 64, device=False, **kw)
    dev = boss.sample_chains(PARAMS, 64, **kw)
    assert dev.tempering.chain.shape == (64, 1, 4, 4, 2)
    same_tempered(dev, ref, "blend: tempered")
    final_state_is_the_likelihoods(boss, dev, D2, "tempered, cold rung")


def test_a_prior_box_wider_than_the_beta_grid(boss, rs3):
    """Proposals past either end of the grid report (-inf, +inf) and are rejected: every kept beta lies in (g[0], g[last]] and
    the run ends without a fault.  Chains started beside the last node with steps of three cells: about half the proposals of
    the first steps leave the grid."""
    g = boss.beta_ccf
    for target, R in ((boss, 1), (rs3, 3)):
        ch = target.sample_chains(WIDE, 64, walkers=8, seed=3, fixed=D2, start={"beta": 0.63, "fsigma8": 0.47}, scatter={"beta": 0.004,
                                  "fsigma8": 0.01}, proposal={"beta": 0.05, "fsigma8": 0.02})
        j = ch.names.index("beta")
        kept = ch.chain[..., j]
        assert kept.shape == (64, R, 8) and np.all((kept > g[0]) & (kept <= g[-1])), (kept.min(), kept.max())
        assert np.all(np.isfinite(ch.lnl_chain)) and np.all(np.isfinite(ch.chi2_chain))
        assert 0.0 < ch.acceptance.mean() < 1.0 and kept.max() > g[-2]


# ------------------------------------------------------------------ 4. nested sampling -----------------------------------------
NESTED = dict(n_live=32, batch=8, steps=4, n_iter=16, seed=1)


def test_nested_sampling(boss, rs3):
    from tests.test_gpu_nested import both, exercised
    for target, what in ((boss, "blend: nested, data vector"), (rs3, "blend: nested, three mocks")):
        dev, ref = both(target, PARAMS, what, fixed=EPS1, **NESTED)
        assert dev.names == ["fsigma8", "beta", "sigma_v"] and dev.dead_lnl.shape == (16, dev.R, 8)
        exercised(ref, what)


# ------------------------------------------------------------------ 5. grid posteriors ------------------------------------------
def guarded(call, g):
    """An ``evaluate`` callable of the definition route over the host blend ``call(batch)`` -> lnL: points outside (g[0],
    g[last]] are evaluated beside g[0] - the launch keeps its rows - and reported as -inf, the device's rule."""
    def evaluate(batch):
        beta = np.asarray(batch["beta"], dtype=float)
        out = ~((beta > g[0]) & (beta <= g[-1]))
        lnl = np.array(call(dict(batch, beta=np.where(out, g[1], beta))), dtype=np.float64)
        lnl[out] = -np.inf
        return lnl
    return evaluate


def beta_range(g):
    """Five bins of 1 / 16 whose first centre is node 15 exactly and whose last centre lies beyond the grid."""
    a = g[15] - 0.03125
    return a, a + 0.3125


@pytest.mark.parametrize("chunk", [7, 64])
def test_grid_posterior(boss, rs3, chunk):
    from victor_amd.grid import grid_posterior
    g = boss.beta_ccf
    kw = dict(bins={"fsigma8": 6, "beta": 5}, ranges={"fsigma8": (0.35, 0.6), "beta": beta_range(g)}, fixed=D2, chunk=chunk,
              pairs=[("fsigma8", "beta")])
    for target, R, call in ((boss, 1, lambda b: boss.log_likelihood_batch(b)[0]), (rs3, 3, lambda b: rs3.log_likelihood(b)[0])):
        dev = target.grid_posterior(WIDE, **kw)
        ref = grid_posterior(None, WIDE, device=False, evaluate=guarded(call, g), **kw)
        nodes = dev.axes["beta"]
        assert dev.shape == (6, 5) and nodes[0] == g[15] and nodes[3] < g[-1] < nodes[4]
        assert dev.n_problems == ref.n_problems == R and dev.chunk == ref.chunk and dev.n_chunks == -(-30 // chunk)
        TG.assert_exact(dev.raw, ref.raw, f"blend: grid, R = {R}, chunk {chunk}")
        assert same_bytes(dev.status, ref.status) and np.all(dev.status == dev.OK)
        TG.assert_sums(dev.raw, ref.raw, dev.n_chunks, f"blend: grid, R = {R}, chunk {chunk}", dev._grid)
        assert np.all(dev.n_finite == 24)                                       # the six cells of the last beta bin are not finite
        assert np.all(dev.marginal("beta")[:, 4] == 0) and np.all(dev.profile("beta")[:, 4] == -np.inf)
        assert np.all(dev.marginal("beta")[:, :4] > 0) and np.all(np.isfinite(dev.ln_evidence))


# ------------------------------------------------------------------ 6. importance-sampled posteriors ---------------------------
def test_importance_posterior_shared_proposal_cross_mode(rs3):
    """n = 256 points of one proposal against the three mocks: cross mode, [2 m][3] raw values per chunk of m points."""
    import victor_amd
    from tests.test_gpu_importance import CENTRE, WIDTH
    names = ["fsigma8", "beta"]
    q = victor_amd.GaussianProposal(names, [CENTRE[n] for n in names], np.diag([WIDTH[n] ** 2 for n in names]))
    kw = dict(n=256, seed=5, fixed=D2, chunk=100, bins=6, pairs=[("fsigma8", "beta")], min_ess=2.0)
    what = "blend: importance, shared proposal"
    dev = rs3.importance_posterior(PARAMS, q, **kw)
    rec = TI.Recorder(lambda batch: rs3.log_likelihood(batch)[0])
    ref = rs3.importance_posterior(PARAMS, q, device=False, evaluate=rec, **kw)
    assert dev.n_problems == ref.n_problems == 3 and dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks == len(rec.chunks) >= 2
    assert dev.n_drawn == ref.n_drawn == 256 and dev.n_inside == ref.n_inside > 128
    TI.assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status) and np.all(dev.n_finite == dev.n_inside)
    TI.assert_sums(dev.raw, ref.raw, TI.abs_sums(ref, rec.chunks), dev.n_chunks, what, dev._layout, dev._sample.x)
    for name in dev.names:
        assert same_bytes(dev.best[name], ref.best[name])
    assert len(set(dev.ln_max)) == 3 and np.all(np.isfinite(dev.ln_evidence))


def test_importance_posterior_a_proposal_per_mock_pairs_mode(stack, rs3):
    """A ProposalSet, n = 64 points per mock: pairs mode, rows [64][3] with their realisation indices duplicated."""
    from tests.test_gpu_importance_own import abs_sums_own, proposals
    from tests.test_importance_own import one_problem
    names = ["fsigma8", "beta"]
    qs = proposals(names, 3)
    kw = dict(n=64, seed=5, fixed=D2, chunk=30, bins=6, min_ess=2.0)
    what = "blend: importance, a proposal per mock"

    class Pairs:
        chunks = []

        def __call__(self, batch, which):
            v = np.asarray(rs3.log_likelihood_pairs(batch, which)[0], dtype=np.float64)
            self.chunks.append(v)
            return v
    rec = Pairs()
    dev = rs3.importance_posterior(PARAMS, qs, **kw)
    ref = rs3.importance_posterior(PARAMS, qs, device=False, evaluate=rec, **kw)
    assert dev.n_problems == ref.n_problems == 3 and dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks == len(rec.chunks) == 3
    assert dev.n_drawn == ref.n_drawn == 64 and np.array_equal(dev.n_inside, ref.n_inside) and np.all(dev.n_inside > 32)
    TI.assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status) and same_bytes(dev.n_finite, dev.n_inside)
    absolute, smp = abs_sums_own(ref, rec.chunks), ref._sample
    for r in range(3):
        TI.assert_sums(one_problem(dev.raw, r), one_problem(ref.raw, r), one_problem(absolute, r), dev.n_chunks, f"{what}, problem {r}",
                       dev._layout, smp.x[smp.inside[:, r], r])
    for name in dev.names:
        assert same_bytes(dev.best[name], ref.best[name]), (what, name)


# ------------------------------------------------------------------ 7. what a handle in this mode refuses ----------------------
def test_c_abi_refusals_of_a_blend_handle(boss):
    """The create call refuses the mode on a fixed data vector; a handle in the mode refuses what needs a point's theory vector,
    in words, and stays usable."""
    import victor_amd
    from victor_amd import _native as N
    from victor_amd.fitting import _Sampled, blend_opts
    q = _Sampled("best_fit", "fitted", PARAMS, D2)
    batch = dict(D2, fsigma8=np.array([0.47]), beta=np.array([0.4]))
    fo = boss._merged_fit({})
    library, h, _ = q.create("vk_fit_create", boss, None, {}, fo, batch, np.arange(1, dtype=np.int32))
    try:
        x, hh = np.array([[0.47, 0.4]]), np.array([[0.01, 0.01]])
        out, st = np.zeros(4), np.zeros(1, dtype=np.int32)
        rc = library.vk_fit_fisher(h, dp(x), dp(hh), None, dp(out), dp(out.copy()), dp(out.copy()), dp(np.zeros(1)), ip(st))
        assert rc == -1 and "two" in library.vk_fit_last_error(h).decode() and "VK_OPT_BETA_BLEND" in library.vk_fit_last_error(h).decode()
    finally:
        library.vk_fit_destroy(h)
    fixed = victor_amd.CCFFit(*stack_options(fixed=True))
    assert fixed.fixed_data
    model = fixed._merged({})
    eng = fixed._get_engine(fixed._engine_key(model), model["simpson_even"])
    opts = eng.make_opts(model, fixed._merged_fit({}))
    assert blend_opts(fixed, fixed._merged_fit(LIKE), opts) is opts            # Python never asks for it there
    opts.reserved = N.VK_OPT_BETA_BLEND
    rows = np.ascontiguousarray(fixed._fit_rows(batch, model), dtype=np.float64)
    cols = np.array([N.P_FSIGMA8, N.P_BETA], dtype=np.int32)
    err = C.create_string_buffer(512)
    none = eng._lib.vk_fit_create(eng._ctx, C.byref(opts), 1, 2, ip(cols), dp(N.f64(q.lo)), dp(N.f64(q.hi)), dp(rows), 1.0, None, err, len(err))
    assert not none and "gridded in beta" in err.value.decode()
