"""Stretch-move ensembles stepped on the GPU (``sample_chains(move="stretch")``, vk_chain_begin_stretch) against the NumPy loop
that defines them (``device=False``: one likelihood call of R W / 2 rows per half-step): with epsilon fixed both routes launch the
same rows in launches of the same shape, so everything is compared byte for byte; with epsilon sampled positions and decisions,
under the decision-margin precondition of tests/test_gpu_chains.py.  Then the refusals of the C entry point against a live
handle, and Metropolis blocks around a stretch block on one handle."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases
from tests.test_chains import assert_sums, same_bytes
from tests.test_gpu_joint_sampled import Case
from tests.test_realisations import stack_options

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
EPS_FIXED = {"epsilon": 1.0}
MARGIN = 1e-6            # as tests/test_gpu_chains.py
# Seed of the epsilon-sampled comparison: the first of 0, 1, 2, ... whose smallest decision margin on the definition route
# (3 realisations, W = 10, 70 sweeps) exceeds MARGIN, picked with the definition route alone.
SEED_EPSILON = 0         # observed smallest margin 3.5e-3
BYTES = ("pivot", "chain", "lnl_chain", "chi2_chain", "x", "lnl", "chi2", "n_accept", "acceptance")
STATE = ("pivot", "x", "lnl", "chi2", "n_accept", "acceptance")
RUN = dict(walkers=8, seed=2, burn=5, thin=3, move="stretch")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def fit():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


@pytest.fixture(scope="module")
def rs9():
    """Nine realisations: with W = 8, 72 walkers - 36 rows per half-launch, a partial wave, two workgroups of walkers."""
    import victor_amd
    return victor_amd.CCFFit(*stack_options()).realisations(list(range(9)))


@pytest.fixture(scope="module")
def ref9(rs9):
    """The definition route's 70 sweeps of the nine ensembles (epsilon fixed), computed once."""
    return rs9.sample_chains(PARAMS, 70, device=False, fixed=EPS_FIXED, **RUN)


def same_run(dev, ref, what, attrs=BYTES):
    assert dev.move == ref.move == "stretch" and dev.rhat is None and ref.rhat is None
    assert dev.n_steps == ref.n_steps and dev.n_kept == ref.n_kept, what
    for a in attrs:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)


# ------------------------------------------------------------------ 7. a single fit and realisations ------------------------
def test_data_vector_ensemble_byte_for_byte(fit):
    ref = fit.sample_chains(PARAMS, 70, device=False, fixed=EPS_FIXED, **RUN)
    dev = fit.sample_chains(PARAMS, 70, fixed=EPS_FIXED, **RUN)
    assert dev.chain.shape == (22, 1, 8, 3) and dev.names == ["fsigma8", "beta", "sigma_v"]
    assert 0.05 < ref.acceptance[0] < 0.95, ref.acceptance
    same_run(dev, ref, "data vector")
    assert_sums(dev.sum1[0], dev.sum2[0], dev.chain[:, 0], dev.pivot[0], "device sums")
    cut = fit.sample_chains(PARAMS, 30, fixed=EPS_FIXED, **RUN).extend(40)            # a cut in the middle of a block
    same_run(cut, ref, "30 + 40")
    assert same_bytes(cut.sum1, dev.sum1) and same_bytes(cut.sum2, dev.sum2)


def test_realisation_ensembles_byte_for_byte(rs9, ref9):
    dev = rs9.sample_chains(PARAMS, 70, fixed=EPS_FIXED, **RUN)
    assert dev.chain.shape == (22, 9, 8, 3) and dev.n_kept == 22
    assert np.all((0.05 < ref9.acceptance) & (ref9.acceptance < 0.95)), ref9.acceptance
    same_run(dev, ref9, "nine realisations")
    assert dev.decision_margin is None and dev.n_outside is None and np.isfinite(ref9.decision_margin)
    for m in range(9):
        assert_sums(dev.sum1[m], dev.sum2[m], dev.chain[:, m], dev.pivot[m], f"device sums, realisation {m}")
    assert dev.mean.shape == (9, 3) and np.all(np.isfinite(dev.cov))


def test_keep_chain_off_and_a_cut_inside_a_block(rs9, ref9):
    lean = rs9.sample_chains(PARAMS, 70, fixed=EPS_FIXED, keep_chain=False, **RUN)
    assert lean.chain is None and lean.lnl_chain is None and lean.rhat is None
    same_run(lean, ref9, "keep_chain=False", STATE)
    cut = rs9.sample_chains(PARAMS, 41, fixed=EPS_FIXED, **RUN).extend(29)             # 41 + 23 | 6: both cuts inside blocks
    same_run(cut, ref9, "41 + 29")
    whole = rs9.sample_chains(PARAMS, 70, fixed=EPS_FIXED, **RUN)
    for a in ("sum1", "sum2", "mean", "cov"):
        assert same_bytes(getattr(cut, a), getattr(whole, a)), a
        assert same_bytes(getattr(lean, a), getattr(whole, a)), a


# ------------------------------------------------------------------ 8. proposals that leave the box -------------------------
def test_a_narrow_prior_box(rs9):
    lo, hi = 360.0, 400.0
    narrow = dict(PARAMS, sigma_v=dict(PARAMS["sigma_v"], prior={"dist": "uniform", "min": lo, "max": hi}, ref={"loc": 380.0, "scale": 5.0}))
    ref = rs9.sample_chains(narrow, 70, device=False, fixed=EPS_FIXED, **RUN)
    print("proposals outside the box:", ref.n_outside.sum(), "of", 70 * 72)
    assert ref.n_outside.sum() > 0
    dev = rs9.sample_chains(narrow, 70, fixed=EPS_FIXED, **RUN)
    j = dev.names.index("sigma_v")
    assert np.all(dev.chain[..., j] >= lo) and np.all(dev.chain[..., j] <= hi)
    same_run(dev, ref, "narrow box")


# ------------------------------------------------------------------ 9. joint fits -------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory.mktemp(name))
        return made[name]
    return get


@pytest.mark.parametrize("name,data", [("dsplit_cov", True), ("dsplit_cov", False), ("dsplit_diag", False)])
def test_joint_ensembles_byte_for_byte(case, name, data):
    c = case(name)
    target = c.joint if data else c.joint.realisations([0, 1, 2])
    kw = dict(RUN, fixed=dict(c.fixed, epsilon=1.0))
    ref = target.sample_chains(PARAMS, 66, device=False, **kw)
    dev = target.sample_chains(PARAMS, 66, **kw)
    assert dev.names == c.without("epsilon") and dev.chain.shape == (21, 1 if data else 3, 8, 2)
    print(name, "data" if data else "mocks", "acceptance of the definition route:", ref.acceptance)
    assert 0.05 < ref.acceptance.mean() < 0.95
    same_run(dev, ref, name)


# ------------------------------------------------------------------ 10. epsilon sampled -------------------------------------
def test_epsilon_sampled():
    import victor_amd
    rs = victor_amd.CCFFit(*stack_options()).realisations([0, 1, 2])
    kw = dict(RUN, walkers=10, seed=SEED_EPSILON)
    ref = rs.sample_chains(PARAMS, 70, device=False, **kw)
    print("smallest decision margin (definition route):", ref.decision_margin)
    assert ref.decision_margin > MARGIN, ref.decision_margin            # a condition on the inputs, not on the code under test
    dev = rs.sample_chains(PARAMS, 70, **kw)
    assert dev.names == ["fsigma8", "beta", "sigma_v", "epsilon"] and dev.chain.shape == (22, 3, 10, 4)
    same_run(dev, ref, "epsilon sampled", ("pivot", "chain", "x", "n_accept", "acceptance"))
    assert np.allclose(dev.lnl_chain, ref.lnl_chain, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ raw handles ---------------------------------------------
class Raw:
    """A chain handle made as sample_chains makes it (epsilon fixed), driven through the C ABI."""

    def __init__(self, rs, x0, W):
        from victor_amd.fitting import _Sampled
        q = _Sampled("sample_chains", "sampled", PARAMS, EPS_FIXED)
        self.names, self.d, self.C, self.W = q.names, len(q.names), len(x0), W
        self.lo, self.hi = q.lo, q.hi
        self.which = np.repeat(np.arange(len(rs), dtype=np.int32), W)
        self.fixed = {k: float(v) for k, v in q.fixed_all.items()}
        self.rs = rs
        self.lib, self.h, self._refresh = q.create("vk_chain_create", rs.fit, rs, {}, q.fit_options(rs.fit, {}), self.batch(x0), self.which)

    def batch(self, x):
        return dict(self.fixed, **{n: np.ascontiguousarray(x[:, j]) for j, n in enumerate(self.names)})

    def error(self):
        return self.lib.vk_chain_last_error(self.h).decode()

    def start(self, x0):
        return self.lib.vk_chain_start(self.h, x0.ctypes.data_as(C.POINTER(C.c_double)))

    def stretch(self, z, lz, logu, k, walkers=None, first=0, n=None):
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        ptr = [None if a is None else np.ascontiguousarray(a).ctypes.data_as(dp) for a in (z, lz, logu)]
        kept = C.c_int32(-1)
        return self.lib.vk_chain_begin_stretch(self.h, len(logu) if n is None else n, self.W if walkers is None else walkers, *ptr,
                                               None if k is None else k.ctypes.data_as(ip), first, 0, 1, 1, C.byref(kept)), kept.value

    def metropolis(self, dz, logu, first):
        dp = C.POINTER(C.c_double)
        kept = C.c_int32(-1)
        return self.lib.vk_chain_begin(self.h, len(dz), dz.ctypes.data_as(dp), logu.ctypes.data_as(dp), first, 0, 1, 1, C.byref(kept)), kept.value

    def finish(self, m):
        dp = C.POINTER(C.c_double)
        hx, hl, hc = np.empty((m, self.C, self.d)), np.empty((m, self.C)), np.empty((m, self.C))
        rc = self.lib.vk_chain_finish(self.h, hx.ctypes.data_as(dp), hl.ctypes.data_as(dp), hc.ctypes.data_as(dp))
        return rc, hx, hl, hc

    def state(self):
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        x, lnl, chi2 = np.empty((self.C, self.d)), np.empty(self.C), np.empty(self.C)
        acc, steps = np.empty(self.C, dtype=np.int64), np.empty(self.C, dtype=np.int64)
        assert self.lib.vk_chain_state(self.h, x.ctypes.data_as(dp), lnl.ctypes.data_as(dp), chi2.ctypes.data_as(dp),
                                       acc.ctypes.data_as(lp), steps.ctypes.data_as(lp), None, None, None, None) == 0, self.error()
        return x, lnl, chi2, acc, steps

    def close(self):
        self.lib.vk_chain_destroy(self.h)
        self.h = None


def stretch_numbers(rng, n, M, half, d):
    z = 0.5 * (rng.random((n, 2, M)) + 1.0) ** 2
    return z, (d - 1) * np.log(z), np.log(rng.random((n, 2, M))), rng.integers(0, half, size=(n, 2, M)).astype(np.int32)


# ------------------------------------------------------------------ 11. the refusals of the C entry point -------------------
def test_c_abi_refusals_leave_the_handle_usable(rs9, ref9):
    x0 = np.ascontiguousarray(ref9.pivot.reshape(72, 3))
    raw = Raw(rs9, x0, 8)
    try:
        z, lz, logu, k = stretch_numbers(np.random.default_rng(1), 3, 36, 4, 3)
        assert raw.stretch(z, lz, logu, k)[0] == -1 and "no start" in raw.error()
        assert raw.start(x0) == 0, raw.error()
        before = raw.state()

        def refused(text, *a, **kw):
            rc, _ = raw.stretch(*a, **kw)
            assert rc == -1 and text in raw.error(), (text, rc, raw.error())
        refused("not a whole number of ensembles", z, lz, logu, k, walkers=10)
        refused("even number of walkers", z, lz, logu, k, walkers=9)
        refused("even number of walkers", z, lz, logu, k, walkers=0)
        for bad in (4, -1, 1 << 30):
            kb = k.copy()
            kb[2, 1, 35] = bad                                       # the very last entry of the block
            refused(f"partner index {bad}", z, lz, logu, kb)
        k6 = (k % 6).astype(np.int32)
        refused("not of the realisation of its ensemble", z, lz, logu, k6, walkers=12)     # 72 = 6 x 12: ensembles across mocks
        for hole in range(4):
            a = [z, lz, logu, k]
            a[hole] = None
            refused("NULL argument", *a, n=3)
        refused("1 <= sweeps <= 64", z, lz, logu, k, n=0)
        refused("1 <= sweeps <= 64", z, lz, logu, k, n=65)
        refused("first_step >= 0", z, lz, logu, k, first=-1)
        for a, b in zip(before, raw.state()):                        # nothing ran
            assert same_bytes(a, b)
        # a block in flight refuses the next, and the handle works on: its three sweeps are the definition route's first three
        rc, m = raw.stretch(z, lz, logu, k)
        assert rc == 0 and m == 3, raw.error()
        refused("has not been finished", z, lz, logu, k)
        rc, hx, hl, hc = raw.finish(3)
        assert rc == 0, raw.error()
        x, lnl, chi2 = x0.copy(), before[1].copy(), before[2].copy()
        which = np.repeat(np.arange(9, dtype=np.int32), 4)
        for t in range(3):                                           # the definition's half-steps, restated on these numbers
            for h in range(2):
                mv = (np.arange(9)[:, None] * 8 + 4 * h + np.arange(4)).ravel()
                p = x[np.repeat(np.arange(9) * 8 + 4 * (1 - h), 4) + k[t, h]]
                prop = p + z[t, h][:, None] * (x[mv] - p)
                inside = ((prop >= raw.lo) & (prop <= raw.hi)).all(axis=1)
                l, c2 = rs9.log_likelihood_pairs(raw.batch(np.where(inside[:, None], prop, x[mv])), which)
                l = np.where(inside, l, -np.inf)
                with np.errstate(invalid="ignore"):
                    acc = logu[t, h] < lz[t, h] + l - lnl[mv]
                x[mv[acc]], lnl[mv[acc]], chi2[mv[acc]] = prop[acc], l[acc], c2[acc]
            assert same_bytes(hx[t], x) and same_bytes(hl[t], lnl) and same_bytes(hc[t], chi2), t
        assert np.all(raw.state()[4] == 3)
    finally:
        raw.close()


# ------------------------------------------------------------------ 12. Metropolis blocks around a stretch block -------------
def test_metropolis_blocks_around_a_stretch_block(rs9, ref9):
    x0 = np.ascontiguousarray(ref9.pivot.reshape(72, 3))
    rng = np.random.default_rng(4)
    width = np.array([PARAMS[n]["proposal"] for n in ("fsigma8", "beta", "sigma_v")], dtype=float)
    dz1, lu1 = width * rng.standard_normal((5, 72, 3)), np.log(rng.random((5, 72)))
    dz2, lu2 = width * rng.standard_normal((6, 72, 3)), np.log(rng.random((6, 72)))
    z, lz, logu, k = stretch_numbers(rng, 4, 36, 4, 3)
    a, b = Raw(rs9, x0, 8), Raw(rs9, x0, 8)
    try:
        first = []
        for raw in (a, b):                                           # (one block in flight on the context at a time)
            assert raw.start(x0) == 0, raw.error()
            rc, m = raw.metropolis(dz1, lu1, 0)
            assert rc == 0 and m == 5, raw.error()
            first.append(raw.finish(5))
        for got, want in zip(first[0], first[1]):
            assert same_bytes(got, want)
        rc, m = a.stretch(z, lz, logu, k, first=5)
        assert rc == 0 and m == 4, a.error()
        assert a.finish(4)[0] == 0, a.error()
        x, lnl, chi2, acc0, steps = a.state()
        assert np.all(steps == 9) and not same_bytes(x, first[0][1][-1])
        rc, m = a.metropolis(dz2, lu2, 9)
        assert rc == 0 and m == 6, a.error()
        rc, hx, hl, hc = a.finish(6)
        assert rc == 0, a.error()
        # ... against the Metropolis definition (victor_amd/chains.py), restated on these numbers from the stretch block's end state
        n_acc = np.zeros(72, dtype=np.int64)
        for t in range(6):
            prop = x + dz2[t]
            inside = ((prop >= a.lo) & (prop <= a.hi)).all(axis=1)
            l, c2 = rs9.log_likelihood_pairs(a.batch(np.where(inside[:, None], prop, x)), a.which)
            l = np.where(inside, l, -np.inf)
            with np.errstate(invalid="ignore"):
                acc = lu2[t] < l - lnl
            x[acc], lnl[acc], chi2[acc] = prop[acc], l[acc], c2[acc]
            n_acc += acc
            assert same_bytes(hx[t], x) and same_bytes(hl[t], lnl) and same_bytes(hc[t], chi2), t
        assert n_acc.sum() > 0
        end = a.state()
        assert same_bytes(end[0], x) and np.array_equal(end[3] - acc0, n_acc) and np.all(end[4] == 15)
    finally:
        a.close()
        b.close()
