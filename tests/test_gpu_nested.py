"""Nested sampling stepped on the GPU (victor_amd/nested.py, vk_nested_begin, vk_kernel_nested.h) against the
NumPy loop that defines it (``device=False``): with epsilon fixed both routes launch the same rows in launches of the same shape,
so the dead record (lnL, chi2, x), the final live points and the counters are compared byte for byte - on the synthetic fit and on
the beta-dependent BOSS fit, mocks and the data vector, rows and live points past one wave, more problems than a wave with repeated
mocks, K = 1, paired models, a joint fit under one covariance and block-diagonal mocks with a dispersion per block; epsilon sampled
at the margin of tests/test_gpu_chains.py; cuts; every dead point against an independent ``log_likelihood_pairs`` call; and the
refusals of the C entry points.  The shapes are the smallest that reach every path of the algorithm; the live-point counts and row
bands the product runs at - the select kernel's loops past one trip, its LDS arrays full, problems across workgroup edges, every
regime of the evaluation up to 8192 rows, stuck walkers and planted ties - are in tests/test_gpu_nested_shapes.py (the ``NESTED``
table of tests/launch_shapes.py), which imports ``both``, ``same_run``, ``exercised`` and ``Raw`` from here.  No assertion is on
elapsed time."""

import ctypes as C
import faulthandler
import os

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_chains import MARGIN
from tests.test_realisations import stack_options
from tests.tolerances import assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
EPS1 = {"epsilon": 1.0}                                   # d = 3: fsigma8, beta, sigma_v
SYNTH = {"fsigma8": {"prior": {"min": 0.3, "max": 0.6}}, "sigma_v": {"prior": {"min": 250.0, "max": 450.0}},
         "beta": {"prior": {"min": 0.3, "max": 0.5}}}
SMALL = dict(n_live=8, batch=2, steps=3, n_iter=6, seed=1)
BYTES = ("dead_lnl", "dead_chi2", "dead_x", "x", "lnl", "chi2", "n_accept", "n_steps", "n_stuck", "ln_evidence", "information",
         "ln_evidence_error", "weights", "samples", "mean", "cov", "status")


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def stack():
    import victor_amd
    return victor_amd.CCFFit(*stack_options())


@pytest.fixture(scope="module")
def rs3(stack):
    return stack.realisations([0, 1, 2])


@pytest.fixture(scope="module")
def boss():
    import victor_amd
    return victor_amd.CCFFit(*cases.boss_options("config"))


@pytest.fixture(scope="module")
def synth3(tmp_path_factory):
    """Three mocks of the isotropic synthetic fit (N = 80): its data vector with 2 % noise."""
    import victor_amd
    tmp = tmp_path_factory.mktemp("nested_synth")
    d = np.load(os.path.join(cases.GOLDEN, "synth", "data2.npy"), allow_pickle=True).item()
    rng = np.random.default_rng(5)
    path = os.path.join(str(tmp), "synth_data_stack.npy")
    np.save(path, dict(d, **{k: d[k][None] * (1.0 + 0.02 * rng.standard_normal((3,) + d[k].shape)) for k in ("monopole", "quadrupole")}),
            allow_pickle=True)
    model, data = cases.synth_options(2)
    data["redshift_space_ccf"].update(data_file=path, simulation_number=0)
    fit = victor_amd.CCFFit(model, data)
    assert len(fit.s) * len(np.atleast_1d(fit.poles_s)) == 80
    return fit.realisations()


def both(obj, params, what, **kw):
    """The definition route and the device route of one call, compared as bytes."""
    ref = obj.nested_sampling(params, device=False, **kw)
    dev = obj.nested_sampling(params, **kw)
    same_run(dev, ref, what)
    assert dev.decision_margin is None and ref.decision_margin is not None
    return dev, ref


def same_run(dev, ref, what):
    assert dev.n_iter == ref.n_iter and dev.names == ref.names, what
    for a in BYTES:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (what, a)


def exercised(ref, what, stuck=False):
    """The definition route's run reached what the test is about (a condition on the inputs, not on the code under test)."""
    print(what, "acceptance", ref.acceptance, "stuck", ref.n_stuck, "margin", ref.decision_margin, "ln Z", ref.ln_evidence)
    assert np.all((0 < ref.n_accept) & (ref.n_accept < ref.n_steps)), what        # both outcomes of a step, in every problem
    assert np.all(np.isfinite(ref.dead_lnl)) and np.all(np.diff(ref.dead_lnl.transpose(1, 0, 2).reshape(ref.R, -1), axis=1) >= 0), what
    if stuck:
        assert ref.n_stuck.sum() > 0, what


# ------------------------------------------------------------------ 1. the device route is the definition route --------------
def test_synthetic_mocks(synth3):
    dev, ref = both(synth3, SYNTH, "synthetic mocks", fixed=EPS1, **SMALL)
    assert dev.names == ["fsigma8", "sigma_v", "beta"] and dev.dead_x.shape == (6, 3, 2, 3) and dev.x.shape == (3, 8, 3)
    exercised(ref, "synthetic mocks")
    assert not same_bytes(dev.dead_lnl[:, 0], dev.dead_lnl[:, 1])


def test_boss_mocks(rs3):
    dev, ref = both(rs3, PARAMS, "BOSS mocks", fixed=EPS1, **SMALL)
    assert dev.names == ["fsigma8", "beta", "sigma_v"] and dev.dead_lnl.shape == (6, 3, 2)
    exercised(ref, "BOSS mocks")


def test_data_vector(boss):
    dev, ref = both(boss, PARAMS, "data vector", fixed=EPS1, **SMALL)
    assert dev.R == 1 and dev.samples.shape == (1, 12 + 8, 3)
    exercised(ref, "data vector")


def test_rows_and_live_points_past_one_wave(boss):
    """160 live points (two and a half waves of the select kernel's strided loops), 80 rows (a whole wave and a quarter)."""
    dev, ref = both(boss, PARAMS, "L = 160, K = 80", fixed=EPS1, n_live=160, batch=80, steps=2, n_iter=3, seed=2)
    assert dev.dead_lnl.shape == (3, 1, 80)
    exercised(ref, "L = 160, K = 80")


def test_more_problems_than_a_wave_with_repeated_mocks(stack):
    rs = stack.realisations(list(np.arange(70) % 16))
    dev, ref = both(rs, PARAMS, "R = 70", fixed=EPS1, n_live=4, batch=2, steps=2, n_iter=3, seed=4)
    assert dev.R == 70 and dev.dead_lnl.shape == (3, 70, 2)
    # problems r and r + 16 run on the same mock from the same start: the first dead points are the same bytes, then they part
    assert same_bytes(dev.dead_lnl[0, :54], dev.dead_lnl[0, 16:]) and same_bytes(dev.dead_x[0, :54], dev.dead_x[0, 16:])
    assert not same_bytes(dev.x[:54], dev.x[16:])


def test_one_walker_per_problem(rs3):
    dev, ref = both(rs3, PARAMS, "K = 1", fixed=EPS1, n_live=4, batch=1, steps=3, n_iter=8, seed=3)
    assert dev.dead_lnl.shape == (8, 3, 1)
    exercised(ref, "K = 1")


def test_paired_models(tmp_path):
    import victor_amd
    from tests.test_paired_realisations import NUMBERS, paired_boss_options
    paired = victor_amd.CCFFit(*paired_boss_options(tmp_path, number=NUMBERS[0])).realisations(NUMBERS, paired_model=True)
    dev, ref = both(paired, PARAMS, "paired models", fixed=EPS1, **SMALL)
    exercised(ref, "paired models")
    shared = paired.fit.realisations(NUMBERS).nested_sampling(PARAMS, fixed=EPS1, **SMALL)
    assert not same_bytes(shared.dead_lnl, dev.dead_lnl)                     # (every mock's own model is read)


@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_joint_fits(tmp_path_factory, name):
    """A joint fit under one covariance (its data vectors, one row for all blocks) and block-diagonal mocks with a velocity
    dispersion per block."""
    from tests.test_gpu_joint_sampled import BETA, Case
    from victor_amd.joint import per_block
    c = Case(name, tmp_path_factory.mktemp("nested_" + name))
    fixed = {"beta": BETA, "epsilon": 1.0}
    if name == "dsplit_cov":
        dev, ref = both(c.joint, PARAMS, name, fixed=fixed, **SMALL)
        assert dev.names == ["fsigma8", "sigma_v"] and dev.R == 1
    else:
        dev, ref = both(c.jr, per_block(PARAMS, ["sigma_v"], 3), name, fixed=fixed, **SMALL)
        assert dev.names == ["fsigma8", "sigma_v@0", "sigma_v@1", "sigma_v@2"] and dev.R == len(c.jr)
        assert not same_bytes(dev.dead_x[..., 1], dev.dead_x[..., 2])
    exercised(ref, name)


# ------------------------------------------------------------------ 2. epsilon sampled ---------------------------------------
def test_device_route_with_epsilon_sampled(rs3, stack):
    """The seed is the first of 0, 1, 2, ... whose smallest margin on the definition route (decisions and the order of the dead
    points) exceeds MARGIN: chosen here, with the definition route alone, before the device route runs."""
    import victor_amd
    ref = None
    for seed in range(8):
        kw = dict(SMALL, seed=seed)
        ref = rs3.nested_sampling(PARAMS, device=False, **kw)
        print("seed", seed, "smallest margin (definition route):", ref.decision_margin)
        if ref.decision_margin > MARGIN:
            break
    assert ref.decision_margin > MARGIN, ref.decision_margin     # a condition on the inputs, not on the code under test
    dev = rs3.nested_sampling(PARAMS, **kw)
    assert dev.names == ["fsigma8", "beta", "sigma_v", "epsilon"]
    for a in ("dead_x", "x", "n_accept", "n_steps", "n_stuck", "samples"):          # identical decisions and order
        assert same_bytes(getattr(dev, a), getattr(ref, a)), a
    for m in range(3):
        fit = victor_amd.CCFFit(*stack_options(simulation_number=m))
        x = np.concatenate([ref.dead_x[:, m].reshape(-1, 4), ref.x[m]])
        bound = chi2_bound(fit, {n: x[:, j] for j, n in enumerate(ref.names)})
        assert_same_chi2(np.concatenate([dev.dead_chi2[:, m].ravel(), dev.chi2[m]]), np.concatenate([ref.dead_chi2[:, m].ravel(), ref.chi2[m]]),
                         bound, what="nested sampling, epsilon sampled: device vs definition route")
        assert_same_lnl(np.concatenate([dev.dead_lnl[:, m].ravel(), dev.lnl[m]]), np.concatenate([ref.dead_lnl[:, m].ravel(), ref.lnl[m]]),
                        bound, what="nested sampling, epsilon sampled: device vs definition route")


# ------------------------------------------------------------------ 3. cuts, and the likelihood ----------------------------
def test_six_iterations_equal_two_plus_four(rs3):
    whole = rs3.nested_sampling(PARAMS, fixed=EPS1, **SMALL)
    cut = rs3.nested_sampling(PARAMS, fixed=EPS1, **dict(SMALL, n_iter=2)).extend(4)
    same_run(cut, whole, "2 + 4")
    again = rs3.nested_sampling(PARAMS, fixed=EPS1, **SMALL)
    same_run(again, whole, "a second run")
    long = rs3.nested_sampling(PARAMS, fixed=EPS1, **dict(SMALL, n_iter=11))           # across a block of 8 iterations
    pieces = rs3.nested_sampling(PARAMS, fixed=EPS1, **dict(SMALL, n_iter=7)).extend(2).extend(2)
    same_run(pieces, long, "7 + 2 + 2")
    assert same_bytes(long.dead_lnl[:6], whole.dead_lnl)
    lean = rs3.nested_sampling(PARAMS, fixed=EPS1, keep_dead=False, **SMALL)
    assert lean.dead_x is None and lean.samples is None and same_bytes(lean.dead_lnl, whole.dead_lnl) and same_bytes(lean.x, whole.x)


def test_every_dead_point_is_what_the_likelihood_says(rs3):
    import victor_amd
    ns = rs3.nested_sampling(PARAMS, fixed=EPS1, **SMALL)
    T, R, K, d = ns.dead_x.shape
    x = np.concatenate([ns.dead_x.reshape(T * R * K, d), ns.x.reshape(-1, d)])
    which = np.concatenate([np.tile(np.repeat(np.arange(R, dtype=np.int32), K), T), np.repeat(np.arange(R, dtype=np.int32), ns.n_live)])
    pts = dict({n: x[:, j] for j, n in enumerate(ns.names)}, epsilon=np.ones(len(x)))
    lnl, chi2 = rs3.log_likelihood_pairs(pts, which)
    bound = np.empty(len(x))
    for m in range(R):
        sel = which == m
        bound[sel] = chi2_bound(victor_amd.CCFFit(*stack_options(simulation_number=m)), {n: v[sel] for n, v in pts.items()})
    assert_same_chi2(np.concatenate([ns.dead_chi2.ravel(), ns.chi2.ravel()]), chi2, bound, what="dead and live points vs log_likelihood_pairs")
    assert_same_lnl(np.concatenate([ns.dead_lnl.ravel(), ns.lnl.ravel()]), lnl, bound, what="dead and live points vs log_likelihood_pairs")
    assert np.all(ns.dead_x >= ns._lo) and np.all(ns.dead_x <= ns._hi)


# ------------------------------------------------------------------ 4. the refusals of the entry points ---------------------
class Raw:
    """A raw vk_nested handle of three mocks (R K rows), for what the public route never asks."""

    def __init__(self, rs, L=8, K=2, S=3, scale=0.3, expect_null=False):
        from victor_amd import _native as N
        from victor_amd.fitting import _Sampled
        self.N = N
        q = _Sampled("nested_sampling", "sampled", PARAMS, EPS1)
        self.R, self.L, self.K, self.S, self.d = len(rs), L, K, S, len(q.names)
        self.lo, self.hi = q.lo, q.hi
        rows = self.R * K
        mid = 0.5 * (q.lo + q.hi)
        batch = dict({k: float(v) for k, v in q.fixed_all.items()}, **{n: np.full(rows, mid[j]) for j, n in enumerate(q.names)})
        which = np.repeat(np.arange(self.R, dtype=np.int32), K)
        self.h = None
        self.lib, self.h, _ = q.create("vk_nested_create", rs.fit, rs, {}, q.fit_options(rs.fit, {}), batch, which, shape=(L, K, S, scale))

    def error(self):
        return (self.lib.vk_nested_last_error(self.h) or b"").decode()

    def x0(self, seed=0):
        u = np.random.default_rng(seed).random((self.R, self.L, self.d))
        return np.ascontiguousarray(self.lo + u * (self.hi - self.lo))

    def numbers(self, n, seed=1):
        rng = np.random.default_rng(seed)
        return rng.random((n, self.R, self.K)), rng.standard_normal((n, self.S, self.R, self.K, self.d))

    def begin(self, n, first, pick=None, dz=None, give=(True, True)):
        p, z = self.numbers(max(n, 1))
        dp = self.N.as_dp
        return self.lib.vk_nested_begin(self.h, n, dp(p) if give[0] else None, dp(z) if give[1] else None, first, 1)

    def close(self):
        if self.h:
            self.lib.vk_nested_destroy(self.h)
            self.h = None


def test_c_abi_refusals(rs3):
    from victor_amd import InputError
    for shape, text in (((1, 1, 3, 0.3), "live points"), ((8, 3, 3, 0.3), "must divide"), ((8, 8, 3, 0.3), "at most half"),
                        ((8, 2, 0, 0.3), "steps"), ((8, 2, 3, 0.0), "scale"), ((8192, 2, 3, 0.3), "4096")):
        with pytest.raises(InputError, match=text):
            Raw(rs3, *shape)
    raw = Raw(rs3)
    dp = raw.N.as_dp
    try:
        lib, h = raw.lib, raw.h
        assert lib.vk_nested_state(h, *[None] * 6) == -1 and "have no start" in raw.error()
        assert raw.begin(2, 0) == -1 and "have no start" in raw.error()
        assert lib.vk_nested_finish(h, None, None, None, None) == -1 and "nothing was begun" in raw.error()
        assert lib.vk_nested_start(h, None) == -1 and "NULL argument" in raw.error()
        out = raw.x0()
        out[1, 3, 0] = raw.hi[0] + 1.0
        assert lib.vk_nested_start(h, dp(out)) == -1 and "live point 3 of problem 1 is outside the box" in raw.error()
        assert lib.vk_nested_start(h, dp(raw.x0())) == 0, raw.error()
        assert raw.begin(2, 0, give=(False, True)) == -1 and "NULL argument" in raw.error()
        assert raw.begin(0, 0) == -1 and raw.begin(9, 0) == -1 and "1 <= iterations <= 8" in raw.error()
        assert raw.begin(2, 3) == -1 and "first_iter must be 0" in raw.error()
        assert raw.begin(2, 0) == 0, raw.error()
        assert raw.begin(2, 2) == -1 and "has not been finished" in raw.error()
        assert lib.vk_nested_state(h, *[None] * 6) == -1 and "awaiting vk_nested_finish" in raw.error()
        dl, live = np.empty((2, 3, 2)), np.empty((3, 8))
        assert lib.vk_nested_finish(h, dp(dl), None, None, dp(live)) == 0, raw.error()
        assert np.all(np.isfinite(dl)) and np.all(dl[0, :, 0] <= dl[0, :, 1]) and np.all(live.min(axis=1) >= dl[1, :, 0])
        assert raw.begin(1, 0) == -1 and "first_iter must be 2" in raw.error()
        n = np.empty(3, dtype=np.int64)
        assert lib.vk_nested_state(h, None, None, None, None, n.ctypes.data_as(C.POINTER(C.c_int64)), None) == 0 and n.tolist() == [12] * 3
    finally:
        raw.close()
