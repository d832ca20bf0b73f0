"""Per-block parameters of a joint fit on the GPU: ``"name@q"`` in ``JointFit`` / ``JointRealisations`` evaluations, best fits
and chains (the ``_blocks`` entry points of ``include/victor_hip.h``; DESIGN.md sections 7a and 7b).

The fixtures are those of tests/test_gpu_joint_sampled.py: three density-split blocks with stacks of 5 realisations, block-diagonal
and under ``correlated(...)``, and the BOSS pair under its covariance gridded on 31 beta slices.  The per-block parameter is the
velocity dispersion, at values at least 20 % apart (300, 380, 460 km/s), where a block's chi-square moves by factors of 3 to 8
(the oracle's figures: 17.2 / 4.46 / 18.3 for block 0 at fsigma8 0.47, beta 0.4, epsilon 1).
"""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases
from tests.test_chains import same_bytes
from tests.test_gpu_joint_cov import RTOL, oracle_joint
from tests.test_gpu_joint_sampled import BETA, GAUSS, HISTORY, MARGIN, PARAMS, Case, fits_of, oracle, same_walk  # noqa: F401
from tests.tolerances import U, _tau, assert_same_chi2, assert_same_lnl, chi2_bound

pytestmark = pytest.mark.gpu
SIGMA = (300.0, 380.0, 460.0)             # the blocks' own velocity dispersions: at least 20 % apart


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(900, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, tmp_path_factory.mktemp(name))
        return made[name]
    return get


def blocked(n_blocks, names=("sigma_v",)):
    from victor_amd.joint import per_block
    return per_block(PARAMS, list(names), n_blocks)


def own_sigma(pts, n_blocks, values=SIGMA):
    """``pts`` with a velocity dispersion of each block's own in place of the shared one."""
    out = {k: v for k, v in pts.items() if k != "sigma_v"}
    n = max([len(v) for v in pts.values() if np.ndim(v)] or [1])
    out.update({f"sigma_v@{q}": np.full(n, float(values[q])) for q in range(n_blocks)})
    return out


def blocks_bound(joint, params, ulps=64):
    """The rounding bound of chi2 at points with ``@`` names: tests/test_gpu_joint_cov.joint_bound with each block's theory
    vector at its own rows (beta: block 0's, as the joint chi-square reads it); block-diagonal the sum of the blocks' own
    ``chi2_bound`` at the values resolved for them."""
    from victor_amd import _native as N
    from victor_amd.joint import block_params
    if joint.covariance is None:
        return sum(chi2_bound(f, block_params(params, q)) for q, f in enumerate(joint.fits))
    rows = joint._block_rows(params, {})
    t = np.concatenate([f.theory_vector_batch(rows[q]) for q, f in enumerate(joint.fits)], axis=1)
    beta = rows[0][:, N.P_BETA]
    d = np.array([joint.multipole_datavector(b if not joint.fixed_data else None) for b in beta])
    absr = np.abs(t - d)
    v = absr + 2.0 * np.concatenate([_tau(f) for f in joint.fits])[None, :]
    absP = np.abs(joint.icov)
    if joint.fixed_covmat:
        amp = np.einsum("ij,jk,ik->i", absr, absP, v)
    else:
        amp = np.empty(len(beta))
        for i in range(len(beta)):
            lo, w = joint._bracket(beta[i])
            P = absP[lo] if w == 0.0 else (1 - w) * absP[lo] + w * absP[-1]
            amp[i] = absr[i] @ P @ v[i]
    return ulps * U * amp


def bound_of_mock(c, m, pts):
    return blocks_bound(c.of(m), pts)


def history_bounds(c, ch, data=False, **fixed):
    n, R, W, d = ch.chain.shape
    out = np.empty((n, R, W))
    for m in range(R):
        pts = c.points(ch.chain[:, m].reshape(n * W, d), ch.names, **fixed)
        out[:, m] = blocks_bound(c.joint if data else c.of(m), pts).reshape(n, W)
    return out


def oracle_blocks(oracle, c, m, point, shared_sigma=False):
    """(lnL, chi2) of realisation m (None: the fits' own data vectors) at ``point`` (name -> float, ``@`` names included) from
    the oracle: each block's theory vector at that block's own point.  ``shared_sigma``: every block at block 0's sigma_v."""
    from tests.test_joint_realisations import with_number
    from victor_amd.joint import block_params
    ofits = [oracle.OracleFit(*o) for o in (c.opts if m is None else with_number(c.opts, m))]
    own = [block_params(point, q) for q in range(len(ofits))]
    if shared_sigma:
        own = [dict(p, sigma_v=own[0]["sigma_v"]) for p in own]
    if c.covariance is None:
        each = [of.log_likelihood(dict(p)) for of, p in zip(ofits, own)]
        return sum(e[0] for e in each), sum(e[1] for e in each)
    theory = [[of.theory_multipole_vector(of.s, dict(p), of.poles_s)] for of, p in zip(ofits, own)]
    ol, oc = oracle_joint(ofits, theory, [own[0]], c.cov_array, c.beta_grid, c.likelihood or GAUSS)
    return ol[0], oc[0]


# ------------------------------------------------------------------ 4. the same value in every block: the shared call's bytes
@pytest.mark.parametrize("name", ["dsplit_diag", "dsplit_cov", "boss_grid"])
def test_the_same_value_in_every_block_returns_the_shared_bytes(case, name):
    c = case(name)
    B, R = len(c.fits), len(c.jr)
    hp = cases.halton_params(23, with_beta=True)                  # 23 points: a partial wave
    same = {k: v for k, v in hp.items() if k != "sigma_v"}
    same.update({f"sigma_v@{q}": hp["sigma_v"] for q in range(B)})
    which = (np.arange(23) * 3) % R
    for what, call in (("data vectors", c.joint.log_likelihood_batch), ("pairs", lambda p: c.jr.log_likelihood_pairs(p, which)),
                       ("every realisation", c.jr.log_likelihood)):
        want, got = call(hp), call(same)
        for a, b in zip(got, want):
            assert same_bytes(a, b), (name, what)
        assert np.all(np.isfinite(want[1])), (name, what)
    one = cases.point(hp, 5)
    blk = {k: v for k, v in one.items() if k != "sigma_v"}
    blk.update({f"sigma_v@{q}": one["sigma_v"] for q in range(B)})
    assert c.joint.log_likelihood(blk) == c.joint.log_likelihood(one)
    got, want = c.jr.log_likelihood(blk), c.jr.log_likelihood(one)
    assert got[0].shape == (R,) and same_bytes(got[0], want[0]) and same_bytes(got[1], want[1])


# ------------------------------------------------------------------ 5. block-diagonal: the blocks' own results, summed in block order
def test_block_diagonal_is_separable_bit_for_bit(case):
    """DESIGN.md section 7b's rule for vk_joint_sum_kernel: 0 + a_0 + a_1 + a_2 in IEEE doubles, a_q the same per-block launch
    (``JointFit([fits[q]])``); a block that fails fails the point."""
    from victor_amd.joint import JointFit, block_params
    c = case("dsplit_diag")
    hp = cases.halton_params(23, with_beta=True)
    pts = own_sigma(hp, 3)
    pts["sigma_v@1"][3] = np.nan                                  # block 1 fails point 3
    pts["epsilon@2"] = np.full(23, 1.02)
    del pts["aperp"], pts["apar"]
    pts["epsilon"] = np.full(23, 0.99)
    lnl, chi2 = c.joint.log_likelihood_batch(pts)
    sl, sc = np.zeros(23), np.zeros(23)
    for q, f in enumerate(c.fits):
        a, b = JointFit([f]).log_likelihood_batch(block_params(pts, q))
        sl, sc = sl + a, sc + b
    bad = ~np.isfinite(sl)
    sl[bad], sc[bad] = -np.inf, np.inf
    assert list(np.flatnonzero(bad)) == [3] and lnl[3] == -np.inf and chi2[3] == np.inf
    assert same_bytes(lnl, sl) and same_bytes(chi2, sc)
    shared = c.joint.log_likelihood_batch(dict(pts, **{f"sigma_v@{q}": pts["sigma_v@0"] for q in range(3)}))[1]
    assert np.all(shared[~bad] != chi2[~bad])                                 # (the blocks read their own values)
    # against the realisations: each block's own Realisations, summed on the host
    R = len(c.jr)
    which = (np.arange(23) * 2) % R
    for got, each in ((c.jr.log_likelihood_pairs(pts, which), lambda r, p: r.log_likelihood_pairs(p, which)),
                      (c.jr.log_likelihood(pts), lambda r, p: r.log_likelihood(p))):
        sl = sc = 0.0
        for q, r in enumerate(c.jr.blocks):
            a, b = each(r, block_params(pts, q))
            sl, sc = sl + a, sc + b
        bad = ~np.isfinite(sl)
        sl[bad], sc[bad] = -np.inf, np.inf
        assert same_bytes(got[0], sl) and same_bytes(got[1], sc)
        assert np.all(np.isneginf(got[0][3])) and np.all(np.isposinf(got[1][3]))


# ------------------------------------------------------------------ 6. under a covariance, against the oracle
@pytest.mark.parametrize("name", ["dsplit_cov", "boss_grid"])
def test_under_a_covariance_against_the_oracle(case, oracle, name):
    c = case(name)
    B = len(c.fits)
    points = [{"fsigma8": 0.47, "beta": 0.4, "epsilon": 1.0}, {"fsigma8": 0.52, "beta": 0.437, "epsilon": 0.98}]
    for i, p in enumerate(points):
        p.update({f"sigma_v@{q}": SIGMA[(q + i) % 3] for q in range(B)})
        ol, oc = oracle_blocks(oracle, c, None, p)
        _, shared = oracle_blocks(oracle, c, None, p, shared_sigma=True)
        print(name, "point", i, "oracle chi2", oc, "with sigma_v@0 in every block", shared)
        assert abs(shared - oc) > 1e-3 * abs(oc), (name, i, oc, shared)       # a condition on the inputs: the parameter matters
        lnl, chi2 = c.joint.log_likelihood(p)
        assert abs(chi2 - oc) <= RTOL * abs(oc) and abs(lnl - ol) <= RTOL * abs(ol), (name, i, chi2, oc, lnl, ol)
        m = len(c.jr) - 1
        ol, oc = oracle_blocks(oracle, c, m, p)
        lnl, chi2 = c.jr.log_likelihood(p)
        assert abs(chi2[m] - oc) <= RTOL * abs(oc) and abs(lnl[m] - ol) <= RTOL * abs(ol), (name, i, m, chi2[m], oc, lnl[m], ol)
        pl, pc = c.jr.log_likelihood_pairs(p, [m])
        assert same_bytes(pl, lnl[m:m + 1]) and same_bytes(pc, chi2[m:m + 1])


# ------------------------------------------------------------------ 7. the chunk border of the host entry point
def test_chunk_border_of_the_realisations_entry_point(case):
    """Pairs mode cuts chunks of 65536 points: n = 65536 + 37 is the smallest batch with a second chunk, whose rows are each
    block's own slice of the upload."""
    c = case("dsplit_cov")
    n = 65536 + 37
    hp = cases.halton_params(n, with_beta=True)
    pts = {k: v for k, v in hp.items() if k != "sigma_v"}
    for q in range(3):
        pts[f"sigma_v@{q}"] = 0.8 * SIGMA[q] + 0.25 * hp["sigma_v"]           # distinct in every block at every point
    which = (np.arange(n) * 3 % len(c.jr)).astype(np.int32)
    lnl, chi2 = c.jr.log_likelihood_pairs(pts, which)
    sl = slice(65530, 65573)
    few = {k: v[sl] for k, v in pts.items()}
    wl, wc = c.jr.log_likelihood_pairs(few, which[sl])
    bound = np.empty(sl.stop - sl.start)
    for m in range(len(c.jr)):
        pick = which[sl] == m
        bound[pick] = bound_of_mock(c, m, {k: v[pick] for k, v in few.items()})
    assert np.all(np.isfinite(wc)) and len(np.unique(wc)) == len(wc)
    assert_same_chi2(chi2[sl], wc, bound, what="chunk border: entries 65530 .. 65572 vs the same rows on their own")
    assert_same_lnl(lnl[sl], wl, bound, what="chunk border: entries 65530 .. 65572 vs the same rows on their own")


# ------------------------------------------------------------------ 8. chains, epsilon fixed: the definition route's bytes
# Seeds: picked with the definition route alone, for an acceptance inside (0.02, 0.98).
@pytest.mark.parametrize("name,data,move", [("dsplit_cov", False, "metropolis"), ("dsplit_diag", False, "metropolis"),
                                            ("dsplit_cov", True, "metropolis"), ("dsplit_diag", True, "metropolis"),
                                            ("dsplit_cov", False, "stretch")])
def test_device_route_is_the_definition_route_bit_for_bit_with_epsilon_fixed(case, name, data, move):
    c = case(name)
    target = c.joint if data else c.jr
    W = 10 if move == "stretch" else 8 if data else 2            # stretch: W >= 2 (d + 1), d = 4
    kw = dict(walkers=W, seed=2, fixed={"beta": BETA, "epsilon": 1.0}, move=move)
    ref = target.sample_chains(blocked(3), 70, device=False, **kw)
    dev = target.sample_chains(blocked(3), 70, **kw)
    R = 1 if data else len(c.jr)
    assert dev.names == ["fsigma8", "sigma_v@0", "sigma_v@1", "sigma_v@2"] and dev.chain.shape == (70, R, W, 4)
    print(name, "data" if data else "mocks", move, "acceptance of the definition route:", ref.acceptance)
    assert 0.02 < ref.acceptance.mean() < 0.98                   # a condition on the inputs
    for a in HISTORY:
        assert same_bytes(getattr(dev, a), getattr(ref, a)), (name, a)
    assert same_bytes(dev.lnl, ref.lnl) and same_bytes(dev.chi2, ref.chi2)
    assert not same_bytes(dev.chain[..., 1], dev.chain[..., 2])  # (the blocks' dispersions walk on their own)


def test_a_fixed_entry_of_one_block_beside_sampled_entries_of_the_others(case):
    """``sigma_v@0`` fixed, ``sigma_v@1`` and ``sigma_v@2`` sampled: block 0's rows keep the fixed value on both routes (the
    same bytes), the reported best fit is the likelihood at the reported point, and the fixed value is read (another one gives
    another chain)."""
    c = case("dsplit_cov")
    blk = {k: v for k, v in blocked(3).items() if k != "sigma_v@0"}
    fixed = {"beta": BETA, "epsilon": 1.0, "sigma_v@0": 300.0}
    kw = dict(walkers=2, seed=2)
    ref = c.jr.sample_chains(blk, 70, device=False, fixed=fixed, **kw)
    dev = c.jr.sample_chains(blk, 70, fixed=fixed, **kw)
    assert dev.names == ["fsigma8", "sigma_v@1", "sigma_v@2"] and dev.fixed["sigma_v@0"] == 300.0
    assert 0.02 < ref.acceptance.mean() < 0.98
    for a in HISTORY + ("lnl", "chi2"):
        assert same_bytes(getattr(dev, a), getattr(ref, a)), a
    other = c.jr.sample_chains(blk, 70, fixed=dict(fixed, **{"sigma_v@0": 380.0}), **kw)
    assert not same_bytes(other.lnl_chain, dev.lnl_chain)
    bf = c.jr.best_fit(blk, fixed=fixed)
    assert np.all(bf.params["sigma_v@0"] == 300.0) and "sigma_v" not in bf.params
    pts = c.points(bf.x, bf.names, **{k: v for k, v in fixed.items() if k != "beta"})
    lnl, chi2 = c.jr.log_likelihood_pairs(pts, np.arange(len(c.jr)))
    bound = np.array([bound_of_mock(c, m, {key: v[m:m + 1] for key, v in pts.items()})[0] for m in range(len(c.jr))])
    assert_same_chi2(bf.chi2, chi2, bound, what="fixed sigma_v@0: best fit vs log_likelihood_pairs")
    assert_same_lnl(bf.lnl, lnl, bound, what="fixed sigma_v@0: best fit vs log_likelihood_pairs")


# ------------------------------------------------------------------ 9. chains, epsilon sampled
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag", "boss_grid"])
def test_device_route_with_epsilon_sampled(case, name):
    """The seed is the first of 0, 1, 2, ... whose smallest decision margin on the definition route exceeds MARGIN: chosen
    here, with the definition route alone, before the device route runs."""
    c = case(name)
    B = len(c.fits)
    ref = None
    for seed in range(8):
        kw = dict(walkers=2, seed=seed, fixed=c.fixed)
        ref = c.jr.sample_chains(blocked(B), 70, device=False, **kw)
        print(name, "seed", seed, "smallest decision margin (definition route):", ref.decision_margin)
        if ref.decision_margin > MARGIN:
            break
    assert ref.decision_margin > MARGIN, ref.decision_margin     # a condition on the inputs, not on the code under test
    dev = c.jr.sample_chains(blocked(B), 70, **kw)
    assert dev.names == [n for n in blocked(B) if n.partition("@")[0] in c.names] and len(dev.names) == len(c.names) - 1 + B
    same_walk(dev, ref, name)
    bound = history_bounds(c, ref)
    assert_same_chi2(dev.chi2_chain, ref.chi2_chain, bound, what=f"{name} chains: device vs definition route")
    assert_same_lnl(dev.lnl_chain, ref.lnl_chain, bound, what=f"{name} chains: device vs definition route")


# ------------------------------------------------------------------ 10. best fits
def tight(names, c):
    width = {n: PARAMS[n.partition("@")[0]]["prior"]["max"] - PARAMS[n.partition("@")[0]]["prior"]["min"] for n in names}
    return dict(xtol={n: 1e-7 * w for n, w in width.items()}, ftol=1e-10, max_iter=5000, restarts=2)


@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag", "boss_grid"])
def test_best_fits_of_every_mock(case, oracle, name):
    c = case(name)
    B, R = len(c.fits), len(c.jr)
    blk = blocked(B)
    names = [n for n in blk if n.partition("@")[0] in c.names]
    bf = c.jr.best_fit(blk, fixed=c.fixed, **tight(names, c))
    again = c.jr.best_fit(blk, fixed=c.fixed, **tight(names, c))
    assert bf.names == names and bf.x.shape == (R, len(names)), bf.names
    print(name, "status", bf.status, "iterations", bf.n_iter, "sigma_v per block", [bf.params[f"sigma_v@{q}"] for q in range(B)])
    for a in ("x", "lnl", "chi2", "status", "n_iter", "n_evals"):
        assert getattr(bf, a).tobytes() == getattr(again, a).tobytes(), a
    assert set(bf.params) == set(names) | set(c.fixed) and "sigma_v" not in bf.params
    pts = c.points(bf.x, names)
    lnl, chi2 = c.jr.log_likelihood_pairs(pts, np.arange(R))
    bound = np.array([bound_of_mock(c, m, {key: v[m:m + 1] for key, v in pts.items()})[0] for m in range(R)])
    assert_same_chi2(bf.chi2, chi2, bound, what=f"{name}: best fit vs log_likelihood_pairs")
    assert_same_lnl(bf.lnl, lnl, bound, what=f"{name}: best fit vs log_likelihood_pairs")
    point = bf.point(1)
    assert set(point) == set(bf.params) and all(isinstance(v, float) for v in point.values())
    ol, oc = oracle_blocks(oracle, c, 1, point)
    assert abs(ol - bf.lnl[1]) <= 1e-9 * abs(ol) and abs(oc - bf.chi2[1]) <= 1e-9 * abs(oc), (name, ol, bf.lnl[1], oc, bf.chi2[1])
    # the workflow of the README: the best fits start a stretch ensemble of every mock
    d = len(names)
    ch = c.jr.sample_chains(blk, 3, walkers=2 * (d + 1), start=bf, move="stretch", fixed=c.fixed)
    assert ch.names == names and ch.chain.shape == (3, R, 2 * (d + 1), d) and np.all(np.isfinite(ch.lnl))
    ch.extend(2)
    assert ch.n_steps == 5


# ------------------------------------------------------------------ 11. noise-free recovery, a truth per block
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_noise_free_stacks_recover_a_dispersion_per_block(case, tmp_path, name):
    """Stacks made of the blocks' theory vectors at sigma_v@q = 300, 380, 460: the per-block fit recovers them (chi2 <= 1e-6),
    the shared-sigma_v fit of the same stacks cannot (chi2 > 1e-3: the oracle's figures put it at order 1 or more)."""
    from victor_amd.joint import JointFit, block_params
    c = case(name)
    rng = np.random.default_rng(5)
    free = ["fsigma8", "epsilon"]
    lo = np.array([PARAMS[n]["prior"]["min"] for n in free], dtype=float)
    hi = np.array([PARAMS[n]["prior"]["max"] for n in free], dtype=float)
    truth = lo + (hi - lo) * (0.3 + 0.4 * rng.random((5, 2)))
    pts = own_sigma({"fsigma8": truth[:, 0], "epsilon": truth[:, 1], "beta": np.full(5, BETA)}, 3)
    opts = []
    for q, ((model, data), fit) in enumerate(zip(c.opts, c.fits)):
        t = fit.theory_vector_batch(block_params(pts, q))
        data = cases.clone(data)
        ccf = data["redshift_space_ccf"]
        stack = dict(np.load(ccf["data_file"], allow_pickle=True).item())
        n_s = len(fit.s)
        for j, key in enumerate(ccf["ccf_keys"][1:]):
            stack[key] = t[:, j * n_s:(j + 1) * n_s].reshape(np.shape(stack[key]))
        ccf["data_file"] = str(tmp_path / f"noise_free_q{q}.npy")
        np.save(ccf["data_file"], stack, allow_pickle=True)
        opts.append((model, data))
    jr = JointFit(fits_of(opts), covariance=c.covariance).realisations()
    at_truth = jr.log_likelihood_pairs(pts, np.arange(5))[0]
    blk = blocked(3)
    names = ["fsigma8", "sigma_v@0", "sigma_v@1", "sigma_v@2", "epsilon"]
    bf = jr.best_fit(blk, fixed=c.fixed, **tight(names, c))
    got = np.array([bf.params[f"sigma_v@{q}"] for q in range(3)]).T
    print(name, "per block: chi2", bf.chi2, "status", bf.status, "sigma_v", got)
    assert bf.names == names and np.all(bf.status == bf.CONVERGED), bf.status
    assert np.all(bf.chi2 <= 1e-6), bf.chi2
    assert np.all(bf.lnl >= at_truth - 1e-6), (bf.lnl, at_truth)
    shared = jr.best_fit(PARAMS, fixed=c.fixed, **tight(c.names, c))
    print(name, "one sigma_v for all blocks: chi2", shared.chi2, "sigma_v", shared.params["sigma_v"])
    assert np.all(shared.chi2 > 1e-3), shared.chi2


# ------------------------------------------------------------------ 12. the C ABI's refusals
def test_c_abi_guards_of_the_create_calls(case):
    """Each refusal returns NULL with its text; a valid call on the same contexts then succeeds."""
    from victor_amd import _native as N
    i32 = C.POINTER(C.c_int32)
    for name in ("dsplit_cov", "boss_grid"):
        c = case(name)
        engines, opts = c.joint._plan_cov({})
        lead = engines[0]
        lib, h, B = lead._lib, c.joint._joint_handle(lead), len(engines)
        c.jr._upload(engines)
        ctxs = (C.c_void_p * B)(*[e._ctx for e in engines])
        R = 2
        rows = N.f64(c.joint._block_rows({"fsigma8": np.array([0.47, 0.5]), "sigma_v": 380.0, "beta": BETA, "epsilon": 1.0,
                                          "sigma_v@1": 300.0}, {}))
        which = np.array([0, 1], dtype=np.int32)

        def create(entry, cols, blocks, hh=h):
            cols, blocks = np.array(cols, dtype=np.int32), np.array(blocks, dtype=np.int32)
            lo, hi = N.f64(np.zeros(len(cols))), N.f64(np.full(len(cols), 1000.0))
            err = C.create_string_buffer(512)
            out = getattr(lib, entry)(ctxs, B, hh, C.byref(opts), R, len(cols), cols.ctypes.data_as(i32), blocks.ctypes.data_as(i32),
                                      N.as_dp(lo), N.as_dp(hi), N.as_dp(rows), 1.0, which.ctypes.data_as(i32), err, len(err))
            return out, err.value.decode()

        F, S, BETA_COL, EPS = N.P_FSIGMA8, N.P_SIGMAV, N.P_BETA, N.VK_WALK_EPSILON
        for entry, destroy in (("vk_fit_create_joint_blocks", lib.vk_fit_destroy), ("vk_chain_create_joint_blocks", lib.vk_chain_destroy)):
            for hh in (h, None):
                out, text = create(entry, [F, S], [-1, B], hh)
                assert not out and f"param_block {B} of parameter 1 is outside -1..{B - 1}" in text, text
                out, text = create(entry, [F, S], [-2, 0], hh)
                assert not out and "param_block -2 of parameter 0" in text, text
                out, text = create(entry, [F, S, S], [-1, 1, 1], hh)
                assert not out and "(column, block) pair a second time" in text, text
                out, text = create(entry, [EPS, EPS], [0, 0], hh)
                assert not out and "(column, block) pair a second time" in text, text
                out, text = create(entry, [F, F], [-1, -1], hh)
                assert not out and "(column, block) pair a second time" in text, text
                out, text = create(entry, [S, F, S], [-1, -1, 1], hh)
                assert not out and "for all blocks or per block, not both" in text, text
                out, text = create(entry, [EPS, EPS], [1, -1], hh)
                assert not out and "for all blocks or per block, not both" in text, text
            out, text = create(entry, [F, BETA_COL], [-1, 1])
            if name == "boss_grid":
                assert not out and "beta cannot be sampled per block under a covariance gridded in beta" in text, text
            else:
                assert out, text                                  # a fixed covariance brackets nothing: allowed
                destroy(out)
            out, text = create(entry, [F, BETA_COL], [-1, 1], None)       # block-diagonal: every block reads its own beta
            assert out, text
            destroy(out)
            err = C.create_string_buffer(64)
            assert not getattr(lib, entry)(ctxs, B, h, C.byref(opts), R, 1, np.array([F], dtype=np.int32).ctypes.data_as(i32), None,
                                           None, None, N.as_dp(rows), 1.0, None, err, len(err)) and b"NULL argument" in err.value
            out, text = create(entry, [F, S, S, EPS, EPS], [-1, 0, 1, 0, 1])
            assert out, text
            destroy(out)
