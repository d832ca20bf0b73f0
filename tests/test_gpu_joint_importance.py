"""Importance-sampled posteriors of joint fits reduced on the GPU (``JointRealisations.importance_posterior`` and, for the joint
data vector, ``victor_amd.importance.importance_posterior(joint, ...)``; ``vk_is_create_joint`` / ``vk_is_create_joint_blocks``;
DESIGN.md section 7e) against the NumPy loop that defines them (``device=False``: one ``JointRealisations.log_likelihood`` /
``JointFit.log_likelihood_batch`` call per chunk): maxima, arg max, counts and statuses as bytes, sums at the derived bounds of
tests/test_importance.py; per-block rows bit for bit; against one independent evaluation of the whole sample with a plain
log-sum-exp; the prior; cuts of ``vk_is_run``; the refusals of the C ABI.

The cases are those of tests/test_gpu_joint_sampled.py - three density-split blocks with stacks of 5 under one correlated
covariance (``dsplit_cov``) and block-diagonal (``dsplit_diag``: the cross-mode block sum), the BOSS pair with stacks of 4 under
the covariance gridded on 31 beta slices (``boss_grid``) - and the samples those of tests/test_gpu_importance.py: 23 kept points,
chunks of 7 (cuts inside the sample) and 23, 4 to 6 bins, so that empty cells occur."""

import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests import cases, tolerances
from tests.test_chains import same_bytes
from tests.test_gpu_importance import CENTRE, G23, RANGES, WIDTH, independent, sample_of
from tests.test_gpu_joint_sampled import Case
from tests.test_importance import EXACT, SUMS, Recorder, abs_sums, assert_exact, assert_sums, sum_bound, terms_of

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
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


def sample_named(block, names, seed=5, kept=G23):
    """``sample_of`` for names that may carry a block (``sigma_v@1``): centre, width and box are the plain name's."""
    from victor_amd import GaussianProposal
    base = [n.partition("@")[0] for n in names]
    d = len(names)
    cov = np.diag([WIDTH[b] ** 2 for b in base])
    for j in range(1, d):
        cov[0, j] = cov[j, 0] = 0.4 * WIDTH[base[0]] * WIDTH[base[j]]
    q = GaussianProposal(names, [CENTRE[b] for b in base], cov)
    pts = GaussianProposal.draw(q.mean, q.chol, None, 400, seed)
    lo, hi = (np.array([block[n]["prior"][k] for n in names]) for k in ("min", "max"))
    inside = np.all((pts >= lo) & (pts <= hi), axis=1)
    end = int(np.flatnonzero(np.cumsum(inside) == kept)[0]) + 1
    assert inside[:end].sum() == kept
    pts = pts[:end]
    return dict(sample=pts, ln_proposal=GaussianProposal.ln_density(pts, q.mean, q.chol, None))


def run(obj, params, **kw):
    """The public route of ``obj``: a JointRealisations' method, or for a JointFit (R = 1) the module function."""
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import JointFit
    if isinstance(obj, JointFit):
        return importance_posterior(obj, params, **kw)
    return obj.importance_posterior(params, **kw)


def both_routes(obj, params, what, **kw):
    """The device route and the definition route of one call, compared: exact outputs as bytes, sums at the bound."""
    from victor_amd.joint import JointFit
    one = obj.log_likelihood_batch if isinstance(obj, JointFit) else obj.log_likelihood
    rec = Recorder(lambda batch: one(batch)[0])
    dev = run(obj, params, **kw)
    ref = run(obj, params, device=False, evaluate=rec, **kw)
    assert dev.n_problems == ref.n_problems and dev.chunk == ref.chunk and dev.n_chunks == ref.n_chunks
    assert dev.n_inside == ref.n_inside == G23 and dev.n_drawn == ref.n_drawn >= G23
    assert_exact(dev.raw, ref.raw, what)
    assert same_bytes(dev.status, ref.status), what
    assert_sums(dev.raw, ref.raw, abs_sums(ref, rec.chunks), dev.n_chunks, what, dev._layout, dev._sample.x)
    for name in dev.names:
        assert same_bytes(dev.best[name], ref.best[name])
    # the definition over the object's own evaluation, no evaluate callable: the same bytes as through the recorder
    plain = run(obj, params, device=False, **kw)
    for name in EXACT + SUMS:
        assert same_bytes(getattr(plain.raw, name), getattr(ref.raw, name)), (what, name)
    return dev, ref


def own_blocks(names):
    """PARAMS with a sigma_v per block of a three-block fit."""
    from victor_amd.joint import per_block
    params = per_block(PARAMS, ["sigma_v"], 3)
    assert [n for n in params if n in names] == names
    return params


OWN = ["fsigma8", "sigma_v@0", "sigma_v@1", "sigma_v@2", "epsilon"]


# ------------------------------------------------------------------ device route against the definition route ---------------
@pytest.mark.parametrize("chunk", [7, 23])
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag", "boss_grid"])
def test_every_joint_realisation(case, name, chunk):
    c = case(name)
    pair = (c.names[-1], c.names[0])
    dev, ref = both_routes(c.jr, PARAMS, f"{name} mocks, chunk {chunk}", fixed=c.fixed, bins=5, ranges=RANGES, pairs=[pair], chunk=chunk,
                           min_ess=2.0, **sample_of(PARAMS, c.names))
    R = len(c.jr)
    assert dev.names == c.names and dev.n_problems == R == (4 if name == "boss_grid" else 5) and dev.n_chunks == -(-G23 // chunk)
    assert np.all(dev.n_finite == G23) and len(set(dev.ln_max)) == R and dev.cov.shape == (R, len(c.names), len(c.names))
    counts = terms_of(dev._layout, dev._sample.x)
    assert np.any(counts["h1"] == 0) and np.any(counts["h2"] == 0)
    assert dev.marginal2d(*pair).shape == (R, 5, 5)


@pytest.mark.parametrize("chunk", [7, 23])
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_a_velocity_dispersion_per_block(case, name, chunk):
    """d = 5: fsigma8, a sigma_v per block, epsilon; every block's theory launch reads its own row set."""
    c = case(name)
    params = own_blocks(OWN)
    dev, ref = both_routes(c.jr, params, f"{name} mocks, sigma_v per block, chunk {chunk}", fixed=c.fixed, bins=4, ranges=RANGES,
                           pairs=[("sigma_v@2", "fsigma8")], chunk=chunk, min_ess=2.0, **sample_named(params, OWN))
    assert dev.names == OWN and dev.n_problems == 5 and np.all(dev.n_finite == G23) and len(set(dev.ln_max)) == 5
    # the blocks' own values matter: the same sample with block 2's column read for every block is another posterior
    x = dev._sample.x
    shared = c.jr.log_likelihood(c.points(x[:, [0, 3, 4]], c.names))[0]
    own = c.jr.log_likelihood(dict(c.points(x[:, [0, 4]], ["fsigma8", "epsilon"]), **{OWN[k]: np.ascontiguousarray(x[:, k]) for k in (1, 2, 3)}))[0]
    assert own.shape == shared.shape == (G23, 5) and not np.any(shared == own)


class JointHandle:
    """A raw vk_is handle of a joint call's arguments (victor_amd.importance.create_handle), for what the public route does not
    expose; ``args()``: the arguments of ``vk_is_create_joint`` for the same call, to hand to the library directly."""

    def __init__(self, joint, params, names, realisations=None, fixed=None, bins=4, ranges=None, pairs=None, chunk=7, spoil=None):
        from victor_amd import importance as I
        from victor_amd.fitting import _Sampled
        self.joint, self.realisations = joint, realisations
        q = self.q = _Sampled("importance_posterior", "sampled", params, fixed)
        assert q.names == names
        q.check_columns(joint)
        self.layout = I.resolve_layout("test", q.names, q.lo, q.hi, bins, ranges, pairs)
        s = sample_named(params, names)
        inside = np.all((s["sample"] >= q.lo) & (s["sample"] <= q.hi), axis=1)
        kept = s["sample"][inside]
        self.sample = I.Sample(kept, kept.mean(axis=0), s["ln_proposal"][inside], len(inside), q.lo, q.hi, None)
        self.lists = I.Lists(self.layout, self.sample.x, chunk)
        if spoil is not None:
            spoil(self.lists)
        self.R = 1 if realisations is None else len(realisations)
        self.fixed = {k: float(v) for k, v in q.fixed_all.items()}
        self.engines = joint._sampled_plan("test", {})[0]
        self.lib, self.h, _ = I.create_handle(q, joint, realisations, {}, q.fit_options(joint, {}), self.layout, self.sample, self.lists,
                                              self.fixed)

    def run(self, first, count):
        return self.lib.vk_is_run(self.h, first, count)

    def error(self):
        return (self.lib.vk_is_last_error(self.h) or b"").decode()

    def result(self):
        from victor_amd import importance as I
        return I.read_result(self.lib, self.h, self.layout, self.R, False)

    def rows(self, first, count, sets):
        out = np.empty((sets, count, 12))
        rc = self.lib.vk_is_rows(self.h, first, count, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0, self.error()
        return out

    def batch(self):
        batch = dict(self.fixed)
        batch.update({n: np.ascontiguousarray(self.sample.x[:, j]) for j, n in enumerate(self.layout.names)})
        return batch

    def create(self, ctxs="own", n_ctx=None, opts="own", x="own"):
        """``(handle or None, error text)`` of ``vk_is_create_joint`` called directly with this call's arguments (no ``@`` names),
        some of them replaced."""
        from victor_amd import _native as N
        joint, L, s = self.joint, self.layout, self.sample
        engines, o, kw = joint._sampled_plan("test", {})
        base, cols, param_block, _ = joint._sampled_rows(L.names, {k: np.atleast_1d(v)[:1] for k, v in self.batch().items()}, kw)
        assert param_block is None
        cov = joint._joint_handle(engines[0]) if joint.covariance is not None else None
        own = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
        i32 = C.POINTER(C.c_int32)
        n_bins, pair_bins = np.array(L.n_bins, dtype=np.int32), np.array(L.pair_bins, dtype=np.int32)
        eps_pow = N.f64(N.epsilon_to_ap(N.f64(s.x[:, L.names.index("epsilon")]), 1.0)[1]) if "epsilon" in L.names else None
        err = C.create_string_buffer(512)
        h = self.lib.vk_is_create_joint(own if isinstance(ctxs, str) else ctxs, len(engines) if n_ctx is None else n_ctx, cov,
                                        C.byref(o) if isinstance(opts, str) else opts, L.d, cols.ctypes.data_as(i32), s.G,
                                        N.as_dp(s.x) if isinstance(x, str) else x, N.as_dp(s.y), None if eps_pow is None else N.as_dp(eps_pow),
                                        N.as_dp(s.lno), None, n_bins.ctypes.data_as(i32), len(pair_bins),
                                        pair_bins.ctypes.data_as(i32) if len(pair_bins) else None, self.lists.entries.ctypes.data_as(i32),
                                        self.lists.offsets.ctypes.data_as(i32), N.as_dp(base), 1.0, 0 if self.realisations is None else 1,
                                        self.lists.chunk, err, len(err))
        return h, err.value.decode()

    def close(self):
        self.lib.vk_is_destroy(self.h)


@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_per_block_rows_are_the_hosts_bit_for_bit(case, name):
    """``vk_is_rows`` of a handle with a row per block, [B][count][VK_NPAR], against ``JointFit._block_rows`` with epsilon
    sampled (the host's own pow) and one block's epsilon-independent value fixed per block."""
    c = case(name)
    params = own_blocks(OWN)
    h = JointHandle(c.joint, params, OWN, realisations=c.jr, fixed=dict(c.fixed, **{"bias@1": 1.7}), bins=4, chunk=7)
    try:
        want = c.joint._block_rows(h.batch(), {})
        assert want.shape == (3, G23, 12)
        got = np.concatenate([h.rows(g0, min(7, G23 - g0), 3) for g0 in range(0, G23, 7)], axis=1)
        assert same_bytes(got, want), np.argwhere(got != want)[:4]
        assert len(set(want[0, :, 3])) == G23                                   # (23 epsilons, 23 apar)
        assert not same_bytes(want[0], want[1]) and not same_bytes(want[1], want[2])      # (the blocks' rows differ)
    finally:
        h.close()


# ------------------------------------------------------------------ past one tile of realisations and one wave of problems ---
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_seventy_joint_realisations(case, name):
    """R = 70: problems r and r + 5 are the same joint realisation and agree byte for byte in every raw output."""
    c = case(name)
    jr70 = c.joint.realisations(np.arange(70) % 5)
    ip = jr70.importance_posterior(PARAMS, fixed=c.fixed, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=7,
                                   **sample_of(PARAMS, c.names))
    assert ip.n_problems == 70
    for attr in EXACT + SUMS:
        a = getattr(ip.raw, attr)
        for r in range(70 - 5):
            assert same_bytes(a[r], a[r + 5]), (attr, r)
    assert len(set(ip.ln_max[:5])) == 5 and np.all(ip.n_finite == G23)
    assert same_bytes(ip.ln_evidence[:5], ip.ln_evidence[65:])


# ------------------------------------------------------------------ a Gaussian prior, a per-block name in it -----------------
def test_gaussian_prior_on_a_per_block_parameter(case):
    from victor_amd.priors import GaussianPrior
    c = case("dsplit_cov")
    params = own_blocks(OWN)
    prior = GaussianPrior(["fsigma8", "sigma_v@1"], [0.45, 365.0], cov=[[0.05 ** 2, 0.5 * 0.05 * 30.0], [0.5 * 0.05 * 30.0, 30.0 ** 2]])
    kw = dict(fixed=c.fixed, bins=4, pairs=[("sigma_v@1", "epsilon")], chunk=7, min_ess=2.0, **sample_named(params, OWN))
    dev, ref = both_routes(c.jr, params, "dsplit_cov with a Gaussian prior on (fsigma8, sigma_v@1)", prior=prior, **kw)
    plain = c.jr.importance_posterior(params, **kw)
    assert not np.any(dev.ln_max == plain.ln_max)
    assert same_bytes(dev.prior_ln_max, ref.prior_ln_max)
    assert abs(dev.prior_total - ref.prior_total) <= sum_bound("total", dev.n_chunks, G23) * ref.prior_total
    want = (dev.ln_max + np.log(dev.raw.total)) - (dev.prior_ln_max + np.log(dev.prior_total))      # section 7e, rule 4
    assert same_bytes(dev.ln_evidence, want)
    assert np.all(np.abs(dev.ln_evidence - ref.ln_evidence) <= 4 * sum_bound("total", dev.n_chunks, G23))


# ------------------------------------------------------------------ against an independent evaluation ----------------------
def lnl_bound(c, joint, batch, lnl):
    """``tests.test_gpu_importance.lnl_bound`` for a joint fit: ``joint_bound`` under a covariance, block-diagonal the sum of
    the blocks' ``chi2_bound`` (``Case.bound_of``)."""
    return 0.51 * c.bound_of(joint, batch) + 16 * tolerances.U * (np.abs(lnl) + 1000.0)


@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_mocks_against_one_call_and_logsumexp(case, name):
    """Mocks 0 and 4: the bound needs the realisation's own data vectors, a joint fit each."""
    c = case(name)
    ip = c.jr.importance_posterior(PARAMS, fixed=c.fixed, bins=5, chunk=7, **sample_of(PARAMS, c.names))
    batch = c.points(ip._sample.x, ip.names)
    lnl = c.jr.log_likelihood(batch)[0]
    assert lnl.shape == (G23, 5)
    for m in (0, 4):
        independent(ip, m, lnl[:, m], lnl_bound(c, c.of(m), batch, lnl[:, m]), f"{name} joint realisation {m}")


def test_the_joint_data_vector(case):
    """R = 1 through the module function: the routes agree, and the evidence is that of one log_likelihood_batch call."""
    c = case("dsplit_cov")
    kw = dict(fixed=c.fixed, bins=6, ranges=RANGES, pairs=[("epsilon", "fsigma8")], chunk=7, min_ess=2.0, **sample_of(PARAMS, c.names))
    dev, ref = both_routes(c.joint, PARAMS, "dsplit_cov joint data vector", **kw)
    assert dev.n_problems == 1 and dev.n_finite[0] == G23
    batch = c.points(dev._sample.x, dev.names)
    lnl = c.joint.log_likelihood_batch(batch)[0]
    independent(dev, 0, lnl, lnl_bound(c, c.joint, batch, lnl), "dsplit_cov joint data vector")


# ------------------------------------------------------------------ cuts, and what the C ABI refuses -----------------------
@pytest.mark.parametrize("name", ["dsplit_cov", "dsplit_diag"])
def test_cuts_and_refusals_of_the_c_abi(case, name):
    from victor_amd.utils import InputError
    c = case(name)
    kw = dict(realisations=c.jr, fixed=c.fixed, bins=5, ranges=RANGES, pairs=[("fsigma8", "epsilon")], chunk=7)
    h = JointHandle(c.joint, PARAMS, c.names, **kw)
    engines = h.engines
    try:
        assert h.run(0, G23) == 0, h.error()
        whole = h.result()[0]
        assert h.run(0, 14) == 0, h.error()
        assert h.lib.vk_is_result(h.h, *([None] * 11)) == -1 and "reached 14 of 23" in h.error()
        assert h.run(7, 7) == -1 and "first must be 0" in h.error()
        # another realisation count on one block: refused at run, and at create
        c.joint.fits[1].realisations(np.arange(3))._upload(engines[1])
        assert h.run(14, 9) == -1 and "context 1 holds 3 realisations, context 0 holds 5" in h.error()
        made, text = h.create()
        assert not made and "vk_is_create_joint" in text and "context 1 holds 3 realisations, context 0 holds 5" in text
        # ... on every block, fewer and more: the handle was made for five
        for q, eng in enumerate(engines):
            c.joint.fits[q].realisations(np.arange(3))._upload(eng)
        assert h.run(14, 9) == -1 and "the contexts hold 3 realisations" in h.error()
        for q, eng in enumerate(engines):
            c.joint.fits[q].realisations(np.arange(8) % 5)._upload(eng)
        assert h.run(14, 9) == -1 and "context 0 holds 8 realisations, the sample was made for 5" in h.error()
        out = np.empty((7, 12))
        assert h.lib.vk_is_rows(h.h, 0, 7, out.ctypes.data_as(C.POINTER(C.c_double))) == -1 and "made for 5" in h.error()
        c.jr._upload(engines)
        # model realisations on a block: no cross mode
        sets = own_sets(c.joint.fits[2], 5)
        engines[2].set_model_realisations(*sets)
        try:
            assert h.run(14, 9) == -1 and "model realisations" in h.error()
            made, text = h.create()
            assert not made and "model realisations" in text
        finally:
            engines[2].set_model_realisations(None, None, None)
        # NULL arguments, no contexts, a point that is not finite
        for kwargs, text in ((dict(ctxs=None), "NULL argument"), (dict(opts=None), "NULL argument"), (dict(x=None), "NULL argument"),
                             (dict(n_ctx=0), "need 1 <= contexts <= 32"), (dict(n_ctx=-1), "need 1 <= contexts <= 32"),
                             (dict(ctxs=(C.c_void_p * len(engines))(engines[0]._ctx)), "is NULL")):
            made, said = h.create(**kwargs)
            assert not made and "vk_is_create_joint: " in said and text in said, (kwargs, said)
        assert h.run(14, 9) == 0, h.error()                                     # every refusal left the handle where it stood
        cut = h.result()[0]
        assert h.run(0, 1 << 40) == 0, h.error()
        again = h.result()[0]
        for attr in EXACT + SUMS:
            assert same_bytes(getattr(whole, attr), getattr(cut, attr)), ("14 + 9", attr)
            assert same_bytes(getattr(whole, attr), getattr(again, attr)), ("twice", attr)
        assert np.all(whole.n_finite == G23)
    finally:
        h.close()

    # a spoiled offset list: the check the three creators share serves the joint ones
    def overrun(lists):
        lists.offsets[3, 6] = 3                                   # the last chunk has two points

    def outside(lists):
        lists.entries[0, 8] = 7                                   # chunk 1 holds points 0 .. 6 of its own

    for spoil, text in ((overrun, "end inside the chunk"), (outside, "outside its chunk")):
        with pytest.raises(InputError, match=text):
            JointHandle(c.joint, PARAMS, c.names, spoil=spoil, **kw)
    with pytest.raises(InputError, match="vk_is_create_joint_blocks: .*end inside the chunk"):
        JointHandle(c.joint, own_blocks(OWN), OWN, spoil=overrun, realisations=c.jr, fixed=c.fixed, bins=5, chunk=7)


def own_sets(fit, n):
    """``n`` copies of the fit's own xi^r tables, as ``Engine.set_model_realisations`` takes them."""
    from victor_amd import tables as T
    from victor_amd.engine import build_tables, table_array_lengths
    t, keep = build_tables(fit, None, fit._engine_key(fit.model), T.simpson_even_rule(fit.model["simpson_even"]))
    lengths = table_array_lengths(t)
    out = []
    for name in ("xi.coef", "uni_xi", "uni_xic"):
        obj = t
        for part in name.split("."):
            obj = getattr(obj, part)
        k = lengths[name]
        out.append(np.ascontiguousarray(np.tile(np.ctypeslib.as_array(obj, shape=(k,)).copy(), (n, 1))) if (k and obj) else None)
    del keep
    return out


def test_refusals_before_any_device_call(case):
    from victor_amd.importance import importance_posterior
    from victor_amd.joint import per_block
    from victor_amd.utils import InputError
    c = case("dsplit_cov")
    s = sample_of(PARAMS, c.names)
    with pytest.raises(InputError, match="beta_interpolation 'likelihood'"):
        case("boss_grid").jr.importance_posterior(PARAMS, beta_interpolation="likelihood", **sample_of(PARAMS, case("boss_grid").names))
    own = per_block(PARAMS, ["epsilon"], 3)
    with pytest.raises(InputError, match="epsilon cannot be sampled per block"):
        c.jr.importance_posterior(own, fixed=c.fixed, **s)
    with pytest.raises(InputError, match="names block 3 of 3"):
        c.jr.importance_posterior(PARAMS, fixed=dict(c.fixed, **{"bias@3": 1.5}), **s)
    with pytest.raises(InputError, match="every block shares one beta"):
        importance_posterior(case("boss_grid").joint, PARAMS, fixed={"beta@1": 0.4}, **sample_of(PARAMS, case("boss_grid").names))
    # a fixed epsilon per block is fine
    names = c.without("epsilon")
    ip = c.jr.importance_posterior(PARAMS, fixed=dict(c.fixed, **{"epsilon": 1.0, "epsilon@0": 0.99, "epsilon@2": 1.01}), bins=4,
                                   chunk=23, min_ess=2.0, **sample_of(PARAMS, names))
    assert ip.names == names and np.all(ip.n_finite == G23)
