"""Every shipped kernel instantiation on the GPU, one test id per instance (tests/kernel_matrix.py: RECIPES).

Each recipe's inputs must make the library launch exactly its instance (``Engine.last_instance()``, which the leaves of the
launch switches name), and what that instance computes is held

- against the live oracle on three prior-box points (aperp, apar off 1; beta on a table knot) at the parity bound RTOL;
- against the generic kernel on the whole batch (tests/tolerances, 1024 ulps: another arithmetic);
- for a fused cells / point-major launch, against the same launch with the chi-square in a kernel of its own (64 ulps);
- for the kaiser instances, under ``rsd_model="euclid_special"`` as well.

K1x instances go through ``theory_xi_batch`` against ``oracle.theory_xi``; the realisation kernels through ``realisations()``
against the oracle per realisation.  Oracle results are cached per (inputs, options, point): instances share them.
"""

import faulthandler
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest

from tests import cases
from tests import kernel_matrix as KM
from tests.tolerances import assert_same_chi2, chi2_bound
from victor_amd import _native

pytestmark = pytest.mark.gpu
RTOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ORACLE = 3


@pytest.fixture(scope="module", autouse=True)
def time_limit():
    """The whole file under one time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(1200, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Inputs:
    """Fits, oracle fits and oracle results, built once per Setup / (Setup, options, point)."""

    def __init__(self, tmp):
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import victor_oracle
        self.vo = victor_oracle
        self.tmp = tmp
        self.fits = {}
        self.answers = {}

    def fit(self, st):
        if st not in self.fits:
            import victor_amd
            model, data = KM.options(st, self.tmp)
            self.fits[st] = (victor_amd.CCFFit(model, data), self.vo.OracleFit(model, data), model, data)
        return self.fits[st]

    def oracle(self, st, what, kw, i, fn):
        key = (st, what, tuple(sorted(kw.items())), i)
        if key not in self.answers:
            self.answers[key] = fn()
        return self.answers[key]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(str(tmp_path_factory.mktemp("kernel_matrix")))


@contextmanager
def knobs(**kv):
    for k, v in kv.items():
        _native.set_knob("VICTOR_HIP_" + k, v)
    try:
        yield
    finally:
        for k in kv:
            _native.set_knob("VICTOR_HIP_" + k, None)


def engine(fit, kw):
    return fit._get_engine(fit._engine_key(fit._merged(kw)))


def check_batch(key, rc, inputs, kw):
    st = rc.setup
    fit, ora, _, _ = inputs.fit(st)
    p = KM.points(fit, rc.n)
    theory, like = KM.parse(key)
    with knobs(**rc.knobs):
        lnl, chi2 = fit.log_likelihood_batch(p, **kw)
        assert engine(fit, kw).last_instance() == key, (kw, engine(fit, kw).last_instance())
        again = fit.log_likelihood_batch(p, **kw)                  # (a second call of a shape may replay a captured graph)
        assert engine(fit, kw).last_instance() == key, (kw, engine(fit, kw).last_instance())
        assert np.array_equal(again[1], chi2)
        rows = fit._fit_rows(p, fit._merged(kw))
        th = fit.theory_vector_batch(rows, **kw)
        assert engine(fit, kw).last_instance() == theory + "+none", engine(fit, kw).last_instance()
    for i in range(N_ORACLE):
        q = cases.point(p, i)
        want = inputs.oracle(st, "like", kw, i, lambda: ora.log_likelihood(dict(q), **kw))
        assert abs(chi2[i] / want[1] - 1) < RTOL, (kw, i, chi2[i], want[1])
        assert abs(lnl[i] - want[0]) < RTOL * (abs(want[0]) + want[1]), (kw, i, lnl[i], want[0])
        t = inputs.oracle(st, "theory", kw, i, lambda: ora.theory_multipole_vector(ora.s, dict(q), ora.poles_s, **kw))
        assert np.max(np.abs(th[i] - t)) <= RTOL * np.max(np.abs(t)), (kw, i)
    if not theory.startswith("generic<"):
        with knobs(**dict(rc.knobs, FORCE_GENERIC="1")):
            ref = fit.log_likelihood_batch(p, **kw)
            assert engine(fit, kw).last_instance().startswith("generic<")
        assert_same_chi2(chi2, ref[1], chi2_bound(fit, p, ulps=1024, **kw), what=f"{key} {kw} vs the generic kernel")
    if like == "fused":
        with knobs(**dict(rc.knobs, NO_FUSE="1")):
            sep = fit.log_likelihood_batch(p, **kw)
            assert engine(fit, kw).last_instance() == theory + "+like_wide", engine(fit, kw).last_instance()
        assert_same_chi2(chi2, sep[1], chi2_bound(fit, p, **kw), what=f"{key} {kw} fused vs separate chi-square")


def check_xi(key, rc, inputs):
    st = rc.setup
    fit, ora, _, _ = inputs.fit(st)
    p = KM.points(fit, rc.n)
    mu = np.linspace(0, 1, 17)
    with knobs(**rc.knobs):
        xi = fit.theory_xi_batch(fit.s, mu, p, **rc.kw)
        assert engine(fit, rc.kw).last_instance() == key, engine(fit, rc.kw).last_instance()
    for pt, i, j in ((0, 0, 0), (1, 16, len(fit.s) - 1), (2, 7, 4)):
        want = inputs.oracle(st, ("xi", i, j), rc.kw, pt, lambda: ora.theory_xi(np.array([fit.s[j]]), np.array([mu[i]]),
                                                                               cases.point(p, pt), **rc.kw)[0, 0])
        assert abs(xi[pt, i, j] - want) < RTOL * max(abs(want), 1e-2), (pt, i, j, xi[pt, i, j], want)


def check_real(key, rc, inputs):
    import victor_amd
    st = rc.setup
    fit, ora, model, data = inputs.fit(st)
    p = KM.points(fit, rc.n)
    with knobs(**rc.knobs):
        lnl, chi2 = fit.realisations().log_likelihood(p, **rc.kw)
        assert engine(fit, rc.kw).last_instance() == key, engine(fit, rc.kw).last_instance()
    assert chi2.shape == (rc.n, st.n_real)
    for m in range(st.n_real):
        d = dict(data, redshift_space_ccf=dict(data["redshift_space_ccf"], simulation_number=m))
        ora_m = ora if m == 0 else inputs.vo.OracleFit(model, d)
        for i in range(N_ORACLE):
            want = inputs.oracle(st, ("real", m), rc.kw, i, lambda: ora_m.log_likelihood(cases.point(p, i), **rc.kw))
            assert abs(chi2[i, m] / want[1] - 1) < RTOL, (m, i)
            assert abs(lnl[i, m] - want[0]) < RTOL * (abs(want[0]) + want[1]), (m, i)
        single = victor_amd.CCFFit(model, d)
        got = single.log_likelihood_batch(p, **rc.kw)
        assert_same_chi2(chi2[:, m], got[1], chi2_bound(single, p, **rc.kw), what=f"{key} realisation {m} vs the single path")
        single._engine = None


@pytest.mark.parametrize("key", list(KM.RECIPES))
def test_instance(key, inputs):
    rc = KM.RECIPES[key]
    if rc.api == "xi":
        check_xi(key, rc, inputs)
    elif rc.api == "real":
        check_real(key, rc, inputs)
    else:
        check_batch(key, rc, inputs, rc.kw)
        if ",kaiser," in key:                                      # kModeKaiser serves euclid_special as well
            check_batch(key, rc, inputs, dict(rc.kw, rsd_model="euclid_special"))
