"""Likelihood-level beta interpolation in the device loops (``beta_interpolation='likelihood'`` on a beta-dependent data vector;
``VK_OPT_BETA_BLEND``, ``victor_amd/csrc/vk_kernel_blend.h``) without a GPU: the refusals that remain - each
before the library is entered -, how the mode reaches the create calls, and the ABI surface.  The kernels and every loop run in
tests/test_gpu_beta_blend.py.
"""

import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cases
from tests.test_realisations import stack_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vk_blend_split", "vk_blend_merge")
LIKE = dict(beta_interpolation="likelihood")
AT = {"fsigma8": 0.47, "beta": 0.4, "sigma_v": 380.0, "epsilon": 1.0}


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the refusal")


@pytest.fixture
def no_library(monkeypatch):
    import victor_amd
    monkeypatch.setattr(victor_amd.CCFFit, "_get_engine", lambda self, *a, **k: _NoLibrary())


def like_fit(options):
    """The fit of ``options`` with ``beta_interpolation: likelihood`` in its data block, as a YAML configures it."""
    import victor_amd
    model, data = options
    fit = victor_amd.CCFFit(model, dict(data, beta_interpolation="likelihood"))
    assert fit.fit_options["beta_interpolation"] == "likelihood" and not fit.fixed_data
    return fit


def proposal(params):
    import victor_amd
    names = [n for n, v in params.items() if isinstance(v, dict) and "prior" in v]
    return victor_amd.GaussianProposal(names, [AT[n] for n in names], np.diag([1e-4] * len(names)))


def test_what_needs_a_theory_vector_is_refused_before_the_library(no_library):
    """``predictive`` on chains (both routes) and on importance samples, ``fisher`` and its ``keep_vectors``: a blended point has
    two theory vectors.  Each message names the mode and the reason."""
    import victor_amd
    from victor_amd import InputError
    params = cases.cobaya_info()["params"]
    fit = like_fit(cases.boss_options("config"))
    rs = like_fit(stack_options()).realisations()
    two = "beta_interpolation 'likelihood'.*two theory vectors"
    for target in (fit, rs):
        for route in (dict(), dict(device=False)):
            with pytest.raises(InputError, match=two):
                target.sample_chains(params, 10, predictive=True, **route)
        with pytest.raises(InputError, match=two):
            target.fisher(params, AT)
        with pytest.raises(InputError, match=two):
            target.fisher(params, AT, keep_vectors=True)
        with pytest.raises(InputError, match=two):
            target.importance_posterior(params, proposal(params), n=8, predictive=True)
    # the option set on a fit after its construction (`fit.fit_options`, public in the reference) is the same request
    late = victor_amd.CCFFit(*cases.boss_options("config"))
    late.fit_options["beta_interpolation"] = "likelihood"
    with pytest.raises(InputError, match=two):
        late.fisher(params, AT)


def test_joint_fits_are_refused_before_the_library(no_library):
    import victor_amd
    from victor_amd import InputError
    from victor_amd.joint import JointFit
    params = cases.cobaya_info()["params"]
    own = "beta_interpolation 'likelihood'.*joint fits.*design of its own"
    for joint, kw in ((JointFit([like_fit(cases.boss_options("config")) for _ in range(2)]), {}),
                      (JointFit([victor_amd.CCFFit(*cases.boss_options("config")) for _ in range(2)]), LIKE)):
        with pytest.raises(InputError, match=own):
            joint.best_fit(params, **kw)
        with pytest.raises(InputError, match=own):
            joint.sample_chains(params, 10, **kw)
        with pytest.raises(InputError, match=own):
            joint.nested_sampling(params, **kw)
        with pytest.raises(InputError, match=own):
            joint.laplace(params, AT, **kw)


def test_the_broker_does_not_serve_the_mode(no_library):
    """The broker serves the fit's single-point plan; in this mode there is none (two rows per point), found without an engine."""
    import inspect
    import victor_amd
    from victor_amd import broker
    model, data = cases.boss_options("config")
    fit = victor_amd.CCFFit(model, dict(data, beta_interpolation="likelihood"))
    assert fit.fit_options["beta_interpolation"] == "likelihood" and fit._single_point_plan() is None
    src = inspect.getsource(broker)
    assert re.search(r"if plan is None:\s+raise InputError\(\"beta_interpolation 'likelihood' evaluates two rows per point: not served "
                     r"by the broker\"\)", src)


def test_the_loops_of_a_fit_in_the_mode_go_on_to_the_device(no_library):
    """What the parent refused (``_Sampled.fit_options``) now reaches the engine: every loop of a single fit whose data block says
    ``beta_interpolation: likelihood``, and of its realisations; giving the option once more per call changes nothing."""
    params = cases.cobaya_info()["params"]
    fit = like_fit(cases.boss_options("config"))
    rs = like_fit(stack_options()).realisations()
    reached = "the library was reached"
    for target in (fit, rs):
        for kw in ({}, LIKE):
            with pytest.raises(AssertionError, match=reached):
                target.best_fit(params, **kw)
            with pytest.raises(AssertionError, match=reached):
                target.sample_chains(params, 10, **kw)
        with pytest.raises(AssertionError, match=reached):
            target.best_fit(params, covariance=True)
        with pytest.raises(AssertionError, match=reached):
            target.laplace(params, AT)
        with pytest.raises(AssertionError, match=reached):
            target.nested_sampling(params)
        with pytest.raises(AssertionError, match=reached):
            target.grid_posterior(params, bins=2)
        with pytest.raises(AssertionError, match=reached):
            target.importance_posterior(params, proposal(params), n=8)


def test_a_per_call_override_into_the_mode_stays_refused(no_library):
    """On a fit configured with ``datavector`` the loops refuse ``beta_interpolation='likelihood'`` given per call, as they always
    did - now pointing at the fit's own option; the override the other way, out of the mode, is an ordinary call."""
    import victor_amd
    from victor_amd import InputError
    params = cases.cobaya_info()["params"]
    fit = victor_amd.CCFFit(*cases.boss_options("config"))
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    on_the_fit = "beta_interpolation 'likelihood'.*per-call option.*set it on the fit"
    for target in (fit, rs):
        for call in (lambda: target.best_fit(params, **LIKE), lambda: target.laplace(params, AT, **LIKE),
                     lambda: target.sample_chains(params, 10, **LIKE), lambda: target.sample_chains(params, 10, device=False, **LIKE),
                     lambda: target.nested_sampling(params, **LIKE), lambda: target.grid_posterior(params, bins=2, **LIKE),
                     lambda: target.importance_posterior(params, proposal(params), n=8, **LIKE)):
            with pytest.raises(InputError, match=on_the_fit):
                call()
    with pytest.raises(AssertionError, match="the library was reached"):
        like_fit(cases.boss_options("config")).best_fit(params, beta_interpolation="datavector")


def test_the_flag_is_set_for_the_create_call_alone():
    """``blend_opts``: a copy with the bit for a beta-dependent data vector in likelihood mode, the same object otherwise; the
    options ``Engine.make_opts`` builds for the evaluation entry points keep the word 0."""
    import inspect
    import victor_amd
    from victor_amd import _native as N
    from victor_amd import engine, fitting, grid, importance
    fit = victor_amd.CCFFit(*cases.boss_options("config"))          # (blend_opts reads the merged options it is handed)
    opts = N.vk_eval_opts()
    opts.niter = 5
    assert fitting.blend_opts(fit, fit._merged_fit({}), opts) is opts
    out = fitting.blend_opts(fit, fit._merged_fit(LIKE), opts)
    assert out is not opts and out.reserved == N.VK_OPT_BETA_BLEND == 1 and opts.reserved == 0 and out.niter == 5

    class Fixed:
        fixed_data = True
    assert fitting.blend_opts(Fixed(), fit._merged_fit(LIKE), opts) is opts
    assert "reserved" not in inspect.getsource(engine.Engine.make_opts)
    for where in (fitting._Sampled.create, grid.create_handle, importance.create_handle, importance.create_own_handle):
        assert "blend_opts(fit, " in inspect.getsource(where), where


def test_abi_surface():
    from victor_amd import _native as N
    header = open(os.path.join(ROOT, "include", "victor_hip.h")).read()
    assert re.search(r"#define VK_ABI_VERSION 22\b", header) and N.VK_ABI_VERSION == 22
    assert re.search(r"#define VK_OPT_BETA_BLEND 1\b", header) and N.VK_OPT_BETA_BLEND == 1
    assert "ccf_fit.py:383-440" in header and "ccf_fit.py:402-410" in header
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), f"include/victor_hip.h does not declare {name}"
        assert name in N.SYMBOLS, name
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert N.SYMBOLS["vk_blend_split"] == (C.c_int, [C.c_int, dp, C.c_int32, dp, ip, C.c_int64, dp, ip, dp, ip])
    assert N.SYMBOLS["vk_blend_merge"] == (C.c_int, [C.c_int, dp, ip, C.c_int64, C.c_int64, dp, dp, dp, dp])
    # the flag word is the struct's last field, where it always was: no layout change
    assert [f[0] for f in N.vk_eval_opts._fields_][-1] == "reserved" and C.sizeof(N.vk_eval_opts) == 56
    csrc = os.path.join(ROOT, "victor_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "vk_kernel_blend.h")).read())
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code
    assert "#pragma clang fp contract(off)" in code and "fma" not in code                # separate roundings, as NumPy's
    unit = open(os.path.join(csrc, "vk_sampled.hip")).read()
    assert '#include "vk_kernel_blend.h"' in unit and "sampled_evaluate_blend" in unit
    for kernels in ("vk_kernel_like.h", "vk_kernel_real.h", "vk_kernel_generic.h", "vk_kernel_cells.h", "vk_kernel_fast.h"):
        text = open(os.path.join(csrc, kernels)).read()                                  # no theory or likelihood kernel knows the mode
        assert "BETA_BLEND" not in text and "BlendArgs" not in text and "reserved" not in text, kernels


def test_library_exports_the_new_symbols_and_refuses_bad_arguments():
    """The stand-alone entry points check their arguments before the first device call (no GPU here)."""
    from victor_amd import _native as N
    lib = N.load()
    for name in NEW:
        assert hasattr(lib, name), name
    g = N.f64([0.1, 0.2, 0.3])
    rows, rows2 = np.zeros((2, 12)), np.zeros((4, 12))
    t, fail = np.zeros(2), np.zeros(2, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    assert lib.vk_blend_split(0, None, 3, N.as_dp(rows), None, 2, N.as_dp(rows2), None, N.as_dp(t), fail.ctypes.data_as(ip)) == -1
    assert lib.vk_blend_split(0, N.as_dp(g), 1, N.as_dp(rows), None, 2, N.as_dp(rows2), None, N.as_dp(t), fail.ctypes.data_as(ip)) == -1
    assert lib.vk_blend_split(0, N.as_dp(g), 3, N.as_dp(rows), None, 0, N.as_dp(rows2), None, N.as_dp(t), fail.ctypes.data_as(ip)) == -1
    which = np.zeros(2, dtype=np.int32)
    assert lib.vk_blend_split(0, N.as_dp(g), 3, N.as_dp(rows), which.ctypes.data_as(ip), 2, N.as_dp(rows2), None, N.as_dp(t),
                              fail.ctypes.data_as(ip)) == -1
    raw, out = np.zeros(4), np.zeros(2)
    assert lib.vk_blend_merge(0, None, fail.ctypes.data_as(ip), 2, 1, N.as_dp(raw), N.as_dp(raw), N.as_dp(out), N.as_dp(out)) == -1
    assert lib.vk_blend_merge(0, N.as_dp(t), fail.ctypes.data_as(ip), 2, 0, N.as_dp(raw), N.as_dp(raw), N.as_dp(out), N.as_dp(out)) == -1
    assert lib.vk_blend_merge(0, N.as_dp(t), fail.ctypes.data_as(ip), 0, 1, N.as_dp(raw), N.as_dp(raw), N.as_dp(out), N.as_dp(out)) == -1
