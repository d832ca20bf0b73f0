"""Which inputs select which kernel instantiation of the shipped library.

``RECIPES`` maps the string ``vk_last_instance`` reports (``Engine.last_instance()``) to the inputs that make the library launch
exactly that pair of kernels: a theory-kernel instantiation of ``vk_instances.h`` and the chi-square kernel that ran with it.
It is the union of ``THEORY`` (one recipe per theory-kernel instantiation) and ``LIKE`` (one per chi-square kernel and number of
data poles, 1 to 3).  ``tests/test_host.py::test_every_shipped_instantiation_has_a_recipe`` holds both against the kernel names
in the library's gfx950 code objects; ``tests/test_gpu_kernel_matrix.py`` runs every recipe on the GPU against the oracle.

A recipe's inputs are built from the committed fixtures (``tests/golden/synth``, ``tests/golden/boss``) into a scratch directory
by :func:`options`:

- data poles (``NL``): the first one, two or three of ``synth/data3`` with the matching block of ``synth/cov3``;
- real-space poles (``NLR``): the first one, two or three keys of ``synth/model.npy``; NLR = 1 through ``assume_isotropic`` on the
  three-pole file on the lattice form, and through a one-key file on the union grid;
- ``GRID`` 1 (union grid): ``r`` and ``rsv`` jittered as in ``test_non_uniform_grids_in_every_fast_mapping``;
- ``SVA`` 1: a three-key sigma_v(r, mu) template (``tests/test_host.py::_aniso_inputs``);
- ``from_data``, the RSD models, ``linear_bias`` and ``empirical_corr`` through the options;
- the batch size: point-major below 20 points, cells from 20 on (victor_hip.hip: ``cells_min``);
- knobs (``_native.set_knob``): ``FORCE_GENERIC`` for the generic kernel and K1x, ``NO_FUSE`` / ``LIKE_WIDE`` /
  ``LIKE_UNTILED`` / ``REAL_VALU`` for the chi-square kernels.
"""

import os
import re
from dataclasses import dataclass, field

import numpy as np

from tests import cases

MODES = ("streaming", "from_data", "dispersion", "dispersion_from_data", "kaiser")     # kMode* (vk_kernel_fast.h)
RSD = {"streaming": "streaming", "dispersion": "dispersion", "kaiser": "kaiser", "euclid": "euclid_special"}   # VK_RSD_* -> rsd_model
FAST_N, CELLS_N, TILED_N = 3, 32, 256


@dataclass(frozen=True)
class Setup:
    """The files of a fit: synthetic (``nlr`` real-space keys, ``nl`` data poles, ``grid``, ``sva``, ``n_real`` realisations
    in the data file) or one of the BOSS combinations (``boss``: 'config' or 'measured')."""
    nlr: int = 3
    nl: int = 3
    grid: int = 0
    sva: bool = False
    from_data: bool = False
    n_real: int = 0
    boss: str = ""


@dataclass
class Recipe:
    setup: Setup
    kw: dict = field(default_factory=dict)      # call options (rsd_model, assume_isotropic, matter_model, ...)
    n: int = FAST_N                             # batch size
    knobs: dict = field(default_factory=dict)   # VICTOR_HIP_<name>: value
    api: str = "batch"                          # "batch": log_likelihood_batch, "xi": theory_xi_batch, "real": realisations()


# Instantiations no input CCFFit accepts can select, with the condition of victor_hip.hip that excludes each.
UNREACHABLE = {}


def parse(key):
    """'cells<3,2,1,dispersion,0>+fused' -> ('cells<3,2,1,dispersion,0>', 'fused')"""
    theory, _, like = key.partition("+")
    return theory, like or None


def data_poles(theory):
    """NL of a theory instance string (K1x: None)."""
    fam, args = re.match(r"(\w+)<(.*)>", theory).groups()
    a = args.split(",")
    return {"cells": int(a[1]), "fast": int(a[1]), "generic": int(a[2])}.get(fam)


def _owned(fam, nlr, nl, grid, mode, sva, n):
    """Recipe of cells<...> / fast<...>."""
    fd = mode in ("from_data", "dispersion_from_data")
    iso = nlr == 1 and grid == 0 and not fd            # NLR = 1 both ways: assume_isotropic on the lattice file, one key elsewhere
    st = Setup(nlr=3 if iso else nlr, nl=nl, grid=grid, sva=bool(sva), from_data=fd)
    kw = {"assume_isotropic": True} if iso else {}
    if mode in ("dispersion", "dispersion_from_data"):
        kw["rsd_model"] = "dispersion"
    elif mode == "kaiser":
        kw["rsd_model"] = "kaiser"
    # the table options on top, where they keep the instance: empirical_corr (fixed tables), linear_bias (kaiser)
    if not sva and not fd and (nlr + nl) % 3 == 0 and mode != "kaiser":
        kw["empirical_corr"] = True
    if mode == "kaiser" and (nlr + nl) % 3 == 1:
        kw["matter_model"] = "linear_bias"
    return Recipe(st, kw, n)


def _theory():
    r = {}
    for nlr in (1, 2, 3):
        for nl in (1, 2, 3):
            for grid in (0, 1):
                for mode in MODES:
                    r[f"cells<{nlr},{nl},{grid},{mode},0>+fused"] = _owned("cells", nlr, nl, grid, mode, 0, CELLS_N)
                    if mode != "kaiser":
                        r[f"fast<{nlr},{nl},{grid},{mode},0>+fused"] = _owned("fast", nlr, nl, grid, mode, 0, FAST_N)
            r[f"cells<{nlr},{nl},0,streaming,1>+fused"] = _owned("cells", nlr, nl, 0, "streaming", 1, CELLS_N)
            r[f"cells<{nlr},{nl},0,dispersion,1>+fused"] = _owned("cells", nlr, nl, 0, "dispersion", 1, CELLS_N)
            r[f"fast<{nlr},{nl},0,streaming,1>+fused"] = _owned("fast", nlr, nl, 0, "streaming", 1, FAST_N)
            for rsd, model in RSD.items():
                kw = {"rsd_model": model, "assume_isotropic": nlr == 1} if nlr != 2 else {"rsd_model": model}
                st = Setup(nlr=3 if nlr == 1 else nlr, nl=nl)
                r[f"generic<{rsd},{nlr},{nl}>+like_wide"] = Recipe(st, kw, FAST_N, {"FORCE_GENERIC": "1"})
        for rsd, model in RSD.items():
            r[f"xi<{rsd},{nlr}>"] = Recipe(Setup(nlr=nlr, nl=1), {"rsd_model": model}, 6, {"FORCE_GENERIC": "1"}, api="xi")
    # beta-dependent tables (BOSS: reconstruction, 31 beta knots, blended covariance) in place of the synthetic fixture for the
    # instances its files select - the points then put beta on a knot of the table
    r["cells<1,2,0,streaming,0>+fused"] = Recipe(Setup(boss="config"), {}, CELLS_N)
    r["cells<2,2,0,kaiser,0>+fused"] = Recipe(Setup(boss="config"), {"rsd_model": "kaiser", "assume_isotropic": False,
                                                                      "matter_model": "linear_bias"}, CELLS_N)
    r["fast<1,2,0,dispersion,0>+fused"] = Recipe(Setup(boss="config"), {"rsd_model": "dispersion", "empirical_corr": True}, FAST_N)
    r["fast<2,2,0,from_data,0>+fused"] = Recipe(Setup(boss="measured"), {"assume_isotropic": False}, FAST_N)
    r["cells<1,2,0,from_data,0>+fused"] = Recipe(Setup(boss="measured"), {"matter_model": "linear_bias"}, CELLS_N)
    return r


def _like():
    """The chi-square kernels at one, two and three data poles, each behind a theory instantiation THEORY runs already."""
    r = {}
    for nl in (1, 2, 3):
        st = Setup(nlr=3, nl=nl)
        r[f"cells<3,{nl},0,streaming,0>+like_wide"] = Recipe(st, {}, CELLS_N, {"NO_FUSE": "1"})
        r[f"generic<streaming,3,{nl}>+like_tiled<8>"] = Recipe(st, {}, TILED_N, {"FORCE_GENERIC": "1", "LIKE_WIDE": "0"})
        r[f"generic<streaming,3,{nl}>+like"] = Recipe(st, {}, TILED_N, {"FORCE_GENERIC": "1", "LIKE_WIDE": "0", "LIKE_UNTILED": "1"})
        st = Setup(nlr=3, nl=nl, n_real=5)
        r[f"fast<3,{nl},0,streaming,0>+like_real<true>"] = Recipe(st, {}, FAST_N, api="real")
        r[f"fast<3,{nl},0,streaming,0>+like_real<false>"] = Recipe(st, {}, FAST_N, {"REAL_VALU": "1"}, api="real")
    return r


THEORY, LIKE = _theory(), _like()
RECIPES = {**THEORY, **LIKE}


# --------------------------------------------------------------------------------------------------------- inputs
def _synth_model(tmp, st):
    src = np.load(os.path.join(cases.GOLDEN, "synth", "model.npy"), allow_pickle=True).item()
    tab = dict(src)
    if st.grid:
        rng = np.random.default_rng(11)
        r = src["r"] + rng.uniform(-0.9, 0.9, len(src["r"]))
        rsv = src["rsv"] + rng.uniform(-2.0, 2.0, len(src["rsv"]))
        tab.update(r=r, rsv=rsv, sigmav=np.interp(rsv, src["rsv"], src["sigmav"]))
        for key in ("monopole", "quadrupole", "hexadecapole"):
            tab[key] = np.interp(r, src["r"], src[key])
    if st.sva:
        mu = np.linspace(0, 1, 9)
        tab["musv"] = mu
        tab["sigmav2d"] = tab["sigmav"][:, None] * (1 + 0.25 * mu[None, :] ** 2 - 0.1 * np.exp(-tab["rsv"][:, None] / 40) * mu[None, :])
    name = f"model_g{st.grid}_s{int(st.sva)}.npy"
    np.save(os.path.join(tmp, name), tab, allow_pickle=True)
    return name


def _synth_data(tmp, st):
    d = np.load(os.path.join(cases.GOLDEN, "synth", "data3.npy"), allow_pickle=True).item()
    cov = np.load(os.path.join(cases.GOLDEN, "synth", "cov3.npy"), allow_pickle=True).item()["covmat"]
    keys = ["s", "monopole", "quadrupole", "hexadecapole"][:1 + st.nl]
    out = {k: np.asarray(d[k], dtype=float) for k in keys}
    if st.n_real:       # realisation m: the data vector scaled by 1 + m / 50 (one file, simulation_number picks the row)
        scale = 1.0 + np.arange(st.n_real)[:, None] / 50.0
        out.update({k: out[k][None, :] * scale for k in keys[1:]})
    m = 40 * st.nl
    dname, cname = f"data_nl{st.nl}_r{st.n_real}.npy", f"cov_nl{st.nl}.npy"
    np.save(os.path.join(tmp, dname), out, allow_pickle=True)
    np.save(os.path.join(tmp, cname), {"covmat": np.ascontiguousarray(cov[:m, :m])}, allow_pickle=True)
    return dname, cname, keys


def options(st, tmp):
    """(model, data) option dictionaries of a Setup, its files written into the directory ``tmp``."""
    if st.boss:
        model, data = cases.boss_options("config")
        if st.boss == "measured":
            model["input_model_data_file"] = "boss/measured_model.npy"
            model["realspace_ccf"]["from_data"] = True
            data["covariance_matrix"]["data_file"] = "boss/cov_md_iso.npy"
        return model, data
    model, data = cases.synth_options(3)
    model["dir"] = data["dir"] = str(tmp)
    model["input_model_data_file"] = _synth_model(tmp, st)
    model["realspace_ccf"]["ccf_keys"] = ["r", "monopole", "quadrupole", "hexadecapole"][:1 + st.nlr]
    model["realspace_ccf"]["assume_isotropic"] = st.nlr == 1
    model["realspace_ccf"]["from_data"] = st.from_data
    if st.sva:
        model["velocity_pdf"]["dispersion"] = {"model": "template", "template_keys": ["rsv", "musv", "sigmav2d"]}
    dname, cname, keys = _synth_data(tmp, st)
    data["redshift_space_ccf"]["data_file"] = dname
    data["redshift_space_ccf"]["ccf_keys"] = keys
    if st.n_real:
        data["redshift_space_ccf"]["simulation_number"] = 0
    data["covariance_matrix"]["data_file"] = cname
    return model, data


def points(fit, n):
    """``n`` rows of the prior box (aperp, apar off 1): Halton points, the third with beta on a knot of the fit's beta table
    (beta-dependent tables) or of the BOSS grid; the nuisance amplitudes the options read (bias, Av) fixed."""
    hp = cases.halton_params(max(n, 3), with_beta=True)
    knots = getattr(fit, "beta_ccf", None)
    hp["beta"][2] = float(knots[len(knots) // 3]) if knots is not None else 0.3
    return dict({k: v[:n] for k, v in hp.items()}, bias=2.0, Av=0.6)
