"""Best fits (victor_amd/fitting.py, vk_fit_run) without a GPU: the simplex transition of victor_amd/csrc/vk_fit_simplex.h compiled
on its own under g++ and driven on analytic functions, checked launch by launch against a one-point-at-a-time NumPy restatement
of the same rules, and bit for bit - phase, live[] and pt[] of every slot of every launch - against the slot-for-slot mirror the
GPU tests hold the device search to (tests/fit_definition.py) at d = 1, 2, 3, 4 and 10; and the refusals of CCFFit.best_fit /
Realisations.best_fit, raised before any device call."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.test_realisations import stack_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf
EXPAND, REFLECT, OUTSIDE, INSIDE, SHRUNK, RESTART, CONVERGED, MAX_ITER, NO_FINITE_START = range(1, 10)
VERTICES = 0
ST_CONVERGED, ST_MAX_ITER, ST_NO_FINITE_START = 0, 1, 2

# The analytic functions, as lnL(x); the same scalar arithmetic in the same order in C++ (DRIVER) and in Python (LNL).
THETA = 0.3


def _rotquad(x):
    # 4-D quadratic in coordinates rotated pairwise by THETA, minimum at m = (1.5, -0.2, 0.4, 0.1): outside the box in x_0
    c, s = math.cos(THETA), math.sin(THETA)
    m = (1.5, -0.2, 0.4, 0.1)
    w = (1.0, 3.0, 0.5, 2.0)
    y = [x[i] - m[i] for i in range(4)]
    z = (c * y[0] - s * y[1], s * y[0] + c * y[1], c * y[2] - s * y[3], s * y[2] + c * y[3])
    f = 0.0
    for i in range(4):
        f = f + w[i] * (z[i] * z[i])
    return -f


def _halfinf(x):
    if x[0] < 0.0:
        return -INF if x[1] > 0.0 else math.nan
    return -((x[0] - 0.3) * (x[0] - 0.3) + 2.0 * ((x[1] + 0.4) * (x[1] + 0.4)))


# The rotated quadratic in every d: coordinates rotated pairwise by the angle whose cosine and sine are PQ_C, PQ_S (decimal
# literals, read alike by both compilers), a last odd coordinate unrotated; minimum at PQ_M (outside [-1, 1] in x_0).
PQ_C, PQ_S = 0.955336489125606, 0.29552020666133955
PQ_M = (1.5, -0.2, 0.4, 0.1, -0.3, 0.25, 0.6, -0.45, 0.05, 0.35)
PQ_W = (1.0, 3.0, 0.5, 2.0, 1.5, 0.75, 2.5, 1.25, 4.0, 0.6)


def _pairquad(x):
    d = len(x)
    y = [x[i] - PQ_M[i] for i in range(d)]
    z = list(y)
    for i in range(0, d - 1, 2):
        z[i] = PQ_C * y[i] - PQ_S * y[i + 1]
        z[i + 1] = PQ_S * y[i] + PQ_C * y[i + 1]
    f = 0.0
    for i in range(d):
        f = f + PQ_W[i] * (z[i] * z[i])
    return -f


def _pairhole(x):
    # the same with x_0 < 0 failing: -inf where the last coordinate is positive, NaN elsewhere
    if x[0] < 0.0:
        return -INF if x[len(x) - 1] > 0.0 else math.nan
    return _pairquad(x)


LNL = {
    "pairquad": _pairquad,
    "pairhole": _pairhole,
    "rosen": lambda x: -(100.0 * ((x[1] - x[0] * x[0]) * (x[1] - x[0] * x[0])) + (1.0 - x[0]) * (1.0 - x[0])),
    "rotquad": _rotquad,
    "halfinf": _halfinf,
    "vee": lambda x: -(abs(x[0] - 0.1) + 2.0 * abs(x[1] + 0.2)),
    "none": lambda x: -INF,
}

DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vk_fit_simplex.h"

static const double THETA = 0.3;
static const double PQ_C = 0.955336489125606, PQ_S = 0.29552020666133955;
static const double PQ_M[10] = {1.5, -0.2, 0.4, 0.1, -0.3, 0.25, 0.6, -0.45, 0.05, 0.35};
static const double PQ_W[10] = {1.0, 3.0, 0.5, 2.0, 1.5, 0.75, 2.5, 1.25, 4.0, 0.6};
static int D = 0;
static double pairquad(const double* x) {
  double y[10], z[10];
  for (int i = 0; i < D; ++i) z[i] = y[i] = x[i] - PQ_M[i];
  for (int i = 0; i + 1 < D; i += 2) {
    z[i] = PQ_C * y[i] - PQ_S * y[i + 1];
    z[i + 1] = PQ_S * y[i] + PQ_C * y[i + 1];
  }
  double f = 0.0;
  for (int i = 0; i < D; ++i) f = f + PQ_W[i] * (z[i] * z[i]);
  return -f;
}
static double lnl_of(const char* fn, const double* x) {
  if (!strcmp(fn, "pairquad")) return pairquad(x);
  if (!strcmp(fn, "pairhole")) {
    if (x[0] < 0.0) return x[D - 1] > 0.0 ? -HUGE_VAL : std::nan("");
    return pairquad(x);
  }
  if (!strcmp(fn, "rosen")) {
    const double a = x[1] - x[0] * x[0];
    return -(100.0 * (a * a) + (1.0 - x[0]) * (1.0 - x[0]));
  }
  if (!strcmp(fn, "rotquad")) {
    const double c = std::cos(THETA), s = std::sin(THETA);
    const double m[4] = {1.5, -0.2, 0.4, 0.1}, w[4] = {1.0, 3.0, 0.5, 2.0};
    double y[4];
    for (int i = 0; i < 4; ++i) y[i] = x[i] - m[i];
    const double z[4] = {c * y[0] - s * y[1], s * y[0] + c * y[1], c * y[2] - s * y[3], s * y[2] + c * y[3]};
    double f = 0.0;
    for (int i = 0; i < 4; ++i) f = f + w[i] * (z[i] * z[i]);
    return -f;
  }
  if (!strcmp(fn, "halfinf")) {
    if (x[0] < 0.0) return x[1] > 0.0 ? -HUGE_VAL : std::nan("");
    return -((x[0] - 0.3) * (x[0] - 0.3) + 2.0 * ((x[1] + 0.4) * (x[1] + 0.4)));
  }
  if (!strcmp(fn, "vee")) return -(std::fabs(x[0] - 0.1) + 2.0 * std::fabs(x[1] + 0.2));
  return -HUGE_VAL;
}

// usage: driver fn d max_iter restarts ftol  then d values each of lo, hi, x0, step, xtol, then the file the launches go to
int main(int argc, char** argv) {
  const char* fn = argv[1];
  vkfit::Params q{};
  q.d = D = atoi(argv[2]);
  q.S = vkfit::slots(q.d);
  q.max_iter = atoi(argv[3]);
  q.restarts = atoi(argv[4]);
  q.ftol = strtod(argv[5], nullptr);
  double x0[vkfit::kMaxP];
  int a = 6;
  for (int j = 0; j < q.d; ++j) q.lo[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < q.d; ++j) q.hi[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < q.d; ++j) x0[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < q.d; ++j) q.step[j] = strtod(argv[a++], nullptr);
  for (int j = 0; j < q.d; ++j) q.xtol[j] = strtod(argv[a++], nullptr);
  static vkfit::State s;
  vkfit::start(s, q, x0);
  FILE* launches = fopen(argv[a], "w");          // per launch: phase, live[0..S), pt[0..S)[0..d) as hexadecimal floats
  while (s.phase != vkfit::kDone) {
    double lnl[vkfit::kMaxS], chi[vkfit::kMaxS];
    fprintf(launches, "%d", s.phase);
    for (int i = 0; i < q.S; ++i) fprintf(launches, " %d", s.live[i]);
    for (int i = 0; i < q.S; ++i)
      for (int j = 0; j < q.d; ++j) fprintf(launches, " %a", s.pt[i][j]);
    fprintf(launches, "\n");
    for (int i = 0; i < q.S; ++i) {
      lnl[i] = lnl_of(fn, s.pt[i]);
      chi[i] = -2.0 * lnl[i];
    }
    printf("%d ", vkfit::transition(s, q, lnl, chi));
  }
  printf("\n%d %d %lld %.17g %.17g", s.status, s.iter, (long long)s.n_evals, -s.f[0], s.chi[0]);
  for (int j = 0; j < q.d; ++j) printf(" %.17g", s.v[0][j]);
  printf("\n%a %a", -s.f[0], s.chi[0]);
  for (int j = 0; j < q.d; ++j) printf(" %a", s.v[0][j]);
  printf("\n");
  fclose(launches);
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("fit_driver")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "victor_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(fn, lo, hi, x0, step, xtol, ftol=1e-8, max_iter=1000, restarts=0):
        args = [str(exe), fn, str(len(x0)), str(max_iter), str(restarts), repr(float(ftol))]
        for arr in (lo, hi, x0, step, xtol):
            args += [repr(float(v)) for v in arr]
        args.append(str(d / "launches.txt"))
        out = subprocess.run(args, check=True, capture_output=True, text=True).stdout.split("\n")
        decisions = [int(t) for t in out[0].split()]
        tail = out[1].split()
        S = max(4, len(x0) + 1)
        launches = []
        for line in (d / "launches.txt").read_text().splitlines():
            t = line.split()
            launches.append((int(t[0]), tuple(int(v) for v in t[1:1 + S]),
                             np.array([float.fromhex(v) for v in t[1 + S:]]).reshape(S, len(x0))))
        exact = [float.fromhex(t) for t in out[2].split()]
        return {"decisions": decisions, "status": int(tail[0]), "iter": int(tail[1]), "n_evals": int(tail[2]),
                "lnl": float(tail[3]), "chi2": float(tail[4]), "x": np.array([float(t) for t in tail[5:]]),
                "launches": launches, "exact": {"lnl": exact[0], "chi2": exact[1], "x": np.array(exact[2:])}}
    return run


def restated(fn, lo, hi, x0, step, xtol, ftol=1e-8, max_iter=1000, restarts=0):
    """The rules of the issue, one point at a time (no speculation): each 'launch' of the device search is one iteration here."""
    lnl_fn = LNL[fn]
    lo, hi, x0, step, xtol = (np.array(a, dtype=float) for a in (lo, hi, x0, step, xtol))
    d = len(x0)
    st = {"n_evals": 0, "iter": 0}

    def F(x):                                   # (f, chi2) of a point; outside the box: +inf, not evaluated
        if not np.all((x >= lo) & (x <= hi)):
            return INF, INF
        st["n_evals"] += 1
        lnl = lnl_fn([float(t) for t in x])
        if not math.isfinite(lnl):
            return INF, INF
        return -lnl, -2.0 * lnl

    def simplex(v0):
        v = [v0.copy()]
        for j in range(d):
            vj = v0.copy()
            up, down = v0[j] + step[j], v0[j] - step[j]
            vj[j] = up if up <= hi[j] else (down if down >= lo[j] else (hi[j] if hi[j] - v0[j] >= v0[j] - lo[j] else lo[j]))
            v.append(vj)
        return v

    decisions = []
    restarts_left = restarts
    v = simplex(x0.copy())
    phase = "init"
    while True:
        st["iter"] += 1
        dec = VERTICES
        if phase == "init":
            fc = [F(x) for x in v]
            f = [a for a, _ in fc]
            chi = [b for _, b in fc]
            if all(a == INF for a in f):
                decisions.append(NO_FINITE_START)
                return dict(decisions=decisions, status=ST_NO_FINITE_START, iter=st["iter"], n_evals=st["n_evals"], lnl=-INF,
                            chi2=INF, x=x0)
        elif phase == "shrink":
            for i in range(1, d + 1):
                f[i], chi[i] = F(v[i])
        else:
            c = v[0].copy()
            for i in range(1, d):
                c = c + v[i]
            c = c / d
            g = c - v[d]
            fr, cr = F(c + g)
            if fr < f[0]:
                fe, ce = F(c + 2.0 * g)
                v[d], f[d], chi[d], dec = (c + 2.0 * g, fe, ce, EXPAND) if fe < fr else (c + g, fr, cr, REFLECT)
            elif fr < f[d - 1]:
                v[d], f[d], chi[d], dec = c + g, fr, cr, REFLECT
            elif fr < f[d]:
                fo, co = F(c + 0.5 * g)
                if fo <= fr:
                    v[d], f[d], chi[d], dec = c + 0.5 * g, fo, co, OUTSIDE
                else:
                    dec = SHRUNK
            else:
                fi, ci = F(c - 0.5 * g)
                if fi < f[d]:
                    v[d], f[d], chi[d], dec = c - 0.5 * g, fi, ci, INSIDE
                else:
                    dec = SHRUNK
            if dec == SHRUNK:
                if st["iter"] >= max_iter:
                    decisions.append(MAX_ITER)
                    return dict(decisions=decisions, status=ST_MAX_ITER, iter=st["iter"], n_evals=st["n_evals"], lnl=-f[0],
                                chi2=chi[0], x=v[0])
                for i in range(1, d + 1):
                    v[i] = v[0] + 0.5 * (v[i] - v[0])
                decisions.append(SHRUNK)
                phase = "shrink"
                continue
        order = np.argsort(np.array(f), kind="stable")
        v, f, chi = [v[i] for i in order], [f[i] for i in order], [chi[i] for i in order]
        spread = np.max(np.abs(np.array(v[1:]) - v[0]), axis=0)
        if np.all(spread <= xtol) and max(a - f[0] for a in f[1:]) <= ftol:
            if restarts_left > 0 and st["iter"] < max_iter:
                restarts_left -= 1
                v = simplex(v[0].copy())
                phase = "init"
                decisions.append(RESTART)
                continue
            decisions.append(CONVERGED)
            return dict(decisions=decisions, status=ST_CONVERGED, iter=st["iter"], n_evals=st["n_evals"], lnl=-f[0], chi2=chi[0],
                        x=v[0])
        if st["iter"] >= max_iter:
            decisions.append(MAX_ITER)
            return dict(decisions=decisions, status=ST_MAX_ITER, iter=st["iter"], n_evals=st["n_evals"], lnl=-f[0], chi2=chi[0],
                        x=v[0])
        decisions.append(dec)
        phase = "cand"


def same(got, want):
    assert got["decisions"] == want["decisions"]
    assert (got["status"], got["iter"], got["n_evals"]) == (want["status"], want["iter"], want["n_evals"])
    assert np.max(np.abs(got["x"] - want["x"])) <= 1e-12, (got["x"], want["x"])
    assert got["lnl"] == want["lnl"] or abs(got["lnl"] - want["lnl"]) <= 1e-12 * max(1.0, abs(want["lnl"]))
    assert got["chi2"] == want["chi2"] or abs(got["chi2"] - want["chi2"]) <= 1e-12 * max(1.0, abs(want["chi2"]))


def test_rosenbrock_reaches_the_minimum(driver):
    case = dict(fn="rosen", lo=[-2, -2], hi=[2, 2], x0=[-1.2, 1.0], step=[0.1, 0.1], xtol=[1e-8, 1e-8], ftol=1e-14, restarts=1)
    got = driver(**case)
    same(got, restated(**case))
    assert got["status"] == ST_CONVERGED
    assert np.all(np.abs(got["x"] - 1.0) <= 1e-6), got["x"]            # within a few xtol of (1, 1) - conditioning 1e3
    assert EXPAND in got["decisions"] and INSIDE in got["decisions"] and RESTART in got["decisions"]


def test_rotated_quadratic_with_its_minimum_outside_the_box_ends_on_the_face(driver):
    lo, hi = [-1.0, -1.0, -1.0, -1.0], [1.0, 1.0, 1.0, 1.0]
    case = dict(fn="rotquad", lo=lo, hi=hi, x0=[0.0, 0.0, 0.0, 0.0], step=[0.2] * 4, xtol=[1e-7] * 4, ftol=1e-12, max_iter=4000,
                restarts=2)
    got = driver(**case)
    same(got, restated(**case))
    assert got["status"] == ST_CONVERGED
    x = got["x"]
    assert np.all(x >= lo) and np.all(x <= hi)
    assert 1.0 - x[0] <= 1e-5, x                                         # on the face x_0 = hi


def test_half_of_the_box_infinite(driver):
    case = dict(fn="halfinf", lo=[-1, -1], hi=[1, 1], x0=[0.05, 0.9], step=[0.5, 0.5], xtol=[1e-9, 1e-9], ftol=1e-14, restarts=1)
    got = driver(**case)
    same(got, restated(**case))
    assert got["status"] == ST_CONVERGED and got["x"][0] >= 0.0
    assert np.max(np.abs(got["x"] - [0.3, -0.4])) <= 1e-7


def test_shrink_and_restart(driver):
    # a start simplex that straddles the infinite half: both contractions fail and the simplex shrinks
    case = dict(fn="halfinf", lo=[-1, -1], hi=[1, 1], x0=[0.3, 0.3], step=[0.8, 0.8], xtol=[1e-10, 1e-10], ftol=1e-14, restarts=2)
    got = driver(**case)
    same(got, restated(**case))
    assert got["decisions"].count(SHRUNK) >= 2 and got["decisions"].count(RESTART) == 2, got["decisions"]
    assert got["status"] == ST_CONVERGED and np.max(np.abs(got["x"] - [0.3, -0.4])) <= 1e-8
    # a start vertex in the infinite half, the others finite: the search goes on
    case = dict(fn="halfinf", lo=[-1, -1], hi=[1, 1], x0=[-0.5, 0.5], step=[0.8, 0.8], xtol=[1e-10, 1e-10], ftol=1e-14)
    got = driver(**case)
    same(got, restated(**case))
    assert got["status"] == ST_CONVERGED and np.max(np.abs(got["x"] - [0.3, -0.4])) <= 1e-8


def test_iteration_limit_and_no_finite_start(driver):
    case = dict(fn="rosen", lo=[-2, -2], hi=[2, 2], x0=[-1.2, 1.0], step=[0.1, 0.1], xtol=[1e-8, 1e-8], max_iter=7)
    got = driver(**case)
    same(got, restated(**case))
    assert got["status"] == ST_MAX_ITER and got["iter"] == 7 and got["lnl"] >= LNL["rosen"]([-1.2, 1.0])
    case = dict(fn="none", lo=[0, 0, 0], hi=[1, 1, 1], x0=[0.5, 0.5, 0.5], step=[0.1] * 3, xtol=[1e-6] * 3)
    got = driver(**case)
    same(got, restated(**case))
    assert got["status"] == ST_NO_FINITE_START and got["iter"] == 1 and got["lnl"] == -INF and got["chi2"] == INF
    assert np.array_equal(got["x"], [0.5, 0.5, 0.5])


def test_start_simplex_falls_back_and_clamps(driver):
    """Vertex j: x0 + step_j, else x0 - step_j, else the box face with more room - visible in the search's first evaluations."""
    for x0, step in (([0.95, -0.95], [0.1, 0.1]), ([0.5, 0.2], [3.0, 3.0])):
        case = dict(fn="vee", lo=[-1, -1], hi=[1, 1], x0=x0, step=step, xtol=[1e-9, 1e-9], ftol=1e-14)
        same(driver(**case), restated(**case))


# ------------------------------------------------------------------ the slot-for-slot mirror (tests/fit_definition.py) -------
def mirrored(fn, lo, hi, x0, step, xtol, ftol=1e-8, max_iter=1000, restarts=0):
    """The same run through tests/fit_definition.run: one problem, the analytic function as its evaluation."""
    from tests import fit_definition as FD

    def evaluate(x, problem):
        lnl = np.array([LNL[fn]([float(t) for t in row]) for row in x])
        return lnl, -2.0 * lnl
    return FD.run(evaluate, [x0], lo, hi, step, xtol, ftol, max_iter, restarts, trace=True)


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def same_as_mirror(got, m, what):
    """Decisions, the slot layout of every launch, and the result: equality, not a tolerance."""
    assert got["decisions"] == m.decisions[0], (what, got["decisions"], m.decisions[0])
    assert (got["status"], got["iter"], got["n_evals"]) == (int(m.status[0]), int(m.n_iter[0]), int(m.n_evals[0])), what
    assert len(got["launches"]) == len(m.trace[0]) == got["iter"], what
    for i, ((phase, live, pt), (m_phase, m_live, m_pt)) in enumerate(zip(got["launches"], m.trace[0])):
        assert phase == m_phase and live == m_live, (what, "launch", i, phase, m_phase, live, m_live)
        assert bits(pt) == bits(m_pt), (what, "launch", i, pt, m_pt)
    e = got["exact"]
    assert bits(e["x"]) == bits(m.x[0]), (what, e["x"], m.x[0])
    assert bits(e["lnl"]) == bits(m.lnl[0]) and bits(e["chi2"]) == bits(m.chi2[0]), (what, e, m.lnl, m.chi2)


def box(d, half=1.0):
    return dict(lo=[-half] * d, hi=[half] * d)


MIRROR_CASES = [
    # the rotated quadratic in d = 1, 2, 3, 4, 10: its minimum lies outside the box in x_0, which cuts candidates off
    *[dict(fn="pairquad", **box(d), x0=[0.0] * d, step=[0.2] * d, xtol=[1e-7] * d, ftol=1e-12, max_iter=400 * d, restarts=r)
      for d in (1, 2, 3, 4, 10) for r in (0, 2)],
    # x_0 < 0 fails: -inf where the last coordinate is positive, NaN elsewhere; starts that straddle the edge
    *[dict(fn="pairhole", **box(d), x0=[0.05] + [0.3] * (d - 1), step=[0.5] * d, xtol=[1e-8] * d, ftol=1e-13, max_iter=400 * d, restarts=r)
      for d in (1, 2, 3, 4, 10) for r in (0, 2)],
    dict(fn="pairhole", **box(10), x0=[-0.5] + [0.3] * 9, step=[0.8] * 10, xtol=[1e-8] * 10, ftol=1e-13, max_iter=60),
    # no finite start vertex: every vertex in the failing half (d = 10), and a function that fails everywhere (d = 3)
    dict(fn="pairhole", **box(10), x0=[-0.9] + [0.3] * 9, step=[0.05] * 10, xtol=[1e-8] * 10, restarts=2),
    dict(fn="none", lo=[0, 0, 0], hi=[1, 1, 1], x0=[0.5, 0.5, 0.5], step=[0.1] * 3, xtol=[1e-6] * 3),
    # the cases of the tests above
    dict(fn="rosen", lo=[-2, -2], hi=[2, 2], x0=[-1.2, 1.0], step=[0.1, 0.1], xtol=[1e-8, 1e-8], ftol=1e-14, restarts=1),
    dict(fn="rosen", lo=[-2, -2], hi=[2, 2], x0=[-1.2, 1.0], step=[0.1, 0.1], xtol=[1e-8, 1e-8], max_iter=7),
    dict(fn="halfinf", lo=[-1, -1], hi=[1, 1], x0=[0.05, 0.9], step=[0.5, 0.5], xtol=[1e-9, 1e-9], ftol=1e-14, restarts=1),
    dict(fn="halfinf", lo=[-1, -1], hi=[1, 1], x0=[0.3, 0.3], step=[0.8, 0.8], xtol=[1e-10, 1e-10], ftol=1e-14, restarts=2),
    dict(fn="halfinf", lo=[-1, -1], hi=[1, 1], x0=[-0.5, 0.5], step=[0.8, 0.8], xtol=[1e-10, 1e-10], ftol=1e-14),
    dict(fn="vee", lo=[-1, -1], hi=[1, 1], x0=[0.95, -0.95], step=[0.1, 0.1], xtol=[1e-9, 1e-9], ftol=1e-14),
    dict(fn="vee", lo=[-1, -1], hi=[1, 1], x0=[0.5, 0.2], step=[3.0, 3.0], xtol=[1e-9, 1e-9], ftol=1e-14),
]


def test_the_mirror_is_the_header_bit_for_bit(driver):
    """tests/fit_definition.py against vk_fit_simplex.h under g++, launch by launch: phase, live[] and pt[] of every slot, the
    decisions, and the final x, f, chi2, iter, n_evals - all by equality.  Every Decision occurs."""
    seen, dead, shrink_cut = set(), 0, 0
    for case in MIRROR_CASES:
        got, m = driver(**case), mirrored(**case)
        what = (case["fn"], len(case["x0"]), case.get("restarts", 0), case.get("max_iter", 1000))
        same_as_mirror(got, m, what)
        same(got, restated(**case))
        seen |= set(got["decisions"])
        dead += int(m.n_dead_candidates[0])
        # the same run cut at its first shrink: the limit ends it inside the candidate launch that asked for the shrink
        if SHRUNK in got["decisions"]:
            cut = dict(case, max_iter=got["decisions"].index(SHRUNK) + 1)
            got_cut, m_cut = driver(**cut), mirrored(**cut)
            same_as_mirror(got_cut, m_cut, what + ("cut at its first shrink",))
            assert got_cut["decisions"] == got["decisions"][:cut["max_iter"] - 1] + [MAX_ITER] and got_cut["status"] == ST_MAX_ITER
            assert got_cut["launches"][-1][0] == 1                     # (kCand: the shrink launch was never laid out)
            shrink_cut += 1
    print("decisions seen:", sorted(seen), "dead candidate slots:", dead, "runs cut inside a shrink:", shrink_cut)
    assert seen == set(range(10)), sorted(seen)
    assert dead > 0 and shrink_cut > 0
    d10 = [c for c in MIRROR_CASES if len(c["x0"]) == 10]
    assert len(d10) >= 4


# ------------------------------------------------------------------ refusals (no GPU) -------
def _no_device(fit):
    def boom(*a, **k):
        raise AssertionError("best_fit reached the device before refusing its input")
    fit._get_engine = boom
    return fit


def test_input_errors_are_raised_before_any_device_call():
    import victor_amd
    from victor_amd import InputError
    params = cases.cobaya_info()["params"]
    fit = _no_device(victor_amd.CCFFit(*cases.boss_options("config")))
    with pytest.raises(InputError, match="likelihood"):
        fit.best_fit(params, beta_interpolation="likelihood")                         # beta-dependent data: host blend
    with pytest.raises(InputError, match="no column"):
        fit.best_fit(dict(params, alpha={"prior": {"min": 0.9, "max": 1.1}, "ref": {"loc": 1.0}, "proposal": 0.01}))
    with pytest.raises(InputError, match="uniform"):
        fit.best_fit(dict(params, sigma_v={"prior": {"dist": "norm", "loc": 380, "scale": 20}, "proposal": 10}))
    with pytest.raises(InputError, match="outside"):
        fit.best_fit(params, start={"fsigma8": 1.6})
    with pytest.raises(InputError, match="outside"):
        fit.best_fit(params, start={"beta": np.array([0.3, 0.7])}, fixed={"sigma_v": np.array([300.0, 400.0])})
    with pytest.raises(InputError, match="step"):
        fit.best_fit(params, step={"epsilon": 0.0})
    with pytest.raises(InputError, match="step"):
        fit.best_fit(params, step={"beta": -0.1})
    with pytest.raises(InputError, match="different lengths"):
        fit.best_fit(params, fixed={"fsigma8": np.linspace(0.3, 0.6, 4), "sigma_v": np.array([300.0, 400.0])})
    rs = victor_amd.CCFFit(*stack_options()).realisations()
    _no_device(rs.fit)
    with pytest.raises(InputError, match="scalars"):
        rs.best_fit(params, fixed={"fsigma8": np.linspace(0.3, 0.6, 16)})
    with pytest.raises(InputError, match="likelihood"):
        rs.best_fit(params, beta_interpolation="likelihood")


def test_row_columns_are_shared_with_the_walkers():
    from victor_amd import _native as N
    from victor_amd.sampler import EnsembleMetropolis
    assert EnsembleMetropolis._COLUMNS is N.ROW_COLUMNS
    assert N.ROW_COLUMNS == {"fsigma8": 0, "sigma_v": 1, "beta": 5, "astar": 6, "M": 7, "Q": 8, "bias": 9, "Av": 10}
