"""The launch shapes the device step loops are tested at (tests/test_gpu_launch_shapes.py; DESIGN.md section 7b, "Launch shapes
under test") and the thresholds of the sources those shapes were chosen against.  No GPU, no library: ``thresholds()`` reads the
numbers out of the sources by regular expression, ``TABLE`` holds one row per case with the property that makes it the smallest
shape that reaches what it is about, and ``tests/test_launch_shapes.py`` checks every property against the numbers as they
stand - when somebody moves a threshold, that test fails and names the row to revisit.  The GPU cases take their shapes from
``TABLE``: nothing is stated twice.

A row: ``R`` problems x ``K`` rungs (1 without tempering) x ``W`` walkers, the move and the route.  ``chains(row)`` is R K W,
``rows(row)`` the rows of one evaluation launch inside the loop - R K W for the Metropolis moves, half of it for the stretch move,
whose half-steps move half of every ensemble - and ``steps(row)`` the step count: 2 BLOCK + 2 up to 600 chains, BLOCK + 2 above
(one block edge plus two).

``STENCILS``, further down, is the same for the two stencil calls - ``laplace`` (vk_fit_hessian) and ``fisher`` (vk_fit_fisher);
tests/test_gpu_stencil_shapes.py; DESIGN.md section 7a, "Launch shapes under test" - whose R M rows go through in chunks of R S
rows: ``slots``, ``points``, ``chunks``.

``NESTED``, at the end, is the same for nested sampling (vk_nested_start, vk_nested_begin; tests/test_gpu_nested_shapes.py;
DESIGN.md section 7d, "Launch shapes under test"): a row is ``R`` problems of ``L`` live points and ``K`` walkers, so
``nested_rows(row)`` rows per launch, ``passes(row)`` start passes and ``select_trips(n, t)`` trips of a select-kernel loop.

``CHUNKS``, before it, is the same for the chunked pipeline of the grid and importance posteriors (vk_grid_run, vk_is_run;
tests/test_gpu_chunk_shapes.py; DESIGN.md sections 7c and 7e, "Launch shapes under test"): a row is ``R`` problems, a ``chunk``
and ``G`` points (for a grid: the product of its ``bins``), so ``chunk_lengths(row)`` launches of the rows, evaluation, max,
tail, weight, accumulate and predict kernels.  The slice and batch geometry of the tail kernels is stated by plain-Python twins
of victor_amd/csrc/vk_is_tail.h (``problems_per_block`` ... ``rows_of``), which tests/test_launch_shapes.py holds to the header
compiled under g++."""

import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "victor_amd", "csrc")
MANY_CHAINS = 600        # up to here two blocks of steps and two more, above one block and two


def _read(*path):
    with open(os.path.join(ROOT, *path)) as fh:
        return fh.read()


def _one(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"{what}: the pattern {pattern!r} no longer matches its source"
    return m


def thresholds():
    """name -> int, read from the sources."""
    hip = _read("victor_amd", "csrc", "victor_hip.hip")
    chains = _read("victor_amd", "chains.py")
    t = {}
    t["kChainBlock"] = int(_one(r"constexpr int kChainBlock = (\d+);", _read("victor_amd", "csrc", "vk_kernel_chain.h"), "kChainBlock").group(1))
    t["kPartialPoints"] = int(_one(r"constexpr long long kPartialPoints = (\d+);", _read("victor_amd", "csrc", "vk_host.h"), "kPartialPoints").group(1))
    m = _one(r"const long long kFuseMaxDefault = (\d+), kFuseBlendedMin = (\d+);", hip, "kFuseMaxDefault / kFuseBlendedMin")
    t["kFuseMaxDefault"], t["kFuseBlendedMin"] = int(m.group(1)), int(m.group(2))
    # the rule the two constants enter: fused up to the one, and from the other on under a covariance gridded in beta
    _one(r"a\.n <= kFuseMaxDefault \|\| \(like && like->n_beta_c > 0 && a\.n >= kFuseBlendedMin\)", hip, "the fuse rule")
    t["cells_min"] = int(_one(r"const long long cells_min = (\d+);", hip, "cells_min").group(1))
    _one(r"n_dec >= cells_min", hip, "the point-major / cells rule")
    # cells per range by row count, streaming model: below band1 rows cpi0, below band2 cpi1, from there on cpi2 ...
    m = _one(r": \(n_dec < (\d+) \? (\d+) : \(n_dec < (\d+) \? (\d+) : (\d+)\)\);", hip, "the range bands")
    t["band1"], t["cpi0"], t["band2"], t["cpi1"], t["cpi2"] = (int(g) for g in m.groups())
    # ... and only up to kPartialPoints rows: above, one workgroup per point
    _one(r"\} else if \(a\.n <= kPartialPoints\) \{", hip, "the partial-sum limit of the ranges")
    _one(r"constexpr int kJointSortChunk = kBlock;", _read("victor_amd", "csrc", "vk_kernel_joint.h"), "kJointSortChunk")
    t["kJointSortChunk"] = int(_one(r"constexpr int kBlock = (\d+);", _read("victor_amd", "csrc", "vk_common.h"), "kBlock").group(1))
    t["kZeroCopyMaxDefault"] = int(_one(r"constexpr int64_t kZeroCopyMaxDefault = (\d+);", hip, "kZeroCopyMaxDefault").group(1))
    t["MAX_CHAINS"] = int(_one(r"(?m)^MAX_CHAINS = (\d+)$", chains, "MAX_CHAINS").group(1))
    _one(r"(?m)^BLOCK = EnsembleMetropolis\.BLOCK$", chains, "BLOCK of chains.py")
    t["BLOCK"] = int(_one(r"(?m)^    BLOCK = (\d+)", _read("victor_amd", "sampler.py"), "EnsembleMetropolis.BLOCK").group(1))
    t["VK_NPAR"] = int(_one(r"#define VK_NPAR (\d+)", _read("include", "victor_hip.h"), "VK_NPAR").group(1))
    # the stencil calls (vk_fit_hessian, vk_fit_fisher): their kernels' workgroups and the LDS ceiling of the Fisher assemble kernel
    t["kHessBlock"] = int(_one(r"constexpr int kHessBlock = (\d+);", _read("victor_amd", "csrc", "vk_kernel_hessian.h"), "kHessBlock").group(1))
    fisher = _read("victor_amd", "csrc", "vk_kernel_fisher.h")
    for name in ("kFisherRowsBlock", "kFisherBlock", "kFisherMaxSeg"):
        t[name] = int(_one(r"constexpr int %s = (\d+);" % name, fisher, name).group(1))
    m = _one(r"constexpr int kFisherLdsDoubles = (\d+) - (\d+);", fisher, "kFisherLdsDoubles")
    t["kFisherLdsDoubles"] = int(m.group(1)) - int(m.group(2))
    # the rules the constants enter: the doubles a workgroup asks for, the slots of a problem in the handle's largest launch, and
    # the chunks both stencil loops cut their R M rows into
    _one(r"fisher_lds_doubles\(int N, int d\) \{ return 2 \* \(size_t\)N \* d \+ 3 \* vkhess::kMaxP \* vkhess::kMaxP; \}", fisher, "fisher_lds_doubles")
    t["kMaxP"] = int(_one(r"constexpr int kMaxP = (\d+);", _read("victor_amd", "csrc", "vk_hessian.h"), "vkhess::kMaxP").group(1))
    _one(r"inline int slots\(int d\) \{ return d \+ 1 > 4 \? d \+ 1 : 4; \}", _read("victor_amd", "csrc", "vk_fit_simplex.h"), "vkfit::slots")
    sampled = _read("victor_amd", "csrc", "vk_sampled.hip")
    _one(r"rows_max = \(size_t\)R \* S;", sampled, "rows_max of a vk_fit handle")
    assert len(re.findall(r"const long long total = \(long long\)\(R \* M\), chunk = \(long long\)f->rows_max", sampled)) == 2, \
        "the chunk loops of hessian_run and fisher_run no longer match their pattern"
    # the chunked pipeline of the grid and importance posteriors (CHUNKS): workgroups and loads in flight of the kernels, the
    # tail's limits (vkist::, keys "tail.*" where a name is shared), the predict kernel's tile rules (vkisp::), the largest chunk
    importance, grid = _read("victor_amd", "csrc", "vk_kernel_importance.h"), _read("victor_amd", "csrc", "vk_kernel_grid.h")
    for name in ("kIsBlock", "kIsAhead", "kIsListAhead"):
        t[name] = int(_one(r"constexpr int %s = (\d+);" % name, importance, name).group(1))
    for name in ("kGridBlock", "kGridAhead"):
        t[name] = int(_one(r"constexpr int %s = (\d+);" % name, grid, name).group(1))
    tail, predict = _read("victor_amd", "csrc", "vk_is_tail.h"), _read("victor_amd", "csrc", "vk_is_predict.h")
    for name, key in (("kBlock", "tail.kBlock"), ("kBatch", "kBatch"), ("kMaxSlices", "kMaxSlices"), ("kSliceRows", "kSliceRows"), ("kMaxK", "kMaxK")):
        t[key] = int(_one(r"constexpr int %s = (\d+);" % name, tail, "vkist::" + name).group(1))
    for name, key in (("kSlices", "predict.kSlices"), ("kAhead", "predict.kAhead"), ("kTile", "predict.kTile"), ("kWave", "predict.kWave")):
        t[key] = int(_one(r"constexpr int %s = (\d+);" % name, predict, "vkisp::" + name).group(1))
    t["MAX_CHUNK"] = int(_one(r"(?m)^MAX_CHUNK = (\d+)$", _read("victor_amd", "grid.py"), "MAX_CHUNK").group(1))
    # the rules the constants enter: the launches of a chunk, the batch loop of the merge kernel, the slices of the max kernels
    for kern, block in (("vk_is_rows_kernel, a.n", "kIsBlock"), ("vk_is_weight_kernel, (long long)a.n * a.Rp", "kIsBlock"),
                        ("vk_grid_rows_kernel, a.n", "kGridBlock"), ("vk_grid_weight_kernel, (long long)a.n * a.Rp", "kGridBlock"),
                        ("vk_grid_accumulate_kernel, f->cells() * a.Rp", "kGridBlock")):
        _one(re.escape(f"sampled_launch(f, {kern}, {block}, a)"), sampled, kern.split(",")[0])
    _one(r"for \(int c0 = 0; c0 < c; c0 \+= kBatch\)", _read("victor_amd", "csrc", "vk_kernel_is_tail.h"), "the merge kernel's batch loop")
    _one(r"const int pr = a\.pr, slices = kIsBlock / pr;", importance, "the slices of vk_is_max_kernel")
    _one(r"const int pr = a\.pr, slices = kGridBlock / pr;", grid, "the slices of vk_grid_max_kernel")
    _one(r"range_ahead<kIsAhead>\(0, a\.n,", importance, "the whole-chunk walk of vk_is_accumulate_kernel")
    _one(r"for \(; i \+ kGridAhead <= a\.n; i \+= kGridAhead\)", grid, "the total's walk of vk_grid_accumulate_kernel")
    _one(r"slice_begin\(int n, int s\) \{ return \(int\)\(\(long long\)n \* s / kSlices\); \}", predict, "vkisp::slice_begin")
    # nested sampling (NESTED): the workgroups of its kernels, the ceiling of the select kernel's LDS arrays, the block of
    # iterations whose random numbers travel together (key "nested.BLOCK") and what victor_amd/nested.py accepts and defaults to
    kernel, step, nested = _read("victor_amd", "csrc", "vk_kernel_nested.h"), _read("victor_amd", "csrc", "vk_nested_step.h"), _read("victor_amd", "nested.py")
    for name in ("kNestedBlock", "kNestedSelect"):
        t[name] = int(_one(r"constexpr int %s = (\d+);" % name, kernel, name).group(1))
    t["kMaxLive"] = int(_one(r"constexpr int kMaxLive = (\d+);", step, "vknest::kMaxLive").group(1))
    t["nested.BLOCK"] = int(_one(r"constexpr int kBlock = (\d+);", step, "vknest::kBlock").group(1))
    assert t["nested.BLOCK"] == int(_one(r"(?m)^BLOCK = (\d+)$", nested, "BLOCK of nested.py").group(1)), "vknest::kBlock is not victor_amd.nested.BLOCK"
    t["MAX_LIVE"] = int(_one(r"(?m)^MAX_LIVE = (\d+)$", nested, "MAX_LIVE").group(1))
    t["MAX_ROWS"] = int(_one(r"(?m)^MAX_ROWS = (\d+)$", nested, "MAX_ROWS").group(1))
    m = _one(r"(?m)^DEFAULT_LIVE, DEFAULT_BATCH, DEFAULT_STEPS = (\d+), (\d+), (\d+)$", nested, "the defaults of nested.py")
    t["nested.DEFAULT_LIVE"], t["nested.DEFAULT_BATCH"] = int(m.group(1)), int(m.group(2))
    # the rules the constants enter: the five strided loops of the select kernel (four over the live points, one over the
    # walkers), its LDS arrays, the thread of a walker in the four per-walker kernels, the select launch, the refusal
    assert len(re.findall(r"for \(int i = tid; i < L; i \+= kNestedSelect\)", kernel)) == 4, "the select kernel's loops over the live points"
    assert len(re.findall(r"for \(int k = tid; k < K; k \+= kNestedSelect\)", kernel)) == 1, "the select kernel's loop over the walkers"
    _one(r"__shared__ double s_lnl\[vknest::kMaxLive\];", kernel, "s_lnl")
    _one(r"__shared__ int s_surv\[vknest::kMaxLive\];", kernel, "s_surv")
    _one(r"__shared__ int s_dead\[vknest::kMaxLive / 2\];", kernel, "s_dead")
    assert len(re.findall(r"const int c = blockIdx\.x \* kNestedBlock \+ threadIdx\.x;\n  if \(c >= a\.R \* a\.K\) return;", kernel)) == 4, \
        "the walker of a thread in the load, adopt, step and commit kernels"
    assert len(re.findall(r"const int r = c / a\.K", kernel)) == 4, "the problem of a walker in the load, adopt, step and commit kernels"
    _one(re.escape("sampled_launch(f, vk_nested_select_kernel, (long long)f->R * kNestedSelect, kNestedSelect, a)"), sampled, "the select launch")
    for kern, count in (("load", 1), ("adopt", 1), ("step", 1), ("commit", 1)):
        assert len(re.findall(re.escape(f"sampled_launch(f, vk_nested_{kern}_kernel, f->RK, kNestedBlock, a)"), sampled)) == count, kern
    _one(r"n_live < 2 \|\| n_live > vknest::kMaxLive", sampled, "the refusal of more live points than the LDS holds")
    _one(r"n_live < 2 or n_live > MAX_LIVE", nested, "the refusal of nested.py")
    _one(r"R \* batch > MAX_ROWS", nested, "the row limit of nested.py")
    return t


# ------------------------------------------------------------------ what a launch of m rows is, by the numbers -------------------
def cells_range(m, t):
    """Cells per range of the theory launch for m rows: 0 for the point-major kernel, -1 for one workgroup per point."""
    if m < t["cells_min"]:
        return 0
    if m > t["kPartialPoints"]:
        return -1
    return t["cpi0"] if m < t["band1"] else t["cpi1"] if m < t["band2"] else t["cpi2"]


def fused(m, t, gridded=True):
    """The data-vector route's chi-square inside the theory kernel (the BOSS fit's covariance is gridded in beta)."""
    return m <= t["kFuseMaxDefault"] or (gridded and m >= t["kFuseBlendedMin"])


def workgroups(n, t):
    return -(-n // t["kChainBlock"])


def pairs_of(K, parity):
    """vktemper::pairs_of (vk_temper_step.h; tests/test_tempering.py holds the header to the NumPy definition)."""
    return (K - parity) // 2 if K - parity > 0 else 0


def chains(row):
    return row["R"] * row.get("K", 1) * row["W"]


def rows(row):
    return chains(row) // 2 if row["move"] == "stretch" else chains(row)


def steps(row, t=None):
    block = 64 if t is None else t["BLOCK"]
    return 2 * block + 2 if chains(row) <= MANY_CHAINS else block + 2


def swap_threads(row):
    """Threads of the swap launches of the two parities."""
    return [row["R"] * pairs_of(row["K"], parity) * row["W"] for parity in (0, 1)]


# ------------------------------------------------------------------ the table -------------------------------------------------------
# ``reaches``: (text, check) pairs; check(row, t) is the property in the numbers of the sources.
def _past(n_groups):
    return lambda r, t: workgroups(rows(r), t) >= n_groups


def _range_is(key):
    return lambda r, t: cells_range(rows(r), t) == (t[key] if isinstance(key, str) else key)


def _straddles(r, t):
    """An ensemble whose movers lie on both sides of the first workgroup edge, wholly inside the launch."""
    half, edge = r["W"] // 2, t["kChainBlock"]
    e = edge // half
    return edge % half != 0 and e * half < edge < (e + 1) * half <= rows(r) and e < r["R"]


LADDER4 = {"betas": [1.0, 0.5, 0.1, 0.0], "swap_every": 3}
LADDER3 = {"betas": [1.0, 0.3, 0.0], "swap_every": 4}
LADDER5 = {"betas": [1.0, 0.5, 0.2, 0.05, 0.0], "swap_every": 3}

TABLE = {
    "M1": dict(move="metropolis", route="mocks", R=5, W=26, reaches=[
        ("three workgroups, the last with two lanes", lambda r, t: workgroups(rows(r), t) == 3 and rows(r) - 2 * t["kChainBlock"] == 2),
        ("ranges of the middle band", _range_is("cpi1"))]),
    "M2": dict(move="metropolis", route="mocks", R=70, W=8, reaches=[
        ("more problems than mocks", lambda r, t: r["R"] > 16),
        ("ranges of the upper band", _range_is("cpi2")),
        ("the smallest W x R above the band", lambda r, t: rows(r) >= t["band2"] and rows(r) <= t["kPartialPoints"])]),
    "M3": dict(move="metropolis", route="mocks", R=5, W=410, reaches=[
        ("one workgroup per point: just past kPartialPoints", lambda r, t: r["R"] * (r["W"] - 1) <= t["kPartialPoints"] < rows(r))]),
    "M4": dict(move="metropolis", route="data", R=1, W=(130, 512, 513, 2048, 2049, 8192), reaches=[
        ("130 rows: fused, ranges of the middle band", lambda r, t: fused(130, t) and cells_range(130, t) == t["cpi1"]),
        ("both sides of the fuse limit", lambda r, t: 512 <= t["kFuseMaxDefault"] < 513 and fused(512, t) and not fused(513, t)),
        ("both sides of the partial-sum limit, unfused", lambda r, t: 2048 <= t["kPartialPoints"] < 2049 and not fused(2048, t) and not fused(2049, t)
         and cells_range(2048, t) == t["cpi2"] and cells_range(2049, t) == -1),
        ("fused again under the gridded covariance", lambda r, t: 8191 < t["kFuseBlendedMin"] <= 8192 and fused(8192, t) and not fused(8192, t, gridded=False)),
        ("8192 rows leave the host entry point's in-place path", lambda r, t: t["kZeroCopyMaxDefault"] < 8192)]),
    "S1": dict(move="stretch", route="mocks", R=13, W=10, reaches=[
        ("two workgroups of movers", lambda r, t: rows(r) > t["kChainBlock"] and workgroups(rows(r), t) == 2),
        ("an ensemble straddles the workgroup edge", _straddles)]),
    "S2": dict(move="stretch", route="mocks", R=5, W=52, reaches=[
        ("ranges of the middle band in the half-launches", _range_is("cpi1")),
        ("three workgroups", _past(3))]),
    "S3": dict(move="stretch", route="data", R=1, W=1026, reaches=[
        ("a chi-square launch of its own between propose and step", lambda r, t: rows(r) == t["kFuseMaxDefault"] + 1 and not fused(rows(r), t))]),
    "T1": dict(move="tempered", route="mocks", R=3, K=4, W=11, temper=LADDER4, reaches=[
        ("the step kernel past two workgroups", _past(3)),
        ("a swap launch past one workgroup, one within", lambda r, t: swap_threads(r) == [66, 33] and swap_threads(r)[0] > t["kChainBlock"] > swap_threads(r)[1]),
        ("W divides neither the workgroup nor the pair groups' edge", lambda r, t: t["kChainBlock"] % r["W"] != 0
         and t["kChainBlock"] % (r["W"] * pairs_of(r["K"], 0)) != 0)]),
    "T2": dict(move="tempered", route="mocks", R=3, K=3, W=23, temper=LADDER3, reaches=[
        ("odd K, both swap launches past one workgroup", lambda r, t: r["K"] % 2 == 1 and min(swap_threads(r)) > t["kChainBlock"]),
        ("a swap behind the last step of a block", lambda r, t: t["BLOCK"] % r["temper"]["swap_every"] == 0)]),
    "T3": dict(move="tempered", route="data", R=1, K=5, W=105, temper=LADDER5, reaches=[
        ("an unfused evaluation between step and swap", lambda r, t: not fused(rows(r), t)),
        ("swap launches past three workgroups", lambda r, t: swap_threads(r) == [210, 210] and workgroups(210, t) > 3)]),
    "O1": dict(move=("metropolis", "stretch"), route="mocks", R=2, W=260, reaches=[
        ("lane_partial over five strides, the last partial", lambda r, t: workgroups(r["W"], t) == 5 and r["W"] % t["kChainBlock"] != 0),
        ("more chains of one problem than a workgroup count into its bins", lambda r, t: r["W"] > 4 * t["kChainBlock"]),
        ("hold and predict at more than eight workgroups of rows", lambda r, t: workgroups(r["R"] * r["W"], t) > 8)]),
    "J1": dict(move=("metropolis", "stretch"), route="dsplit_cov mocks", R=3, W=44, reaches=[
        ("the blocks' streams forked and joined per step past one workgroup", lambda r, t: workgroups(r["R"] * r["W"], t) == 3
         and r["R"] * r["W"] // 2 > t["kChainBlock"])]),
    "J2": dict(move="metropolis", route="dsplit_cov data", R=1, W=520, reaches=[
        ("the joint chi-square kernel past two sort chunks of rows, ranges of the upper band", lambda r, t: rows(r) > 2 * t["kJointSortChunk"]
         and cells_range(rows(r), t) == t["cpi2"])]),
    "J3": dict(move="metropolis", route="dsplit_diag mocks", R=3, W=44, reaches=[
        ("vk_joint_sum_kernel past one workgroup of rows", _past(3))]),
    "J4": dict(move="metropolis", route="boss_grid mocks", R=4, W=130, reaches=[
        ("the counting sort over three workgroups", lambda r, t: -(-rows(r) // t["kJointSortChunk"]) == 3)]),
    "J5": dict(move="metropolis", route="five blocks, ten parameters", R=3, W=44, reaches=[
        ("sampled_row's row-set loop at a stride of 132 rows", lambda r, t: rows(r) * t["VK_NPAR"] == 132 * t["VK_NPAR"] and _past(3)(r, t))]),
}

# What stays untested: everything above 8192 chains - in particular the 16384 chains DESIGN.md section 7b times and the
# MAX_CHAINS = 65536 the product accepts.
LARGEST_TESTED = 8192


def variants(row):
    """The (move, W) combinations of a row."""
    moves = row["move"] if isinstance(row["move"], tuple) else (row["move"],)
    widths = row["W"] if isinstance(row["W"], tuple) else (row["W"],)
    return [dict(row, move=m, W=w) for m in moves for w in widths]


# ------------------------------------------------------------------ the stencil calls: laplace and fisher -------------------------
# vk_fit_hessian and vk_fit_fisher cut the R M stencil rows of a call into chunks of rows_max = R S rows (S the slots of a
# problem in the search's launches), each chunk an evaluation launch of its own: the full chunks have R S rows, the last one
# the remainder - which may lie in another regime of the evaluator than the chunks before it.  A row of ``STENCILS``: the
# ``call`` ("laplace", "fisher" or both), the ``route``, d sampled parameters and R problems (one or several), and ``reaches``
# as in ``TABLE``.  A row that claims to be the smallest on its threshold names the property in ``smallest``: it holds at the
# row's largest R and not one problem below.
def slots(d):
    """vkfit::slots (vk_fit_simplex.h)."""
    return max(4, d + 1)


def points(call, d):
    """Stencil points per problem: vkhess::n_points, vkfisher::n_rows."""
    return {"laplace": 2 * d * d + 1, "fisher": 2 * d + 1}[call]


def chunks(row):
    """The chunk lengths of the R M rows of a call, in launch order."""
    total, chunk = row["R"] * points(row["call"], row["d"]), row["R"] * slots(row["d"])
    return [min(chunk, total - g0) for g0 in range(0, total, chunk)]


def fisher_lds_doubles(n_entries, d, t):
    """fisher_lds_doubles of vk_kernel_fisher.h: the dynamic LDS of the Fisher assemble kernel, in doubles."""
    return 2 * n_entries * d + 3 * t["kMaxP"] * t["kMaxP"]


def _full(r):
    return chunks(r)[:-1]


def _last(r):
    return chunks(r)[-1]


def _all_full(check):
    return lambda r, t: len(_full(r)) > 0 and all(check(m, t) for m in _full(r))


def _is(*lengths):
    """The chunks are exactly these."""
    return lambda r, t: chunks(r) == list(lengths)


BOSS_N, DSPLIT_N = 60, 120          # entries of the BOSS theory vector (30 s bins, two poles) and of a density-split block's

STENCILS = {
    "H1": dict(call="laplace", route="data", d=3, R=5, reaches=[
        ("the first chunk exactly at cells_min", lambda r, t: chunks(r)[0] == t["cells_min"] and cells_range(chunks(r)[0], t) == t["cpi0"]),
        ("the last chunk on the point-major kernel", lambda r, t: cells_range(_last(r), t) == 0)],
        smallest=lambda r, t: cells_range(chunks(r)[0], t) != 0),
    "H2": dict(call="laplace", route="data", d=3, R=32, reaches=[
        ("four chunks of 128 and one of 96", _is(128, 128, 128, 128, 96)),
        ("full chunks in the middle band, the last in the lower band", lambda r, t: _all_full(lambda m, t: cells_range(m, t) == t["cpi1"])(r, t)
         and cells_range(_last(r), t) == t["cpi0"]),
        ("every chunk fused", lambda r, t: all(fused(m, t) for m in chunks(r)))]),
    "H3": dict(call="laplace", route="data", d=3, R=(128, 129), reaches=[
        ("R = 128: every chunk fused, the full ones at the fuse limit", lambda r, t: r["R"] != 128 or (chunks(r)[0] == t["kFuseMaxDefault"]
         and all(fused(m, t) for m in chunks(r)))),
        ("R = 129: the full chunks unfused, the last chunk fused", lambda r, t: r["R"] != 129 or (_all_full(lambda m, t: not fused(m, t))(r, t)
         and fused(_last(r), t)))],
        smallest=lambda r, t: not fused(chunks(r)[0], t)),
    "H4": dict(call="laplace", route="data", d=3, R=513, reaches=[
        ("full chunks one workgroup per point", _all_full(lambda m, t: cells_range(m, t) == -1)),
        ("the last chunk back on partial sums", lambda r, t: cells_range(_last(r), t) == t["cpi2"]),
        ("every chunk unfused", lambda r, t: not any(fused(m, t) for m in chunks(r)))],
        smallest=lambda r, t: cells_range(chunks(r)[0], t) == -1),
    "H5": dict(call="laplace", route="data", d=3, R=2048, reaches=[
        ("full chunks fused again under the gridded covariance", _all_full(lambda m, t: m >= t["kFuseBlendedMin"] and fused(m, t) and not fused(m, t, gridded=False))),
        ("the last chunk unfused, one workgroup per point", lambda r, t: not fused(_last(r), t) and cells_range(_last(r), t) == -1),
        ("2048 workgroups of the assemble kernel, 32 full workgroups of the rows kernel per chunk", lambda r, t: r["R"] == 2048
         and chunks(r)[0] % t["kHessBlock"] == 0)],
        smallest=lambda r, t: fused(chunks(r)[0], t)),
    "H6": dict(call="laplace", route="data", d=1, R=513, reaches=[
        ("M < S: one chunk, shorter than the buffer", lambda r, t: points("laplace", r["d"]) < slots(r["d"]) and len(chunks(r)) == 1),
        ("the chunk on partial sums, the buffer's length one workgroup per point", lambda r, t: cells_range(chunks(r)[0], t) == t["cpi2"]
         and cells_range(r["R"] * slots(r["d"]), t) == -1)]),
    "H7": dict(call="laplace", route="mocks", d=3, R=513, reaches=[
        ("the pairs-mode realisation kernel at one workgroup per point, then on partial sums", lambda r, t: cells_range(chunks(r)[0], t) == -1
         and cells_range(_last(r), t) == t["cpi2"]),
        ("row_which over 33 workgroups of the rows kernel", lambda r, t: -(-chunks(r)[0] // t["kHessBlock"]) == 33)]),
    "F1": dict(call="fisher", route="data", d=3, R=(4, 5), reaches=[
        ("R = 4: point-major", lambda r, t: r["R"] != 4 or all(cells_range(m, t) == 0 for m in chunks(r))),
        ("R = 5: the first chunk exactly at cells_min", lambda r, t: r["R"] != 5 or (chunks(r)[0] == t["cells_min"] and cells_range(_last(r), t) == 0))],
        smallest=lambda r, t: cells_range(chunks(r)[0], t) != 0),
    "F2": dict(call="fisher", route="data", d=3, R=32, reaches=[
        ("middle and lower band", lambda r, t: chunks(r) == [128, 96] and cells_range(128, t) == t["cpi1"] and cells_range(96, t) == t["cpi0"])]),
    "F3": dict(call="fisher", route="data", d=3, R=64, reaches=[
        ("upper and middle band", lambda r, t: chunks(r) == [256, 192] and cells_range(256, t) == t["cpi2"] and cells_range(192, t) == t["cpi1"])]),
    "F4": dict(call="fisher", route="data", d=3, R=513, reaches=[
        ("one workgroup per point, then partial sums", lambda r, t: chunks(r) == [2052, 1539] and cells_range(2052, t) == -1
         and cells_range(1539, t) == t["cpi2"]),
        ("the second chunk written at an offset of 2052 N doubles, past one workgroup of the rows kernel", lambda r, t: chunks(r)[0] * BOSS_N == 123120
         and chunks(r)[0] > t["kFisherRowsBlock"])],
        smallest=lambda r, t: cells_range(chunks(r)[0], t) == -1),
    "J6": dict(call=("laplace", "fisher"), route=("five_cov", "five_diag"), d=2, R=130, reaches=[
        ("520 rows per chunk: more than two sort chunks of the joint chi-square kernels, past the fuse limit", lambda r, t: chunks(r)[0] == 520
         and chunks(r)[0] > 2 * t["kJointSortChunk"] and chunks(r)[0] > t["kFuseMaxDefault"]),
        ("a shorter last chunk", lambda r, t: 0 < _last(r) < chunks(r)[0])]),
    "J7": dict(call="laplace", route="boss_grid", d=3, R=130, reaches=[
        ("the counting sort over three chunks", lambda r, t: -(-chunks(r)[0] // t["kJointSortChunk"]) == 3 and chunks(r)[0] == 520)]),
    "J8": dict(call=("laplace", "fisher"), route="five_cov", d=10, R=24, reaches=[
        ("264 rows per chunk; M = 201 for laplace", lambda r, t: chunks(r)[0] == 264 and (r["call"] != "laplace" or points("laplace", r["d"]) == 201)),
        ("96 KiB of LDS in 24 workgroups of the Fisher assemble kernel", lambda r, t: r["call"] != "fisher"
         or (64 * 1024 < 8 * fisher_lds_doubles(5 * DSPLIT_N, r["d"], t) <= 8 * t["kFisherLdsDoubles"] and r["R"] == 24))]),
}
SMALLEST = ("H1", "H3", "H4", "H5", "F1", "F4")

# The LDS ceiling of the Fisher assemble kernel (tests/test_gpu_stencil_shapes.py, section 4): block-diagonal joint fits of
# fixed-covariance BOSS blocks of BOSS_N entries each - the largest N d the library accepts in 16 of its 32 segments, and the
# first it refuses.
CEILING = dict(accepted=dict(blocks=16, d=10, R=2), refused=dict(blocks=17, d=10, R=2), below=dict(blocks=17, d=9, R=2))

# What stays untested: the stencil calls above 8192 rows per chunk, and ``refine`` passes at these sizes.
LARGEST_STENCIL_CHUNK = 8192


def stencil_variants(row):
    """The (call, route, R) combinations of a stencil row."""
    def each(v):
        return v if isinstance(v, tuple) else (v,)
    return [dict(row, call=c, route=p, R=n) for c in each(row["call"]) for p in each(row["route"]) for n in each(row["R"])]


# ------------------------------------------------------------------ the chunked pipeline: grid and importance posteriors ----------
# vk_is_run and vk_grid_run send G points through in chunks of ``chunk`` rows; per chunk a rows kernel, the evaluation of n rows,
# a max kernel, with a tail the filter and merge kernels, a weight kernel, an accumulate kernel and, with ``predictive``, the
# predict kernel.  A row of ``CHUNKS``: ``kind`` ("importance" or "grid"), the ``route``, R problems (``prior``: one more, the
# prior's own), ``chunk`` and ``G`` (a grid: the product of ``bins``, last axis fastest), the ``tail`` sizes M the row runs at
# ("all": G - 1, None: the default size), whether it runs with ``predictive``, and ``reaches`` as in ``TABLE``.
def chunk_lengths(row):
    """The rows of every chunk of a row, in launch order."""
    return [min(row["chunk"], row["G"] - g0) for g0 in range(0, row["G"], row["chunk"])]


def problems_of_a_workgroup(R):
    """The power of two >= R, at most 64: ``pr`` of the max kernels, vkisp::problems_per_wave, vkist::problems_per_block."""
    pr = 1
    while pr < 64 and pr < R:
        pr *= 2
    return pr


# the twins of victor_amd/csrc/vk_is_tail.h
def problems_per_block(R):
    return problems_of_a_workgroup(R)


def slices_per_block(pr, t):
    return t["tail.kBlock"] // pr


def row_blocks(n, pr, t):
    per = slices_per_block(pr, t)
    most = t["kMaxSlices"] // per
    want = (n + per * t["kSliceRows"] - 1) // (per * t["kSliceRows"])
    return 1 if want < 1 else min(want, most)


def block_begin(n, gy, y):
    return n * y // gy


def slice_of(n, pr, gy, s, t):
    """``(first, end, step)`` of slice s of a chunk of n rows."""
    per = slices_per_block(pr, t)
    y, sl = divmod(s, per)
    return block_begin(n, gy, y) + sl, block_begin(n, gy, y + 1), per


def rows_of(c):
    first, end, step = c
    return (end - first + step - 1) // step if first < end else 0


def tail_shape(n, R, t):
    """``(pr, gy, S)`` of the filter launch of a chunk of n rows: problems of a workgroup, blocks of rows, slices."""
    pr = problems_per_block(R)
    gy = row_blocks(n, pr, t)
    return pr, gy, gy * slices_per_block(pr, t)


def batches(c, t):
    """The candidates of every batch of a merge of c candidates."""
    return [min(t["kBatch"], c - c0) for c0 in range(0, c, t["kBatch"])]


def tail_entries(row, size):
    """K, the entries held per problem, of a tail of ``size`` (M + 1; None: the default M of victor_amd.importance)."""
    G = row["G"]
    if size is None:
        m = min(int(0.2 * G), math.ceil(3 * math.sqrt(G)), 4095)                # default_tail_size of victor_amd/importance.py
    else:
        m = G - 1 if size == "all" else size
    return m + 1


def max_slice_rows(n, Rp, block):
    """The most rows a thread of a max kernel sees: the chunk over block / pr slices."""
    return -(-n // (block // problems_of_a_workgroup(Rp)))


def _groups(threads, block):
    return -(-threads // block)


def _chunks_are(*lengths):
    return lambda r, t: chunk_lengths(r) == list(lengths)


def _tail_is(n, pr, gy, S):
    return lambda r, t: tail_shape(n, r["R"], t) == (pr, gy, S)


def _batches_are(n, *sizes):
    return lambda r, t: batches(n, t) == list(sizes)


def _smallest_n_of_a_second_block(r, t):
    """At pr = 64 the filter launch gets a second block of rows at the smallest n of all pr, and this chunk is past it."""
    first = {pr: next((n for n in range(1, t["MAX_CHUNK"] + 1) if row_blocks(n, pr, t) > 1), math.inf) for pr in (1, 2, 4, 8, 16, 32, 64)}
    return problems_per_block(r["R"]) == 64 and first[64] == min(first.values()) == 65 and first[64] <= r["chunk"] < 3 * first[64]


def _empty_slices(n, R, t):
    pr, gy, S = tail_shape(n, R, t)
    return sum(1 for s in range(S) if rows_of(slice_of(n, pr, gy, s, t)) == 0)


def grid_cells(row):
    """Accumulators of a problem of a grid row: the total, a cell per node of every axis and per node pair of every pair."""
    bins = row["bins"]
    return 1 + sum(bins) + sum(bins[a] * bins[b] for a, b in row.get("pairs", ()))


def _edges_inside_runs(r, t):
    """Every chunk edge lies inside a run of every axis but the fastest (whose runs are single indices), and inside a period of
    every axis: no chunk starts or ends where a run does."""
    bins, G = r["bins"], r["G"]
    strides = [math.prod(bins[j + 1:]) for j in range(len(bins))]
    edges = list(range(r["chunk"], G, r["chunk"]))
    return len(edges) > 0 and all(e % (s * n) != 0 for e in edges for s, n in zip(strides, bins) if s * n < G) \
        and all(e % s != 0 for e in edges for s in strides if s > 1)


CHUNKS = {
    "I1": dict(kind="importance", route="synthetic mocks", R=3, chunk=300, G=700, tail=(7, 100), predictive=True, reaches=[
        ("chunks of 300, 300 and 100", _chunks_are(300, 300, 100)),
        ("the rows kernel in two workgroups, the last partial", lambda r, t: _groups(300, t["kIsBlock"]) == 2 and 300 % t["kIsBlock"] != 0),
        ("the weight kernel in four workgroups", lambda r, t: _groups(300 * r["R"], t["kIsBlock"]) == 4),
        ("max-kernel slices of five rows", lambda r, t: max_slice_rows(300, r["R"], t["kIsBlock"]) == 5),
        ("range_ahead over 18 full batches and 12 rows", lambda r, t: divmod(300, t["kIsAhead"]) == (18, 12)),
        ("predict slices of 75 rows: nine kAhead batches and three rows", lambda r, t: 300 // t["predict.kSlices"] == 75
         and divmod(75, t["predict.kAhead"]) == (9, 3)),
        ("the evaluator in the upper cells band", lambda r, t: cells_range(300, t) == t["cpi2"]),
        ("one block of rows in the filter kernel: the tail's geometry is that of the small tests", _tail_is(300, 4, 1, 64))]),
    "I2": dict(kind="importance", route="synthetic mocks, repeated", R=70, chunk=130, G=300, tail=(20,), predictive=True, reaches=[
        ("chunks of 130, 130 and 40", _chunks_are(130, 130, 40)),
        ("pr = 64, three blocks of rows, twelve slices", _tail_is(130, 64, 3, 12)),
        ("blockIdx.y > 0 where it starts at the smallest n", _smallest_n_of_a_second_block),
        ("uneven cuts of the blocks: 43 and 86", lambda r, t: [block_begin(130, 3, y) for y in range(4)] == [0, 43, 86, 130]),
        ("then a chunk with fewer slices than the one before", lambda r, t: tail_shape(40, r["R"], t)[2] < tail_shape(130, r["R"], t)[2]),
        ("the wide predict kernel over two problem tiles", lambda r, t: problems_of_a_workgroup(r["R"]) == t["predict.kWave"]
         and _groups(r["R"], t["predict.kWave"]) == 2)]),
    "I3": dict(kind="importance", route="synthetic mocks", R=3, chunk=1100, G=2300, tail=(300, "all"), predictive=False, reaches=[
        ("chunks of 1100, 1100 and 100", _chunks_are(1100, 1100, 100)),
        ("two blocks of rows, 128 slices", _tail_is(1100, 4, 2, 128)),
        ("1100 candidates: two batches, 1024 and 76", _batches_are(1100, 1024, 76)),
        ("the evaluator unfused on partial sums", lambda r, t: not fused(1100, t) and cells_range(1100, t) == t["cpi2"]),
        ("size 300: K = 301 past one workgroup, a threshold after chunk 1", lambda r, t: t["tail.kBlock"] < tail_entries(r, 300) <= r["chunk"]),
        ("size G - 1: K = 2300 past a batch, never a threshold; chunk 2 merges 1100 into h = 1100 > kBatch", lambda r, t: tail_entries(r, "all") == r["G"]
         and r["G"] > t["kBatch"] and r["chunk"] > t["kBatch"] and tail_entries(r, "all") <= t["kMaxK"])]),
    "I4": dict(kind="importance", route="synthetic mocks", R=3, chunk=2049, G=2600, tail=(50,), predictive=True, reaches=[
        ("chunks of 2049 and 551", _chunks_are(2049, 551)),
        ("one workgroup per point just past kPartialPoints, the last chunk back on partial sums", lambda r, t: cells_range(2048, t) == t["cpi2"]
         and cells_range(2049, t) == -1 and cells_range(551, t) == t["cpi2"]),
        ("three blocks of rows, 192 slices", _tail_is(2049, 4, 3, 192)),
        ("three batches: 1024, 1024 and 1", _batches_are(2049, 1024, 1024, 1))]),
    "I5": dict(kind="importance", route="synthetic mocks, repeated", R=70, chunk=4200, G=4250, tail=(20, 4095), predictive=False, reaches=[
        ("chunks of 4200 and 50", _chunks_are(4200, 50)),
        ("the blocks of rows clamped at 64: S = 256 = kMaxSlices = kBlock", lambda r, t: tail_shape(4200, r["R"], t) == (64, 64, 256)
         and -(-4200 // (slices_per_block(64, t) * t["kSliceRows"])) > 64 and t["kMaxSlices"] == t["tail.kBlock"] == 256),
        ("five batches", lambda r, t: len(batches(4200, t)) == 5),
        ("the weight kernel past 1000 workgroups", lambda r, t: _groups(4200 * r["R"], t["kIsBlock"]) > 1000),
        ("size 4095: K = kMaxK", lambda r, t: tail_entries(r, 4095) == t["kMaxK"] <= r["G"])]),
    "I6": dict(kind="importance", route="BOSS data vector", R=1, chunk=8192, G=8292, tail=(None, 2000), predictive=False, reaches=[
        ("chunks of 8192 and 100", _chunks_are(8192, 100)),
        ("pr = 1: 256 slices of 32 rows", lambda r, t: tail_shape(8192, 1, t) == (1, 1, 256)
         and {rows_of(slice_of(8192, 1, 1, s, t)) for s in range(256)} == {32}),
        ("exactly eight full batches", lambda r, t: 8192 % t["kBatch"] == 0 and batches(8192, t) == [t["kBatch"]] * 8),
        ("the evaluator fused again under the gridded covariance, past the in-place path", lambda r, t: fused(8192, t)
         and not fused(8192, t, gridded=False) and t["kZeroCopyMaxDefault"] < 8192),
        ("the last chunk with 156 empty slices", lambda r, t: tail_shape(100, 1, t)[2] == 256 and _empty_slices(100, 1, t) == 156),
        ("the default size holds K = 275", lambda r, t: tail_entries(r, None) == 275)]),
    "I7": dict(kind="importance", route="dsplit_cov joint mocks", R=3, chunk=530, G=1100, tail=(10,), predictive=True, reaches=[
        ("chunks of 530, 530 and 40", _chunks_are(530, 530, 40)),
        ("the joint chi-square kernel past two sort chunks, past the fuse limit", lambda r, t: 530 > 2 * t["kJointSortChunk"]
         and 530 > t["kFuseMaxDefault"])]),
    "G1": dict(kind="grid", route="synthetic mocks", R=3, bins=(40, 30), pairs=((0, 1),), chunk=500, G=1200, reaches=[
        ("chunks of 500, 500 and 200", _chunks_are(500, 500, 200)),
        ("every chunk cuts runs at both ends", _edges_inside_runs),
        ("a chunk holds several periods of the fast axis", lambda r, t: min(chunk_lengths(r)) >= 2 * r["bins"][-1]),
        ("the rows kernel in two workgroups", lambda r, t: _groups(500, t["kGridBlock"]) == 2),
        ("the total's walk over 15 batches and 20 rows", lambda r, t: divmod(500, t["kGridAhead"]) == (15, 20))]),
    "G2": dict(kind="grid", route="synthetic mocks, repeated", R=70, bins=(60, 40), pairs=((0, 1),), chunk=2049, G=2400, reaches=[
        ("chunks of 2049 and 351", _chunks_are(2049, 351)),
        ("the max kernel over two problem tiles", lambda r, t: _groups(r["R"], problems_of_a_workgroup(r["R"])) == 2),
        ("the accumulate kernel over tens of thousands of (cell, problem) threads", lambda r, t: grid_cells(r) * r["R"] >= 10000),
        ("the evaluator one workgroup per point, then on partial sums", lambda r, t: cells_range(2049, t) == -1
         and cells_range(351, t) == t["cpi2"])]),
    "G3": dict(kind="grid", route="BOSS data vector", R=1, prior=True, bins=(24, 20, 18), pairs=(), chunk=8192, G=8640, reaches=[
        ("chunks of 8192 and 448", _chunks_are(8192, 448)),
        ("the prior's own problem: Rp = 2, lnprior[] at 8192 rows", lambda r, t: r["R"] + int(r["prior"]) == 2),
        ("the fused-blended evaluator regime", lambda r, t: fused(8192, t) and not fused(8192, t, gridded=False)),
        ("a chunk edge inside runs of all three axes", _edges_inside_runs)]),
}

# What stays untested: chunks above 8192 rows, up to the MAX_CHUNK = 65536 the product accepts (the default chunk of a call with
# few problems).
LARGEST_CHUNK_TESTED = 8192


# ------------------------------------------------------------------ nested sampling ---------------------------------------------
# vk_nested_start and vk_nested_begin launch R K rows at a time - row r K + k walker k of problem r: L / K start passes (load,
# evaluation, adopt), then per iteration the select kernel (one workgroup of kNestedSelect threads per problem, strided loops
# over the L live points and the K walkers, LDS arrays of kMaxLive entries), S times (evaluation, step kernel) and the commit
# kernel; the load, adopt, step and commit kernels have one thread per walker in workgroups of kNestedBlock.  A row of
# ``NESTED``: the ``route``, R problems, L live points, K walkers (tuples of equal length: one variant per pair), S steps,
# ``n_iter`` iterations, the ``seed``, and ``reaches`` as in ``TABLE``.
def nested_rows(row):
    """The rows of every launch of a run."""
    return row["R"] * row["K"]


def passes(row):
    """The start passes: launches of load, evaluation and adopt."""
    return row["L"] // row["K"]


def select_trips(n, t):
    """The trips a loop of the select kernel makes over n entries."""
    return -(-n // t["kNestedSelect"])


def walker_groups(row, t):
    """The workgroups of the per-walker kernels."""
    return -(-nested_rows(row) // t["kNestedBlock"])


def split_problems(row, t):
    """The problems whose walkers lie in two workgroups of the per-walker kernels: a workgroup edge inside their K rows."""
    K, block = row["K"], t["kNestedBlock"]
    return sum(1 for r in range(row["R"]) if (r * K) // block != (r * K + K - 1) // block)


def _lds_full(r, t):
    """Every LDS array of the select kernel is used to its last entry: s_lnl and s_surv hold L, s_dead holds K."""
    return r["L"] == t["kMaxLive"] == t["MAX_LIVE"] and 2 * r["K"] == t["kMaxLive"]


def _nested_range_is(key):
    return lambda r, t: cells_range(nested_rows(r), t) == (t[key] if isinstance(key, str) else key)


NESTED = {
    "N1": dict(route="mocks", R=16, L=256, K=32, S=2, n_iter=9, seed=1, reaches=[
        ("the product's default live points and batch on the 16 golden mocks", lambda r, t: (r["L"], r["K"], r["R"]) == (t["nested.DEFAULT_LIVE"], t["nested.DEFAULT_BATCH"], 16)),
        ("L == kNestedSelect: one full trip of every loop over the live points", lambda r, t: r["L"] == t["kNestedSelect"] and select_trips(r["L"], t) == 1),
        ("512 rows: ranges of the upper band", lambda r, t: nested_rows(r) == 512 and _nested_range_is("cpi2")(r, t)),
        ("nine iterations cross a block of random numbers", lambda r, t: t["nested.BLOCK"] < r["n_iter"] < 2 * t["nested.BLOCK"])]),
    "N2": dict(route="data", R=1, L=258, K=129, S=2, n_iter=3, seed=2, reaches=[
        ("a second trip over the live points with two lanes", lambda r, t: r["L"] == t["kNestedSelect"] + 2 and select_trips(r["L"], t) == 2),
        ("the walkers past two workgroups, one lane in the third", lambda r, t: walker_groups(r, t) == 3 and nested_rows(r) - 2 * t["kNestedBlock"] == 1),
        ("fused, ranges of the middle band", lambda r, t: fused(nested_rows(r), t) and _nested_range_is("cpi1")(r, t))]),
    "N3": dict(route="data", R=1, L=(1024, 1026), K=(512, 513), S=2, n_iter=3, seed=3, reaches=[
        ("both sides of the fuse limit on the data-vector route", lambda r, t: nested_rows(r) - t["kFuseMaxDefault"] in (0, 1)
         and fused(nested_rows(r), t) == (nested_rows(r) == t["kFuseMaxDefault"]) and fused(512, t) and not fused(513, t)),
        ("K = 513: a third trip of the walker loop with one lane", lambda r, t: r["K"] != 513 or (r["K"] == 2 * t["kNestedSelect"] + 1 and select_trips(r["K"], t) == 3)),
        ("K = 512: two full trips of the walker loop, four of the loops over the live points", lambda r, t: r["K"] != 512
         or (r["K"] == 2 * t["kNestedSelect"] and select_trips(r["L"], t) == 4 and r["L"] % t["kNestedSelect"] == 0)),
        ("L = 1026: not a multiple of a wave", lambda r, t: r["L"] != 1026 or (r["L"] % 64 == 2 and select_trips(r["L"], t) == 5)),
        ("ranges of the upper band", _nested_range_is("cpi2"))]),
    "N4": dict(route="data", R=1, L=4096, K=2048, S=2, n_iter=3, seed=4, reaches=[
        ("L == kMaxLive, K == kMaxLive / 2: every LDS array full", _lds_full),
        ("rows exactly at kPartialPoints, unfused on partial sums", lambda r, t: nested_rows(r) == t["kPartialPoints"] and not fused(nested_rows(r), t)
         and _nested_range_is("cpi2")(r, t)),
        ("16 trips of the rank loop, 8 of the walker loop", lambda r, t: select_trips(r["L"], t) == 16 and select_trips(r["K"], t) == 8)]),
    "N5": dict(route="mocks", R=3, L=1366, K=683, S=2, n_iter=3, seed=5, reaches=[
        ("the smallest R K past kPartialPoints at R = 3: one workgroup per point", lambda r, t: r["R"] * (r["K"] - 1) <= t["kPartialPoints"] < nested_rows(r)
         and _nested_range_is(-1)(r, t)),
        ("K is no multiple of a workgroup: every problem edge inside a workgroup of the load, adopt, step and commit kernels",
         lambda r, t: r["R"] > 1 and t["kNestedBlock"] % r["K"] != 0 and all((q * r["K"]) % t["kNestedBlock"] != 0 for q in range(1, r["R"]))),
        ("L % 64 == 22: a partial wave in the last trip over the live points", lambda r, t: r["L"] % 64 == 22 and select_trips(r["L"], t) == 6)]),
    "N6": dict(route="mocks, repeated", R=4, L=4096, K=2048, S=2, n_iter=3, seed=6, reaches=[
        ("8192 rows: the largest launch under test, one workgroup per point", lambda r, t: nested_rows(r) == 8192 == LARGEST_NESTED_ROWS_TESTED
         and _nested_range_is(-1)(r, t)),
        ("four select workgroups, each with every LDS array full", lambda r, t: r["R"] == 4 and _lds_full(r, t)),
        ("the definition route's log_likelihood_pairs past the in-place host path", lambda r, t: t["kZeroCopyMaxDefault"] < nested_rows(r))]),
    "N7": dict(route="mocks, repeated", R=300, L=6, K=3, S=2, n_iter=3, seed=7, reaches=[
        ("more problems than the select kernel has threads, more than mocks", lambda r, t: r["R"] > t["kNestedSelect"] and r["R"] > 16 + 16),
        ("900 rows: ranges of the upper band", lambda r, t: nested_rows(r) == 900 and _nested_range_is("cpi2")(r, t)),
        ("K = 3 does not divide a workgroup: ten of the fourteen workgroup edges split a problem", lambda r, t: t["kNestedBlock"] % r["K"] != 0
         and walker_groups(r, t) == 15 and split_problems(r, t) == 10)]),
    "N8": dict(route="mocks", R=3, L=320, K=5, S=2, n_iter=3, seed=8, reaches=[
        ("64 start passes: pass K addressing of load and adopt", lambda r, t: passes(r) == 64),
        ("L % kNestedSelect == 64: a second trip of one wave", lambda r, t: r["L"] % t["kNestedSelect"] == 64 and select_trips(r["L"], t) == 2),
        ("15 rows: the point-major kernel", _nested_range_is(0))]),
    "N9": dict(route="paired models", R=3, L=48, K=24, S=2, n_iter=3, seed=9, reaches=[
        ("72 rows: row_which written by select and step across a workgroup edge", lambda r, t: nested_rows(r) == 72 > t["kNestedBlock"]
         and t["kNestedBlock"] % r["K"] != 0 and split_problems(r, t) == 1)]),
    "N10": dict(route="dsplit_diag joint mocks, sigma_v@q per block", R=5, L=176, K=88, S=2, n_iter=3, seed=10, reaches=[
        ("R K past kJointSortChunk: sampled_row's row-set loop at a stride of 440 rows", lambda r, t: nested_rows(r) == 440 > t["kJointSortChunk"]),
        ("problems split across workgroups of the per-walker kernels", lambda r, t: t["kNestedBlock"] % r["K"] != 0 and split_problems(r, t) >= 4)]),
}

# What stays untested: launches above 8192 rows, up to the MAX_ROWS = 65536 the product accepts - in particular the 32768 rows
# (R = 1024 at the default batch) DESIGN.md section 7d times - and NO_FINITE / NaN log-likelihoods on the device.
LARGEST_NESTED_ROWS_TESTED = 8192


def nested_variants(row):
    """The (L, K) combinations of a nested row."""
    Ls = row["L"] if isinstance(row["L"], tuple) else (row["L"],)
    Ks = row["K"] if isinstance(row["K"], tuple) else (row["K"],)
    assert len(Ls) == len(Ks)
    return [dict(row, L=L, K=K) for L, K in zip(Ls, Ks)]
