"""The shape table of tests/launch_shapes.py against the sources, without a GPU: every row still reaches what it was chosen
for at the thresholds as they stand in victor_hip.hip, vk_host.h, the kernel headers and chains.py, every row is a case of
tests/test_gpu_launch_shapes.py, and no shape exceeds what ``sample_chains`` accepts.  The same for ``STENCILS``, the shapes of the
two stencil calls (tests/test_gpu_stencil_shapes.py), and for the cases at the LDS ceiling of the Fisher assemble kernel, and for ``CHUNKS``, the
shapes of the chunked grid and importance pipeline (tests/test_gpu_chunk_shapes.py), whose tail geometry is stated by Python
twins of victor_amd/csrc/vk_is_tail.h that are held to the header under g++, and for ``NESTED``, the shapes of nested sampling
(tests/test_gpu_nested_shapes.py): K | L, K <= L / 2 and R K <= MAX_ROWS in every row.  A failure names the row to revisit."""

import numpy as np
import pytest

from tests import launch_shapes as LS
from tests.test_importance_tail import tail_driver  # noqa: F401  (a fixture: vk_is_tail.h under g++)


@pytest.fixture(scope="module")
def t():
    return LS.thresholds()


def test_the_thresholds_are_found_and_in_order(t):
    print(t)
    assert t["kChainBlock"] == 64 == t["BLOCK"], "one wave per workgroup and blocks of 64 steps: every shape of the table assumes both"
    assert 0 < t["cells_min"] < t["band1"] < t["band2"] <= t["kPartialPoints"]
    assert 0 < t["cpi0"] < t["cpi1"] < t["cpi2"]
    assert t["kFuseMaxDefault"] < t["kPartialPoints"] < t["kFuseBlendedMin"] <= LS.LARGEST_TESTED < t["MAX_CHAINS"]
    assert t["kZeroCopyMaxDefault"] < LS.LARGEST_TESTED


@pytest.mark.parametrize("case", sorted(LS.TABLE))
def test_a_row_reaches_what_it_is_about(t, case):
    row = LS.TABLE[case]
    for v in LS.variants(row):
        assert 0 < LS.chains(v) <= t["MAX_CHAINS"], (case, LS.chains(v))
        assert LS.chains(v) <= LS.LARGEST_TESTED, (case, "LARGEST_TESTED and the paragraph of DESIGN.md section 7b no longer say what is tested")
        assert LS.steps(v, t) == (2 * t["BLOCK"] + 2 if LS.chains(v) <= LS.MANY_CHAINS else t["BLOCK"] + 2)
        if v["move"] == "stretch":
            assert v["W"] % 2 == 0 and LS.rows(v) == v["R"] * (v["W"] // 2)
        for text, check in row["reaches"]:
            assert check(v, t), f"row {case} ({v['move']}, R = {v['R']}, W = {v['W']}) no longer reaches: {text} - revisit its shape"


def test_the_table_is_the_smallest_on_its_thresholds(t):
    """One below the shape, the property is gone: the sizes are the smallest that cross each threshold."""
    assert LS.cells_range(t["band1"] - 1, t) == t["cpi0"] and LS.cells_range(t["band1"], t) == t["cpi1"]
    assert LS.cells_range(t["band2"] - 1, t) == t["cpi1"] and LS.cells_range(t["band2"], t) == t["cpi2"]
    assert LS.cells_range(t["cells_min"] - 1, t) == 0 and LS.cells_range(t["cells_min"], t) == t["cpi0"]
    s1 = LS.TABLE["S1"]
    assert LS.rows(dict(s1, R=s1["R"] - 1)) <= t["kChainBlock"]                   # twelve ensembles of ten: 60 movers, one workgroup
    t1 = LS.TABLE["T1"]
    assert max(LS.swap_threads(dict(t1, W=t1["W"] - 1))) <= t["kChainBlock"]      # W = 10: 60 pairs at most


def test_every_row_is_a_gpu_case():
    """The GPU file's parametrisation is built from the table: every row, every variant."""
    import tests.test_gpu_launch_shapes as G
    ids = [i for ids in G.IDS.values() for i in ids]
    assert len(ids) == len(set(ids))
    for case, row in LS.TABLE.items():
        mine = [i for i in ids if i.split("-")[0] == case]
        assert len(mine) >= len(LS.variants(row)), (case, mine)
    assert {i.split("-")[0] for i in ids} == set(LS.TABLE)


# ------------------------------------------------------------------ the stencil calls ------------------------------------------------
def test_the_stencil_thresholds_are_found_and_in_order(t):
    assert t["kHessBlock"] == 64 == t["kFisherRowsBlock"], "one wave per workgroup of both rows kernels: every stencil row assumes it"
    assert t["kFisherMaxSeg"] <= t["kFisherBlock"] and t["kMaxP"] == 10
    assert 64 * 1024 < 8 * t["kFisherLdsDoubles"] <= 160 * 1024
    assert LS.slots(1) == LS.slots(3) == 4 and LS.slots(4) == 5 and LS.slots(10) == 11
    assert LS.points("laplace", 3) == 19 and LS.points("fisher", 3) == 7 and LS.points("laplace", 10) == 201 and LS.points("fisher", 10) == 21
    assert LS.chunks(dict(call="laplace", d=4, R=16)) == [80] * 6 + [48]          # (the shapes tests/test_gpu_hessian.py states)
    assert LS.chunks(dict(call="fisher", d=4, R=16)) == [80, 64] and LS.chunks(dict(call="fisher", d=1, R=70)) == [210]


@pytest.mark.parametrize("case", sorted(LS.STENCILS))
def test_a_stencil_row_reaches_what_it_is_about(t, case):
    row = LS.STENCILS[case]
    for v in LS.stencil_variants(row):
        lengths = LS.chunks(v)
        assert sum(lengths) == v["R"] * LS.points(v["call"], v["d"]) and max(lengths) == lengths[0] <= v["R"] * LS.slots(v["d"])
        assert max(lengths) <= LS.LARGEST_STENCIL_CHUNK, (case, "LARGEST_STENCIL_CHUNK and the paragraph of DESIGN.md section 7a no longer say what is tested")
        assert 1 <= v["d"] <= t["kMaxP"]
        for text, check in row["reaches"]:
            assert check(v, t), f"stencil row {case} ({v['call']}, {v['route']}, R = {v['R']}, d = {v['d']}) no longer reaches: {text} - revisit its shape"


@pytest.mark.parametrize("case", LS.SMALLEST)
def test_a_stencil_row_is_the_smallest_on_its_threshold(t, case):
    """One problem fewer, and the property is gone."""
    row = LS.STENCILS[case]
    v = max(LS.stencil_variants(row), key=lambda v: v["R"])
    assert row["smallest"](v, t), f"stencil row {case} at R = {v['R']} no longer has the property it is the smallest for - revisit its shape"
    assert not row["smallest"](dict(v, R=v["R"] - 1), t), f"stencil row {case}: R = {v['R'] - 1} has the property too - revisit its shape"


def test_the_lds_ceiling_cases_sit_on_the_limit(t):
    """The accepted case is the largest N d in whole BOSS blocks at d = 10, the refused one the next, and d = 9 fits again."""
    c = LS.CEILING
    def doubles(k):
        return LS.fisher_lds_doubles(c[k]["blocks"] * LS.BOSS_N, c[k]["d"], t)
    assert doubles("accepted") <= t["kFisherLdsDoubles"] < doubles("refused"), "the LDS ceiling moved: revisit CEILING"
    assert doubles("below") <= t["kFisherLdsDoubles"]
    assert c["refused"]["blocks"] == c["accepted"]["blocks"] + 1 == c["below"]["blocks"] and c["refused"]["blocks"] <= t["kFisherMaxSeg"]
    assert 8 * doubles("accepted") > 150 * 1024 and c["accepted"]["blocks"] > 5


def test_every_stencil_row_is_a_gpu_case():
    """The GPU file's parametrisation is built from the table: every row, every variant."""
    import tests.test_gpu_stencil_shapes as G
    ids = [i for ids in G.IDS.values() for i in ids]
    assert len(ids) == len(set(ids))
    for case, row in LS.STENCILS.items():
        mine = [i for i in ids if i.split("-")[0] == case]
        assert len(mine) == len(LS.stencil_variants(row)), (case, mine)
    assert {i.split("-")[0] for i in ids} == set(LS.STENCILS)


# ------------------------------------------------------------------ the chunked pipeline: grid and importance posteriors ------------
def test_the_chunk_thresholds_are_found_and_in_order(t):
    assert t["kIsBlock"] == t["kGridBlock"] == t["tail.kBlock"] == 256, "workgroups of 256 threads: every row of CHUNKS assumes it"
    assert t["kMaxSlices"] <= t["tail.kBlock"] and t["kBatch"] % t["tail.kBlock"] == 0 and t["kBatch"] < t["kMaxK"]
    assert t["predict.kWave"] == 64 and t["predict.kSlices"] * t["predict.kWave"] == 256
    assert 0 < t["kIsListAhead"] < t["kIsAhead"] < t["kGridAhead"] and t["predict.kAhead"] > 1 and t["predict.kTile"] > 0
    assert max(max(LS.chunk_lengths(r)) for r in LS.CHUNKS.values()) == LS.LARGEST_CHUNK_TESTED < t["MAX_CHUNK"], \
        "LARGEST_CHUNK_TESTED and the paragraphs of DESIGN.md sections 7c and 7e no longer say what is tested"
    assert LS.problems_of_a_workgroup(1) == 1 and LS.problems_of_a_workgroup(3) == 4 and LS.problems_of_a_workgroup(70) == 64
    # the chunk sizes the GPU suite ran before CHUNKS: one block of rows, one batch, whatever R
    for n in (7, 20, 23, 40, 48, 60, 64):
        for R in (1, 3, 16, 70):
            assert LS.tail_shape(n, R, t)[1] == 1 and len(LS.batches(n, t)) == 1


@pytest.mark.parametrize("case", sorted(LS.CHUNKS))
def test_a_chunk_row_reaches_what_it_is_about(t, case):
    row = LS.CHUNKS[case]
    lengths = LS.chunk_lengths(row)
    assert sum(lengths) == row["G"] and max(lengths) == lengths[0] == row["chunk"] <= t["MAX_CHUNK"] and 0 < lengths[-1] < row["chunk"]
    assert row["kind"] in ("importance", "grid") and 1 <= row["R"]
    if row["kind"] == "grid":
        assert np.prod(row["bins"]) == row["G"]
    else:
        for size in row["tail"]:
            assert 2 <= LS.tail_entries(row, size) <= min(row["G"], t["kMaxK"]), (case, size)
    for text, check in row["reaches"]:
        assert check(row, t), f"chunk row {case} (R = {row['R']}, chunk {row['chunk']}, G = {row['G']}) no longer reaches: {text} - revisit its shape"


@pytest.mark.parametrize("case", sorted(k for k, r in LS.CHUNKS.items() if r["kind"] == "importance"))
def test_the_tail_twins_are_the_header(t, tail_driver, case):
    """``problems_per_block``, ``slices_per_block``, ``row_blocks``, ``block_begin``, ``slice_of`` and ``rows_of`` of
    tests/launch_shapes.py against victor_amd/csrc/vk_is_tail.h under g++, at every (n, R) of the row."""
    row = LS.CHUNKS[case]
    for n in sorted(set(LS.chunk_lengths(row))):
        (pr, per, gy, S), cuts, slices = tail_driver.geometry(n, row["R"])
        assert (pr, per) == (LS.problems_per_block(row["R"]), LS.slices_per_block(pr, t)), (case, n)
        assert (pr, gy, S) == LS.tail_shape(n, row["R"], t) and gy == LS.row_blocks(n, pr, t), (case, n)
        assert list(cuts) == [LS.block_begin(n, gy, y) for y in range(gy + 1)], (case, n)
        assert len(slices) == S <= t["kMaxSlices"]
        seen = np.zeros(n, dtype=int)
        for s, (first, end, step, rows) in enumerate(slices):
            mine = LS.slice_of(n, pr, gy, s, t)
            assert (first, end, step) == mine and rows == LS.rows_of(mine), (case, n, s)
            seen[first:end:step] += 1
        assert np.all(seen == 1), (case, n)                          # every row in exactly one slice


# ------------------------------------------------------------------ nested sampling -------------------------------------------------
def test_the_nested_thresholds_are_found_and_in_order(t):
    assert t["kNestedBlock"] == 64, "one wave per workgroup of the per-walker kernels: every row of NESTED assumes it"
    assert t["kNestedSelect"] == 256 and t["kNestedSelect"] % 64 == 0 and t["kMaxLive"] % t["kNestedSelect"] == 0
    assert t["kMaxLive"] == t["MAX_LIVE"] and t["nested.BLOCK"] == 8
    assert (8 + 4 + 2) * t["kMaxLive"] <= 64 * 1024, "s_lnl, s_surv and s_dead at kMaxLive entries no longer fit 64 KiB of LDS"
    assert max(LS.nested_rows(v) for r in LS.NESTED.values() for v in LS.nested_variants(r)) == LS.LARGEST_NESTED_ROWS_TESTED < t["MAX_ROWS"], \
        "LARGEST_NESTED_ROWS_TESTED and the paragraph of DESIGN.md section 7d no longer say what is tested"
    assert LS.select_trips(1, t) == 1 and LS.select_trips(t["kNestedSelect"], t) == 1 and LS.select_trips(t["kNestedSelect"] + 1, t) == 2
    # the shapes tests/test_gpu_nested.py runs: every loop of the select kernel in one trip, every problem with R > 1 inside one
    # workgroup of the per-walker kernels
    for R, L, K in ((3, 8, 2), (1, 8, 2), (1, 160, 80), (70, 4, 2), (3, 4, 1)):
        row = dict(R=R, L=L, K=K)
        assert LS.select_trips(L, t) == LS.select_trips(K, t) == 1 and (R == 1 or LS.split_problems(row, t) == 0), (R, L, K)


@pytest.mark.parametrize("case", sorted(LS.NESTED))
def test_a_nested_row_reaches_what_it_is_about(t, case):
    row = LS.NESTED[case]
    assert {"route", "R", "L", "K", "S", "n_iter", "seed", "reaches"} <= set(row)
    for v in LS.nested_variants(row):
        R, L, K = v["R"], v["L"], v["K"]
        assert L % K == 0 and 1 <= K <= L // 2 and 2 <= L <= t["MAX_LIVE"], (case, L, K)
        assert 1 <= LS.nested_rows(v) <= t["MAX_ROWS"] and LS.nested_rows(v) <= LS.LARGEST_NESTED_ROWS_TESTED, (case, LS.nested_rows(v))
        assert LS.passes(v) * K == L and v["S"] >= 1 and v["n_iter"] >= 1
        for text, check in row["reaches"]:
            assert check(v, t), f"nested row {case} ({v['route']}, R = {R}, L = {L}, K = {K}) no longer reaches: {text} - revisit its shape"


def test_the_nested_table_is_the_smallest_on_its_thresholds(t):
    """One below the shape, the property is gone."""
    n2, n5 = LS.NESTED["N2"], LS.NESTED["N5"]
    assert LS.select_trips(n2["L"] - 2, t) == 1 and LS.walker_groups(dict(n2, K=n2["K"] - 1), t) == 2
    assert LS.cells_range(LS.nested_rows(dict(n5, K=n5["K"] - 1)), t) == t["cpi2"]
    assert LS.split_problems(dict(LS.NESTED["N9"], R=2), t) == 0


def test_every_nested_row_is_a_gpu_case():
    """The GPU file's parametrisation is built from the table: every row, every variant."""
    import tests.test_gpu_nested_shapes as G
    ids = G.IDS["test_a_row"]
    assert len(ids) == len(set(ids)) and {i.split("-")[0] for i in ids} == set(LS.NESTED)
    for case, row in LS.NESTED.items():
        assert [i for i in ids if i.split("-")[0] == case] == [f"{case}-{v['L']}x{v['K']}" for v in LS.nested_variants(row)], case


def test_every_chunk_row_is_a_gpu_case():
    """The GPU file's parametrisation is built from the table: every row, every tail size, every predictive row."""
    import tests.test_gpu_chunk_shapes as G
    ids = [i for ids in G.IDS.values() for i in ids]
    assert {i.split("-")[0] for i in ids} == set(LS.CHUNKS)
    for case, row in LS.CHUNKS.items():
        mine = {name: [i for i in ids_ if i.split("-")[0] == case] for name, ids_ in G.IDS.items()}
        if row["kind"] == "grid":
            assert mine["test_grid"] == [f"{case}-grid"], (case, mine)
            continue
        assert mine["test_importance"] == [f"{case}-plain"], (case, mine)
        assert mine["test_tail"][:len(row["tail"])] == [f"{case}-{size}" for size in row["tail"]], (case, mine)
        assert (mine["test_predictive"] == [f"{case}-predictive"]) == row["predictive"], (case, mine)
