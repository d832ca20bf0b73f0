"""The streaming cells kernel takes the velocity nodes of a cell in blocks of four table entries with one shared reciprocal per block
(vk_kernel_cells.h: stream_cell): every block shape and every position of a weight group's end inside a block against the
point-major kernel, which takes the same nodes one at a time (uni_point, recip_nr); the bench's regime against small batches; and
bit-for-bit determinism."""

import numpy as np
import pytest

import victor_amd
from tests import cases
from tests.tolerances import assert_same_chi2, chi2_bound

pytestmark = pytest.mark.gpu

CELLS, POINT = "vk_theory_cells_kernel", "vk_theory_fast_kernel"
N_SMALL = 24            # >= 20 points: the cells kernel, every point's cells split into ranges
POINT_MAX = 19          # calls of at most 19 points take the point-major kernel


def _rule(name):
    """Weight rules by which every block shape occurs.  The table holds the nodes in groups of equal weight, first occurrence first,
    zero weights left out, and is cut into quads plus one triple, pair or single: what varies is where the groups end inside the
    blocks and what is left at the end of the table."""
    from victor_amd import tables as T
    real = T.simpson_weights
    if name in ("simpson", "avg"):                          # groups of 1, 23, 23, 1, 1, 1 / of 2, 2, 46: 12 quads and a pair
        return lambda n, even=None: real(n, name)
    if name == "equal":                                     # one group of 50: closed in the last block, a pair
        return lambda n, even=None: np.full(n, real(n, "simpson").sum() / n)
    if name in ("drop2", "drop3"):                          # 'simpson' without 2 / 3 of its nodes: 12 quads and nothing / 11 quads and a triple
        def dropped(n, even=None):
            w = real(n, "simpson").copy()
            w[[4, 31, 17][:int(name[-1])]] = 0.0
            return w
        return dropped
    if name == "distinct":                                  # 50 groups of one: every node of every block closes a group
        return lambda n, even=None: real(n, "simpson") * (1.0 + 0.01 * np.arange(n))

    def groups(n, even=None):                               # groups of 1, 2, ..., 9 and five zero weights: 45 nodes, 11 quads and a single
        assert n == 50
        w = np.zeros(n)
        ids = np.repeat(np.arange(1, 10), np.arange(1, 10))                      # group g has g members
        np.random.default_rng(5).shuffle(ids)                                    # ... scattered over the nodes
        w[np.setdiff1d(np.arange(n), [0, 7, 20, 21, n - 1])] = 0.5 + 0.1 * ids
        return w * (real(n, "simpson").sum() / w.sum())
    assert name == "groups"
    return groups


def _wide_rows(n, with_beta):
    """Halton points of the prior box with its corners among them - aperp, apar at 0.8 and 1.2, sigma_v at 100 and 500 - so that
    trips whose radii leave the table (`inside` false) occur beside those that stay inside."""
    hp = cases.halton_params(n, with_beta=with_beta)
    hp = {k: np.array(v, float) for k, v in hp.items()}
    corners = [(0.8, 0.8, 100.0), (1.2, 1.2, 500.0), (0.8, 1.2, 500.0), (1.2, 0.8, 100.0), (1.2, 1.2, 100.0), (0.8, 0.8, 500.0)]
    for r, (aperp, apar, sv) in enumerate(corners):
        hp["aperp"][3 * r], hp["apar"][3 * r], hp["sigma_v"][3 * r] = aperp, apar, sv
    return hp


def _take(hp, idx):
    return {k: v[idx] for k, v in hp.items()}


def _options(workload):
    return cases.synth_options(3) if workload == "config3" else cases.boss_options()


def _in_calls_of(fit, hp, n, size, kernel):
    lnl, chi2 = np.empty(n), np.empty(n)
    for lo in range(0, n, size):
        lo = min(lo, max(n - size, 0))              # the last call takes the last `size` rows: every call is a full one
        idx = np.arange(lo, min(lo + size, n))
        out = fit.log_likelihood_batch(_take(hp, idx))
        assert fit._get_engine().last_kernel() == kernel
        lnl[idx], chi2[idx] = out[0], out[1]
    return lnl, chi2


@pytest.mark.parametrize("workload", ["config3", "boss"])
@pytest.mark.parametrize("rule", ["simpson", "avg", "equal", "distinct", "groups", "drop2", "drop3"])
def test_blocks_of_nodes_against_the_one_node_loop(monkeypatch, workload, rule):
    """24 points on the cells kernel (split ranges) against the same points in calls of at most 19, which take the point-major
    kernel and the one-node uni_point: two mappings of the same arithmetic, 64 ulps (tests/tolerances.py).  The rules leave a
    pair ('simpson', 'avg', equal, distinct: 50 nodes), a single (groups: 45), nothing (drop2: 48) and a triple (drop3: 47) at the end
    of the table and put the ends of weight groups at every position of a block."""
    from victor_amd import tables as T
    monkeypatch.setattr(T, "simpson_weights", _rule(rule))
    fit = victor_amd.CCFFit(*_options(workload))
    hp = _wide_rows(N_SMALL, with_beta=workload == "boss")
    cells = fit.log_likelihood_batch(hp)
    eng = fit._get_engine()
    assert eng.last_kernel() == CELLS
    _, chi2_point = _in_calls_of(fit, hp, N_SMALL, POINT_MAX, POINT)
    assert np.all(np.isfinite(cells[1])) and np.all(np.isfinite(chi2_point))
    assert_same_chi2(cells[1], chi2_point, chi2_bound(fit, hp), what=f"node blocks, {workload}, rule {rule}: cells vs point-major")


def test_whole_point_workgroups_against_split_ranges():
    """2048 points (one workgroup per point, the bench's regime) against the same rows in batches of 24 (ranges of a point on
    several workgroups): the same arithmetic in another split, 64 ulps."""
    fit = victor_amd.CCFFit(*_options("config3"))
    n = 2048
    hp = _wide_rows(n, with_beta=False)
    big = fit.log_likelihood_batch(hp)
    assert fit._get_engine().last_kernel() == CELLS
    _, chi2_small = _in_calls_of(fit, hp, n, N_SMALL, CELLS)
    assert_same_chi2(big[1], chi2_small, chi2_bound(fit, hp), what="node blocks: 2048 points vs batches of 24")


@pytest.mark.parametrize("workload", ["config3", "boss"])
def test_node_blocks_are_deterministic_and_rows_independent(workload):
    """The blocks are a property of the context's table: the same batch twice gives the same bits, a row's bits do not depend on
    its position in the batch, and a row whose sigma_v is NaN - it poisons the reciprocals of ITS cells' blocks - fails alone."""
    fit = victor_amd.CCFFit(*_options(workload))
    hp = _wide_rows(N_SMALL, with_beta=workload == "boss")
    eng = fit._get_engine()
    first = fit.log_likelihood_batch(hp)
    assert eng.last_kernel() == CELLS
    again = fit.log_likelihood_batch(hp)
    for a, b in zip(first[:2], again[:2]):
        assert np.array_equal(a, b)
    perm = np.random.default_rng(11).permutation(N_SMALL)
    moved = fit.log_likelihood_batch(_take(hp, perm))
    assert eng.last_kernel() == CELLS
    for a, b in zip(first[:2], moved[:2]):
        assert np.array_equal(a[perm], b)
    bad = 5
    hp_nan = {k: v.copy() for k, v in hp.items()}
    hp_nan["sigma_v"][bad] = np.nan
    out = fit.log_likelihood_batch(hp_nan)
    assert eng.last_kernel() == CELLS
    others = np.arange(N_SMALL) != bad
    for a, b in zip(first[:2], out[:2]):
        assert np.array_equal(a[others], b[others])
    # the row itself fails as it always did: (-inf, +inf), the reference's answer to a non-finite likelihood (ccf_fit.py:477-481)
    assert out[0][bad] == -np.inf and out[1][bad] == np.inf
