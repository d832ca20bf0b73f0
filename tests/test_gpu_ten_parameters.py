"""The chain loops at d = kMaxP = 10 on the GPU (``vk_chain_step_kernel``, the stretch kernels, the histograms' pair list, the
prior's packed triangle): ``kMaxP = 10``, ``kMaxTri = 55`` and ``kMaxPairs = 45`` size the kernels'
by-value arguments and the per-chain state, and an off-by-one in any of them shows only when they are full.

The five density-split blocks under the joint covariance with fsigma8 and sigma_v of every block sampled (the ten names of
tests/test_gpu_hessian.py's ``test_ten_per_block_parameters``), beta and epsilon fixed - so both routes launch the same rows - under
a 10 x 10 correlated Gaussian prior whose precision matrix has no zero (all 55 triangle entries are read), with the histograms
of all 45 pairs and the autocorrelation series: the device route against ``device=False`` byte for byte.
"""

import faulthandler

import numpy as np
import pytest

from tests import cases
from tests.test_chains import assert_sums, same_bytes
from tests.test_gpu_chains import same_series
from tests.test_gpu_priors import BETA, Five, resolved, same_run
from tests.test_marginals import same_marginals

pytestmark = pytest.mark.gpu
PARAMS = cases.cobaya_info()["params"]
TEN = [f"fsigma8@{q}" for q in range(5)] + [f"sigma_v@{q}" for q in range(5)]
FIXED = {"beta": BETA, "epsilon": 1.0}
OPTIONS = dict(marginals={"bins": 16, "pairs": "all", "bins2d": 8}, autocorr={"max_lag": 16}, burn=5, thin=2, seed=2)


@pytest.fixture(autouse=True)
def time_limit():
    """Every test of this file under its own time limit: tracebacks and exit instead of a hang."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    return Five(tmp_path_factory.mktemp("five_cov"), True)


def block():
    from victor_amd.joint import per_block
    return per_block(PARAMS, ["fsigma8", "sigma_v"], 5)


def full_prior():
    """Means inside the box, widths of 0.05 and 25 km/s, correlations between 0.30 and 0.34 everywhere: positive definite
    (an equicorrelation of 0.3 has smallest eigenvalue 0.7, the perturbation's norm is below 0.2) with a dense inverse."""
    from victor_amd import GaussianPrior
    mean = [0.45 + 0.01 * q for q in range(5)] + [350.0 + 10.0 * q for q in range(5)]
    sigma = np.array([0.05] * 5 + [25.0] * 5)
    i, j = np.indices((10, 10))
    corr = np.where(i == j, 1.0, 0.30 + 0.02 * ((i + j) % 3))
    return GaussianPrior(TEN, mean, cov=corr * sigma[:, None] * sigma[None, :])


def compare(dev, ref, what, R, W, n_kept):
    assert dev.names == TEN and dev.chain.shape == (n_kept, R, W, 10)
    print(what, "acceptance of the definition route:", ref.acceptance)
    assert 0.02 < ref.acceptance.mean() < 0.98                   # a condition on the inputs
    same_run(dev, ref, what)
    r = resolved(full_prior(), TEN)
    assert np.all(r.pp != 0.0) and len(r.pp) == 55
    assert same_bytes(dev.lnprior_chain, r.lnprior(dev.chain)) and np.all(dev.lnprior_chain < 0.0)
    same_marginals(dev.marginals, ref.marginals, what)
    assert len(dev.marginals.counts2d) == 45 and dev.marginals.n.tolist() == [n_kept * W] * R
    assert all(np.all(h.sum(axis=(1, 2)) <= n_kept * W) and h.sum() > 0 for h in dev.marginals.counts2d.values())
    same_series(dev, ref, what)
    assert dev.autocorr.n == n_kept
    for m in range(R):                                           # (the sums hold products the device may contract: a bound)
        assert_sums(dev.sum1[m], dev.sum2[m], dev.chain[:, m], dev.pivot[m], f"{what}: device sums, mock {m}")
        assert np.all(dev.sum2[m] == np.swapaxes(dev.sum2[m], 1, 2))


def test_metropolis_chains_of_ten_parameters(five):
    """3 mocks x 4 chains, 70 steps across the block of 64, kept steps 5, 7, .. 69."""
    jr = five.joint.realisations([0, 1, 2])
    kw = dict(OPTIONS, walkers=4, fixed=FIXED, prior=full_prior())
    ref = jr.sample_chains(block(), 70, device=False, **kw)
    dev = jr.sample_chains(block(), 70, **kw)
    compare(dev, ref, "metropolis, d = 10", 3, 4, 33)


def test_stretch_ensembles_of_ten_parameters(five):
    """2 mocks x 22 walkers, the fewest the move takes at d = 10 (2 (d + 1)): half-launches of 22 rows."""
    jr = five.joint.realisations([0, 1])
    kw = dict(OPTIONS, walkers=22, fixed=FIXED, prior=full_prior(), move="stretch")
    ref = jr.sample_chains(block(), 20, device=False, **kw)
    dev = jr.sample_chains(block(), 20, **kw)
    compare(dev, ref, "stretch, d = 10", 2, 22, 8)
