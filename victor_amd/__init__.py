"""victor_amd - MI355X-native likelihood engine with victor's CCFModel / CCFFit interface.

The public names match the reference package (``victor/__init__.py:3-9``) for everything on the
likelihood path; evaluation runs in hand-written HIP kernels behind ``libvictor_hip.so``.
"""

from . import utils
from .ccf_fit import CCFFit
from .ccf_model import CCFModel
from .cosmology import BackgroundCosmology
from .fitting import BestFit
from .chains import Chains
from .joint import JointFit, JointRealisations
from .priors import GaussianPrior
from .laplace import Laplace
from .fisher import Fisher
from .grid import GridPosterior
from .importance import GaussianProposal, ImportancePosterior, ProposalSet
from .realisations import Realisations
from .cuts import CutRealisations, ScaleCut
from .utils import InputError

__version__ = "0.1.0"
__all__ = ["CCFModel", "CCFFit", "BackgroundCosmology", "BestFit", "Chains", "Fisher", "GaussianPrior", "GaussianProposal", "GridPosterior", "ImportancePosterior", "InputError", "JointFit", "JointRealisations", "Laplace", "ProposalSet", "Realisations", "CutRealisations", "ScaleCut", "utils", "__version__"]
