from .vae import VAESolver
from .intro import IntroSolver
from .tc import TCSovler
from .intro_tc import IntroTCSovler
from .dip import DIPSolver, IntroDIPSolver
from .mmd import MMDSolver, IntroMMDSolver
from .factor import FactorSolver
from .ada import AdaGVAESolver
from .joint import JointVAESolver, AnnealedVAESolver
# the semi-supervised family takes (x, y) batches: imported by name (``from solvers import S2VAESolver``); ``__all__``
# stays the twelve solvers that train from images alone
from .semi import S2VAESolver, S2TCSolver, S2DIPSolver, S2FactorSolver
# the importance-weighted bound: imported by name too (``from solvers import IWAESolver``)
from .iwae import IWAESolver
# the learned mixture prior: imported by name too (``from solvers import VampSolver``)
from .vamp import VampSolver
# the sliced-Wasserstein autoencoder, the sibling of the MMD pair: imported by name too (``from solvers import SWAESolver``)
from .swae import SWAESolver, IntroSWAESolver

__all__ = ["VAESolver", "IntroSolver", "TCSovler", "IntroTCSovler", "DIPSolver", "IntroDIPSolver", "MMDSolver",
           "IntroMMDSolver", "FactorSolver", "AdaGVAESolver", "JointVAESolver", "AnnealedVAESolver"]
