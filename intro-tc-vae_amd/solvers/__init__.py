from .vae import VAESolver
from .intro import IntroSolver
from .tc import TCSovler
from .intro_tc import IntroTCSovler
from .dip import DIPSolver, IntroDIPSolver
from .mmd import MMDSolver, IntroMMDSolver
from .factor import FactorSolver
from .ada import AdaGVAESolver
from .joint import JointVAESolver, AnnealedVAESolver

__all__ = ["VAESolver", "IntroSolver", "TCSovler", "IntroTCSovler", "DIPSolver", "IntroDIPSolver", "MMDSolver",
           "IntroMMDSolver", "FactorSolver", "AdaGVAESolver", "JointVAESolver", "AnnealedVAESolver"]
