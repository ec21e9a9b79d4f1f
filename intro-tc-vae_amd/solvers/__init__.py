from .vae import VAESolver
from .intro import IntroSolver
from .mmd import MMDSolver, IntroMMDSolver
from .factor import FactorSolver
from .ada import AdaGVAESolver
from .joint import JointVAESolver, AnnealedVAESolver
