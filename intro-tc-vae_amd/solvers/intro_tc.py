"""IntroTCSovler (sic): the Soft-Intro step with the beta-TC KL hook
(/root/reference/solvers/intro_tc.py:7-17) -- the configuration the headline metric is quoted on.
``kl_loss="full"`` trains with the full decomposition instead (solvers/tc.py:91-144)."""
from solvers.intro import IntroSolver
from solvers.tc import TcHook


class IntroTCSovler(TcHook, IntroSolver):
    """The Soft-Intro step with the beta-TC hook."""
