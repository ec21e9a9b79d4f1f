"""IntroTCSovler (sic): the Soft-Intro step with the beta-TC KL hook
(/root/reference/solvers/intro_tc.py:7-17) -- the configuration the headline metric is quoted on.
``kl_loss="full"`` trains with the full decomposition instead (solvers/tc.py:91-144)."""
from typing import Optional

from torch import Tensor

from solvers.intro import IntroSolver
from solvers.tc import KlLossMode, TCSovler


class IntroTCSovler(IntroSolver):
    kl_loss = KlLossMode()

    def __init__(self, *args, kl_loss: str = "simple", **kwargs):
        self.kl_loss = kl_loss
        super().__init__(*args, **kwargs)

    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        return TCSovler.compute_kl_loss(self, z, mu, logvar, reduce, beta, write)

    kl_decomposition = TCSovler.kl_decomposition
