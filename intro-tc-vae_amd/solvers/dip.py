"""DIPSolver / IntroDIPSolver: the VAE and Soft-Intro steps with the DIP-VAE-I / DIP-VAE-II KL hook (Kumar et al. 2018;
disentanglement_lib's ``dip_vae`` with ``dip_type`` "i" / "ii").  The reference has no such solver: DIP is the
moment-matching counterpart of beta-TC, the baseline its disentanglement scores are usually compared against.

    m = mean_b mu_b,  C = sum_b (mu_b - m)(mu_b - m)^T / B   [+ diag(mean_b exp(logvar_b)) for "ii"]
    hook = beta * KL + lambda_od * sum_{i != j} C_ij^2 + lambda_d * sum_i (C_ii - 1)^2

in the fused launches of ``ops.dip_kl_loss`` (two forward, one backward)."""
from typing import Optional

from torch import Tensor

import ops
from hipvae import ddp
from solvers.hyper import Choice, Number
from solvers.intro import IntroSolver
from solvers.vae import VAESolver
from utils import SingletonWriter

DIP_TYPES = ("i", "ii")


class DipHook:
    """The DIP hyperparameters, KL hook and graph-key entries, mixed in front of ``VAESolver`` or ``IntroSolver``.
    ``lambda_d`` None follows the sweep convention of disentanglement_lib at every read: 10 * lambda_od for "i",
    lambda_od for "ii"."""
    dip_type = Choice(DIP_TYPES, "i")
    lambda_od = Number()
    lambda_d = Number(optional=True, fallback=lambda s: (10.0 if s.dip_type == "i" else 1.0) * s.lambda_od)

    def __init__(self, *args, dip_type: str = "i", lambda_od: float = 10.0, lambda_d: Optional[float] = None, **kwargs):
        self.dip_type = dip_type
        self.lambda_od = lambda_od
        self.lambda_d = lambda_d
        super().__init__(*args, **kwargs)

    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        """``reduce="mean"``: beta * KL + the DIP regulariser, fused.  The regulariser is a property of the batch and has
        no per-sample form: ``reduce="none"`` and ``reduce="sum"`` return exactly ``VAESolver.compute_kl_loss``, the
        plain beta * KL.  With ``write`` and a writer: ``kl_loss_unscaled`` and the record ``dip`` {offdiag, diag}.

        In a data-parallel run every rank evaluates the regulariser of the WHOLE global batch from the all-gathered
        (mu, logvar) pair (one packed collective), and the KL of its own rows.  The gather's reduce-scatter adjoint sums
        the world's copies of the regulariser's gradient, the gradient average of the step then divides by the world
        size: the result is the gradient of (global mean KL + regulariser), which is why no extra scaling appears."""
        if reduce != "mean":
            return VAESolver.compute_kl_loss(self, z, mu, logvar, reduce, beta, write)
        if beta is None:
            beta = self.beta_kl
        mu_all, logvar_all = ddp.all_gather_mu_logvar(mu, logvar)
        off = ddp.row_offset(mu.shape[0])
        args = (mu, logvar, beta, self.lambda_od, self.lambda_d, self.dip_type, mu_all, logvar_all, off)
        if not (write and self.writer):
            return ops.dip_kl_loss(*args)
        loss, terms = ops.dip_kl_loss(*args, with_terms=True)
        terms = terms.clone()
        ddp.mean_scalars_(terms)                # the KL is this rank's; the other two are equal on every rank
        kl, offdiag, diag = terms.tolist()
        sw = SingletonWriter()
        self.writer.add_scalar("kl_loss_unscaled", kl, global_step=sw.cur_iter)
        self.writer.add_scalars("dip", {"offdiag": offdiag, "diag": diag}, global_step=sw.cur_iter)
        return loss

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (self.dip_type, self.lambda_od, self.lambda_d)


class DIPSolver(DipHook, VAESolver):
    """The VAE step with the DIP hook."""


class IntroDIPSolver(DipHook, IntroSolver):
    """The Soft-Intro step with the DIP hook: every ``reduce="mean"`` call of the step (the real batch, and the decoder
    phase's reconstructions and fakes) carries the regulariser; the per-sample soft-exp terms (``reduce="none"``,
    ``beta_neg``) stay plain KL."""
