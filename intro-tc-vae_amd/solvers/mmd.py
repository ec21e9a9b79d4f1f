"""MMDSolver / IntroMMDSolver: the VAE and Soft-Intro steps with the InfoVAE / MMD-VAE KL hook (Zhao, Song and Ermon 2017;
the penalty of WAE-MMD, Tolstikhin et al. 2018).  The reference has no such solver: where beta-TC and DIP regularise the
moments or densities of the encoder's Gaussians, this family matches the SAMPLES of the aggregate posterior to draws from
the prior with a kernel two-sample statistic.

    MMD^2 = sum_{i != j} k(z_i, z_j) / (B (B - 1)) + sum_{i != j} k(p_i, p_j) / (B (B - 1)) - 2 sum_{i, j} k(z_i, p_j) / B^2
    hook  = beta * KL + lambda_mmd * MMD^2(z, prior),   prior = ops.noise(z.shape)  (one more N(0, I) draw per call)

in the fused launches of ``ops.mmd_kl_loss`` (two forward, one backward); ``mmd_kernel`` is "imq" (WAE's multi-scale
inverse multiquadric) or "rbf", ``mmd_bandwidth`` the bandwidth h (None: 2 * zdim).

InfoVAE's objective  rec + (1 - alpha) KL + (alpha + lambda - 1) MMD^2  maps to ``beta_kl = 1 - alpha`` and
``lambda_mmd = alpha + lambda - 1``; MMD-VAE (alpha = 1) is ``beta_kl = 0``, ``lambda_mmd = lambda``."""
from typing import Optional

import torch
from torch import Tensor

import ops
from hipvae import ddp
from solvers.hyper import Choice, Number
from solvers.intro import IntroSolver
from solvers.vae import VAESolver
from utils import SingletonWriter

MMD_KERNELS = ("imq", "rbf")


class MmdHook:
    """The MMD hyperparameters, KL hook and graph-key entries, mixed in front of ``VAESolver`` or ``IntroSolver``.
    ``mmd_bandwidth`` None: 2 * D at every call."""
    lambda_mmd = Number()
    mmd_kernel = Choice(MMD_KERNELS, "imq")
    mmd_bandwidth = Number(positive=True, optional=True)

    def __init__(self, *args, lambda_mmd: float = 10.0, mmd_kernel: str = "imq", mmd_bandwidth: Optional[float] = None,
                 **kwargs):
        self.lambda_mmd = lambda_mmd
        self.mmd_kernel = mmd_kernel
        self.mmd_bandwidth = mmd_bandwidth
        super().__init__(*args, **kwargs)

    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        """``reduce="mean"``: beta * KL + lambda_mmd * MMD^2(z, prior), fused; ``prior = ops.noise(z.shape, z.device)``
        comes from the project's noise source, so recorded draws and graph capture work as for ``reparameterize``.  The
        statistic is a property of the batch and has no per-sample form: ``reduce="none"`` and ``reduce="sum"`` return
        exactly ``VAESolver.compute_kl_loss``, the plain beta * KL, and draw nothing.  With ``write`` and a writer:
        ``kl_loss_unscaled`` and the record ``mmd`` {mmd2, k_zz, k_pp, k_zp}.

        In a data-parallel run every rank evaluates the statistic of the WHOLE global batch (``ddp.all_gather_rows`` of
        its samples) against ONE global prior (the ranks' draws, gathered without gradient), and the KL of its own rows.
        The gather's reduce-scatter adjoint sums the world's copies of the statistic's gradient, the gradient average of
        the step then divides by the world size: the result is the gradient of (global mean KL + statistic), which is
        why no extra scaling appears."""
        if reduce != "mean":
            return VAESolver.compute_kl_loss(self, z, mu, logvar, reduce, beta, write)
        if z is None:
            raise ValueError("the MMD hook needs the sampled latents z (got None)")
        if beta is None:
            beta = self.beta_kl
        prior = ops.noise(z.shape, z.device)
        z_all = ddp.all_gather_rows(z)
        with torch.no_grad():
            prior_all = ddp.all_gather_rows(prior)
        args = (z, mu, logvar, prior, beta, self.lambda_mmd, self.mmd_kernel, self.mmd_bandwidth, z_all, prior_all)
        if not (write and self.writer):
            return ops.mmd_kl_loss(*args)
        loss, terms = ops.mmd_kl_loss(*args, with_terms=True)
        terms = terms.clone()
        ddp.mean_scalars_(terms)                # the KL is this rank's; the other four are equal on every rank
        kl, mmd2, k_zz, k_pp, k_zp = terms.tolist()
        sw = SingletonWriter()
        self.writer.add_scalar("kl_loss_unscaled", kl, global_step=sw.cur_iter)
        self.writer.add_scalars("mmd", {"mmd2": mmd2, "k_zz": k_zz, "k_pp": k_pp, "k_zp": k_zp}, global_step=sw.cur_iter)
        return loss

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (self.lambda_mmd, self.mmd_kernel, self.mmd_bandwidth)


class MMDSolver(MmdHook, VAESolver):
    """The VAE step with the MMD hook: two draws a step."""


class IntroMMDSolver(MmdHook, IntroSolver):
    """The Soft-Intro step with the MMD hook: every ``reduce="mean"`` call of the step (the real batch, and the decoder
    phase's reconstructions and fakes: three prior draws a step) carries the statistic; the per-sample soft-exp terms
    (``reduce="none"``, ``beta_neg``) stay plain KL."""
