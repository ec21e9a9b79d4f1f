"""SWAESolver / IntroSWAESolver: the VAE and Soft-Intro steps with the sliced-Wasserstein KL hook (Kolouri et al. 2018,
"Sliced-Wasserstein Auto-Encoders").  The reference has no such solver.  It is the sibling of solvers/mmd.py in the family
that matches the SAMPLES of the aggregate posterior to draws from the prior: where MMD needs a kernel and a bandwidth and
its U-statistic may be negative, the sliced distance has neither choice, is a true metric, and costs O(L B log B).

    SW^2 = (1 / L) sum_l (1 / B) sum_i (sort(z theta_l)_i - sort(prior theta_l)_i)^2,   theta_l = t_l / |t_l|
    hook = beta * KL + lambda_sw * SW^2(z, prior),   prior = ops.noise(z.shape), t = ops.noise((L, D))

(two more N(0, I) draws per call, in that order) in the fused launches of ``ops.sw_kl_loss`` (two forward, one backward);
``num_projections`` is L.  The pure SWAE (no KL term) is ``beta_kl = 0``."""
from typing import Optional

import torch
from torch import Tensor

import ops
from hipvae import ddp
from solvers.hyper import Number
from solvers.intro import IntroSolver
from solvers.vae import VAESolver
from utils import SingletonWriter

MAX_PROJECTIONS = 4096


class _NumProjections:
    """An integer 1 <= L <= 4096, checked on every assignment; part of the graph key."""

    def __get__(self, obj, cls=None):
        return self if obj is None else obj.__dict__["_num_projections"]

    def __set__(self, obj, value):
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= MAX_PROJECTIONS:
            raise ValueError(f"num_projections must be an integer in 1..{MAX_PROJECTIONS} (got {value!r})")
        obj.__dict__["_num_projections"] = value


class SwHook:
    """The sliced-Wasserstein hyperparameters, KL hook and graph-key entries, mixed in front of ``VAESolver`` or
    ``IntroSolver``."""
    lambda_sw = Number()
    num_projections = _NumProjections()

    def __init__(self, *args, lambda_sw: float = 10.0, num_projections: int = 50, **kwargs):
        self.lambda_sw = lambda_sw
        self.num_projections = num_projections
        super().__init__(*args, **kwargs)

    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        """``reduce="mean"``: beta * KL + lambda_sw * SW^2(z, prior), fused; ``prior = ops.noise(z.shape, z.device)`` and
        then ``t = ops.noise((num_projections, D), z.device)`` come from the project's noise source, so recorded draws and
        graph capture work as for ``reparameterize``.  The distance is a property of the batch and has no per-sample
        form: ``reduce="none"`` and ``reduce="sum"`` return exactly ``VAESolver.compute_kl_loss``, the plain beta * KL,
        and draw nothing.  With ``write`` and a writer: ``kl_loss_unscaled`` and the record ``sw`` {sw2, sw2_max}.

        In a data-parallel run every rank evaluates the distance of the WHOLE global batch (``ddp.all_gather_rows`` of
        its samples) against ONE global prior (the ranks' draws, gathered without gradient) over ONE set of directions
        (rank 0's rows of the gathered draw), and the KL of its own rows.  The gather's reduce-scatter adjoint sums the
        world's copies of the distance's gradient, the gradient average of the step then divides by the world size: the
        result is the gradient of (global mean KL + distance), which is why no extra scaling appears."""
        if reduce != "mean":
            return VAESolver.compute_kl_loss(self, z, mu, logvar, reduce, beta, write)
        if z is None:
            raise ValueError("the sliced-Wasserstein hook needs the sampled latents z (got None)")
        if beta is None:
            beta = self.beta_kl
        L = self.num_projections
        prior = ops.noise(z.shape, z.device)
        t = ops.noise((L, z.shape[1]), z.device)
        z_all = ddp.all_gather_rows(z)
        with torch.no_grad():
            prior_all = ddp.all_gather_rows(prior)
            t = ddp.all_gather_rows(t)[:L]
        args = (z, mu, logvar, prior, t, beta, self.lambda_sw, z_all, prior_all)
        if not (write and self.writer):
            return ops.sw_kl_loss(*args)
        loss, terms = ops.sw_kl_loss(*args, with_terms=True)
        terms = terms.clone()
        ddp.mean_scalars_(terms)                # the KL is this rank's; the other two are equal on every rank
        kl, sw2, sw2_max = terms.tolist()
        sw = SingletonWriter()
        self.writer.add_scalar("kl_loss_unscaled", kl, global_step=sw.cur_iter)
        self.writer.add_scalars("sw", {"sw2": sw2, "sw2_max": sw2_max}, global_step=sw.cur_iter)
        return loss

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (self.lambda_sw, self.num_projections)


class SWAESolver(SwHook, VAESolver):
    """The VAE step with the sliced-Wasserstein hook: three draws a step."""


class IntroSWAESolver(SwHook, IntroSolver):
    """The Soft-Intro step with the sliced-Wasserstein hook: every ``reduce="mean"`` call of the step (the real batch, and
    the decoder phase's reconstructions and fakes: three prior draws and three direction draws a step) carries the
    distance; the per-sample soft-exp terms (``reduce="none"``, ``beta_neg``) stay plain KL."""
