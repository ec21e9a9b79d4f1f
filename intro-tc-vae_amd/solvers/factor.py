"""FactorSolver: the VAE step with the FactorVAE objective (Kim & Mnih 2018; disentanglement_lib's ``factor_vae``).  The
reference has no such solver.  Where beta-TC-VAE estimates the total correlation of q(z) by minibatch-stratified
sampling, FactorVAE estimates the same quantity with the density-ratio trick, from a discriminator D that tells samples
of q(z) from samples of the product of its marginals (z with every dimension permuted over the batch on its own):

    z_perm[:, d] = z[argsort(keys[:, d]), d]     keys = ops.noise(z.shape): one more draw a step, after the
                                                 reparameterisation draw
    l = D(z), l' = D(z_perm)                     ONE forward of the MLP over the 2B stacked rows
    tc     = mean_i (l[i, 0] - l[i, 1])
    vae    = scale * (beta_rec * rec + beta_kl * KL + gamma * tc)       -> encoder and decoder
    d_loss = 0.5 mean_i CE(l[i], 0) + 0.5 mean_i CE(l'[i], 1)           -> D alone; z and z_perm are constants

Both updates of a step use D's weights from before the step and the same z.  The VAE walk runs the data-gradient chain
of the first B rows and leaves D's gradients alone; D's walk computes its weight and bias gradients from all 2B rows and
stops in front of the first layer's input.  D is a third flat parameter group ("discriminator") next to the encoder's and
the decoder's: the same zero / backward / average / fused-update path, inside the captured step.

``optimizer_disc``: the paper and the library train D with Adam, lr 1e-4, betas (0.5, 0.9):
``torch.optim.Adam(discriminator.parameters(), lr=1e-4, betas=(0.5, 0.9))``.  An optimiser without a fused update falls
back to ``optimizer_disc.step()`` and the step to eager execution, as for the other two.  ``clip`` bounds the norm of the
encoder's and decoder's gradients only: neither paper nor library clips D.

In a data-parallel run every rank permutes its OWN rows (the permutation never crosses ranks; the discriminator sees 2B
rows per rank) and D's gradients are averaged over the ranks like the others.

Not here: a Soft-Intro variant.  The intro step's shared decoder pass makes three mean-KL calls a step, and when D should
be updated among them needs a design of its own."""
from typing import Optional

from torch import Tensor

import ops
from hipvae.flat import fused_update
from solvers.hyper import Number
from solvers.vae import VAESolver


class FactorSolver(VAESolver):
    gamma = Number()
    _updates = ("encoder", "decoder", "discriminator")

    def __init__(self, *args, discriminator, optimizer_disc, gamma: float = 10.0, **kwargs):
        self.gamma = gamma
        self.discriminator = discriminator
        self.optimizer_disc = optimizer_disc
        self._disc_pass = None
        super().__init__(*args, **kwargs)

    # ---- the third parameter group ----------------------------------------------------------------------------------
    def _module(self, part):
        return self.discriminator if part == "discriminator" else super()._module(part)

    def _optimizer(self, part):
        return self.optimizer_disc if part == "discriminator" else super()._optimizer(part)

    def _graph_ok(self, specs=None):
        return super()._graph_ok(specs) and fused_update(self.optimizer_disc) is not None

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (self.gamma, fused_update(self.optimizer_disc))

    # ---- the hook ----------------------------------------------------------------------------------------------------
    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        """``reduce="mean"``: beta * KL + gamma * tc, tc from one forward of the discriminator over [z; permute_dims(z)]
        (``ops.factor_pass``; the keys of the permutation are one ``ops.noise`` draw).  The pass is kept for the
        discriminator's own walk of the same step.  The estimate is a property of the batch and has no per-sample form:
        ``reduce="none"`` and ``reduce="sum"`` return exactly ``VAESolver.compute_kl_loss``, the plain beta * KL, and
        draw nothing."""
        if reduce != "mean":
            return VAESolver.compute_kl_loss(self, z, mu, logvar, reduce, beta, write)
        if z is None:
            raise ValueError("the FactorVAE hook needs the sampled latents z (got None)")
        kl = VAESolver.compute_kl_loss(self, z, mu, logvar, reduce, beta, write)
        dp = self._disc_pass = ops.factor_pass(z, self.discriminator)
        if self.gamma == 0:
            return kl                     # the discriminator still trains; the VAE's loss and walk are the plain ones
        return self._lincomb((1.0, self.gamma), kl, ops.factor_tc(z, self.discriminator, shared=dp))

    # ---- the step: the plain forward, then D's own loss and walk from the pass the hook kept ------------------------------
    def _losses(self, real: Tensor):
        z, loss_rec, loss_kl, _ = super()._losses(real)
        return z, loss_rec, loss_kl, self._disc_pass.stats

    def _side_walk(self, z: Tensor):
        dp, self._disc_pass = self._disc_pass, None
        self._backward(ops.factor_disc_loss(z, self.discriminator, shared=dp), ("discriminator",))

    def _write_losses(self, cur_iter, v_kl, v_rec, v_tc, v_disc, v_acc):
        super()._write_losses(cur_iter, v_kl, v_rec)
        self.writer.add_scalars("factor", dict(tc=v_tc, d_loss=v_disc, d_acc=v_acc), global_step=cur_iter)

    def _extra_results(self, v_tc, v_disc, v_acc) -> dict:
        return {"loss_tc": v_tc, "loss_disc": v_disc, "disc_acc": v_acc}
