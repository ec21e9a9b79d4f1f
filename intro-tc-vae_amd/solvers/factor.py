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
import math
import numbers
from typing import Optional

import torch
from torch import Tensor

import ops
from hipvae import ddp
from hipvae.flat import FlatGroup, fused_update
from solvers.vae import VAESolver


class FactorNumber:
    """``gamma`` (a finite number >= 0): checked on every assignment; a scalar kernel argument frozen into a captured
    step and therefore part of the graph's key."""

    def __init__(self, name):
        self.name = name

    def __get__(self, obj, cls=None):
        return self if obj is None else obj.__dict__.get("_" + self.name)

    def __set__(self, obj, value):
        if isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value) or value < 0:
            raise ValueError(f"{self.name} must be a finite number >= 0 (got {value!r})")
        obj.__dict__["_" + self.name] = float(value)


class FactorSolver(VAESolver):
    gamma = FactorNumber("gamma")

    def __init__(self, *args, discriminator, optimizer_disc, gamma: float = 10.0, **kwargs):
        self.gamma = gamma
        self.discriminator = discriminator
        self.optimizer_disc = optimizer_disc
        self._disc_pass = None
        super().__init__(*args, **kwargs)

    # ---- the third parameter group ----------------------------------------------------------------------------------
    def _params(self, part):
        if part != "discriminator":
            return super()._params(part)
        mod = self.discriminator
        ent = self.__dict__.setdefault("_plists", {}).get(part)
        if ent is None or ent[0] is not mod:
            ent = self._plists[part] = (mod, list(mod.parameters()))
        return ent[1]

    def _group(self, part) -> FlatGroup:
        if part != "discriminator":
            return super()._group(part)
        params = self._params(part)
        g = self._flat.get(part)
        if g is None or not g.owns(params):
            g = self._flat[part] = FlatGroup(params, inherit=g)
        return g

    def _step(self, part):
        if part != "discriminator":
            return super()._step(part)
        opt = self.optimizer_disc
        spec = fused_update(opt)
        if spec is None:
            opt.step()
        else:
            g = self._group(part)
            g.bind_optimizer(opt, spec)
            g.fused_step(spec)

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

    # ---- the step ----------------------------------------------------------------------------------------------------
    def _device_step(self, real: Tensor) -> Tensor:
        self._set_trainable(True, True)
        mu, logvar, z, rec = self.model(real)
        loss_rec = self.compute_rec_loss(real, rec, reduction="mean", write=True)
        loss_kl = self.compute_kl_loss(z, mu, logvar, write=True)
        loss = self._lincomb((self.scale, self.scale), loss_rec, loss_kl)
        dp, self._disc_pass = self._disc_pass, None
        self._backward(loss, ("decoder", "encoder"))
        d_loss = ops.factor_disc_loss(z, self.discriminator, shared=dp)
        self._backward(d_loss, ("discriminator",))
        norm = self._clip()
        self._step("encoder")
        self._step("decoder")
        self._step("discriminator")
        stats = torch.cat([torch.stack([loss.detach(), loss_kl.detach(), loss_rec.detach()]), dp.stats])
        ddp.mean_scalars_(stats)
        return torch.cat([stats, norm if norm is not None else stats.new_zeros(1)])

    def train_step(self, batch: Tensor, cur_iter: int) -> dict:
        if batch.dim() == 3:
            batch = batch.unsqueeze(0)
        real = batch.to(self.device)
        v_loss, v_kl, v_rec, v_tc, v_disc, v_acc, v_norm = self._run(real).tolist()     # the step's only host read-back
        if v_loss != v_loss:
            raise RuntimeError
        if self.writer:
            self.write_scalars(cur_iter, losses=dict(r_loss=v_rec, kl_loss=v_kl))
            self.writer.add_scalars("factor", dict(tc=v_tc, d_loss=v_disc, d_acc=v_acc), global_step=cur_iter)
            if self.clip:
                self.writer.add_scalar("total_norm", v_norm, global_step=cur_iter)
            self.write_gradient_norm(cur_iter)
            self._write_images_helper(real, cur_iter)
            self.write_disentanglemnt_scores(cur_iter)
            self.writer.flush()
        return {"loss_enc": v_loss, "loss_dec": v_loss, "loss_kl": v_kl, "loss_rec": v_rec,
                "L2": v_norm if self.clip else None, "loss_tc": v_tc, "loss_disc": v_disc, "disc_acc": v_acc}
