"""VampSolver: the VAE step with a VampPrior (Tomczak & Welling 2018, "VAE with a VampPrior").  The reference has no such
solver.  Where ``aggregate_decomp`` states the mismatch between the aggregate posterior q(z) and N(0, I), and
``hipvae.density`` fits a mixture to q(z) after training, this objective learns the prior with the model:

    p(z) = (1 / K) sum_k q(z | u_k)          u_1..u_K: K learned pseudo-inputs pushed through the model's own encoder

    mu, logvar     = encode(real)
    p_mu, p_logvar = encode(pseudo_inputs())         a SECOND encode: BatchNorm sees the two batches in that order
    z, kl          = ops.vamp_latent(mu, logvar, p_mu, p_logvar, beta=beta_kl)     one sample per image, as in the paper
    loss           = scale * (beta_rec * mean rec(real, decode(z)) + kl),   kl = beta_kl * mean_b (log q(z_b | x_b) - log p(z_b))

The pseudo-inputs are a third flat parameter group ("prior") next to the encoder's and the decoder's.  ONE backward walks
decoder, encoder and prior together: the gradient of the pseudo-inputs arrives through the data gradient of the encoder's
stem convolution and is accumulated by autograd into the group's flat gradient buffer; the same zero / average /
fused-update path then serves all three, inside the captured step.

``optimizer_prior``: ``torch.optim.Adam(pseudo_inputs.parameters(), ...)``.  An optimiser without a fused update falls back
to ``optimizer_prior.step()`` and the step to eager execution, as for the other two.  ``clip`` bounds the norm of the
encoder's and decoder's gradients only, as for FactorVAE's discriminator.

Under data parallel nothing is added: every rank encodes all K pseudo-inputs and applies the term to its OWN rows; the
average of the gradients over the ranks is then the gradient of the global batch's mean, for the pseudo-inputs too.
(BatchNorm's statistics of the second encode are per rank, or synchronised, exactly as the first's.)

``train_step`` also returns ``log_q`` and ``log_p`` (the batch means of log q(z | x) and log p(z)); with a writer the record
``vamp`` {kl, log_q, log_p} is logged and the written images decode samples of the learned prior, not of N(0, I).
"sample_quality" and "latent_density" use the model's own prior when their params name none.

Out of scope: a Soft-Intro variant; the prior inside ``compute_log_likelihood`` / ``iwae_bound`` ("log_likelihood" in
``extra_scores`` raises ``NotImplementedError``: that kernel has log N(0, I) inside); combination with the TC / DIP / MMD
hooks (``compute_kl_loss`` is not called by this step); learned mixture weights; a hierarchical (two-layer) VampPrior; more
than one sample per image."""
import torch
from torch import Tensor

import ops
from hipvae import functional as HF
from hipvae.flat import fused_update
from solvers.vae import VAESolver


class VampSolver(VAESolver):
    """``train_step(batch, cur_iter)`` returns the ``VAESolver`` dict plus ``"log_q"`` and ``"log_p"``."""
    _updates = ("encoder", "decoder", "prior")
    _walk = ("decoder", "encoder", "prior")

    def __init__(self, *args, pseudo_inputs, optimizer_prior, **kwargs):
        self.pseudo_inputs = pseudo_inputs
        self.optimizer_prior = optimizer_prior
        super().__init__(*args, **kwargs)
        enc = self.model.encoder
        geom = (getattr(pseudo_inputs, "cdim", None), getattr(pseudo_inputs, "image_size", None))
        if geom != (self.model.cdim, enc.image_size):
            raise ValueError(f"pseudo_inputs are (cdim, image_size) = {geom}, the encoder takes "
                             f"{(self.model.cdim, enc.image_size)}")
        HF.vamp_check_shapes(int(self.batch_size), int(pseudo_inputs.num), int(self.model.zdim), "VampSolver")

    # ---- the third parameter group ----------------------------------------------------------------------------------
    def _module(self, part):
        return self.pseudo_inputs if part == "prior" else super()._module(part)

    def _optimizer(self, part):
        return self.optimizer_prior if part == "prior" else super()._optimizer(part)

    def _graph_ok(self, specs=None):
        return super()._graph_ok(specs) and fused_update(self.optimizer_prior) is not None

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (fused_update(self.optimizer_prior),)

    # ---- the step ----------------------------------------------------------------------------------------------------
    def _losses(self, real: Tensor):
        mu, logvar = self.model.encode(real)
        p_mu, p_logvar = self.model.encode(self.pseudo_inputs())
        z, loss_kl, terms = ops.vamp_latent(mu, logvar, p_mu, p_logvar, beta=self.beta_kl, with_terms=True)
        loss_rec = self.compute_rec_loss(real, self.model.decode(z), reduction="mean", write=True)
        return z, loss_rec, loss_kl, terms

    def _write_losses(self, cur_iter, v_kl, v_rec, v_klu, v_logq, v_logp):
        self.writer.add_scalar("kl_loss_unscaled", v_klu, global_step=cur_iter)
        super()._write_losses(cur_iter, v_kl, v_rec)
        self.writer.add_scalars("vamp", dict(kl=v_klu, log_q=v_logq, log_p=v_logp), global_step=cur_iter)

    def _extra_results(self, v_klu, v_logq, v_logp) -> dict:
        return {"log_q": v_logq, "log_p": v_logp}

    # ---- scores and images: the model's own prior ----------------------------------------------------------------------
    def _eval_prior(self):
        from hipvae import density
        return density.vamp_prior(self.model, self.pseudo_inputs, self.batch_size)

    def _write_images_helper(self, batch, cur_iter):
        if self.writer is not None and cur_iter % self.test_iter == 0:
            from hipvae import density
            z = density.vamp_sample(self._eval_prior(), batch.size(0), seed=cur_iter)
            with torch.no_grad():
                fake = self.model.sample(z)
            self.write_images(batch, fake, cur_iter)

    def write_disentanglemnt_scores(self, cur_iter: int, num_samples: int = 10000):
        if "log_likelihood" in tuple(self.extra_scores or ()):
            raise NotImplementedError('extra_scores: "log_likelihood" estimates log p(x) under N(0, I) (the prior is inside '
                                      "the iwae_bound kernel); a VampPrior there is out of scope")
        return super().write_disentanglemnt_scores(cur_iter, num_samples)
