"""AdaGVAESolver: the VAE step on PAIRS of images with the weakly-supervised latent op of Ada-GVAE / Ada-ML-VAE (Locatello
et al. 2020, "Weakly-Supervised Disentanglement Without Compromises"; disentanglement_lib's ``weak`` module,
``GroupVAEBase`` with ``aggregate_argmax``).  The reference has no such solver: every other objective here is
unsupervised, this one trains on pairs that differ in a few unknown factors (``hipvae.dataset.DevicePairLoader``).

A batch is ``[2B, C, H, W]``, rows ``b`` and ``B + b`` a pair.  The encoder runs ONCE over the 2B rows (BatchNorm sees 2B
rows, exactly as a ``VAESolver`` step at batch 2B); ``ops.ada_group`` decides per pair which latent dimensions are shared
(the per-dimension KL of one posterior from the other, thresholded half way between its smallest and largest value), replaces those dimensions' posteriors by their average (``averaging`` "gvae": of means and variances;
"mlvae": the product of the Gaussians), samples both latents and returns beta_kl * mean KL of the adapted posteriors;
the decoder and the reconstruction loss see the 2B rows:

    loss = scale * (beta_rec * mean_{2B} rec + beta_kl * mean_{2B} KL(adapted posterior || N(0, I)))

``own_mask`` (None, or a [B, D] device tensor, non-zero: the dimension keeps its own posterior) replaces the adaptive
threshold: GVAE (Hosoya) / ML-VAE (Bouchacourt et al.) with known groups.

Under data parallel nothing crosses ranks beyond what ``VAESolver`` does: the pairs of a rank stay on it.

Out of scope: the per-sample (``reduce="none"``) form of the KL of the adapted posteriors, and with it a Soft-Intro
variant (whose soft-exp terms are per sample); ``compute_kl_loss`` is not called by this step."""
from torch import Tensor

import ops
from solvers.hyper import Choice
from solvers.vae import VAESolver

ADA_AVERAGINGS = tuple(ops.ADA_AVERAGINGS)


class AdaGVAESolver(VAESolver):
    """``train_step(batch, cur_iter)``: ``batch`` [2B, C, H, W], rows b and B + b a pair.  Returns the ``VAESolver`` dict
    plus ``"shared_dims"``: the mean number of latent dimensions a pair shares."""
    averaging = Choice(ADA_AVERAGINGS, "gvae")

    def __init__(self, *args, averaging: str = "gvae", **kwargs):
        self.averaging = averaging
        self.own_mask = None
        super().__init__(*args, **kwargs)

    def _graph_key_extra(self) -> tuple:
        m = self.own_mask
        return super()._graph_key_extra() + (self.averaging, None if m is None else (m.data_ptr(), tuple(m.shape)))

    def _batch(self, batch: Tensor) -> Tensor:
        if batch.dim() != 4 or batch.size(0) < 2 or batch.size(0) % 2:
            raise ValueError(f"the batch is [2B, C, H, W], rows b and B + b a pair (got {tuple(batch.shape)})")
        return batch

    def _losses(self, real: Tensor):
        mu, logvar = self.model.encode(real)
        z, loss_kl, _, terms = ops.ada_group(mu, logvar, self.beta_kl, self.averaging, own=self.own_mask, with_terms=True)
        loss_rec = self.compute_rec_loss(real, self.model.decode(z), reduction="mean", write=True)
        return z, loss_rec, loss_kl, terms

    def _write_losses(self, cur_iter, v_kl, v_rec, v_klu, v_shared):
        self.writer.add_scalar("kl_loss_unscaled", v_klu, global_step=cur_iter)
        super()._write_losses(cur_iter, v_kl, v_rec)
        self.writer.add_scalars("ada", {"shared_dims": v_shared}, global_step=cur_iter)

    def _extra_results(self, v_klu, v_shared) -> dict:
        return {"shared_dims": v_shared}
