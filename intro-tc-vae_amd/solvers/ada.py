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
import torch
from torch import Tensor

import ops
from hipvae import ddp
from solvers.vae import VAESolver

ADA_AVERAGINGS = tuple(ops.ADA_AVERAGINGS)


class AdaAveraging:
    """The ``averaging`` attribute of the solver: "gvae" or "mlvae".  Checked on every assignment; part of the captured
    graph's key, so a change re-captures."""

    def __get__(self, obj, cls=None):
        return self if obj is None else obj.__dict__.get("_averaging", "gvae")

    def __set__(self, obj, value):
        if value not in ADA_AVERAGINGS:
            raise ValueError(f"averaging must be one of {ADA_AVERAGINGS} (got {value!r})")
        obj.__dict__["_averaging"] = value


class AdaGVAESolver(VAESolver):
    averaging = AdaAveraging()

    def __init__(self, *args, averaging: str = "gvae", **kwargs):
        self.averaging = averaging
        self.own_mask = None
        super().__init__(*args, **kwargs)

    def _graph_key_extra(self) -> tuple:
        m = self.own_mask
        return super()._graph_key_extra() + (self.averaging, None if m is None else (m.data_ptr(), tuple(m.shape)))

    def _device_step(self, real: Tensor) -> Tensor:
        self._set_trainable(True, True)
        mu, logvar = self.model.encode(real)
        z, loss_kl, _, terms = ops.ada_group(mu, logvar, self.beta_kl, self.averaging, own=self.own_mask, with_terms=True)
        rec = self.model.decode(z)
        loss_rec = self.compute_rec_loss(real, rec, reduction="mean", write=True)
        loss = self._lincomb((self.scale, self.scale), loss_rec, loss_kl)      # scale * (loss_rec + loss_kl)
        self._backward(loss, ("decoder", "encoder"))
        norm = self._clip()
        self._step("encoder")
        self._step("decoder")
        stats = torch.cat([torch.stack([loss.detach(), loss_kl.detach(), loss_rec.detach()]), terms])
        ddp.mean_scalars_(stats)
        return torch.cat([stats, norm if norm is not None else stats.new_zeros(1)])

    def train_step(self, batch: Tensor, cur_iter: int) -> dict:
        """``batch`` [2B, C, H, W], rows b and B + b a pair.  Returns the ``VAESolver`` dict plus ``"shared_dims"``: the
        mean number of latent dimensions a pair shares."""
        if batch.dim() != 4 or batch.size(0) < 2 or batch.size(0) % 2:
            raise ValueError(f"the batch is [2B, C, H, W], rows b and B + b a pair (got {tuple(batch.shape)})")
        real = batch.to(self.device)
        v_loss, v_kl, v_rec, v_klu, v_shared, v_norm = self._run(real).tolist()     # the step's only host read-back
        if v_loss != v_loss:
            raise RuntimeError
        if self.writer:
            self.writer.add_scalar("kl_loss_unscaled", v_klu, global_step=cur_iter)
            self.write_scalars(cur_iter, losses=dict(r_loss=v_rec, kl_loss=v_kl))
            self.writer.add_scalars("ada", {"shared_dims": v_shared}, global_step=cur_iter)
            if self.clip:
                self.writer.add_scalar("total_norm", v_norm, global_step=cur_iter)
            self.write_gradient_norm(cur_iter)
            self._write_images_helper(real, cur_iter)
            self.write_disentanglemnt_scores(cur_iter)
            self.writer.flush()
        return {"loss_enc": v_loss, "loss_dec": v_loss, "loss_kl": v_kl, "loss_rec": v_rec,
                "L2": v_norm if self.clip else None, "shared_dims": v_shared}
