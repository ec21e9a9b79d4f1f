"""IWAESolver: the VAE step on the K-sample importance-weighted bound (Burda, Grosse and Salakhutdinov 2016, "Importance
Weighted Autoencoders"), with the plain reparameterised gradient ("iwae"), the sticking-the-landing estimator ("stl",
Roeder et al. 2017) or the doubly reparameterised one ("dreg", Tucker et al. 2019) into the encoder.  The reference has
none of them.

The model is an unchanged ``SoftIntroVAE``.  A step encodes the B images once, draws ``num_samples`` = K latents per image
(``ops.iwae_sample``; row ``k B + b`` is sample k of image b, ONE recorded draw), decodes the K B rows in one pass -- so
BatchNorm sees K B rows -- and differentiates (``ops.iwae_bound``)

    loss = scale * -mean_b (logsumexp_k logw_kb - log K),    logw = -(beta_rec rec + beta_kl (log q(z|x) - log p(z)))

with ``rec`` the summed reconstruction error of the row against its image, which is read in place and never copied K times.
K = 1 with "iwae" is the beta-VAE step with a sampled KL in place of the analytic one.  "stl" and "dreg" change only the
gradient that reaches the encoder through ``(mu, logvar)``: the direct dependence of log q on them is dropped, and under
"dreg" the gradient that arrives at ``z_r`` is multiplied by ``w_r`` once more.  The decoder's BatchNorm (training mode)
couples the K B rows of a step; the weight goes with the row the gradient arrives at, which for a decoder that treats its rows
independently is the estimator of the paper.

This loss is not ``loss_rec + loss_kl``: ``train_step`` returns the ``VAESolver`` dict with ``loss_rec`` / ``loss_kl`` the
self-normalised weighted means ``beta mean_b sum_k w_kb term_kb`` (w the normalised importance weights; at K = 1 the two
terms of the loss), plus ``bound`` (mean_b of the bound, unscaled) and ``ess`` (mean effective sample size, 1..K).

Under data parallel nothing is added: the bound is a mean over images, so the rank average of the shard gradients is the
gradient of the global objective.  Out of scope: a Soft-Intro variant, combination with the other solvers' KL hooks,
multiple-importance or annealed sampling, a learned observation variance.  ``compute_kl_loss`` and ``compute_rec_loss``
are not called by this step."""
import torch
from torch import Tensor

import ops
from solvers.hyper import Choice
from solvers.vae import VAESolver

IWAE_ESTIMATORS = ops.IWAE_ESTIMATORS


class _NumSamples:
    """An integer 1 <= K <= 1024, checked on every assignment; part of the graph key."""

    def __get__(self, obj, cls=None):
        return self if obj is None else obj.__dict__["_num_samples"]

    def __set__(self, obj, value):
        if isinstance(value, bool) or not isinstance(value, int) or not 1 <= value <= 1024:
            raise ValueError(f"num_samples must be an integer in 1..1024 (got {value!r})")
        obj.__dict__["_num_samples"] = value


class IWAESolver(VAESolver):
    num_samples = _NumSamples()
    estimator = Choice(IWAE_ESTIMATORS, "iwae")

    def __init__(self, *args, num_samples: int = 8, estimator: str = "iwae", **kwargs):
        self.num_samples = num_samples                       # refused before anything is built
        self.estimator = estimator
        super().__init__(*args, **kwargs)

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (self.num_samples, self.estimator)

    def _losses(self, real: Tensor):
        mu, logvar = self.model.encode(real)
        sample = ops.iwae_sample(mu, logvar, self.num_samples)
        rec = self.model.decode(sample.z)
        self._bound_loss, terms = ops.iwae_bound(real, rec, sample, self.beta_rec, self.beta_kl, self.recon_loss_type,
                                                 self.estimator, with_terms=True)
        return sample.z, terms[0], terms[1], terms[2:]

    def _total_loss(self, loss_rec: Tensor, loss_kl: Tensor) -> Tensor:
        loss, self._bound_loss = self._bound_loss, None
        return self._lincomb((self.scale,), loss)

    def _write_losses(self, cur_iter, v_kl, v_rec, *terms):
        super()._write_losses(cur_iter, v_kl, v_rec)
        self.writer.add_scalars("iwae", self._extra_results(*terms), global_step=cur_iter)

    def _extra_results(self, v_bound, v_ess) -> dict:
        return dict(bound=v_bound, ess=v_ess)
