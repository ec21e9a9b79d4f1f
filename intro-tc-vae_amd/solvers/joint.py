"""JointVAESolver and AnnealedVAESolver: the VAE step with a capacity-controlled latent op.  JointVAE (Dupont 2018,
"Learning Disentangled Joint Continuous and Discrete Representations") is the one member of the comparison with DISCRETE
latents; AnnealedVAE (Burgess et al. 2018, "Understanding disentangling in beta-VAE"; disentanglement_lib's
``annealed_vae``) is the same objective with no discrete variables.  The reference has neither.

The model is an unchanged ``SoftIntroVAE`` with ``zdim = cont + sum(disc)``: columns [0, cont) of the encoder's
(mu, logvar) are the continuous posterior, the remaining columns of mu the logits of ``len(disc)`` categorical variables
with ``disc[i]`` categories side by side (the same columns of logvar are unused and get a zero gradient), and the decoder
sees ``[z_cont | y_1 | .. | y_G]`` with Gumbel-softmax samples ``y_i`` at ``temperature``.  ``ops.joint_latent`` does all
of it between ``encode`` and ``decode``:

    loss = scale * (beta_rec * mean rec + beta_kl * (gamma_cont |KL_z - C_z(t)| + gamma_disc |KL_c - C_c(t)|))

The capacities follow Dupont's trainer and the library's ``annealed_vae``: with ``(C_min, C_max, iters, gamma)`` per block
and ``t`` the number of training steps this solver has taken, ``C(t) = min(C_max, C_min + (C_max - C_min) t / iters)``, the
discrete one capped at ``sum_i log K_i`` (a categorical variable cannot carry more) and an empty block's at 0.
``train_step`` writes (C_z, C_c) into a persistent [2] float64 device tensor BEFORE the step runs and outside the captured
region; the kernel reads it when it runs, so a captured step replays with the new capacity and is never re-captured for it.

Out of scope: a Soft-Intro variant (its soft-exp terms are per sample, this loss is a function of a batch mean);
the global-batch form under data parallel (each rank applies the capacity term to its own shard's mean KL: the global form
needs a collective between the two forward launches); temperature annealing.  ``compute_kl_loss`` is not called by this
step."""
import math

import torch
from torch import Tensor

import ops
from solvers.hyper import Number
from solvers.vae import VAESolver


def _capacity(value, what):
    """(C_min, C_max, iters, gamma) checked; returns ((C_min, C_max, iters), gamma)."""
    try:
        lo, hi, iters, gamma = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} is (C_min, C_max, iters, gamma) (got {value!r})") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo >= 0.0 and hi >= 0.0):
        raise ValueError(f"{what}: C_min and C_max must be finite and not negative (got {lo}, {hi})")
    if not (math.isfinite(iters) and iters > 0):
        raise ValueError(f"{what}: iters must be a positive number of steps (got {iters})")
    return (lo, hi, iters), gamma


class _LatentSpec:
    """``dict(cont=n, disc=(K_1, .., K_G))``, read back as the same dict with ``disc`` a tuple.  Checked on every
    assignment (ops.joint_spec; against the model's zdim once the solver has its model); part of the graph key."""

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        cont, disc = obj.__dict__["_latent_spec"]
        return dict(cont=cont, disc=disc)

    def __set__(self, obj, value):
        if not isinstance(value, dict) or set(value) - {"cont", "disc"} or not value:
            raise ValueError(f"latent_spec is dict(cont=n, disc=(K_1, ..)) (got {value!r})")
        model = obj.__dict__.get("model")
        cont, disc, _ = ops.joint_spec(value.get("cont", 0), value.get("disc", ()), None if model is None else model.zdim)
        obj.__dict__["_latent_spec"] = (cont, disc)


class JointVAESolver(VAESolver):
    latent_spec = _LatentSpec()
    temperature = Number(positive=True)          # of the Gumbel-softmax
    gamma_cont = Number()                        # the capacity weights
    gamma_disc = Number()

    def __init__(self, *args, latent_spec=None, cont_capacity=(0.0, 5.0, 25000, 30.0),
                 disc_capacity=(0.0, 5.0, 25000, 30.0), temperature: float = 0.67, **kwargs):
        self.temperature = temperature
        self.cont_capacity, self.gamma_cont = _capacity(cont_capacity, "cont_capacity")
        self.disc_capacity, self.gamma_disc = _capacity(disc_capacity, "disc_capacity")
        if latent_spec is not None:
            self.latent_spec = latent_spec                 # refused before anything is built
        super().__init__(*args, **kwargs)
        # the constructor's check of zdim == cont + sum(disc); no spec: every latent dimension continuous
        self.latent_spec = dict(cont=self.model.zdim, disc=()) if latent_spec is None else latent_spec
        self.steps_taken = 0                               # t of C(t): the training steps this solver has taken
        self._cap = torch.zeros(2, dtype=torch.float64, device=self.device)      # (C_z, C_c): what the kernel reads

    def capacity_at(self, t: int) -> tuple:
        """(C_z, C_c) after ``t`` training steps."""
        def ramp(c):
            lo, hi, iters = c
            return min(hi, lo + (hi - lo) * t / iters)

        cont, disc = self._latent_spec
        return (ramp(self.cont_capacity) if cont else 0.0,
                min(ramp(self.disc_capacity), sum(math.log(k) for k in disc)))

    def _graph_key_extra(self) -> tuple:
        return super()._graph_key_extra() + (self._latent_spec, self.temperature, self.gamma_cont, self.gamma_disc,
                                             self._cap.data_ptr())

    def _run(self, real: Tensor) -> Tensor:
        # outside the captured region: a replay reads what is written here
        self._cap.copy_(torch.tensor(self.capacity_at(self.steps_taken), dtype=torch.float64))
        stats = super()._run(real)
        self.steps_taken += 1
        return stats

    def _losses(self, real: Tensor):
        cont, disc = self._latent_spec
        mu, logvar = self.model.encode(real)
        z, loss_kl, terms = ops.joint_latent(mu, logvar, cont, disc, self._cap, self.gamma_cont, self.gamma_disc,
                                             beta=self.beta_kl, temperature=self.temperature, with_terms=True)
        loss_rec = self.compute_rec_loss(real, self.model.decode(z), reduction="mean", write=True)
        return z, loss_rec, loss_kl, terms

    def _write_losses(self, cur_iter, v_kl, v_rec, *terms):
        self.writer.add_scalar("kl_loss_unscaled", terms[0] + terms[1], global_step=cur_iter)
        super()._write_losses(cur_iter, v_kl, v_rec)
        self.writer.add_scalars("joint", self._extra_results(*terms), global_step=cur_iter)

    def _extra_results(self, v_klz, v_klc, v_cz, v_cc) -> dict:
        """``train_step`` returns the ``VAESolver`` dict (``loss_kl``: the weighted capacity loss) plus ``kl_cont``,
        ``kl_disc`` (the two batch-mean KLs) and ``cap_cont``, ``cap_disc`` (the capacities this step was held to)."""
        return dict(kl_cont=v_klz, kl_disc=v_klc, cap_cont=v_cz, cap_disc=v_cc)

    # ---- images: fakes from the joint prior, reconstructions from the deterministic code --------------------------------
    def _write_images_helper(self, batch, cur_iter):
        if self.writer is not None and cur_iter % self.test_iter == 0:
            cont, disc = self._latent_spec
            with torch.no_grad():
                fake = self.model.sample(ops.joint_prior_sample(batch.size(0), cont, disc, self.device))
            self.write_images(batch, fake, cur_iter)

    def write_images(self, batch, fake_batch, cur_iter):
        if self.writer is not None and cur_iter % self.test_iter == 0:
            cont, disc = self._latent_spec
            with torch.no_grad():
                mu, logvar = self.model.encode(batch)
                # z_cont = mu and the one-hot of every variable's most likely category: never raw logits to the decoder
                rec_det = self.model.decode(ops.joint_latent(mu, logvar, cont, disc, None, 0.0, 0.0, hard=True))
            k = min(batch.size(0), 16)
            grid = torch.cat([batch[:k], rec_det[:k], fake_batch[:k]], dim=0).data.cpu()
            self.writer.add_images("reconstructions", grid, global_step=cur_iter)


class AnnealedVAESolver(JointVAESolver):
    """AnnealedVAE: ``beta_kl * gamma |KL - C(t)|`` with ``C(t) = min(c_max, c_max t / iteration_threshold)``: the
    ``disc=()`` case of ``JointVAESolver`` with ``C_min = 0``.  ``gamma`` is ``gamma_cont``."""

    def __init__(self, *args, gamma: float = 1000.0, c_max: float = 25.0, iteration_threshold: int = 100000, **kwargs):
        super().__init__(*args, latent_spec=None, cont_capacity=(0.0, c_max, iteration_threshold, gamma),
                         disc_capacity=(0.0, 0.0, 1, 0.0), **kwargs)

    @property
    def gamma(self) -> float:
        return self.gamma_cont

    @gamma.setter
    def gamma(self, value):
        self.gamma_cont = value
