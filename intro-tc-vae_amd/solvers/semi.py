"""The semi-supervised S2 solvers (Locatello et al. 2020, "Disentangling Factors of Variation Using Few Labels";
disentanglement_lib's ``semi_supervised_vae``: S2-beta-VAE, S2-beta-TC-VAE, S2-DIP-VAE, S2-FactorVAE).  The reference has
none of them.  Each is an unsupervised objective of this package plus ONE term, which ties the first F latent means of a
small labelled batch to that batch's factor values (``ops.supervised_regularizer``):

    loss = scale * (beta_rec * mean_B rec + hook(first B rows) + gamma_sup(t) * sup(mu(x_l), y))

A batch is the pair ``(x, y)``: ``x`` [B + B_l, C, H, W] whose LAST ``B_l = y.shape[0]`` rows are the labelled ones, ``y``
[B_l, F] their integer factor values (``hipvae.dataset.DeviceLabelledLoader`` yields exactly this).  The wrapped objective
runs unchanged on the first B rows; the labelled rows go through a second ``model.encode`` call -- BatchNorm sees the two
batches in that order, which equals ``bn_groups(2)`` stacking -- and are neither decoded nor reconstructed.

``sup`` is a SUM over the labelled batch, as the library defines it.  Its weight follows ``sup_schedule`` over the steps
this solver has taken, t, with T = ``sup_threshold``:

    "fixed": gamma_sup        "anneal": gamma_sup * min(1, t / T)        "fine_tune": gamma_sup * min(1, max(0, t - T))

``train_step`` writes gamma_sup(t) into a persistent [1] float64 device tensor BEFORE the step runs and outside the
captured region, and copies ``y`` into a persistent device buffer there too; the kernel reads the weight when it runs, so
a captured step replays with the new weight and is never re-captured for it.

Out of scope: the library's ``embed`` form and l2's learnable scale (both add parameters outside the two flat groups);
its label-noise transformations (permuted / noisy / binned labels); a Soft-Intro variant; the global-batch form under data
parallel (each rank applies the term to its own labelled shard)."""
from typing import Optional

import torch
from torch import Tensor

import ops
from hipvae.functional import SUP_MAX_F
from solvers.dip import DIPSolver
from solvers.factor import FactorSolver
from solvers.hyper import Choice, Number
from solvers.tc import TCSovler
from solvers.vae import VAESolver

SUP_KINDS = tuple(ops.SUP_KINDS)
SUP_SCHEDULES = ("fixed", "anneal", "fine_tune")


def gamma_sup_at(schedule: str, gamma: float, threshold: float, t: int) -> float:
    """The weight of the label term after ``t`` training steps."""
    if schedule == "fixed":
        return gamma
    if schedule == "anneal":
        return gamma * (1.0 if threshold == 0 else min(1.0, t / threshold))
    if schedule == "fine_tune":
        return gamma * min(1.0, max(0.0, t - threshold))
    raise ValueError(f"sup_schedule must be one of {SUP_SCHEDULES} (got {schedule!r})")


def _factor_sizes(value):
    try:
        sizes = tuple(value)
        ok = all(not isinstance(k, bool) and int(k) == k and k >= 1 for k in sizes)
    except (TypeError, ValueError):
        sizes, ok = (), False
    if not ok or not 1 <= len(sizes) <= SUP_MAX_F:
        raise ValueError(f"factor_sizes is the tuple of the 1 .. {SUP_MAX_F} label columns' sizes, each an integer >= 1 "
                         f"(got {value!r})")
    return tuple(int(k) for k in sizes)


class SupervisedHook:
    """The label term, its schedule and graph-key entries, mixed in front of a VAE-step solver.  ``train_step((x, y),
    cur_iter)`` returns the wrapped solver's dict (``loss_kl`` includes the weighted term) plus ``loss_sup`` (unweighted)
    and ``gamma_sup`` (the weight this step ran with)."""
    sup_kind = Choice(SUP_KINDS, "xent")
    sup_schedule = Choice(SUP_SCHEDULES, "fixed")
    gamma_sup = Number()
    sup_threshold = Number()
    sup_scale = Number()                      # of the l2 form

    def __init__(self, *args, factor_sizes=None, sup_kind: str = "xent", gamma_sup: float = 1.0,
                 sup_schedule: str = "fixed", sup_threshold: float = 100000, sup_scale: float = 1.0, **kwargs):
        self.factor_sizes = _factor_sizes(factor_sizes)            # refused before anything is built
        self.sup_kind, self.sup_schedule = sup_kind, sup_schedule
        self.gamma_sup, self.sup_threshold, self.sup_scale = gamma_sup, sup_threshold, sup_scale
        super().__init__(*args, **kwargs)
        if len(self.factor_sizes) > self.model.zdim:
            raise ValueError(f"{len(self.factor_sizes)} factors need at least as many latent dimensions "
                             f"(zdim = {self.model.zdim})")
        self.steps_taken = 0                                       # t of gamma_sup(t)
        self._gsup = torch.zeros(1, dtype=torch.float64, device=self.device)     # what the kernel reads
        self._labels: Optional[Tensor] = None                     # [B_l, F] fp32: this step's labels

    def gamma_sup_at(self, t: int) -> float:
        return gamma_sup_at(self.sup_schedule, self.gamma_sup, self.sup_threshold, t)

    def _graph_key_extra(self) -> tuple:
        y = self._labels
        return super()._graph_key_extra() + (self.sup_kind, self.sup_scale, self.factor_sizes,
                                             None if y is None else (y.data_ptr(), tuple(y.shape)),
                                             self._gsup.data_ptr())

    def _batch(self, batch) -> Tensor:
        F = len(self.factor_sizes)
        x, y = batch if isinstance(batch, (tuple, list)) and len(batch) == 2 else (None, None)
        if not (isinstance(x, Tensor) and isinstance(y, Tensor) and x.dim() == 4 and y.dim() == 2
                and 1 <= y.shape[0] < x.shape[0] and y.shape[1] == F):
            got = tuple(tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__ for t in (x, y)) \
                if x is not None or y is not None else type(batch).__name__
            raise ValueError(f"the batch is (x [B + B_l, C, H, W], y [B_l, {F}]) with B >= 1, the last B_l rows of x "
                             f"labelled (got {got})")
        if self._labels is None or self._labels.shape != y.shape:
            self._labels = torch.empty(tuple(y.shape), dtype=torch.float32, device=self.device)
        self._labels.copy_(y)                                      # outside the captured region
        return x

    def _run(self, real: Tensor) -> Tensor:
        # outside the captured region: a replay reads what is written here
        self._gsup.fill_(self.gamma_sup_at(self.steps_taken))
        stats = super()._run(real)
        self.steps_taken += 1
        return stats

    def _losses(self, real: Tensor):
        B = real.shape[0] - self._labels.shape[0]
        z, loss_rec, loss_kl, extra = super()._losses(real[:B])
        mu_l, _ = self.model.encode(real[B:])
        sup, terms = ops.supervised_regularizer(mu_l, self._labels, self.sup_kind,
                                                self.factor_sizes if self.sup_kind == "xent" else None,
                                                gamma=self._gsup, scale=self.sup_scale, with_terms=True)
        loss_kl = self._lincomb((1.0, 1.0), loss_kl, sup)
        return z, loss_rec, loss_kl, terms if extra is None else torch.cat([extra, terms])

    def _write_losses(self, cur_iter, v_kl, v_rec, *extra):
        super()._write_losses(cur_iter, v_kl, v_rec, *extra[:-2])
        self.writer.add_scalars("sup", dict(loss=extra[-2], gamma=extra[-1]), global_step=cur_iter)

    def _extra_results(self, *extra) -> dict:
        return {**super()._extra_results(*extra[:-2]), "loss_sup": extra[-2], "gamma_sup": extra[-1]}


class S2VAESolver(SupervisedHook, VAESolver):
    """S2-beta-VAE: the VAE step plus the label term."""


class S2TCSolver(SupervisedHook, TCSovler):
    """S2-beta-TC-VAE: the beta-TC hook on the unlabelled rows plus the label term."""


class S2DIPSolver(SupervisedHook, DIPSolver):
    """S2-DIP-VAE: the DIP-VAE-I / II hook on the unlabelled rows plus the label term."""


class S2FactorSolver(SupervisedHook, FactorSolver):
    """S2-FactorVAE: the FactorVAE step (its discriminator sees the unlabelled rows' z) plus the label term."""
