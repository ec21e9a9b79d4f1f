"""TCSovler (sic): VAESolver whose KL hook is the beta-TC-VAE term (beta-1)*TC + KL
(/root/reference/solvers/tc.py:22-89), or -- ``kl_loss="full"`` -- the full decomposition
mi + beta*tc + dwkl of the reference's ``_compute_kl_loss_full`` (tc.py:91-144), which is also
offered as per-sample metrics (``kl_decomposition``)."""
from typing import Optional

from torch import Tensor

import ops
from hipvae import ddp
from ops import kl_divergence, tc_decomposition, tc_kl_loss, total_correlation
from solvers.hyper import Choice
from solvers.vae import VAESolver
from utils import SingletonWriter

KL_LOSSES = ("simple", "full")


class TcHook:
    """The beta-TC KL hooks, mixed in front of ``VAESolver`` or ``IntroSolver``.  ``kl_loss`` says which one
    ``compute_kl_loss`` runs: "simple" (tc.py:69-89, the reference's) or "full" (tc.py:91-144); it selects kernels, and
    the captured graph's key ends with it (solvers/vae.py)."""
    kl_loss = Choice(KL_LOSSES, "simple")

    def __init__(self, *args, kl_loss: str = "simple", **kwargs):
        self.kl_loss = kl_loss
        super().__init__(*args, **kwargs)

    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        if getattr(self, "kl_loss", "simple") == "full":
            return TcHook._compute_kl_loss_full(self, z, mu, logvar, reduce, beta, write)
        return TcHook._compute_kl_loss_simple(self, z, mu, logvar, reduce, beta, write)

    def _compute_kl_loss_simple(self, z, mu, logvar, reduce="mean", beta=None, write=False) -> Tensor:
        """tc.py:69-89.  In a data-parallel run the estimator sees the whole global batch: the means
        are all-gathered (the variance is the sample row's own, ops.py:81) and the importance weights
        use global batch size and row indices."""
        if beta is None:
            beta = self.beta_kl
        dataset_size = len(self.dataset)
        if not (write and self.writer):       # the whole hook inside the estimator's own launches
            return tc_kl_loss(z, mu, logvar, dataset_size, beta, reduce, mu_all=ddp.all_gather_rows(mu),
                              row_offset=ddp.row_offset(mu.shape[0]))
        kl_loss = kl_divergence(logvar, mu, reduce=reduce)
        tc = total_correlation(z, mu, logvar, dataset_size, reduce=reduce, mu_all=ddp.all_gather_rows(mu),
                               row_offset=ddp.row_offset(mu.shape[0]))
        self.write_scalar(SingletonWriter().cur_iter, "kl_loss_unscaled", kl_loss)
        return (beta - 1.0) * tc + kl_loss

    def _compute_kl_loss_full(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                              beta: float = None, write: bool = False) -> Tensor:
        """tc.py:91-144: mi + beta * tc + dwkl (per sample, or their means with ``reduce="mean"``), in the fused
        estimator's launches.  In a data-parallel run the estimator sees the whole global batch: this hook takes the
        variance of component i, so means and log-variances are all-gathered together (one collective)."""
        if z is None:
            raise ValueError("_compute_kl_loss_full needs the sampled latents z (got None)")
        if beta is None:
            beta = self.beta_kl
        dataset_size = len(self.dataset)
        mu_all, logvar_all = ddp.all_gather_mu_logvar(mu, logvar)
        off = ddp.row_offset(mu.shape[0])
        sw = SingletonWriter()
        log_decomp = bool(sw.writer) and reduce == "mean"
        if not (log_decomp or (write and self.writer)):
            return ops.tc_full_loss(z, mu, logvar, dataset_size, 1.0, beta, 1.0, reduce, mu_all=mu_all,
                                    logvar_all=logvar_all, row_offset=off)
        loss, comps = ops._tc_full(z, mu, logvar, dataset_size, 1.0, beta, 1.0, reduce, mu_all, logvar_all, off)
        if reduce == "mean":
            terms = comps.mean(1)
            ddp.mean_scalars_(terms)            # the global batch's means (equal shards)
            if log_decomp:
                mi, tc, kl = terms.tolist()
                sw.writer.add_scalars("tc_decomp", {"mi": mi, "tc": tc, "kl": kl}, global_step=sw.cur_iter)
            unscaled = terms.sum()
        else:
            unscaled = comps.sum(0)
        if write:
            self.write_scalar(sw.cur_iter, "kl_loss_unscaled", unscaled)
        return loss

    def kl_decomposition(self, z, mu, logvar):
        """Per-sample (mi, tc, dwkl) of tc.py:104-121 as metrics (no gradient).  In a data-parallel run: this rank's
        rows of the global batch's estimate (means and log-variances all-gathered, global row indices)."""
        if ddp.get() is None:
            return tc_decomposition(z, mu, logvar, len(self.dataset))
        mu_all, logvar_all = ddp.all_gather_mu_logvar(mu.detach(), logvar.detach())
        return tc_decomposition(z, mu, logvar, len(self.dataset), mu_all=mu_all, logvar_all=logvar_all,
                                row_offset=ddp.row_offset(mu.shape[0]))


class TCSovler(TcHook, VAESolver):
    """The VAE step with the beta-TC hook."""
