"""The decomposition of the aggregate KL over a whole dataset, on the device: index-code mutual information, total
correlation and dimension-wise KL (the evaluation the beta-TC-VAE objective is named for), with the dataset's aggregate
posterior q(z) = sum_n w_n q(z | x_n) taken over ALL components by the streaming kernel of csrc/aggregate.hip
(``functional.aggregate_logdensity``).  The minibatch estimate the solvers log as ``tc_decomp`` caps MI at log B and
depends on the batch size; this one does not.

For samples z_j ~ q(z | x_rows[j]):
    mi_j   = log q(z_j | x_rows[j]) - log q(z_j)
    tc_j   = log q(z_j) - sum_l log q_l(z_jl)
    dwkl_j = sum_l log q_l(z_jl) - log p(z_j)
with the ops.py:24-29 density throughout (the same function as training's full decomposition; only the weights differ:
exact log weights over all components instead of the stratified matrix).  mi_j + tc_j + dwkl_j telescopes to
log q(z_j | x) - log p(z_j), whose mean estimates the analytic KL."""
import numpy as np
import torch

from . import functional as HF
from .abi import call, ptr, stream
from .inference import device_of, eval_mode, images

KEYS = ("mi", "tc", "dwkl", "kl", "kl_analytic", "joint_entropy", "marginal_entropies", "dimwise_kl")
_HALF_LOG_2PI = 0.9189385332046727


def elbo_decomposition(z, rows, mu, logvar, logw=None):
    """``z`` [S, D]: samples, ``rows`` int64 [S]: the component each was drawn from, ``(mu, logvar)`` [N, D]: the
    components, ``logw`` [N]: their log weights (None: uniform).  Returns a dict of Python floats ``mi``, ``tc``, ``dwkl``,
    ``kl`` (their sum), ``kl_analytic`` (the mean of ops.py:161-163 over ``rows``), ``joint_entropy`` (-mean log q(z)),
    and fp64 numpy arrays ``marginal_entropies`` [D] (-mean log q_l(z_l)) and ``dimwise_kl`` [D].  Per-sample terms are
    fp32 kernel outputs; the means over the samples are taken in fp64 on the device and read back once.  Non-finite
    inputs, or rows outside the components, raise ``ValueError``."""
    if rows.dtype != torch.int64 or rows.dim() != 1 or rows.shape[0] != z.shape[0]:
        raise ValueError("elbo_decomposition: rows must be an int64 vector with one entry per sample")
    S, D = z.shape
    N = mu.shape[0]
    logqz, lse = HF.aggregate_logdensity(z, mu, logvar, logw)
    in_range = ((rows >= 0) & (rows < N)).all()
    safe = rows.clamp(0, N - 1)
    mu_r, lv_r = mu.index_select(0, safe).contiguous(), logvar.index_select(0, safe).contiguous()
    logqcx, logpz = HF.diag_logdensity_rows(z, mu_r, lv_r)
    kl_rows = torch.empty((S,), dtype=torch.float32, device=z.device)
    call("itcv_kl_rows_fwd", ptr(lv_r), ptr(mu_r), ptr(kl_rows), S, D, stream())
    d64 = torch.float64
    prodm = lse.to(d64).sum(1)
    lq, lcx, lpz = logqz.to(d64), logqcx.to(d64), logpz.to(d64)
    # log p(z_jl) of the dimension-wise term, clamped as the kernels clamp it (ops.py:29)
    lp_dim = (-0.5 * z.to(d64) ** 2 - _HALF_LOG_2PI).clamp(min=-50.0)
    finite = torch.stack([torch.isfinite(t).all() for t in (z, mu, logvar) + (() if logw is None else (logw,))]).all()
    head = torch.stack([(lcx - lq).mean(), (lq - prodm).mean(), (prodm - lpz).mean(), kl_rows.to(d64).mean(), -lq.mean(),
                        (finite & in_range).to(d64)])
    out = torch.cat([head, -lse.to(d64).mean(0), (lse.to(d64) - lp_dim).mean(0)]).cpu().numpy()     # the one read-back
    if out[5] != 1.0:
        raise ValueError("elbo_decomposition: non-finite inputs or rows outside the components")
    mi, tc, dwkl = float(out[0]), float(out[1]), float(out[2])
    return dict(mi=mi, tc=tc, dwkl=dwkl, kl=mi + tc + dwkl, kl_analytic=float(out[3]), joint_entropy=float(out[4]),
                marginal_entropies=out[6:6 + D].copy(), dimwise_kl=out[6 + D:6 + 2 * D].copy())


def dataset_posteriors(source, model, indices, batch_size=64):
    """``(mu, logvar)`` [N, D] fp32 on the device: ``model.encode`` of the images at ``indices``, batch by batch, in eval
    mode and without gradients, written into two preallocated buffers.  ``source``: a ``DeviceImageTable`` (one
    ``gather`` per batch) or a dataset (``__getitem__``; an item is an image or a tuple that starts with one)."""
    indices = np.asarray(indices, dtype=np.int64)
    if indices.ndim != 1 or not len(indices):
        raise ValueError("dataset_posteriors: indices must be a non-empty 1-D integer array")
    device = device_of(model)
    mu = logvar = None
    with eval_mode(model):
        for a in range(0, len(indices), int(batch_size)):
            idx = indices[a:a + int(batch_size)]
            m, lv = model.encode(images(source, idx, device))
            if mu is None:
                mu = torch.empty((len(indices), m.shape[1]), dtype=torch.float32, device=m.device)
                logvar = torch.empty_like(mu)
            mu[a:a + len(idx)].copy_(m)
            logvar[a:a + len(idx)].copy_(lv)
    return mu, logvar


def draw_plan(num_images, num_samples, num_components, seed):
    """The documented draws of ``compute_elbo_decomposition``, from one ``np.random.RandomState(seed)`` in this order:
    1. components: all images when ``num_components`` is None or >= ``num_images``, otherwise
       ``sort(choice(num_images, num_components, replace=False))``;
    2. sample rows: ``randint(Nc, size=num_samples)`` -- indices AMONG the components, so a sample's own component is
       always in the mixture and MI <= log Nc;
    3. ``randint(2**31 - 1)``: the seed of the CPU ``torch.Generator`` the noise is drawn from.
    Returns ``(components int64 [Nc], rows int64 [S], eps_seed)``."""
    rs = np.random.RandomState(seed)
    if num_components is None or num_components >= num_images:
        comps = np.arange(num_images, dtype=np.int64)
    else:
        comps = np.sort(rs.choice(num_images, int(num_components), replace=False)).astype(np.int64)
    rows = rs.randint(len(comps), size=int(num_samples)).astype(np.int64)
    return comps, rows, int(rs.randint(2 ** 31 - 1))


def compute_elbo_decomposition(source, model, num_samples=10000, num_components=None, batch_size=64, seed=None,
                               return_inputs=False):
    """``elbo_decomposition`` of ``model`` on ``source`` (a ``DeviceImageTable`` or a dataset): the components are the
    posteriors of the images ``draw_plan`` picks, the samples z = mu + eps * exp(logvar / 2) (itcv_reparam_fwd) of the
    rows it picks, eps ~ N(0, 1) [S, D] from a CPU ``torch.Generator`` seeded by it.  torch's global generators are
    not touched.  With ``return_inputs`` also ``(z, rows, mu, logvar)``."""
    comps, rows, eps_seed = draw_plan(len(source), num_samples, num_components, seed)
    mu, logvar = dataset_posteriors(source, model, comps, batch_size)
    dev = mu.device
    rows_d = torch.from_numpy(rows).to(dev)
    eps = torch.randn((len(rows), mu.shape[1]), generator=torch.Generator().manual_seed(eps_seed)).to(dev)
    mu_r, lv_r = mu.index_select(0, rows_d).contiguous(), logvar.index_select(0, rows_d).contiguous()
    z = torch.empty_like(mu_r)
    call("itcv_reparam_fwd", ptr(mu_r), ptr(lv_r), ptr(eps), ptr(z), z.numel(), stream())
    scores = elbo_decomposition(z, rows_d, mu, logvar)
    return (scores, (z, rows_d, mu, logvar)) if return_inputs else scores

