"""The marginal log-likelihood log p(x) of held-out images, estimated with K importance samples from the encoder (Burda,
Grosse and Salakhutdinov 2016): log p(x) ~ logsumexp_k (log p(x | z_k) + log p(z_k) - log q(z_k | x)) - log K, z_k ~ q(z | x).
The samples are decoded in chunks and folded into a per-image fp64 state on the device (csrc/iwae.hip: itcv_iwae_accumulate),
so K is not bounded by memory."""
import math

import numpy as np
import torch

import ops
from . import functional as HF
from .inference import device_of, eval_mode, images

MAX_ROWS = 4096          # rows of one decoder pass under the default ``chunk``


def compute_log_likelihood(source, model, num_samples=1000, chunk=None, batch_size=64, num_images=None, indices=None,
                           seed=0, loss_type="mse", beta_rec=1.0):
    """Importance-weighted estimate of log p(x) under ``model`` for images of ``source`` (a ``DeviceImageTable`` or a
    dataset whose items are images or tuples that start with one), with ``num_samples`` = K samples per image.

    Returns ``dict(log_px, bits_per_dim, elbo, ess, per_image)``: the means over the images of the K-sample estimate, of
    ``-log_px / (P ln 2)`` (P values per image), of the one-sample bound (the mean of logw: the ELBO) and of the effective
    sample size; ``per_image`` holds the three per-image vectors (``log_px``, ``elbo``, ``ess``, numpy fp64) and the
    ``indices`` used.  Here logw = -(beta_rec rec + log q(z|x) - log p(z)) with ``rec`` the summed error of
    ``ops.reconstruction_loss``.  ONLY ``loss_type="bce"`` with ``beta_rec=1`` is a normalised likelihood (Bernoulli
    pixels); "mse" / "l1" estimate log p(x) up to the additive constant of the fixed-scale Gaussian / Laplace observation
    model that the reconstruction loss stands for (mse with beta_rec: N(recon, 1 / (2 beta_rec)) per value), so their
    ``bits_per_dim`` compares models trained alike and is not an absolute code length.  The structural types "ssim" and
    "ssim_l1" of ``ops.reconstruction_loss`` stand for no observation model of independent values and raise
    NotImplementedError here, like every unknown name.

    ``indices``: which images (default: all, or the first ``num_images``).  The images go through in batches of
    ``batch_size``; per batch of B the K samples are decoded ``chunk`` per image at a time (default: as many as keep
    ``B * chunk`` <= 4096 rows, at most 1024).  The model runs in eval mode under ``no_grad``; its training flag is put
    back and its BatchNorm buffers are not written.  The noise comes from a private CPU ``torch.Generator`` seeded by
    ``seed``, one draw per chunk in a fixed order: torch's global generators are untouched and two calls with one seed
    give the same bits."""
    if isinstance(num_samples, bool) or int(num_samples) != num_samples or num_samples < 1:
        raise ValueError(f"num_samples must be a positive integer (got {num_samples!r})")
    if loss_type not in HF.abi.LOSS_TYPES:
        raise NotImplementedError
    K, batch_size = int(num_samples), int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    if indices is None:
        n = len(source) if num_images is None else min(int(num_images), len(source))
        indices = np.arange(n, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    if indices.ndim != 1 or not len(indices):
        raise ValueError("compute_log_likelihood: indices must be a non-empty 1-D integer array")
    if chunk is not None and (int(chunk) != chunk or not 1 <= chunk <= HF.IWAE_MAX_K):
        raise ValueError(f"chunk must be an integer in 1..{HF.IWAE_MAX_K} (got {chunk!r})")
    device = device_of(model)
    gen = torch.Generator().manual_seed(int(seed))
    lt = HF.abi.LOSS_TYPES[loss_type]
    outs, P = [], None
    with eval_mode(model):
        for a in range(0, len(indices), batch_size):
            x = images(source, indices[a:a + batch_size], device)
            B = x.shape[0]
            P = x.numel() // B
            kc = int(chunk) if chunk is not None else max(1, min(HF.IWAE_MAX_K, MAX_ROWS // B))
            mu, logvar = model.encode(x)
            state = torch.zeros((5, B), dtype=torch.float64, device=device)
            for k0 in range(0, K, kc):
                k = min(kc, K - k0)
                eps = torch.randn((k * B, mu.shape[1]), generator=gen).to(device)
                sample = ops.iwae_sample(mu, logvar, k, eps=eps)
                rows = HF.IwaeRowsFn.apply(x.reshape(B, -1), model.decode(sample.z).reshape(k * B, -1), lt)
                HF.iwae_accumulate(rows, sample.lat, state, beta_rec, 1.0)
            outs.append(torch.stack(HF.iwae_finalize(state)))
    got = torch.cat(outs, dim=1).cpu().numpy()                      # the one read-back
    log_px, elbo, ess = got[0], got[1], got[2]
    return dict(log_px=float(log_px.mean()), bits_per_dim=float(-log_px.mean() / (P * math.log(2.0))),
                elbo=float(elbo.mean()), ess=float(ess.mean()),
                per_image=dict(log_px=log_px, elbo=elbo, ess=ess, indices=indices))
