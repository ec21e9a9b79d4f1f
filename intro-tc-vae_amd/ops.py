"""Drop-in mirror of the reference's ``ops`` module surface, backed by HIP kernels.

Same names, argument order and error behaviour as /root/reference/ops.py (cited per
function); the arithmetic runs in libitcv_hip.so (hipvae.functional).  Differences that a
caller can observe are limited to:
  * ``total_correlation`` never materialises the [B,B,D] pairwise tensor (fused kernels; ``tc_components`` /
    ``tc_decomposition`` expose the fused estimator); the reference's building blocks that produce or take that
    tensor -- ``gaussian_log_density_torch``, ``gaussian_log_density``, ``minibatch_stratified_sampling``,
    ``minibatch_weighted_sampling``, ``on_off_diag`` -- exist under their own names in materialising form, so code
    that imports them (solvers/tc.py:5-11) keeps working;
  * the N(0,1) draws of ``reparameterize`` come from ``noise`` (device generator by default;
    ``set_noise_mode("host")`` reproduces the reference's CPU stream, ``noise_queue`` injects
    recorded draws for parity tests).
"""
import contextlib
import math

import numpy as np
import torch

from hipvae import abi
from hipvae import functional as HF

# ---------------------------------------------------------------------------- noise source
_noise = {"mode": "device", "queue": None}


def set_noise_mode(mode):
    """'device': torch.randn on the tensor's device (ops.py:184 on a GPU run);
    'host': CPU generator then copy (bit-identical to the reference's --device -1 stream)."""
    assert mode in ("device", "host")
    _noise["mode"] = mode


@contextlib.contextmanager
def noise_queue(draws):
    """Feed recorded N(0,1) tensors, in draw order, to every ``noise()`` call inside the block."""
    prev = _noise["queue"]
    _noise["queue"] = list(draws)
    try:
        yield
    finally:
        _noise["queue"] = prev


def noise(shape, device):
    q = _noise["queue"]
    if q is not None:
        if not q:
            raise RuntimeError("noise_queue exhausted")
        t = q.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(device=device, dtype=torch.float32)
    if _noise["mode"] == "host":
        return torch.randn(shape).to(device)
    return torch.randn(shape, device=device)


def uniform_noise(shape, device):
    """U[0, 1) draws (``torch.rand``: fp32 multiples of 2^-24) from the same source as ``noise``: the device generator,
    the host's in "host" mode, or the next recorded tensor inside a ``noise_queue`` block."""
    q = _noise["queue"]
    if q is not None:
        if not q:
            raise RuntimeError("noise_queue exhausted")
        t = q.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(device=device, dtype=torch.float32)
    if _noise["mode"] == "host":
        return torch.rand(shape).to(device)
    return torch.rand(shape, device=device)


# ---------------------------------------------------------------------------- ops surface
def reparameterize(mu, logvar):
    """ops.py:166-185."""
    return HF.ReparamFn.apply(mu, logvar, noise(mu.shape, mu.device))


def kl_no_reduce(logvar, mu):
    """ops.py:161-163 (argument order: logvar, mu)."""
    return HF.KlRowsFn.apply(logvar, mu)


def kl_divergence(logvar, mu, reduce="sum", scale=1.0):
    """ops.py:136-158 (any ``reduce`` other than 'sum' / 'mean' returns the per-sample vector, as there), in ONE launch;
    ``scale`` (extension) multiplies the result inside that launch -- the solver hooks pass their beta."""
    return HF.KlLossFn.apply(logvar, mu, {"sum": 1, "mean": 2}.get(reduce, 0), float(scale))


def reconstruction_loss(x, recon_x, loss_type="mse", reduction="sum", scale=1.0):
    """ops.py:188-236; NotImplementedError for unknown loss_type / reduction, AssertionError on
    an empty batch, x is detached.  The reduction runs inside the kernels (two launches in all); ``scale`` (extension)
    multiplies the result there -- the solver hooks pass their beta.  Two structural types (extension, not in the
    reference) go to ``ssim_loss`` and need the 4-D images: "ssim" (alpha = 1) and "ssim_l1" (alpha = 0.84, the mix of
    Zhao et al. 2017)."""
    batch_size = x.size(0)
    assert batch_size != 0
    if reduction not in ("sum", "mean", "none"):
        raise NotImplementedError
    if loss_type in SSIM_LOSS_ALPHA:
        if x.dim() != 4 or recon_x.dim() != 4:
            raise ValueError(f'loss_type "{loss_type}" needs [B, C, H, W] images (got {tuple(x.shape)}, '
                             f"{tuple(recon_x.shape)})")
        return ssim_loss(x, recon_x, reduction, scale, alpha=SSIM_LOSS_ALPHA[loss_type])
    if loss_type not in abi.LOSS_TYPES:
        raise NotImplementedError
    return HF.ReconLossFn.apply(x.detach().reshape(x.size(0), -1), recon_x.reshape(recon_x.size(0), -1),
                                abi.LOSS_TYPES[loss_type], HF._REDUCTION[reduction], float(scale))


SSIM_LOSS_ALPHA = {"ssim": 1.0, "ssim_l1": 0.84}      # reconstruction_loss's structural types -> alpha of ssim_loss


def ssim_loss(x, recon, reduction="sum", scale=1.0, alpha=1.0, window=11, sigma=1.5):
    """Structural-similarity reconstruction loss (Wang et al. 2004; as a training loss Snell et al. 2017, mixed with L1
    Zhao et al. 2017), in the units of the other reconstruction losses.  With SSIM_b the mean over channels and positions
    of the SSIM map of image b (a ``window``-tap Gaussian of width ``sigma``, valid filtering, C1 = 0.01^2, C2 = 0.03^2)
    and P = C H W:  rows[b] = P alpha (1 - SSIM_b) + (1 - alpha) sum_p |recon - x|;  ``reduction`` and ``scale`` as in
    ``reconstruction_loss``.  fp32 out, fp64 inside; x is detached.  Two launches forward, one backward
    (itcv_ssim_loss_fwd / _bwd).  ValueError: alpha outside [0, 1], a window that is not an odd number in 3..15, images that
    are not 4-D or smaller than the window; NotImplementedError: an unknown reduction."""
    if reduction not in ("sum", "mean", "none"):
        raise NotImplementedError
    alpha, window = float(alpha), int(window)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"ssim_loss: alpha must lie in [0, 1] (got {alpha})")
    if window < 3 or window > 15 or window % 2 == 0:
        raise ValueError(f"ssim_loss: window must be an odd number of taps in 3..15 (got {window})")
    if x.dim() != 4 or recon.shape != x.shape:
        raise ValueError(f"ssim_loss: x and recon must be [B, C, H, W] images of one shape (got {tuple(x.shape)}, "
                         f"{tuple(recon.shape)})")
    if min(x.shape[2], x.shape[3]) < window:
        raise ValueError(f"ssim_loss: H, W = {x.shape[2]}, {x.shape[3]} are below window = {window}")
    return HF.SsimLossFn.apply(x.detach(), recon, HF._REDUCTION[reduction], float(scale), alpha, window, float(sigma))


def gaussian_log_density_torch(x, mu, logvar):
    """ops.py:15-21: -gaussian_nll_loss(x, mu, exp(logvar), eps=1e-4, full=True) clamped at -50, elementwise over the
    broadcast of the three operands; the variance floor passes the gradient straight through (as F.gaussian_nll_loss
    does), the -50 clamp blocks it."""
    return HF.GaussLogDensityFn.apply(x, mu, logvar, True)


def gaussian_log_density(x, mu, logvar):
    """ops.py:24-29: -0.5 * ((x-mu)^2 exp(-logvar) + logvar + log 2 pi) clamped at -50."""
    return HF.GaussLogDensityFn.apply(x, mu, logvar, False)


def minibatch_weighted_sampling(log_qz_prob, batch_size, dataset_size):
    """ops.py:92-101 on a materialised [B,B,D] tensor -> (logqz_prodmarginals [B], log_qz [B])."""
    assert log_qz_prob.size(0) == batch_size
    return HF.SamplingFn.apply(log_qz_prob, int(dataset_size), True)


def minibatch_stratified_sampling(log_qz_prob, batch_size, dataset_size):
    """ops.py:104-115 on a materialised [B,B,D] tensor -> (logqz_prodmarginals [B], log_qz [B])."""
    assert log_qz_prob.size(0) == batch_size
    return HF.SamplingFn.apply(log_qz_prob, int(dataset_size), False)


def on_off_diag(x):
    """ops.py:118-122 (never called by the reference): (torch.diagonal(x), x - torch.diag_embed(x)) for a 2-D x.
    No gradient is recorded."""
    return HF.on_off_diag(x)


def total_correlation(z, mu, logvar, dataset_size, reduce="mean", mu_all=None, row_offset=0):
    """ops.py:52-89.  ``mu_all``/``row_offset`` are the data-parallel extension: the means of the
    whole global batch (all-gathered) and this rank's first global row."""
    tc = HF.TcRowsFn.apply(z, mu if mu_all is None else mu_all, logvar, int(dataset_size), int(row_offset))
    return tc.mean() if reduce == "mean" else tc


def tc_kl_loss(z, mu, logvar, dataset_size, beta, reduce="mean", mu_all=None, row_offset=0):
    """(beta - 1) * total_correlation(z, mu, logvar, N, reduce) + kl_divergence(logvar, mu, reduce): the KL hook of the TC
    solvers (solvers/tc.py:69-89) fused into the estimator's launches (3 forward, 2 backward).  ``reduce`` as in the
    reference: 'mean', else per sample."""
    return HF.TcKlFn.apply(z, mu if mu_all is None else mu_all, logvar, int(dataset_size), int(row_offset), float(beta) - 1.0,
                           1.0, 2 if reduce == "mean" else 0)


def tc_full_loss(z, mu, logvar, dataset_size, alpha=1.0, beta=1.0, gamma=1.0, reduce="mean", mu_all=None,
                 logvar_all=None, row_offset=0):
    """alpha * mi + beta * tc + gamma * dwkl per sample: the full decomposition loss of solvers/tc.py:91-144 (the
    reference's is alpha = gamma = 1) -- ops.py:24-29 density, variance of component i, stratified sampler -- fused into
    the estimator's launches (3 forward, 2 backward), with gradients.  ``reduce`` as in the reference: 'mean', else per
    sample.  ``mu_all`` / ``logvar_all`` / ``row_offset``: the data-parallel extension (the whole global batch's means
    and log-variances, e.g. from ``hipvae.ddp.all_gather_mu_logvar``, and this rank's first global row); the local
    ``mu`` / ``logvar`` are then not read."""
    return _tc_full(z, mu, logvar, dataset_size, alpha, beta, gamma, reduce, mu_all, logvar_all, row_offset)[0]


def _tc_full(z, mu, logvar, dataset_size, alpha, beta, gamma, reduce, mu_all=None, logvar_all=None, row_offset=0):
    """tc_full_loss and the per-sample (mi, tc, dwkl) [3, B] of the same launches (no gradient)."""
    if (mu_all is None) != (logvar_all is None):
        raise ValueError("mu_all and logvar_all are given together")
    if mu_all is None:
        mu_all, logvar_all = mu, logvar
    return HF.TcFullFn.apply(z, mu_all, logvar_all, int(dataset_size), int(row_offset), float(alpha), float(beta),
                             float(gamma), 2 if reduce == "mean" else 0)


DIP_KINDS = {"i": 1, "ii": 2}


def dip_kl_loss(mu, logvar, beta, lambda_od, lambda_d, kind="i", mu_all=None, logvar_all=None, row_offset=0,
                with_terms=False):
    """The KL hook of DIP-VAE-I / DIP-VAE-II (Kumar et al. 2018; disentanglement_lib's ``dip_vae`` with ``dip_type``
    "i" / "ii"; not in the reference): beta * kl_divergence(logvar, mu, "mean") + lambda_od * sum_{i != j} C_ij^2 +
    lambda_d * sum_i (C_ii - 1)^2, with C the covariance (divisor Bt) of the means of the whole batch, plus
    diag(mean_b exp(logvar)) for kind "ii" -- two launches forward, one backward, bitwise reproducible.
    ``mu_all`` / ``logvar_all`` / ``row_offset``: the data-parallel extension, as in ``tc_full_loss`` (the regulariser is
    that of the global batch, the KL that of this rank's ``mu.shape[0]`` rows of it; the local ``mu`` / ``logvar`` are
    then not read).  ``with_terms``: also return the device vector (mean KL, off-diagonal term, diagonal term), no
    gradient."""
    if kind not in DIP_KINDS:
        raise ValueError(f"kind must be one of {tuple(DIP_KINDS)} (got {kind!r})")
    if (mu_all is None) != (logvar_all is None):
        raise ValueError("mu_all and logvar_all are given together")
    if mu_all is None:
        mu_all, logvar_all = mu, logvar
    out, terms = HF.DipKlFn.apply(mu_all, logvar_all, int(mu.shape[0]), int(row_offset), DIP_KINDS[kind], float(lambda_od),
                                  float(lambda_d), float(beta))
    return (out, terms) if with_terms else out


def dip_regularizer(mu, logvar, lambda_od, lambda_d, kind="i", mu_all=None, logvar_all=None, row_offset=0,
                    with_terms=False):
    """``dip_kl_loss`` without its KL term (beta = 0): the covariance regulariser alone."""
    return dip_kl_loss(mu, logvar, 0.0, lambda_od, lambda_d, kind, mu_all, logvar_all, row_offset, with_terms)


MMD_KERNELS = HF.MMD_KERNELS


def mmd_kl_loss(z, mu, logvar, prior, beta, lambda_mmd, kernel="imq", bandwidth=None, z_all=None, prior_all=None,
                with_terms=False):
    """The KL hook of InfoVAE / MMD-VAE (Zhao, Song and Ermon 2017) and WAE-MMD (Tolstikhin et al. 2018; not in the
    reference): beta * kl_divergence(logvar, mu, "mean") + lambda_mmd * MMD^2(z, prior), the unbiased U-statistic

        MMD^2 = sum_{i != j} k(z_i, z_j) / (B (B - 1)) + sum_{i != j} k(p_i, p_j) / (P (P - 1)) - 2 sum_{i, j} k(z_i, p_j) / (B P)

    (it may be negative) between the sampled latents ``z`` [B, D] and ``prior`` [P, D], draws from N(0, I) that receive
    no gradient.  With d2 = |a - b|^2 (fp64, difference form) and the bandwidth h (``bandwidth``; None: 2 D, WAE's Cbase
    for a unit-variance prior): ``kernel`` "rbf" is k = exp(-d2 / h); "imq" is WAE's multi-scale inverse multiquadric
    k = sum_s s h / (s h + d2), s in (0.1, 0.2, 0.5, 1, 2, 5, 10).  Two launches forward, one backward, fp64 throughout,
    bitwise reproducible.  ``z_all`` / ``prior_all``: the data-parallel extension -- the samples and prior draws of the
    whole global batch (given together); the statistic is then that of the global batch, the KL that of this rank's
    ``mu`` / ``logvar``, and the local ``z`` / ``prior`` are not read.  ``with_terms``: also return the device vector
    (mean KL, MMD^2, S_zz, S_pp, S_zp), no gradient."""
    if kernel not in MMD_KERNELS:
        raise ValueError(f"kernel must be one of {tuple(MMD_KERNELS)} (got {kernel!r})")
    if (z_all is None) != (prior_all is None):
        raise ValueError("z_all and prior_all are given together")
    if z_all is None:
        z_all, prior_all = z, prior
    D = z_all.shape[-1]
    if z_all.dim() != 2 or prior_all.dim() != 2 or prior_all.shape[1] != D or mu.shape != logvar.shape \
            or mu.dim() != 2 or mu.shape[1] != D:
        raise ValueError(f"z, prior, mu and logvar must be matrices that share D (got {tuple(z_all.shape)}, "
                         f"{tuple(prior_all.shape)}, {tuple(mu.shape)}, {tuple(logvar.shape)})")
    h = 2.0 * D if bandwidth is None else float(bandwidth)
    out, terms = HF.MmdKlFn.apply(z_all, prior_all.detach(), mu, logvar, MMD_KERNELS[kernel], h, float(lambda_mmd),
                                  float(beta))
    return (out, terms) if with_terms else out


def mmd_regularizer(z, prior, lambda_mmd, kernel="imq", bandwidth=None, with_terms=False):
    """``mmd_kl_loss`` without its KL term (beta = 0): lambda_mmd * MMD^2(z, prior) alone.  There is no ``mu`` /
    ``logvar`` to read: ``z`` stands in for both, and with beta = 0 their values do not reach the result."""
    zd = z.detach()
    return mmd_kl_loss(z, zd, zd, prior, 0.0, lambda_mmd, kernel, bandwidth, with_terms=with_terms)


def sw_kl_loss(z, mu, logvar, prior, theta, beta, lambda_sw, z_all=None, prior_all=None, with_terms=False):
    """The KL hook of the sliced-Wasserstein autoencoder (Kolouri et al. 2018; not in the reference):
    beta * kl_divergence(logvar, mu, "mean") + lambda_sw * SW^2(z, prior) with

        SW^2 = (1 / L) sum_l (1 / B) sum_i (sort(z theta_l)_i - sort(prior theta_l)_i)^2,   theta_l = t_l / |t_l|

    between the sampled latents ``z`` [B, D] and as many draws ``prior`` [B, D] from N(0, I), over the L directions given
    as the rows of ``theta`` [L, D] (N(0, I) draws; they are normalised by the kernel).  Neither ``prior`` nor ``theta``
    receives a gradient.  The order of z's projections is the stable one (ties by row index).  Two launches forward, one
    backward, fp64 throughout, bitwise reproducible.  ``z_all`` / ``prior_all``: the data-parallel extension -- the
    samples and prior draws of the whole global batch (given together); the distance is then that of the global batch,
    the KL that of this rank's ``mu`` / ``logvar``, and the local ``z`` / ``prior`` are not read.  ``with_terms``: also
    return the device vector (mean KL, SW^2, max_l SW_l^2), no gradient."""
    if (z_all is None) != (prior_all is None):
        raise ValueError("z_all and prior_all are given together")
    if z_all is None:
        z_all, prior_all = z, prior
    D = z_all.shape[-1]
    if z_all.dim() != 2 or prior_all.shape != z_all.shape or theta.dim() != 2 or theta.shape[1] != D \
            or mu.shape != logvar.shape or mu.dim() != 2 or mu.shape[1] != D:
        raise ValueError(f"z and prior must share one [B, D] shape, theta [L, D], mu and logvar [Bl, D] its D (got "
                         f"{tuple(z_all.shape)}, {tuple(prior_all.shape)}, {tuple(theta.shape)}, {tuple(mu.shape)}, "
                         f"{tuple(logvar.shape)})")
    lambda_sw, beta = float(lambda_sw), float(beta)
    if not (lambda_sw >= 0.0 and math.isfinite(lambda_sw)) or not math.isfinite(beta):
        raise ValueError(f"lambda_sw must be a finite number >= 0 and beta finite (got {lambda_sw!r}, {beta!r})")
    out, terms = HF.SwKlFn.apply(z_all, prior_all.detach(), theta.detach(), mu, logvar, lambda_sw, beta)
    return (out, terms) if with_terms else out


def sw_regularizer(z, prior, theta, lambda_sw, with_terms=False):
    """``sw_kl_loss`` without its KL term (beta = 0): lambda_sw * SW^2(z, prior) alone.  There is no ``mu`` / ``logvar``
    to read: ``z`` stands in for both, and with beta = 0 their values do not reach the result."""
    zd = z.detach()
    return sw_kl_loss(z, zd, zd, prior, theta, 0.0, lambda_sw, with_terms=with_terms)


def sliced_wasserstein(a, b, theta):
    """(SW^2 as a device scalar, the per-direction SW_l^2 [L] in fp64) between the rows of ``a`` and ``b`` [N, D] (equal
    counts) over the directions ``theta`` [L, D]: the forward of ``sw_kl_loss`` alone, no gradient, nothing of size
    L x N written."""
    if a.dim() != 2 or b.shape != a.shape or theta.dim() != 2 or theta.shape[1] != a.shape[1]:
        raise ValueError(f"a and b must share one [N, D] shape and theta [L, D] its D (got {tuple(a.shape)}, "
                         f"{tuple(b.shape)}, {tuple(theta.shape)})")
    return HF.sw_distance(a, b, theta)


ADA_AVERAGINGS = HF.ADA_AVERAGINGS


def ada_group(mu, logvar, beta, averaging="gvae", own=None, eps=None, with_terms=False):
    """The latent op of Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020, "Weakly-Supervised Disentanglement Without
    Compromises"; disentanglement_lib's ``weak`` module, ``GroupVAEBase`` with ``aggregate_argmax``; not in the
    reference) on ``B`` pairs stacked as ``2B`` rows, rows ``b`` and ``B + b`` a pair (m1, l1), (m2, l2):

        delta = exp(l1 - l2) + (m2 - m1)^2 exp(-l2) - 1 + l2 - l1,   tau = (min_d delta + max_d delta) / 2,
        own   = delta >= tau                  (D = 1 or all-equal delta: every dimension keeps its own posterior)
        "gvae":  mb = (m1 + m2) / 2, vb = (e^l1 + e^l2) / 2;   "mlvae": vb = 2 e^l1 e^l2 / (e^l1 + e^l2),
                 mb = vb (m1 e^-l1 + m2 e^-l2) / 2
        z_i   = mt_i + eps_i exp(lt_i / 2) with (mt_i, lt_i) = (m_i, l_i) where own, (mb, log vb) elsewhere
        loss  = beta * mean over the 2B rows of -1/2 sum_d (1 + lt - mt^2 - e^lt)

    Returns ``(z [2B, D], loss)``, both differentiable in ``mu`` and ``logvar`` (the mask is a constant of the backward
    pass, as with ``tf.where``); with ``with_terms`` also the mask as used (uint8 [B, D]) and the device vector (mean KL,
    mean number of shared dimensions per pair), no gradient.  ``own`` [B, D] replaces the threshold (non-zero: own) --
    GVAE / ML-VAE with known groups.  ``eps`` None: ONE draw ``noise(mu.shape, mu.device)``, so recorded draws and graph
    capture work as for ``reparameterize``.  Two launches forward, one backward, fp64 inside, bitwise reproducible;
    1 <= D <= 512."""
    if averaging not in ADA_AVERAGINGS:
        raise ValueError(f"averaging must be one of {tuple(ADA_AVERAGINGS)} (got {averaging!r})")
    if mu.dim() != 2 or mu.shape != logvar.shape:
        raise ValueError(f"mu and logvar must share one [2B, D] shape (got {tuple(mu.shape)}, {tuple(logvar.shape)})")
    R, D = mu.shape
    if R < 2 or R % 2:
        raise ValueError(f"the rows are pairs (b, B + b): an even, positive number of them (got {R})")
    if not 1 <= D <= HF.ADA_MAX_D:
        raise ValueError(f"ada_group takes 1 <= D <= {HF.ADA_MAX_D} (got {D})")
    if own is not None and tuple(own.shape) != (R // 2, D):
        raise ValueError(f"own must be a [B, D] = {(R // 2, D)} mask (got {tuple(own.shape)})")
    if eps is not None and eps.shape != mu.shape:
        raise ValueError(f"eps must have mu's shape {tuple(mu.shape)} (got {tuple(eps.shape)})")
    abi.need_device(mu, logvar)
    if eps is None:
        eps = noise(mu.shape, mu.device)
    z, loss, mask, terms = HF.AdaGroupFn.apply(mu, logvar, eps.detach(), None if own is None else own.detach(),
                                               ADA_AVERAGINGS[averaging], float(beta))
    return (z, loss, mask, terms) if with_terms else (z, loss)


VAMP_REDUCES = tuple(HF.VAMP_REDUCES)


def _vamp_components(p_mu, p_logvar, D):
    if p_mu.dim() != 2 or p_mu.shape != p_logvar.shape or p_mu.shape[1] != D:
        raise ValueError(f"p_mu and p_logvar must share one [K, D] shape with D = {D} (got {tuple(p_mu.shape)}, "
                         f"{tuple(p_logvar.shape)})")
    return p_mu.shape[0]


def vamp_latent(mu, logvar, p_mu, p_logvar, beta=1.0, eps=None, reduce="mean", with_terms=False):
    """The latent op of a VAE with a VampPrior (Tomczak & Welling 2018, "VAE with a VampPrior"; not in the reference): one
    sample per row of the posterior ``(mu, logvar)`` [B, D] against the uniform mixture of the K diagonal Gaussians
    ``(p_mu, p_logvar)`` [K, D] -- the encoder's outputs on the pseudo-inputs.  With c = log 2 pi:

        z      = mu + eps exp(logvar / 2),          logq_b = -1/2 sum_d (c + logvar + eps^2)
        L_bk   = -1/2 sum_d (c + p_logvar_kd + (z_bd - p_mu_kd)^2 exp(-p_logvar_kd))
        logp_b = logsumexp_k L_bk - log K,          rows_b = beta (logq_b - logp_b)

    Returns ``(z [B, D], loss)`` with ``loss`` the mean ("mean"), the sum ("sum") or the vector ("none") of ``rows``; both
    are differentiable in all four inputs.  With ``with_terms`` also the device vector (mean KL unscaled, mean logq, mean
    logp), no gradient.  ``eps`` None: ONE draw ``noise(mu.shape, mu.device)``, so recorded draws and graph capture work as
    for ``reparameterize``.  A form that takes a sampled z is deliberately not offered: at small variances the direct mu
    and z gradients of log q are large and of opposite sign, and they would be rounded to fp32 before autograd cancels
    them.  Two launches forward, one backward, fp64 inside, bitwise reproducible; 1 <= B, K <= 4096, B K <= 2^22,
    1 <= D <= 512."""
    if reduce not in HF.VAMP_REDUCES:
        raise ValueError(f"reduce must be one of {VAMP_REDUCES} (got {reduce!r})")
    if mu.dim() != 2 or mu.shape != logvar.shape:
        raise ValueError(f"mu and logvar must share one [B, D] shape (got {tuple(mu.shape)}, {tuple(logvar.shape)})")
    B, D = mu.shape
    K = _vamp_components(p_mu, p_logvar, D)
    HF.vamp_check_shapes(B, K, D, "vamp_latent")
    if eps is not None and eps.shape != mu.shape:
        raise ValueError(f"eps must have mu's shape {tuple(mu.shape)} (got {tuple(eps.shape)})")
    beta = float(beta)
    if not math.isfinite(beta):
        raise ValueError(f"beta must be finite (got {beta})")
    abi.need_device(mu, logvar, p_mu, p_logvar)
    if eps is None:
        eps = noise(mu.shape, mu.device)
    z, loss, terms, _, _, _ = HF.VampLatentFn.apply(mu, logvar, eps.detach(), p_mu, p_logvar, beta,
                                                    HF.VAMP_REDUCES[reduce])
    return (z, loss, terms) if with_terms else (z, loss)


def vamp_log_prob(x, p_mu, p_logvar):
    """fp64 [N]: ``log (1 / K) sum_k N(x_n; p_mu_k, diag exp(p_logvar_k))`` of the rows ``x`` [N, D] under the mixture of
    ``vamp_latent``, by the same pair pass: on the ``z`` that op returned it gives that op's logp bit for bit.  No
    gradient.  1 <= N, K <= 4096, N K <= 2^22, 1 <= D <= 512 (``hipvae.density.vamp_log_prob`` chunks longer inputs)."""
    if x.dim() != 2:
        raise ValueError(f"x must be [N, D] (got {tuple(x.shape)})")
    N, D = x.shape
    K = _vamp_components(p_mu, p_logvar, D)
    HF.vamp_check_shapes(N, K, D, "vamp_log_prob")
    abi.need_device(x, p_mu, p_logvar)
    return HF.vamp_log_prob(x.detach(), p_mu.detach(), p_logvar.detach())


_JOINT_SEG = {}


def joint_spec(n_cont, disc_sizes, D=None):
    """``(n_cont, disc_sizes as a tuple of ints, n_disc)`` of a latent spec, checked: n_cont >= 0, every K_i >= 2,
    1 <= n_cont + sum K_i <= 512 and, when ``D`` is given, equal to it."""
    disc = tuple(disc_sizes)
    if isinstance(n_cont, bool) or int(n_cont) != n_cont or n_cont < 0:
        raise ValueError(f"n_cont must be a non-negative integer (got {n_cont!r})")
    if any(isinstance(k, bool) or int(k) != k or k < 2 for k in disc):
        raise ValueError(f"every discrete variable needs K >= 2 categories (got {disc})")
    n_cont, disc = int(n_cont), tuple(int(k) for k in disc)
    n_disc = sum(disc)
    if not 1 <= n_cont + n_disc <= HF.JOINT_MAX_D:
        raise ValueError(f"joint_latent takes 1 <= D <= {HF.JOINT_MAX_D} (got n_cont + sum K = {n_cont + n_disc})")
    if D is not None and n_cont + n_disc != D:
        raise ValueError(f"n_cont + sum K = {n_cont} + {n_disc} is not D = {D}")
    return n_cont, disc, n_disc


def joint_segments(disc_sizes, device):
    """The device table [n_disc, 2] int32 of a discrete block: per column the first and the one-past-last column of its
    group, counted from the first discrete column.  Built once per (sizes, device) and kept."""
    key = (tuple(disc_sizes), torch.device(device))
    seg = _JOINT_SEG.get(key)
    if seg is None:
        ends = np.cumsum(key[0])
        rows = [(e - k, e) for k, e in zip(key[0], ends) for _ in range(k)]
        seg = _JOINT_SEG[key] = torch.tensor(rows, dtype=torch.int32).reshape(-1, 2).to(device)
    return seg


def joint_latent(mu, logvar, n_cont, disc_sizes, capacity, gamma_cont, gamma_disc, beta=1.0, temperature=0.67, eps=None,
                 u=None, hard=False, with_terms=False):
    """The latent op of JointVAE (Dupont 2018, "Learning Disentangled Joint Continuous and Discrete Representations") and,
    with ``disc_sizes=()``, of AnnealedVAE (Burgess et al. 2018; disentanglement_lib's ``annealed_vae``); neither is in
    the reference.  ``mu``, ``logvar`` [B, D] with D = n_cont + sum K_i: columns [0, n_cont) are the continuous posterior,
    the rest of ``mu`` the logits ``a`` of G categorical variables with K_1 .. K_G categories side by side; the same
    columns of ``logvar`` are never read and get an exactly zero gradient.

        z_cont = m + eps exp(l / 2),                            KL_z = mean_b -1/2 sum_d (1 + l - m^2 - e^l)
        per group: log alpha = a - logsumexp(a),  g = -log(-log u)  (u = 0 is taken as 2^-25),
                   y = softmax((a + g) / temperature),          KL_c = sum_i mean_b (log K_i + sum_k alpha_k log alpha_k)
        loss = beta (gamma_cont |KL_z - C_z| + gamma_disc |KL_c - C_c|),   (C_z, C_c) = capacity

    ``capacity`` is a [2] float64 DEVICE tensor that the kernel reads when it runs: a captured step replays with the
    value it holds then.  Returns ``(z [B, D] = [z_cont | y_1 | .. | y_G], loss)``, both differentiable in ``mu`` and
    ``logvar``; with ``with_terms`` also the device vector (KL_z, KL_c, C_z, C_c), no gradient.  ``eps`` None: a draw
    ``noise((B, n_cont))``, then ``u`` None: a draw ``uniform_noise((B, n_disc))`` -- in this order, and none for an
    empty block -- so recorded draws and graph capture work as for ``reparameterize``.  ``hard=True`` returns the
    deterministic code alone: z_cont = mu bit for bit and per group the one-hot of the first maximum of the logits; no
    loss, no gradient, one launch (``capacity`` and the weights are not looked at).  Two launches forward, one backward,
    fp64 inside, bitwise reproducible; 1 <= D <= 512, every K_i >= 2."""
    if mu.dim() != 2 or mu.shape != logvar.shape:
        raise ValueError(f"mu and logvar must share one [B, D] shape (got {tuple(mu.shape)}, {tuple(logvar.shape)})")
    B, D = mu.shape
    if B < 1:
        raise ValueError("joint_latent needs at least one row")
    n_cont, disc, n_disc = joint_spec(n_cont, disc_sizes, D)
    if hard:
        abi.need_device(mu)
        return HF.joint_latent_hard(mu, joint_segments(disc, mu.device) if n_disc else None, n_cont, n_disc)
    temperature, gamma_cont, gamma_disc, beta = float(temperature), float(gamma_cont), float(gamma_disc), float(beta)
    if not (0.0 < temperature < math.inf):
        raise ValueError(f"temperature must be a finite number above 0 (got {temperature})")
    if not (0.0 <= gamma_cont < math.inf and 0.0 <= gamma_disc < math.inf):
        raise ValueError(f"gamma_cont and gamma_disc must be finite and not negative (got {gamma_cont}, {gamma_disc})")
    if not math.isfinite(beta):
        raise ValueError(f"beta must be finite (got {beta})")
    if eps is not None and tuple(eps.shape) != (B, n_cont):
        raise ValueError(f"eps must be [B, n_cont] = {(B, n_cont)} (got {tuple(eps.shape)})")
    if u is not None and tuple(u.shape) != (B, n_disc):
        raise ValueError(f"u must be [B, n_disc] = {(B, n_disc)} (got {tuple(u.shape)})")
    abi.need_device(mu, logvar)
    if not isinstance(capacity, torch.Tensor) or tuple(capacity.shape) != (2,) or capacity.dtype != torch.float64 \
            or not capacity.is_cuda:
        raise ValueError("capacity must be a [2] float64 device tensor (C_z, C_c): the kernel reads it when it runs")
    if n_cont and eps is None:
        eps = noise((B, n_cont), mu.device)
    if n_disc and u is None:
        u = uniform_noise((B, n_disc), mu.device)
    z, loss, terms = HF.JointLatentFn.apply(mu, logvar, eps.detach() if n_cont else None, u.detach() if n_disc else None,
                                            joint_segments(disc, mu.device) if n_disc else None, capacity.detach(),
                                            n_cont, n_disc, temperature, gamma_cont, gamma_disc, beta)
    return (z, loss, terms) if with_terms else (z, loss)


def joint_prior_sample(n, n_cont, disc_sizes, device):
    """``n`` draws [n, n_cont + sum K_i] of the JointVAE prior: standard normal columns, then per discrete variable the
    one-hot of a uniformly drawn category.  Plain torch; not on the hot path."""
    n_cont, disc, _ = joint_spec(n_cont, disc_sizes)
    cols = [torch.randn((n, n_cont), device=device)]
    for k in disc:
        cols.append(torch.nn.functional.one_hot(torch.randint(k, (n,), device=device), k).to(torch.float32))
    return torch.cat(cols, dim=1)


SUP_KINDS = HF.SUP_KINDS


def supervised_regularizer(mu, labels, kind="xent", factor_sizes=None, gamma=1.0, scale=1.0, with_terms=False):
    """The label term of the semi-supervised S2 objectives (Locatello et al. 2020, "Disentangling Factors of Variation
    Using Few Labels"; disentanglement_lib's ``semi_supervised_vae``, ``supervised_regularizer_xent`` / ``_l2`` /
    ``_cov``; not in the reference).  ``mu`` [B_l, D]: the encoder means of the labelled rows (a row-strided view is read
    in place); ``labels`` [B_l, F]: their factor values, fp32 holding integers; 1 <= F <= min(D, 64), D <= 512.  The first
    F latent means are tied to the F factors.  All three forms are SUMS over the labelled batch, not means: the library
    defines them so, and published ``gamma_sup`` values assume it.

        "xent": t = y_bf / K_f,  sup = sum_b sum_{f<F} (max(m, 0) - m t + log1p(exp(-|m|))),  m = mu[b, f]
                (``factor_sizes`` = (K_1, .., K_F), required)
        "l2":   sup = sum_b sum_{f<F} (scale mu[b, f] - y_bf)^2         (``scale`` a fixed number)
        "cov":  C = (1 / B_l) sum_b (mu_b - mean)(y_b - ybar)^T [D, F],  W = C with W_ii = 0,  sup = sum_ij W_ij^2

    Columns >= F of ``mu`` receive an exactly zero gradient under xent and l2; under cov they are penalised, because all
    of C off the zeroed diagonal counts.  ``logvar`` is not an input.  Returns ``gamma * sup``, differentiable in ``mu``;
    with ``with_terms`` also the device vector (sup, gamma), no gradient.  ``gamma``: a Python float, or a [1] float64
    DEVICE tensor that the kernel reads when it runs, so that a captured step replays with the value it holds then.
    Two launches forward, one backward, fp64 inside, bitwise reproducible.  Launched eagerly the term costs 50 - 75 us
    forward + backward on an MI355X, bound by the host's launch rate.

    Out of scope: the library's ``embed`` form and l2's learnable scale (both add parameters outside the encoder's and the
    decoder's flat groups), and its label-noise transformations (permuted / noisy / binned labels)."""
    if kind not in SUP_KINDS:
        raise ValueError(f"kind must be one of {tuple(SUP_KINDS)} (got {kind!r})")
    if not isinstance(mu, torch.Tensor) or mu.dim() != 2 or mu.shape[0] < 1:
        raise ValueError(f"mu must be a [B_l, D] matrix with B_l >= 1 (got {tuple(getattr(mu, 'shape', ()))})")
    B, D = mu.shape
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or labels.shape[0] != B or labels.shape[1] < 1:
        raise ValueError(f"labels must be a [B_l, F] = [{B}, F] tensor on the device "
                         f"(got {tuple(getattr(labels, 'shape', ()))})")
    F = labels.shape[1]
    if F > D or F > HF.SUP_MAX_F or D > HF.SUP_MAX_D:
        raise ValueError(f"supervised_regularizer takes 1 <= F <= min(D, {HF.SUP_MAX_F}) and D <= {HF.SUP_MAX_D} "
                         f"(got F = {F}, D = {D})")
    sizes = None
    if kind == "xent":
        if factor_sizes is None:
            raise ValueError('kind "xent" needs factor_sizes = (K_1, .., K_F): its targets are y / K')
        sizes = tuple(factor_sizes)
        if len(sizes) != F or any(isinstance(k, bool) or int(k) != k or k < 1 for k in sizes):
            raise ValueError(f"factor_sizes must be {F} integers >= 1, one per label column (got {sizes})")
        sizes = tuple(int(k) for k in sizes)
    if isinstance(gamma, torch.Tensor):
        if tuple(gamma.shape) != (1,) or gamma.dtype != torch.float64:
            raise ValueError(f"gamma must be a number or a [1] float64 device tensor (got {tuple(gamma.shape)}, "
                             f"{gamma.dtype})")
        gamma = gamma.detach()
    elif not math.isfinite(float(gamma)):
        raise ValueError(f"gamma must be finite (got {gamma})")
    if not math.isfinite(float(scale)):
        raise ValueError(f"scale must be finite (got {scale})")
    abi.need_device(mu)
    if not labels.is_cuda or labels.device != mu.device:
        raise ValueError(f"labels must be a [B_l, F] = [{B}, F] tensor on the device (got one on {labels.device})")
    out, terms = HF.SupRegFn.apply(mu, labels.detach(), SUP_KINDS[kind], sizes, gamma, float(scale))
    return (out, terms) if with_terms else out


IWAE_ESTIMATORS = tuple(HF.IWAE_ESTIMATORS)


def iwae_sample(mu, logvar, K, eps=None):
    """K reparameterised samples of each of the B posteriors ``(mu, logvar)`` [B, D] for the importance-weighted bound
    (Burda, Grosse and Salakhutdinov 2016; not in the reference).  Row ``r = k B + b`` is sample k of image b, so slab
    ``k = 0`` has the layout of a plain batch:

        z_r = mu_b + exp(logvar_b / 2) eps_r,      lat_r = 1/2 sum_d (z_rd^2 - eps_rd^2 - logvar_bd) = log q(z_r | x_b) - log p(z_r)

    with no clamp and no variance floor.  Returns an ``HF.IwaeSample``: ``z`` [K B, D] fp32 for the decoder, ``lat`` [K B]
    fp64, both differentiable in ``mu`` and ``logvar`` (row-strided views are read in place), and the buffer ``weights``
    that ``iwae_bound`` fills.  ``eps`` None: ONE draw ``noise((K B, D))``, so recorded draws and graph capture work as for
    ``reparameterize``.  One launch forward, one backward, fp64 inside, bitwise reproducible; 1 <= D <= 512,
    1 <= K <= 1024, K B <= 2^24."""
    if mu.dim() != 2 or mu.shape != logvar.shape or mu.shape[0] < 1:
        raise ValueError(f"mu and logvar must share one [B, D] shape (got {tuple(mu.shape)}, {tuple(logvar.shape)})")
    B, D = mu.shape
    if isinstance(K, bool) or int(K) != K or not 1 <= K <= HF.IWAE_MAX_K or K * B > HF.IWAE_MAX_ROWS:
        raise ValueError(f"iwae_sample takes an integer 1 <= K <= {HF.IWAE_MAX_K} with K B <= 2^24 (got K = {K!r}, B = {B})")
    if not 1 <= D <= HF.IWAE_MAX_D:
        raise ValueError(f"iwae_sample takes 1 <= D <= {HF.IWAE_MAX_D} (got {D})")
    K = int(K)
    if eps is not None and tuple(eps.shape) != (K * B, D):
        raise ValueError(f"eps must be [K B, D] = {(K * B, D)} (got {tuple(eps.shape)})")
    abi.need_device(mu, logvar)
    if eps is None:
        eps = noise((K * B, D), mu.device)
    sample = HF.IwaeSample(B, K, mu.device)
    sample.z, sample.lat = HF.IwaeSampleFn.apply(mu, logvar, eps.detach(), sample)
    return sample


def iwae_bound(x, recon, sample, beta_rec, beta_kl, loss_type="mse", estimator="iwae", with_terms=False):
    """The K-sample importance-weighted bound of ``x`` [B, ...] from the reconstructions ``recon`` [K B, ...] of
    ``sample.z`` (``sample``: what ``iwae_sample`` returned).  With err that of ``reconstruction_loss``:

        rows_r = sum_p err(recon_rp, x_bp),   logw_r = -(beta_rec rows_r + beta_kl lat_r),   w_r = softmax_k(logw)_r
        bound_b = logsumexp_k logw_r - log K,   loss = -mean_b bound_b

    ``x`` is read in place by every one of its K rows, never copied.  Returns ``loss``, differentiable in ``recon`` and,
    through ``sample``, in ``mu`` and ``logvar``; with ``with_terms`` also the device vector (beta_rec mean_b sum_k w rows,
    beta_kl mean_b sum_k w lat, mean_b bound_b, mean_b ess_b), ess_b = 1 / sum_k w_r^2, no gradient.  ``estimator`` selects
    the gradient that reaches ``mu`` and ``logvar``: "iwae" the plain reparameterised one; "stl" (Roeder et al. 2017) drops
    the direct dependence of log q on them and keeps the path through z; "dreg" (Tucker et al. 2019) weights that path by
    w once more.  The decoder's gradient is the same under all three, and so is every forward value.  Unknown
    ``estimator``: ValueError; unknown ``loss_type``: NotImplementedError -- "ssim" and "ssim_l1" among them: they are
    not likelihoods of independent elements and have no broadcast-row kernel.  Four launches forward, two backward (plus
    the sample's one), fp64 inside, bitwise reproducible."""
    if estimator not in HF.IWAE_ESTIMATORS:
        raise ValueError(f"estimator must be one of {IWAE_ESTIMATORS} (got {estimator!r})")
    if loss_type not in abi.LOSS_TYPES:
        raise NotImplementedError
    if not isinstance(sample, HF.IwaeSample):
        raise ValueError("sample must be what iwae_sample returned")
    B, K = sample.B, sample.K
    if x.size(0) != B or recon.size(0) != K * B or x.numel() * K != recon.numel():
        raise ValueError(f"x must hold B = {B} images and recon K B = {K * B} of the same size "
                         f"(got {tuple(x.shape)}, {tuple(recon.shape)})")
    beta_rec, beta_kl = float(beta_rec), float(beta_kl)
    if not (math.isfinite(beta_rec) and math.isfinite(beta_kl)):
        raise ValueError(f"beta_rec and beta_kl must be finite (got {beta_rec}, {beta_kl})")
    abi.need_device(x, recon)
    rows = HF.IwaeRowsFn.apply(x.detach().reshape(B, -1), recon.reshape(K * B, -1), abi.LOSS_TYPES[loss_type])
    loss, terms, _ = HF.IwaeCombineFn.apply(rows, sample.lat, sample, beta_rec, beta_kl, HF.IWAE_ESTIMATORS[estimator])
    return (loss, terms) if with_terms else loss


def tc_components(z, mu, logvar, dataset_size, *, var_from_row=True, eps_density=True, weighted=False):
    """Fused ops.py:80-84 + :92-115: returns (logqz_prodmarginals [B], log_qz [B]) of the stratified
    (default) or weighted sampler, for either density flavour / variance orientation.  No grad."""
    flags = (abi.TC_VAR_FROM_ROW if var_from_row else 0) | (abi.TC_EPS_DENSITY if eps_density else 0) | (
        abi.TC_WEIGHTED if weighted else 0)
    with torch.no_grad():
        prodm, logqz, _ = HF.tc_components(z, mu, logvar, dataset_size, 0, flags)
    return prodm, logqz


def tc_decomposition(z, mu, logvar, dataset_size, mu_all=None, logvar_all=None, row_offset=0):
    """solvers/tc.py:104-121 per-sample (mi, tc, dwkl): the decomposition of the reference's full hook
    (un-eps'd density, variance indexed by component), offered as metrics.  ``mu_all`` / ``logvar_all`` /
    ``row_offset``: the data-parallel extension, as in ``tc_full_loss``."""
    if (mu_all is None) != (logvar_all is None):
        raise ValueError("mu_all and logvar_all are given together")
    with torch.no_grad():
        logq_cx, logpz = HF.diag_logdensity_rows(z, mu, logvar)
        if mu_all is None:
            prodm, logqz, _ = HF.tc_components(z, mu, logvar, dataset_size, 0, 0)
        else:
            prodm, logqz, _ = HF.tc_components(z, mu_all, logvar_all, dataset_size, row_offset, 0)
    return logq_cx - logqz, logqz - prodm, prodm - logpz


def log_importance_weight_matrix(batch_size, dataset_size):
    """ops.py:32-49 (host helper; the kernels evaluate these three values inline)."""
    n, m = dataset_size, batch_size - 1
    strat = (n - m) / (n * m)
    w = np.full((batch_size, batch_size), 1.0 / m, dtype=np.float32)
    w[:, 0] = 1.0 / n
    w[:, 1] = strat
    w[m - 1, 0] = strat
    return torch.from_numpy(np.log(w))


def entropy(x, base=None, axis=0, eps=1e-9):
    """ops.py:125-133 (numpy, evaluation only)."""
    if not isinstance(x, np.ndarray):
        raise TypeError("Input x has to be a numpy.ndarray object!")
    shifted = x + eps
    prob = shifted / shifted.sum(axis=axis, keepdims=True)
    h = -(prob * np.log(prob + eps)).sum(axis=axis)
    return h if base is None else h / math.log(base + eps)


# ---------------------------------------------------------------------------- FactorVAE
def permute_dims(z, keys=None):
    """FactorVAE's ``shuffle_codes``: every column of ``z`` [B, D] permuted over the batch on its own, in one launch:
    ``out[:, d] = z[argsort(keys[:, d], stable), d]``.  ``keys`` None: one N(0, 1) draw per element from ``noise`` (the
    project's noise source, so recorded draws and graph capture work as for ``reparameterize``): argsort of i.i.d.
    continuous keys is a uniform random permutation.  Any keys give a permutation (ties go by row index).  The result
    carries no gradient.  B <= 4096, D <= 512."""
    abi.need_device(z)
    if keys is None:
        keys = noise(z.shape, z.device)
    return HF.permute_dims(z, keys)


def factor_pass(z, discriminator, z_perm=None, keys=None, permute=True):
    """ONE forward of ``discriminator`` (models.Discriminator) over the 2B stacked rows [z; z_perm], both detached, for
    ``factor_tc`` and ``factor_disc_loss`` to share (``shared=``): both then see the same weights and the same z.
    ``z_perm`` None: ``permute_dims(z, keys)``, written straight into the stacked buffer together with the copy of z (one
    launch).  ``permute=False``: the B rows of z alone, enough for ``factor_tc``."""
    abi.need_device(z)
    if z.dim() != 2 or z.shape[1] != discriminator.zdim:
        raise ValueError(f"z must be [B, {discriminator.zdim}] (got {tuple(z.shape)})")
    B, D = z.shape
    if not permute and z_perm is None:
        return discriminator.run(z.detach(), B)
    if z_perm is not None:
        if z_perm.shape != z.shape:
            raise ValueError(f"z_perm {tuple(z_perm.shape)} must have z's shape {tuple(z.shape)}")
        return discriminator.run(torch.cat([z.detach(), z_perm.detach()]), B)
    if keys is None:
        keys = noise(z.shape, z.device)
    x = torch.empty((2 * B, D), dtype=torch.float32, device=z.device)
    HF.permute_dims(z, keys, out=x[B:], zcopy=x[:B])
    return discriminator.run(x, B)


def factor_tc(z, discriminator, with_terms=False, shared=None):
    """FactorVAE's density-ratio estimate of the total correlation of q(z): tc = mean_i (l_i0 - l_i1), l = D(z) the
    discriminator's logits; differentiable in ``z`` ONLY (the data-gradient chain of the fused layers; the
    discriminator's parameters are constants and their ``.grad`` is not touched).  ``shared``: a ``factor_pass`` of this
    z to read the logits from (None: the forward runs here, over z alone).  ``with_terms``: also the device vector
    (tc, d_loss, d_acc) of the pass, no gradient."""
    dp = factor_pass(z, discriminator, permute=False) if shared is None else shared
    tc = HF.DiscTcFn.apply(z, dp)
    return (tc, dp.stats) if with_terms else tc


def factor_disc_loss(z, discriminator, z_perm=None, keys=None, with_terms=False, shared=None):
    """The discriminator's loss 0.5 mean_i CE(D(z_i), 0) + 0.5 mean_i CE(D(z_perm_i), 1), differentiable in the
    discriminator's parameters ONLY: z and z_perm are detached, the first layer's data gradient is not computed.  CE is
    the stable softplus of the logit difference.  ``z_perm`` / ``keys`` / ``shared``: as in ``factor_pass``.
    ``with_terms``: also the device vector (tc, d_loss, d_acc), no gradient; d_acc is the share of the 2B rows the
    discriminator classifies correctly."""
    dp = factor_pass(z, discriminator, z_perm, keys) if shared is None else shared
    loss = HF.DiscLossFn.apply(dp, *discriminator.flat_parameters())
    return (loss, dp.stats) if with_terms else loss
