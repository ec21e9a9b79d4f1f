"""fp64 restatement of the VampPrior latent op (csrc/vamp.hip, ops.vamp_latent): numpy for the kernel tests, torch (any
dtype) for the step oracle.  With c = log 2 pi, the posterior (mu, logvar) [B, D], one draw eps and the K components
(p_mu, p_logvar) [K, D]:

    z_bd   = mu_bd + eps_bd exp(logvar_bd / 2)
    logq_b = -1/2 sum_d (c + logvar_bd + eps_bd^2)
    L_bk   = -1/2 sum_d (c + p_logvar_kd + (z_bd - p_mu_kd)^2 exp(-p_logvar_kd))
    logp_b = logsumexp_k L_bk - log K,   r_bk = softmax_k L_bk
    rows_b = beta (logq_b - logp_b),     loss = mean_b rows_b ("sum", "none" likewise)

and the gradients for an upstream weight G_b of rows_b and an upstream gradient gz of z, written out (not autograd):

    A_bd = sum_k r_bk (z_bd - p_mu_kd) iv_kd,  t = gz + G beta A,  dmu = t,  dlogvar = exp(logvar / 2) eps t / 2 - G beta / 2
    dp_mu_kd = -beta sum_b G_b r_bk (z_bd - p_mu_kd) iv_kd,   dp_logvar_kd = beta / 2 sum_b G_b r_bk (1 - (z_bd - p_mu_kd)^2 iv_kd)
"""
import math

import numpy as np

LOG2PI = math.log(2.0 * math.pi)
REDUCES = ("none", "mean", "sum")


def make_inputs(B, K, D, seed):
    """fp32 (mu, logvar, eps, p_mu, p_logvar): posteriors of moderate width and components that share a common offset, so
    that no row's softmax over the components is a disguised arg-max and the KL is not a small difference of its parts."""
    rng = np.random.RandomState(seed)
    mu = 0.5 * rng.randn(B, D)
    logvar = rng.uniform(-1.0, 0.5, (B, D))
    eps = rng.randn(B, D)
    p_mu = 0.3 * rng.randn(1, D) + rng.randn(K, D) / math.sqrt(D)
    p_logvar = 0.4 + rng.uniform(-1.0, 1.0, (K, D)) / math.sqrt(D)
    return tuple(a.astype(np.float32) for a in (mu, logvar, eps, p_mu, p_logvar))


def vamp(mu, logvar, eps, p_mu, p_logvar, beta=1.0, reduce="mean", g=1.0, gz=None, z=None):
    """Everything the op computes, in fp64 from the given arrays.  ``g``: the upstream gradient of the loss (a scalar, or
    [B] under "none"); ``gz``: that of z (None: zero).  ``z``: the fp32 sample the device formed (None: the fp64 one); the
    kernels form L from the rounded sample they return, the difference is below the fp32 bar either way."""
    mu, logvar, eps, p_mu, p_logvar = (np.asarray(a, np.float64) for a in (mu, logvar, eps, p_mu, p_logvar))
    (B, D), K = mu.shape, p_mu.shape[0]
    zz = mu + eps * np.exp(0.5 * logvar) if z is None else np.asarray(z, np.float64)
    logq = -0.5 * (LOG2PI + logvar + eps * eps).sum(1)
    iv = np.exp(-p_logvar)
    diff = zz[:, None, :] - p_mu[None, :, :]                                  # [B, K, D]
    L = -0.5 * (LOG2PI + p_logvar[None] + diff * diff * iv[None]).sum(2)
    m = L.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(L - m).sum(1))
    r = np.exp(L - lse[:, None])
    logp = lse - math.log(K)
    kl = logq - logp
    rows = beta * kl
    loss = rows if reduce == "none" else rows.mean() if reduce == "mean" else rows.sum()
    G = np.broadcast_to(np.asarray(g, np.float64), (B,)) * (1.0 / B if reduce == "mean" else 1.0)
    gz = np.zeros_like(zz) if gz is None else np.asarray(gz, np.float64)
    w = diff * iv[None]                                                        # (z - p_mu) iv
    A = (r[:, :, None] * w).sum(1)
    t = gz + (G * beta)[:, None] * A
    Gr = G[:, None] * r                                                        # [B, K]
    return dict(z=zz, logq=logq, logp=logp, r=r, rows=rows, loss=loss,
                terms=np.array([kl.mean(), logq.mean(), logp.mean()]),
                dmu=t, dlogvar=0.5 * np.exp(0.5 * logvar) * eps * t - 0.5 * (G * beta)[:, None],
                dp_mu=-beta * (Gr[:, :, None] * w).sum(0),
                dp_logvar=0.5 * beta * (Gr[:, :, None] * (1.0 - diff * w)).sum(0))


def conditions(ref):
    """The two conditions a stored case satisfies: (|mean KL| / max(|mean logq|, |mean logp|), the largest responsibility
    of any row)."""
    kl, lq, lp = ref["terms"]
    return abs(kl) / max(abs(lq), abs(lp)), float(ref["r"].max())


def torch_vamp(mu, logvar, eps, p_mu, p_logvar, beta=1.0, reduce="mean"):
    """(z, loss, logq, logp) in torch, any dtype, differentiable by autograd: what the step oracle calls."""
    import torch
    z = mu + eps * torch.exp(0.5 * logvar)
    logq = -0.5 * (LOG2PI + logvar + eps * eps).sum(1)
    diff = z[:, None, :] - p_mu[None, :, :]
    L = -0.5 * (LOG2PI + p_logvar[None] + diff * diff * torch.exp(-p_logvar)[None]).sum(2)
    logp = torch.logsumexp(L, dim=1) - math.log(p_mu.shape[0])
    rows = beta * (logq - logp)
    loss = rows if reduce == "none" else rows.mean() if reduce == "mean" else rows.sum()
    return z, loss, logq, logp


def torch_log_prob(x, p_mu, p_logvar):
    import torch
    diff = x[:, None, :] - p_mu[None, :, :]
    L = -0.5 * (LOG2PI + p_logvar[None] + diff * diff * torch.exp(-p_logvar)[None]).sum(2)
    return torch.logsumexp(L, dim=1) - math.log(p_mu.shape[0])


# (B, K, D) of the stored cases: the issue's shapes, then the -1 / 0 / +1 edges of what csrc/vamp.hip tiles by.  Forward:
# 32 x 32 tiles of [B, K], D staged in chunks of 32 (log q: 64 columns a wave trip) -> B, K, D in {31, 32, 33}.  Backward,
# both parts: 16 rows (components) x 64 columns over chunks of 32 components (rows) -> B, K in {15, 16, 17} (and the 31 /
# 32 / 33 above), D in {63, 64, 65}.  Finish: 16 rows a block and trip turn L into r, at most 128 blocks (4096 rows take
# two trips); block 0 walks the rows 256 at a time and sums them in 256 runs -> B in {255, 256, 257}; the forward-only
# finish walks 8 x 256 rows a trip (4096 again).
SHAPES = [(1, 1, 1), (2, 3, 3), (5, 7, 10), (64, 500, 128), (33, 65, 130), (7, 9, 512), (4096, 8, 4), (3, 4096, 2),
          (31, 33, 31), (32, 32, 32), (33, 31, 33), (15, 17, 63), (16, 16, 64), (17, 15, 65), (255, 8, 3), (256, 9, 2),
          (257, 8, 2), (64, 50, 10)]
BETA = 0.75           # the stored losses' beta


def seed_of(B, K, D):
    return 1000003 * B + 1009 * K + D
