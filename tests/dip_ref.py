"""fp64 restatement of the DIP-VAE-I / II KL hook (Kumar et al. 2018; disentanglement_lib's ``dip_vae``), the yardstick
of csrc/dip.hip: numpy for the kernel tests, torch (autograd, any dtype) for the step tests.

    m = mean_b mu_all[b],  X = mu_all - m,  C = X^T X / Bt  (divisor Bt)  [+ diag(mean_b exp(logvar_all[b])) for kind "ii"]
    reg  = lambda_od sum_{i != j} C_ij^2 + lambda_d sum_i (C_ii - 1)^2
    hook = beta * mean_{local rows} KL + reg,   KL_b = -1/2 sum_l (1 + logvar - mu^2 - exp(logvar))
"""
import numpy as np

KINDS = ("i", "ii")


def covariance(mu_all, logvar_all, kind, centred=True):
    """C in fp64: the centred two-pass form, or E[mu mu^T] - m m^T (which cancels in fp32; the two agree in fp64)."""
    mu = np.asarray(mu_all, np.float64)
    Bt = mu.shape[0]
    m = mu.mean(0)
    if centred:
        X = mu - m
        C = X.T @ X / Bt
    else:
        C = mu.T @ mu / Bt - np.outer(m, m)
    if kind == "ii":
        C = C + np.diag(np.exp(np.asarray(logvar_all, np.float64)).mean(0))
    elif kind != "i":
        raise ValueError(kind)
    return C


def kl_rows(mu, logvar):
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum(1)


def weights(C, lambda_od, lambda_d):
    """W = 2 lambda_od offdiag(C) + diag(2 lambda_d (C_ii - 1)) = d reg / d C (symmetric)."""
    W = 2.0 * lambda_od * C
    np.fill_diagonal(W, 2.0 * lambda_d * (np.diag(C) - 1.0))
    return W


def dip(mu_all, logvar_all, kind, lambda_od, lambda_d, beta=0.0, row_offset=0, Bl=None, centred=True):
    """dict(loss, terms = (mean KL of the local rows, off-diagonal term, diagonal term), C, W, dmu, dlogvar): the hook and
    its gradients with respect to the whole [Bt, D] pair."""
    mu, lv = np.asarray(mu_all, np.float64), np.asarray(logvar_all, np.float64)
    Bt, D = mu.shape
    Bl = Bt - row_offset if Bl is None else Bl
    loc = slice(row_offset, row_offset + Bl)
    C = covariance(mu, lv, kind, centred)
    d = np.diag(C)
    off = lambda_od * ((C * C).sum() - (d * d).sum())
    dia = lambda_d * ((d - 1.0) ** 2).sum()
    kl = kl_rows(mu[loc], lv[loc]).mean()
    W = weights(C, lambda_od, lambda_d)
    X = mu - mu.mean(0)
    dmu = (2.0 / Bt) * X @ W                         # the centring term vanishes: sum_b X_b = 0
    dlv = np.exp(lv) * np.diag(W) / Bt if kind == "ii" else np.zeros_like(lv)
    if beta != 0.0:
        dmu[loc] += beta / Bl * mu[loc]
        dlv[loc] += beta / Bl * (-0.5) * (1.0 - np.exp(lv[loc]))
    return dict(loss=(beta * kl if beta != 0.0 else 0.0) + off + dia, terms=np.array([kl, off, dia]), C=C, W=W, dmu=dmu,
                dlogvar=dlv)


def loss_only(mu_all, logvar_all, kind, lambda_od, lambda_d, beta=0.0, row_offset=0, Bl=None):
    return dip(mu_all, logvar_all, kind, lambda_od, lambda_d, beta, row_offset, Bl)["loss"]


def central_differences(mu_all, logvar_all, kind, lambda_od, lambda_d, beta=0.0, row_offset=0, Bl=None, h=1e-5):
    """(dmu, dlogvar) of ``loss_only`` by central differences in fp64."""
    mu, lv = np.array(mu_all, np.float64), np.array(logvar_all, np.float64)
    out = []
    for k in range(2):
        g = np.zeros_like(mu)
        for idx in np.ndindex(*mu.shape):
            pair = [mu.copy(), lv.copy()]
            pair[k][idx] += h
            up = loss_only(pair[0], pair[1], kind, lambda_od, lambda_d, beta, row_offset, Bl)
            pair[k][idx] -= 2 * h
            dn = loss_only(pair[0], pair[1], kind, lambda_od, lambda_d, beta, row_offset, Bl)
            g[idx] = (up - dn) / (2 * h)
        out.append(g)
    return out


def torch_hook(mu, logvar, kind, lambda_od, lambda_d, beta):
    """The hook on torch tensors of any dtype, differentiable by autograd (single rank: the batch is the global batch)."""
    import torch
    Bt = mu.shape[0]
    X = mu - mu.mean(0, keepdim=True)
    C = X.t() @ X / Bt
    if kind == "ii":
        C = C + torch.diag(logvar.exp().mean(0))
    elif kind != "i":
        raise ValueError(kind)
    d = torch.diagonal(C)
    reg = lambda_od * ((C * C).sum() - (d * d).sum()) + lambda_d * ((d - 1.0) ** 2).sum()
    kl = (-0.5 * (1.0 + logvar - mu * mu - logvar.exp()).sum(1)).mean()
    return beta * kl + reg


def make_inputs(Bt, D, seed):
    """The generator of the stored vectors: columns alternate std 0.5 / 1.6 plus a column offset, logvar ~ N(-1.5, 0.5^2)."""
    rng = np.random.default_rng(seed)
    std = np.where(np.arange(D) % 2 == 0, 0.5, 1.6)
    offset = rng.normal(0.0, 2.0, size=D)
    mu = (rng.normal(size=(Bt, D)) * std + offset).astype(np.float32)
    lv = rng.normal(-1.5, 0.5, size=(Bt, D)).astype(np.float32)
    return mu, lv
