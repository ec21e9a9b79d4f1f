"""fp64 restatement of the InfoVAE / MMD-VAE (Zhao et al. 2017) and WAE-MMD (Tolstikhin et al. 2018) KL hook, the
yardstick of csrc/mmd.hip: numpy for the kernel tests, torch (autograd, any dtype) for the step tests.

    d2(a, b) = sum_l (a_l - b_l)^2,  bandwidth h > 0 (default 2 D)
    "rbf": k = exp(-d2 / h), k' = -k / h
    "imq": k = sum_s C_s / (C_s + d2), k' = -sum_s C_s / (C_s + d2)^2, C_s = s h, s in SCALES
    S_zz = sum_{i != j} k(z_i, z_j) / (Bt (Bt - 1)),  S_pp = sum_{i != j} k(p_i, p_j) / (P (P - 1)),
    S_zp = sum_{i, j} k(z_i, p_j) / (Bt P),  MMD^2 = S_zz + S_pp - 2 S_zp  (unbiased; may be negative)
    hook = beta * mean_b KL_b + lam * MMD^2,   KL_b = -1/2 sum_l (1 + logvar - mu^2 - exp(logvar))
    A_ij = k'(d2(z_i, z_j)) 2 / (Bt (Bt - 1)) (A_ii = 0),  C_ij = k'(d2(z_i, p_j)) (-2) / (Bt P),  Wt = (A | C), rs = rows' sums
    dMMD^2 / dz_i = 2 (rs_i z_i - sum_j A_ij z_j - sum_j C_ij p_j)
"""
import numpy as np

KERNELS = ("rbf", "imq")
SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


def sqdist(a, b):
    """d2 in the difference form, fp64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for r in range(0, a.shape[0], 64):             # row blocks: the [64, P, D] differences, never [Bt, P, D]
        d = a[r:r + 64, None, :] - b[None, :, :]
        out[r:r + 64] = (d * d).sum(-1)
    return out


def kernel_values(d2, kernel, h):
    """(k, k') elementwise."""
    if kernel == "rbf":
        k = np.exp(-d2 / h)
        return k, -k / h
    if kernel != "imq":
        raise ValueError(kernel)
    k, kp = np.zeros_like(d2), np.zeros_like(d2)
    for s in SCALES:
        c = s * h
        k += c / (c + d2)
        kp -= c / (c + d2) ** 2
    return k, kp


def kl_rows(mu, logvar):
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum(1)


def _parts(z_all, prior, kernel, h):
    """(S_zz, S_pp, S_zp), k'(zz) with a zero diagonal, k'(zp): fp64."""
    z, p = np.asarray(z_all, np.float64), np.asarray(prior, np.float64)
    Bt, P = z.shape[0], p.shape[0]
    kzz, dzz = kernel_values(sqdist(z, z), kernel, h)
    kpp = kernel_values(sqdist(p, p), kernel, h)[0]
    kzp, dzp = kernel_values(sqdist(z, p), kernel, h)
    np.fill_diagonal(kzz, 0.0)
    np.fill_diagonal(kpp, 0.0)
    np.fill_diagonal(dzz, 0.0)
    return (kzz.sum() / (Bt * (Bt - 1)), kpp.sum() / (P * (P - 1)), kzp.sum() / (Bt * P)), dzz, dzp


def sums(z_all, prior, kernel, h):
    """(S_zz, S_pp, S_zp) in fp64."""
    return _parts(z_all, prior, kernel, h)[0]


def mmd(z_all, prior, mu, logvar, kernel, h, lam, beta):
    """dict(loss, terms = (mean KL, MMD^2, S_zz, S_pp, S_zp), Wt, rs, dz, dmu, dlogvar): the hook and its gradients with
    respect to z_all [Bt, D] and this rank's mu / logvar [Bl, D]."""
    z, p = np.asarray(z_all, np.float64), np.asarray(prior, np.float64)
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    Bt, P, Bl = z.shape[0], p.shape[0], mu.shape[0]
    (s_zz, s_pp, s_zp), dzz, dzp = _parts(z, p, kernel, h)
    mmd2 = s_zz + s_pp - 2.0 * s_zp
    kl = kl_rows(mu, lv).mean()
    A = dzz * (2.0 / (Bt * (Bt - 1)))
    C = dzp * (-2.0 / (Bt * P))
    Wt = np.concatenate([A, C], axis=1)
    rs = Wt.sum(1)
    dz = lam * 2.0 * (rs[:, None] * z - Wt @ np.concatenate([z, p], axis=0))
    if beta != 0.0:
        dmu, dlv = beta / Bl * mu, beta / Bl * (-0.5) * (1.0 - np.exp(lv))
    else:
        dmu, dlv = np.zeros_like(mu), np.zeros_like(lv)
    return dict(loss=(beta * kl if beta != 0.0 else 0.0) + lam * mmd2, terms=np.array([kl, mmd2, s_zz, s_pp, s_zp]), Wt=Wt,
                rs=rs, dz=dz, dmu=dmu, dlogvar=dlv)


def loss_only(z_all, prior, mu, logvar, kernel, h, lam, beta):
    s_zz, s_pp, s_zp = sums(z_all, prior, kernel, h)
    return (beta * kl_rows(mu, logvar).mean() if beta != 0.0 else 0.0) + lam * (s_zz + s_pp - 2.0 * s_zp)


def central_differences(z_all, prior, mu, logvar, kernel, h, lam, beta, step=1e-5, wrt=("z", "mu", "logvar")):
    """Gradients of ``loss_only`` by central differences in fp64, in the order of ``wrt`` (any of "z", "prior", "mu",
    "logvar")."""
    base = dict(z=np.array(z_all, np.float64), prior=np.array(prior, np.float64), mu=np.array(mu, np.float64),
                logvar=np.array(logvar, np.float64))
    out = []
    for name in wrt:
        g = np.zeros_like(base[name])
        for idx in np.ndindex(*g.shape):
            x = {k: v.copy() for k, v in base.items()}
            x[name][idx] += step
            up = loss_only(x["z"], x["prior"], x["mu"], x["logvar"], kernel, h, lam, beta)
            x[name][idx] -= 2 * step
            dn = loss_only(x["z"], x["prior"], x["mu"], x["logvar"], kernel, h, lam, beta)
            g[idx] = (up - dn) / (2 * step)
        out.append(g)
    return out


def torch_hook(z, prior, mu, logvar, kernel, h, lam, beta):
    """The hook on torch tensors of any dtype, differentiable by autograd (single rank: the batch is the global batch);
    ``h`` None: 2 D."""
    import torch
    D = z.shape[1]
    h = 2.0 * D if h is None else h
    prior = prior.detach().to(z.dtype)

    def ker(a, b):
        d = a[:, None, :] - b[None, :, :]
        d2 = (d * d).sum(-1)
        if kernel == "rbf":
            return torch.exp(-d2 / h)
        if kernel != "imq":
            raise ValueError(kernel)
        return sum((s * h) / (s * h + d2) for s in SCALES)

    Bt, P = z.shape[0], prior.shape[0]
    kzz, kpp, kzp = ker(z, z), ker(prior, prior), ker(z, prior)
    s_zz = (kzz.sum() - torch.diagonal(kzz).sum()) / (Bt * (Bt - 1))
    s_pp = (kpp.sum() - torch.diagonal(kpp).sum()) / (P * (P - 1))
    mmd2 = s_zz + s_pp - 2.0 * kzp.sum() / (Bt * P)
    kl = (-0.5 * (1.0 + logvar - mu * mu - logvar.exp()).sum(1)).mean()
    return beta * kl + lam * mmd2


def make_inputs(Bt, P, D, seed):
    """The generator of the stored vectors: (z [Bt, D], prior [P, D], mu [Bt, D], logvar [Bt, D]), all fp32.  z columns
    alternate std 0.6 / 1.3 plus a column offset N(0, 0.5^2); mu as z's own draw of the same law; logvar ~ N(-1.5, 0.5^2);
    prior ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    std = np.where(np.arange(D) % 2 == 0, 0.6, 1.3)
    offset = rng.normal(0.0, 0.5, size=D)
    z = (rng.normal(size=(Bt, D)) * std + offset).astype(np.float32)
    prior = rng.normal(size=(P, D)).astype(np.float32)
    mu = (rng.normal(size=(Bt, D)) * std + offset).astype(np.float32)
    lv = rng.normal(-1.5, 0.5, size=(Bt, D)).astype(np.float32)
    return z, prior, mu, lv
