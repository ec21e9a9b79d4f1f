"""fp64 restatement of the sliced-Wasserstein autoencoder's KL hook (Kolouri et al. 2018) and of the sliced-Wasserstein
distance as a score (Deshpande et al. 2018), the yardstick of csrc/sw.hip: numpy for the kernel tests, torch (autograd, any
dtype) for the step tests.

    theta_l = t_l / |t_l|  (a row of norm 0 gives theta_l = 0)
    u_l[i] = theta_l . z_i,  v_l[i] = theta_l . p_i
    pi_l = the ascending order of u_l, ties broken by the smaller row index (np.argsort(kind="stable")); v_l sorted
    SW_l^2 = (1 / Bt) sum_i (u_l[pi_l(i)] - v_l(i))^2,  SW^2 = (1 / L) sum_l SW_l^2
    hook = beta * mean_b KL_b + lam * SW^2,   KL_b = -1/2 sum_d (1 + logvar - mu^2 - exp(logvar))
    G[l][pi_l(i)] = u_l[pi_l(i)] - v_l(i);  dSW^2 / dz_i = (2 / (L Bt)) sum_l G[l][i] theta_l
"""
import numpy as np


def directions(t):
    """Theta [L, D] fp64: the rows of t normalised, a zero row left zero."""
    t = np.asarray(t, np.float64)
    n = np.sqrt((t * t).sum(1, keepdims=True))
    return np.divide(t, n, out=np.zeros_like(t), where=n > 0)


def projections(z_all, prior, t):
    """(u [L, Bt], v [L, Bt], Theta [L, D]) in fp64."""
    Theta = directions(t)
    return Theta @ np.asarray(z_all, np.float64).T, Theta @ np.asarray(prior, np.float64).T, Theta


def kl_rows(mu, logvar):
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum(1)


def distance(a, b, t):
    """dict(sw2, per [L], G [L, Bt], Theta [L, D], order [L, Bt]) of two sets of as many rows."""
    u, v, Theta = projections(a, b, t)
    L, Bt = u.shape
    order = np.argsort(u, axis=1, kind="stable")
    vs = np.sort(v, axis=1)
    diff = np.take_along_axis(u, order, 1) - vs
    G = np.empty_like(u)
    np.put_along_axis(G, order, diff, 1)
    per = (diff * diff).sum(1) / Bt
    return dict(sw2=per.sum() / L, per=per, G=G, Theta=Theta, order=order)


def sw(z_all, prior, t, mu, logvar, lam, beta):
    """dict(loss, terms = (mean KL, SW^2, max_l SW_l^2), per, G, Theta, dz, dmu, dlogvar): the hook and its gradients with
    respect to z_all [Bt, D] and this rank's mu / logvar [Bl, D]."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    d = distance(z_all, prior, t)
    (L, Bt), Bl = d["G"].shape, mu.shape[0]
    kl = kl_rows(mu, lv).mean()
    dz = lam * (2.0 / (L * Bt)) * (d["G"].T @ d["Theta"])
    if beta != 0.0:
        dmu, dlv = beta / Bl * mu, beta / Bl * (-0.5) * (1.0 - np.exp(lv))
    else:
        dmu, dlv = np.zeros_like(mu), np.zeros_like(lv)
    return dict(loss=(beta * kl if beta != 0.0 else 0.0) + lam * d["sw2"], terms=np.array([kl, d["sw2"], d["per"].max()]),
                per=d["per"], G=d["G"], Theta=d["Theta"], dz=dz, dmu=dmu, dlogvar=dlv)


def loss_only(z_all, prior, t, mu, logvar, lam, beta):
    return (beta * kl_rows(mu, logvar).mean() if beta != 0.0 else 0.0) + lam * distance(z_all, prior, t)["sw2"]


def min_gap(z_all, prior, t):
    """The smallest gap between adjacent sorted projections, of u and of v, relative to max |u|: the condition under which
    an evaluation with a projection error far below it sorts as the restatement does (inf for one row)."""
    u, v, _ = projections(z_all, prior, t)
    if u.shape[1] < 2:
        return np.inf
    gu, gv = np.diff(np.sort(u, axis=1), axis=1).min(), np.diff(np.sort(v, axis=1), axis=1).min()
    return min(gu, gv) / np.abs(u).max()


def central_differences(z_all, prior, t, mu, logvar, lam, beta, step):
    """Gradients of ``loss_only`` by central differences in fp64 with respect to (z_all, mu, logvar)."""
    base = [np.array(a, np.float64) for a in (z_all, mu, logvar)]
    out = []
    for k in range(3):
        g = np.zeros_like(base[k])
        for idx in np.ndindex(*g.shape):
            x = [a.copy() for a in base]
            x[k][idx] += step
            up = loss_only(x[0], prior, t, x[1], x[2], lam, beta)
            x[k][idx] -= 2 * step
            dn = loss_only(x[0], prior, t, x[1], x[2], lam, beta)
            g[idx] = (up - dn) / (2 * step)
        out.append(g)
    return out


def torch_hook(z, prior, t, mu, logvar, lam, beta):
    """The hook on torch tensors of any dtype, differentiable by autograd (single rank: the batch is the global batch).
    ``torch.sort(stable=True)`` is the order of the definition."""
    import torch
    prior, t = prior.detach().to(z.dtype), t.detach().to(z.dtype)
    n = t.norm(dim=1, keepdim=True)
    theta = torch.where(n > 0, t / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(t))
    u, _ = torch.sort(z @ theta.t(), dim=0, stable=True)
    v, _ = torch.sort(prior @ theta.t(), dim=0)
    sw2 = ((u - v) ** 2).mean(0).mean()
    kl = (-0.5 * (1.0 + logvar - mu * mu - logvar.exp()).sum(1)).mean()
    return beta * kl + lam * sw2


def make_inputs(Bt, D, L, seed):
    """The generator of the stored vectors: (z [Bt, D], prior [Bt, D], t [L, D], mu [Bt, D], logvar [Bt, D]), all fp32.  z
    columns alternate std 0.6 / 1.3 plus a column offset N(0, 0.5^2); mu as z's own draw of the same law; logvar ~
    N(-1.5, 0.5^2); prior and t ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    std = np.where(np.arange(D) % 2 == 0, 0.6, 1.3)
    offset = rng.normal(0.0, 0.5, size=D)
    z = (rng.normal(size=(Bt, D)) * std + offset).astype(np.float32)
    prior = rng.normal(size=(Bt, D)).astype(np.float32)
    t = rng.normal(size=(L, D)).astype(np.float32)
    mu = (rng.normal(size=(Bt, D)) * std + offset).astype(np.float32)
    lv = rng.normal(-1.5, 0.5, size=(Bt, D)).astype(np.float32)
    return z, prior, t, mu, lv
