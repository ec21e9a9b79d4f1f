"""fp64 restatement of the FactorVAE objective (Kim & Mnih 2018; disentanglement_lib's ``factor_vae``), the yardstick of
csrc/factor.hip and of the fused discriminator layers: numpy for the kernel tests, torch (autograd, any dtype) for the
step tests.

    z_perm[:, d] = z[order_d, d],  order_d = stable argsort of key_image(keys[:, d])
    D: x -> lrelu(x W_0^T + b_0) -> ... -> h W_L^T + b_L = logits [R, 2]     lrelu(a) = a if a > 0 else slope * a
    d_i = l_i0 - l_i1;  tc = mean_{i < R0} d_i
    d_loss = 0.5 mean_{i < R0} softplus(-d_i) + 0.5 mean_{i >= R0} softplus(d_i)      (CE with labels 0 / 1)
    d_acc  = share of the R rows whose argmax (the first of two equal logits) is their label
    softplus(x) = max(x, 0) + log1p(exp(-|x|)),  sigmoid(x) = exp(min(x, 0)) / (1 + exp(-|x|))
"""
import numpy as np


# ---- permutation -------------------------------------------------------------------------------------------------------
def key_image(keys):
    """The monotone uint32 image of fp32 keys: ascending in the numeric order of the floats, +0 and -0 on one value,
    negative-sign NaN below -inf and positive-sign NaN above +inf.  Defined for every bit pattern."""
    u = np.ascontiguousarray(keys, dtype=np.float32).view(np.uint32).copy()
    u[(u << np.uint32(1)) == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def permute_order(keys):
    """order[:, d]: the rows of column d in ascending key image, ties by row index."""
    return np.argsort(key_image(keys), axis=0, kind="stable")


def permute_dims(z, keys):
    z = np.asarray(z)
    return np.take_along_axis(z, permute_order(keys), axis=0)


# ---- the MLP -----------------------------------------------------------------------------------------------------------
def lrelu(a, slope):
    return np.where(a > 0, a, slope * a)


def mlp_forward(x, Ws, bs, slope):
    """(pre-activations of the hidden layers, their activations, logits), fp64."""
    h = np.asarray(x, np.float64)
    pres, acts = [], []
    for W, b in zip(Ws[:-1], bs[:-1]):
        a = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        h = lrelu(a, slope)
        pres.append(a)
        acts.append(h)
    return pres, acts, h @ np.asarray(Ws[-1], np.float64).T + np.asarray(bs[-1], np.float64)


def linear_lrelu(x, W, b, slope):
    a = np.asarray(x, np.float64) @ np.asarray(W, np.float64).T
    if b is not None:
        a = a + np.asarray(b, np.float64)
    return lrelu(a, slope)


def dgrad_lrelu(dy, W, y_prev, slope):
    """(dy W) o lrelu'(.) with the mask read from the activation's output: > 0 -> 1, else (zero included) slope."""
    g = np.asarray(dy, np.float64) @ np.asarray(W, np.float64)
    return g * np.where(np.asarray(y_prev, np.float64) > 0, 1.0, slope)


# ---- the head ------------------------------------------------------------------------------------------------------------
def softplus(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def head(logits, R0):
    """dict(tc, d_loss, d_acc, dl_tc [R0, 2] = d tc / d logits, dl_d [R, 2] = d d_loss / d logits (None when R == R0))."""
    l = np.asarray(logits, np.float64)
    R = l.shape[0]
    d = l[:, 0] - l[:, 1]
    tc = d[:R0].mean()
    w = np.full(R0, 1.0 / R0)
    out = dict(tc=tc, dl_tc=np.stack([w, -w], axis=1))
    correct = (d[:R0] >= 0).sum() + (d[R0:] < 0).sum()
    out["d_acc"] = correct / R
    if R == R0:
        out["d_loss"], out["dl_d"] = 0.5 * softplus(-d).mean(), None
        return out
    R1 = R - R0
    out["d_loss"] = 0.5 * softplus(-d[:R0]).mean() + 0.5 * softplus(d[R0:]).mean()
    w = np.concatenate([-0.5 / R0 * sigmoid(-d[:R0]), 0.5 / R1 * sigmoid(d[R0:])])
    out["dl_d"] = np.stack([w, -w], axis=1)
    return out


# ---- the two walks ---------------------------------------------------------------------------------------------------------
def factor(z, z_perm, Ws, bs, slope):
    """The objective on the stacked rows [z; z_perm] with every gradient: dict(logits, tc, d_loss, d_acc, dz = d tc / d z
    (the VAE walk: rows of z only, no parameter gradient), dW / db = lists of d d_loss / d parameters (the
    discriminator's walk: all rows, nothing to z))."""
    z = np.asarray(z, np.float64)
    x = np.concatenate([z, np.asarray(z_perm, np.float64)], axis=0)
    B, L = z.shape[0], len(Ws)
    pres, acts, logits = mlp_forward(x, Ws, bs, slope)
    out = head(logits, B)
    out["logits"] = logits
    W64 = [np.asarray(W, np.float64) for W in Ws]
    g = out["dl_tc"]
    for l in range(L - 1, 0, -1):
        g = (g @ W64[l]) * np.where(pres[l - 1][:B] > 0, 1.0, slope)
    out["dz"] = g @ W64[0]
    g = out["dl_d"]
    dW, db = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        inp = acts[l - 1] if l else x
        dW[l], db[l] = g.T @ inp, g.sum(0)
        if l:
            g = (g @ W64[l]) * np.where(pres[l - 1] > 0, 1.0, slope)
    out["dW"], out["db"] = dW, db
    return out


def values_only(z, z_perm, Ws, bs, slope):
    """(tc, d_loss) for central differences."""
    x = np.concatenate([np.asarray(z, np.float64), np.asarray(z_perm, np.float64)], axis=0)
    h = head(mlp_forward(x, Ws, bs, slope)[2], np.asarray(z).shape[0])
    return h["tc"], h["d_loss"]


# ---- torch forms (any dtype) -------------------------------------------------------------------------------------------------
def torch_permute(z, keys):
    """z (torch, any dtype) permuted by the fp32 keys: the restatement's order."""
    import torch
    order = torch.from_numpy(permute_order(keys.detach().cpu().float().numpy())).to(z.device)
    return torch.gather(z.detach(), 0, order)


def torch_logits(x, params, slope):
    import torch.nn.functional as F
    h = x
    for W, b in params[:-1]:
        h = F.leaky_relu(F.linear(h, W, b), slope)
    return F.linear(h, *params[-1])


def torch_hook(z, keys, mu, logvar, params, slope, gamma, beta):
    """(beta * mean KL + gamma * tc, d_loss, tc) on torch tensors of any dtype; ``params``: [(W, b), ...] of the dtype of
    z.  The hook's value is differentiable in z / mu / logvar with the parameters constant; d_loss is differentiable in
    the parameters with z and z_perm constant (build it from detached copies when both are walked)."""
    import torch
    import torch.nn.functional as F
    B = z.shape[0]
    frozen = [(W.detach(), b.detach()) for W, b in params]
    l = torch_logits(z, frozen, slope)
    tc = (l[:, 0] - l[:, 1]).mean()
    kl = (-0.5 * (1.0 + logvar - mu * mu - logvar.exp()).sum(1)).mean()
    x = torch.cat([z.detach(), torch_permute(z, keys)])
    l2 = torch_logits(x, params, slope)
    zeros, ones = (torch.zeros(B, dtype=torch.long, device=z.device), torch.ones(B, dtype=torch.long, device=z.device))
    d_loss = 0.5 * F.cross_entropy(l2[:B], zeros) + 0.5 * F.cross_entropy(l2[B:], ones)
    return beta * kl + gamma * tc, d_loss, tc


# ---- the generator of the stored vectors ---------------------------------------------------------------------------------------
def make_mlp(zdim, hidden, layers, seed):
    """[(W, b), ...] fp32 with torch's nn.Linear default law: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for both."""
    rng = np.random.default_rng(seed)
    Ws, bs, width = [], [], zdim
    for out in [hidden] * layers + [2]:
        bound = 1.0 / np.sqrt(width)
        Ws.append(rng.uniform(-bound, bound, size=(out, width)).astype(np.float32))
        bs.append(rng.uniform(-bound, bound, size=out).astype(np.float32))
        width = out
    return Ws, bs


def make_inputs(B, zdim, seed):
    """(z [B, zdim], keys [B, zdim]) fp32: z columns alternate std 0.6 / 1.3 plus a column offset ~ N(0, 0.5^2), keys ~
    N(0, 1)."""
    rng = np.random.default_rng(seed)
    std = np.where(np.arange(zdim) % 2 == 0, 0.6, 1.3)
    z = (rng.normal(size=(B, zdim)) * std + rng.normal(0.0, 0.5, size=zdim)).astype(np.float32)
    return z, rng.normal(size=(B, zdim)).astype(np.float32)


def make_logits(R0, seed, spread=3.0):
    """Head inputs [2 R0, 2] fp32: the label-0 rows lean to class 0 and the others to class 1 by 0.7, under noise of std
    ``spread`` -- so that the accuracy is strictly between 0 and 1 and |tc| is not small against mean |l0 - l1|.  For R0
    = 1 the two rows are set by hand (one right, one wrong)."""
    rng = np.random.default_rng(seed)
    l = rng.normal(0.0, spread, size=(2 * R0, 2))
    l[:R0, 0] += 0.7 * spread
    l[R0:, 1] += 0.7 * spread
    if R0 <= 2:
        l[0] = (1.5, -0.5)          # label 0, right
        l[-1] = (0.75, -0.25)       # label 1, wrong
    return l.astype(np.float32)
