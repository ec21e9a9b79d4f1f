"""fp64 restatement of the label regulariser of the semi-supervised S2 objectives (Locatello et al. 2020, "Disentangling
Factors of Variation Using Few Labels"; disentanglement_lib's ``supervised_regularizer_xent`` / ``_l2`` / ``_cov``), the
yardstick of csrc/sup.hip: numpy for the kernel tests, torch (autograd, any dtype) as the independent expression and for
the step tests.  All three forms are SUMS over the labelled batch, not means.

    xent: t = y / K,  sup = sum_b sum_{f<F} (max(m, 0) - m t + log1p(exp(-|m|))),  m = mu[b, f];   d/dm = sigmoid(m) - t
    l2:   sup = sum_b sum_{f<F} (s mu[b, f] - y_bf)^2;                                             d/dm = 2 s (s m - y)
    cov:  C = (1 / B) sum_b (mu_b - mean)(y_b - ybar)^T [D, F],  W = C with W_ii = 0,  sup = sum_ij W_ij^2;
          d/dmu[b, i] = (2 / B) sum_j W_ij (y_bj - ybar_j)
"""
import numpy as np

KINDS = ("xent", "l2", "cov")


def sup(mu, y, kind, factor_sizes=None, gamma=1.0, scale=1.0):
    """dict(loss = gamma * sup, sup, dmu = d loss / d mu [B, D]; cov also W [D, F])."""
    mu, y = np.asarray(mu, np.float64), np.asarray(y, np.float64)
    (B, D), F = mu.shape, y.shape[1]
    assert y.shape[0] == B and 1 <= F <= D
    dmu = np.zeros_like(mu)
    out = {}
    if kind == "xent":
        m = mu[:, :F]
        t = y / np.asarray(factor_sizes, np.float64)
        s = (np.maximum(m, 0.0) - m * t + np.log1p(np.exp(-np.abs(m)))).sum()
        e = np.exp(-np.abs(m))
        dmu[:, :F] = np.where(m >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e)) - t
    elif kind == "l2":
        d = scale * mu[:, :F] - y
        s = (d * d).sum()
        dmu[:, :F] = 2.0 * scale * d
    elif kind == "cov":
        X, Y = mu - mu.mean(0), y - y.mean(0)
        W = X.T @ Y / B
        k = min(D, F)
        W[np.arange(k), np.arange(k)] = 0.0
        s = (W * W).sum()
        dmu = (2.0 / B) * Y @ W.T                     # the centring term vanishes: sum_b Y_b = 0
        out["W"] = W
    else:
        raise ValueError(kind)
    g = float(gamma)
    out.update(loss=g * s if g != 0.0 else 0.0, sup=s, dmu=g * dmu if g != 0.0 else np.zeros_like(mu))
    return out


def torch_sup(mu, y, kind, factor_sizes=None, scale=1.0):
    """The unweighted term as an INDEPENDENT torch expression, differentiable by autograd in ``mu``'s dtype: torch's own
    binary cross-entropy with logits, a plain squared error, an explicit centred outer-product covariance."""
    import torch
    F = y.shape[1]
    y = y.to(mu.dtype)
    if kind == "xent":
        t = y / torch.tensor([float(k) for k in factor_sizes], dtype=mu.dtype, device=mu.device)
        return torch.nn.functional.binary_cross_entropy_with_logits(mu[:, :F], t, reduction="sum")
    if kind == "l2":
        return ((scale * mu[:, :F] - y) ** 2).sum()
    if kind == "cov":
        B, D = mu.shape
        xc, yc = mu - mu.mean(0, keepdim=True), y - y.mean(0, keepdim=True)
        C = (xc.unsqueeze(2) * yc.unsqueeze(1)).sum(0) / B
        k = min(D, F)
        mask = torch.ones_like(C)
        mask[torch.arange(k), torch.arange(k)] = 0.0
        return ((C * mask) ** 2).sum()
    raise ValueError(kind)


def gamma_sup(schedule, gamma, T, t):
    """The schedules of the weight, restated: fixed, anneal (a linear ramp over T steps), fine_tune (off until T, then a
    one-step ramp to gamma)."""
    if schedule == "fixed":
        return gamma
    if schedule == "anneal":
        return gamma * min(1.0, t / T)
    if schedule == "fine_tune":
        return gamma * min(1.0, max(0.0, t - T))
    raise ValueError(schedule)


def default_sizes(F):
    """Factor sizes 1, 3, 6, 10, 15, 40, 2, 4, ...: mixed, with a size-1 factor first."""
    base = (1, 3, 6, 10, 15, 40, 2, 4)
    return tuple(base[f % len(base)] for f in range(F))


def make_inputs(B, D, F, seed, spread=1.0):
    """The generator of the stored vectors: mu ~ spread * N(0, 1.5^2) plus a column offset, y integers uniform in
    [0, K_f) as fp32.  Returns (mu fp32 [B, D], y fp32 [B, F], sizes)."""
    rng = np.random.default_rng(seed)
    sizes = default_sizes(F)
    offset = rng.normal(0.0, 1.0, size=D)
    mu = (spread * (rng.normal(size=(B, D)) * 1.5 + offset)).astype(np.float32)
    y = np.stack([rng.integers(0, k, size=B) for k in sizes], axis=1).astype(np.float32)
    return mu, y, sizes


def make_big_inputs(B, D, F, seed):
    """``make_inputs`` at 25 times the spread, clipped to |mu| <= 80, with +80 and -80 present among the first F columns:
    exp(80) overflows fp32, so a softplus written as log(1 + exp(m)) in fp32 would."""
    mu, y, sizes = make_inputs(B, D, F, seed, spread=25.0)
    mu = np.clip(mu, -80.0, 80.0)
    mu[0, 0], mu[B - 1, F - 1] = 80.0, -80.0
    if B == 1 and F == 1:
        mu[0, 0] = 80.0
    return mu.astype(np.float32), y, sizes
