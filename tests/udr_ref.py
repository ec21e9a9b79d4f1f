"""numpy fp64 restatement of the UDR rules of include/itcv_hip.h (csrc/udr.hip, hipvae/disentangle.py): doubled
tie-averaged ranks, the Spearman and Lasso similarity matrices, relative strength and the ranking itself.  Plain loops where
the rule fixes an order; nothing here imports scipy, sklearn or the package."""
import numpy as np


def ref_cov(x):
    """C [D, D]: two passes over centred values, ddof = 1, the upper triangle mirrored (as tests/unsup_ref.py)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    xc = x - x.sum(0) / N
    C = xc.T @ xc / (N - 1)
    return np.triu(C) + np.triu(C, 1).T


def ref_ranks2(x):
    """fp32 [N, D]: L + H + 1 per column, L = #{smaller}, H = #{smaller or equal}: twice the tie-averaged rank.  The
    comparison is numeric (-0.0 == +0.0; numpy keeps denormals)."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.float32)
    for d in range(x.shape[1]):
        s = np.sort(x[:, d])
        L, H = np.searchsorted(s, x[:, d], side="left"), np.searchsorted(s, x[:, d], side="right")
        out[:, d] = (L + H + 1).astype(np.float32)
    return out


def ref_correlation(C):
    """R_kl = C_kl / sqrt(C_kk C_ll); the row and column of a column with C_kk == 0 are 0, the diagonal included."""
    d = np.diag(C)
    live = (d != 0)[:, None] & (d != 0)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        R = C / np.sqrt(d[:, None] * d[None, :])
    return np.where(live, R, 0.0)


def ref_spearman(a, b):
    """[Da, Db]: |R| of the cross block of the covariance of the doubled ranks of [a | b]."""
    Da = a.shape[1]
    R = ref_correlation(ref_cov(np.concatenate([ref_ranks2(a), ref_ranks2(b)], 1)))
    return np.abs(R[:Da, Da:])


def ref_lasso_cd(G, c, alpha=0.1, gtol=1e-12, max_sweeps=1000):
    """(w, sweeps, converged, v): cyclic coordinate descent in index order from 0 on 1/2 w'Gw - c'w + alpha |w|_1; after
    every sweep v = max_k (w_k != 0 ? |g_k + alpha sign w_k| : max(|g_k| - alpha, 0)), g = Gw - c; stop at v <= gtol."""
    D = len(c)
    w = np.zeros(D)
    sweeps, v = 0, np.inf
    while True:
        for k in range(D):
            if G[k, k] == 0.0:
                w[k] = 0.0
                continue
            rho = c[k] - (G[k] @ w - G[k, k] * w[k])
            w[k] = (rho - alpha if rho > alpha else (rho + alpha if rho < -alpha else 0.0)) / G[k, k]
        sweeps += 1
        g = G @ w - c
        v = np.where(w != 0, np.abs(g + alpha * np.sign(w)), np.maximum(np.abs(g) - alpha, 0.0)).max()
        if v <= gtol:
            return w, sweeps, True, v
        if sweeps >= max_sweeps:
            return w, sweeps, False, v


def ref_lasso_cov(C, Da, Db, alpha=0.1, gtol=1e-12, max_sweeps=1000, details=False):
    """W [Da, Db] = |w_t[k]| from the covariance C of [a | b]: for every column t of b the Lasso on the normalised
    covariance.  With ``details`` also (signed w [Da, Db], sweeps [Db], converged [Db], G, c [Da, Db])."""
    R = ref_correlation(np.asarray(C, dtype=np.float64))
    G, cs = R[:Da, :Da], R[:Da, Da:]
    w = np.zeros((Da, Db))
    sweeps, conv = np.zeros(Db, dtype=int), np.zeros(Db, dtype=bool)
    for t in range(Db):
        w[:, t], sweeps[t], conv[t], _ = ref_lasso_cd(G, cs[:, t], alpha, gtol, max_sweeps)
    return (np.abs(w), w, sweeps, conv, G, cs) if details else np.abs(w)


def ref_lasso(a, b, alpha=0.1, gtol=1e-12, max_sweeps=1000, details=False):
    """``ref_lasso_cov`` of the covariance of the fp32 columns [a | b]."""
    C = ref_cov(np.concatenate([np.asarray(a, np.float32), np.asarray(b, np.float32)], 1))
    return ref_lasso_cov(C, a.shape[1], b.shape[1], alpha, gtol, max_sweeps, details)


def _ordered_sum(t):
    tot = np.array(t[0], dtype=np.float64)
    for part in t[1:]:
        tot = tot + part
    return tot


def ref_relative_strength(corr):
    """(sx + sy) / 2, sx = mean_j (max_i c_ij)^2 / sum_i c_ij, sy the same over rows; a term whose sum is 0 counts as 0; no
    rows or no columns: nan.  Sums in index order."""
    corr = np.asarray(corr, dtype=np.float64)
    if corr.shape[0] == 0 or corr.shape[1] == 0:
        return float("nan")

    def side(c):
        top, tot = c.max(0), _ordered_sum(c)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(tot != 0, top * top / tot, 0.0)
        return _ordered_sum(term) / float(c.shape[1])

    return float((side(corr) + side(corr.T)) / 2.0)


def ref_kl(mu, logvar):
    mu, logvar = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return (0.5 * (mu * mu + np.exp(logvar) - logvar - 1.0)).mean(0)


def ref_median(values):
    v = sorted(values)
    n = len(v)
    if not n:
        return float("nan")
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def ref_udr(mus, logvars=None, correlation="lasso", kl_filter_threshold=0.01, alpha=0.1):
    """dict(model_scores, pairwise [M, M] (nan diagonal), raw {(i, j): [D_i, D_j]}, kl_masks, kl_divergence)."""
    M = len(mus)
    kls = None if logvars is None else [ref_kl(m, lv) for m, lv in zip(mus, logvars)]
    masks = [np.ones(m.shape[1], dtype=bool) for m in mus] if kls is None else [k > kl_filter_threshold for k in kls]
    pairwise, raw = np.full((M, M), np.nan), {}
    for i in range(M):
        for j in range(M):
            if i == j:
                continue
            raw[i, j] = ref_spearman(mus[i], mus[j]) if correlation == "spearman" else ref_lasso(mus[i], mus[j], alpha)
            pairwise[i, j] = ref_relative_strength(raw[i, j][masks[i]][:, masks[j]])
    scores = [ref_median([pairwise[j, i] for j in range(M) if j != i and not np.isnan(pairwise[j, i])]) for i in range(M)]
    return dict(model_scores=scores, pairwise=pairwise, raw=raw, kl_masks=masks, kl_divergence=kls)
