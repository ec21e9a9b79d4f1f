"""numpy fp64 restatement of the unsupervised-score and IRS rules of include/itcv_hip.h (csrc/unsup_scores.hip,
hipvae/disentangle.py).  Plain loops where the rule fixes an order; nothing here imports scipy or the package."""
import numpy as np

MI_BINS = 20
JACOBI_TOL, JACOBI_MAX_SWEEPS = 1e-14, 60


def ref_cov(x):
    """(mean [D], C [D, D]): two passes over centred values, ddof = 1, the upper triangle mirrored."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    m = x.sum(0) / N
    xc = x - m
    C = xc.T @ xc / (N - 1)
    return m, np.triu(C) + np.triu(C, 1).T


def ref_cholesky_logdet(C):
    """(logdet, failed dimension or -1): right-looking Cholesky, a pivot <= 0 or non-finite fails."""
    A = np.array(C, dtype=np.float64)
    D = A.shape[0]
    for j in range(D):
        piv = A[j, j]
        if not (piv > 0.0) or not np.isfinite(piv):
            return np.nan, j
        l = np.sqrt(piv)
        A[j, j] = l
        A[j + 1:, j] = A[j + 1:, j] / l
        for i in range(j + 1, D):
            A[i, j + 1:i + 1] = A[i, j + 1:i + 1] - A[i, j] * A[j + 1:i + 1, j]
    s = 0.0
    for d in range(D):
        s += np.log(A[d, d])
    return 2.0 * s, -1


def ref_scaled(C):
    """S = D^1/2 C D^1/2: the lower triangle (sqrt(C_ii) C_ij) sqrt(C_jj), mirrored."""
    sd = np.sqrt(np.diag(C))
    S = (sd[:, None] * C) * sd[None, :]
    return np.tril(S) + np.tril(S, -1).T


def ref_jacobi(S):
    """(eigenvalues in index order, sweeps, converged): the round-robin cyclic Jacobi of the rule."""
    A = np.array(S, dtype=np.float64)
    D = A.shape[0]
    Dp = (D + 1) & ~1
    M = Dp - 1
    sweeps = 0
    while True:
        tot = np.sqrt((A * A).sum())
        off =np.sqrt(((A - np.diag(np.diag(A))) ** 2).sum())
        if off <= JACOBI_TOL * tot:
            return np.diag(A).copy(), sweeps, True
        if sweeps == JACOBI_MAX_SWEEPS:
            return np.diag(A).copy(), sweeps, False
        for r in range(M):
            rot = []
            for k in range(Dp // 2):
                a, b = (r, M) if k == 0 else ((r + k) % M, (r + M - k) % M)
                p, q = min(a, b), max(a, b)
                if q >= D or A[p, q] == 0.0:
                    continue
                app, aqq, apq = A[p, p], A[q, q], A[p, q]
                g = abs(apq)
                if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):   # negligible: the identity rotation
                    rot.append((p, q, 1.0, 0.0, app, aqq))
                    continue
                tau = (aqq - app) / (2.0 * apq)
                t = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                rot.append((p, q, c, t * c, app - t * apq, aqq + t * apq))
            for p, q, c, s, _, _ in rot:
                rp, rq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * rp - s * rq, s * rp + c * rq
            for p, q, c, s, npp, nqq in rot:
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                A[p, p], A[p, q], A[q, p], A[q, q] = npp, 0.0, 0.0, nqq
        sweeps += 1


def ref_gauss(C):
    """dict(tc, w, w_norm, trace, logdet, eig (index order), fail_dim, converged, sweeps) of a covariance."""
    C = np.asarray(C, dtype=np.float64)
    D = C.shape[0]
    logdet, fail = ref_cholesky_logdet(C)
    if fail >= 0:
        return dict(tc=np.nan, w=np.nan, w_norm=np.nan, trace=np.nan, logdet=np.nan, eig=np.full(D, np.nan),
                    fail_dim=fail, converged=True, sweeps=0)
    sumlog = tr = 0.0
    for d in range(D):
        sumlog += np.log(C[d, d])
        tr += C[d, d]
    eig, sweeps, conv = ref_jacobi(ref_scaled(C))
    ws = 0.0
    for d in range(D):
        ws += np.sqrt(max(eig[d], 0.0))
    w = 2.0 * tr - 2.0 * ws
    return dict(tc=0.5 * (sumlog - logdet), w=w, w_norm=w / tr, trace=tr, logdet=logdet, eig=eig, fail_dim=-1,
                converged=conv, sweeps=sweeps)


def ref_bins(x, bins=MI_BINS):
    """The project's binning rule (include/itcv_hip.h): bin numbers 1..bins of every column, fp64."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.int64)
    for d in range(x.shape[1]):
        lo, hi = float(x[:, d].min()), float(x[:, d].max())
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        w = (hi - lo) / bins
        col = x[:, d].astype(np.float64)
        out[:, d] = sum((col >= lo + j * w).astype(np.int64) for j in range(bins))
    return out


def ref_mi_pair(a, b, bins=MI_BINS):
    """Mutual information in nats of two columns of 0-based bin numbers, from the joint table (itcv_disent_mi's form)."""
    N = len(a)
    tab = np.zeros((bins, bins), dtype=np.int64)
    np.add.at(tab, (a, b), 1)
    r, s = tab.sum(1), tab.sum(0)
    mi = 0.0
    for i in range(bins):
        for j in range(bins):
            c = tab[i, j]
            if c > 0:
                mi += (c / N) * (np.log(c) - np.log(r[i]) - np.log(s[j]) + np.log(N))
    return max(mi, 0.0)


def ref_mi_matrix(x):
    """(MI [D, D], score): the upper triangle computed and mirrored; score = sum_{i != j} MI / (D^2 - D), nan for D = 1."""
    b = ref_bins(x) - 1
    D = b.shape[1]
    mi = np.zeros((D, D))
    for i in range(D):
        for j in range(i, D):
            mi[i, j] = mi[j, i] = ref_mi_pair(b[:, i], b[:, j])
    off = mi - np.diag(np.diag(mi))
    with np.errstate(invalid="ignore", divide="ignore"):
        score = np.float64(off.sum()) / np.float64(D * D - D)
    return mi, float(score)


def ref_quantile(a_sorted, q):
    """np.percentile's linear rule on an ascending fp64 array."""
    n = len(a_sorted)
    h = (n - 1) * q
    lo = int(np.floor(h))
    t = h - lo
    hi = min(lo + 1, n - 1)
    alo, ahi = a_sorted[lo], a_sorted[hi]
    return alo + (ahi - alo) * t if t < 0.5 else ahi - (ahi - alo) * (1.0 - t)


def ref_irs(x, factors, sizes, q=0.99):
    """dict(avg_score, num_active_dims, active, max_deviations [D], cum [D, K], IRS_matrix [D, K], scores [D], parents
    [D]) over ALL dimensions (``active``: the mask min < max; the rows of an inactive dimension are 0 in IRS_matrix)."""
    x32 = np.asarray(x, dtype=np.float32)
    x = x32.astype(np.float64)
    factors = np.asarray(factors)
    N, D = x.shape
    K = len(sizes)
    active = x32.min(0) < x32.max(0)
    m = x.sum(0) / N
    maxdev = np.abs(x - m).max(0)
    cum = np.zeros((D, K))
    for k in range(K):
        tot = np.zeros(D)
        present = 0
        for v in range(int(sizes[k])):
            G = x[factors[:, k] == v]
            n = len(G)
            if n == 0:
                continue
            present += 1
            e = G.sum(0) / n
            a = np.sort(np.abs(G - e), axis=0)
            tot = tot + np.array([ref_quantile(a[:, d], q) for d in range(D)])
        cum[:, k] = tot / present
    M = np.zeros((D, K))
    scores, parents = np.zeros(D), np.zeros(D, dtype=np.int64)
    num = den = 0.0
    for d in range(D):
        if not active[d]:
            continue
        M[d] = 1.0 - cum[d] / maxdev[d]
        parents[d] = int(np.argmax(M[d]))
        scores[d] = M[d, parents[d]]
        num += scores[d] * maxdev[d]
        den += maxdev[d]
    na = int(active.sum())
    return dict(avg_score=(num / den) if na else 0.0, num_active_dims=na, active=active, max_deviations=maxdev, cum=cum,
                IRS_matrix=M, scores=scores, parents=parents)
