"""A numpy fp64 restatement of the Gaussian-mixture kernels (csrc/gmm.hip; rules: include/itcv_hip.h), and the inputs the
tests share.  Every sum over rows and every sum over columns is taken in the kernels' order, so that wherever the device
adds in a documented order the restatement adds in the same one:

* the M-step's column sums: per slice of ``slice_rows(N)`` rows, four interleaved sequential sums (rows r0 + w, r0 + w + 4,
  ...) added in wave order, the slices folded ascending;
* the factor: the right-looking Cholesky loop and the right-looking forward substitution, element by element;
* |y|^2 of the E-step in ascending column order, the log-sum-exp over ascending k, the block sums of the log-likelihood
  (the xor butterfly of a wave, the four waves in order) folded in block order;
* the sampler's sum over ascending columns.

Only the two matrix-core products (y = Linv (x - m), and the centred covariance of a slice) have no documented order inside
one v_mfma_f64_16x16x4_f64; the restatement takes numpy's product there and hands the tests sum |terms| to bound the
difference with."""
import functools

import numpy as np

U = 2.0 ** -53
LOG2PI = 1.8378770664093453                     # kLog2Pi of csrc/gmm.hip
NK_GUARD = 10.0 * np.finfo(np.float64).eps
SLICE_ROWS, MAX_SLICES = 512, 64

# (N, D, K): what each crosses is listed in tests/test_hip_gmm.py
SHAPES = [(7, 1, 1), (40, 3, 2), (600, 5, 3), (130, 17, 3), (300, 33, 4), (1100, 128, 5), (700, 131, 2), (1200, 512, 1)]
# the shapes a fit runs on: every component can keep Nk >= 2 D there ((1100, 128, 5) has 220 rows a component < 2 D, so it
# is exercised by the single launches only)
FIT_SHAPES = [s for s in SHAPES if s != (1100, 128, 5)]
# cluster separation of make_data and the seed of the k-means initialisation, where the defaults (3.0, 0) would let a
# component fall below 2 D rows
INPUTS = {(600, 5, 3): dict(sep=2.0, seed=0), (300, 33, 4): dict(sep=4.0, seed=2)}
KMEANS_ITERS = 4
FIT_ITERS = 20
FIT_EYE_TOL = 1e-7
ORDER_SENSITIVITY = 4e-15                       # measured and pinned by tests/test_gmm_ref_host.py
COND_MAX = 64.0                                 # |L_k|_2 |Linv_k|_2 of every factor of every test input stays below this


def cdiv(a, b):
    return -(-a // b)


def slice_rows(N):
    ns = min(cdiv(N, SLICE_ROWS), MAX_SLICES)
    return cdiv(cdiv(N, ns), 4) * 4


def make_data(N, D, K, seed=0, sep=3.0):
    """fp32 ``x [N, D]``: K Gaussian clusters of (almost) equal size with full covariances whose centres lie about
    ``sep * sqrt(2)`` standard deviations apart, so that neighbours overlap and EM takes several iterations; rows shuffled."""
    rng = np.random.default_rng([seed, N, D, K])
    sizes = [N // K + (1 if k < N % K else 0) for k in range(K)]
    parts = []
    for k, n in enumerate(sizes):
        A = np.eye(D) + 0.3 * rng.standard_normal((D, D)) / np.sqrt(D)
        centre = sep * rng.standard_normal(D) / np.sqrt(D)
        parts.append(centre + rng.standard_normal((n, D)) @ A.T)
    x = np.concatenate(parts, 0)
    return x[rng.permutation(N)].astype(np.float32)


def shape_input(N, D, K):
    """``(x, seed)`` of a shape of SHAPES: the rows and the seed its k-means initialisation uses."""
    cfg = INPUTS.get((N, D, K), {})
    return make_data(N, D, K, sep=cfg.get("sep", 3.0)), cfg.get("seed", 0)


def make_params(D, K, seed=0):
    """Well-conditioned mixture parameters ``(weights, means, covariances)`` for the single-launch tests."""
    rng = np.random.default_rng([seed, D, K, 7])
    w = rng.uniform(0.5, 1.5, K)
    w = w / w.sum()
    means = rng.standard_normal((K, D))
    cov = np.empty((K, D, D))
    for k in range(K):
        A = np.eye(D) + 0.4 * rng.standard_normal((D, D)) / np.sqrt(D)
        cov[k] = A @ A.T * rng.uniform(0.5, 2.0)
        cov[k] = 0.5 * (cov[k] + cov[k].T)
    return w, means, cov


# ---- M-step ------------------------------------------------------------------------------------------------------------
def _seq_sum(a):
    """Sequential sum along axis 0, from 0.0 (np.cumsum adds in order)."""
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a, axis=0)[-1] + 0.0


def row_sum(terms, N=None):
    """The kernels' sum over rows of ``terms [N, ...]``: slices, four interleaved waves, slices folded ascending."""
    N = terms.shape[0]
    rows = slice_rows(N)
    total = np.zeros(terms.shape[1:])
    for r0 in range(0, N, rows):
        sl = terms[r0:min(N, r0 + rows)]
        w = [_seq_sum(sl[i::4]) for i in range(4)]
        total = total + (((w[0] + w[1]) + w[2]) + w[3])
    return total


def mstep(x, resp, reg=0.0, with_cov=True, bounds=False):
    """``(nk, weights, means, covariances)`` of the M-step rule; ``bounds``: also sum |terms| of every covariance sum."""
    x = np.asarray(x, np.float64)
    N, D = x.shape
    K = resp.shape[1]
    nk = np.empty(K)
    means = np.empty((K, D))
    for k in range(K):
        nk[k] = row_sum(resp[:, k:k + 1])[0] + NK_GUARD
        means[k] = row_sum(resp[:, k:k + 1] * x) / nk[k]
    tot = 0.0
    for k in range(K):
        tot = tot + nk[k]
    w = nk / tot
    if not with_cov:
        return nk, w, means, None
    cov = np.empty((K, D, D))
    mag = np.empty((K, D, D))
    rows = slice_rows(N)
    for k in range(K):
        b = x - means[k]
        a = resp[:, k:k + 1] * b
        s, m = np.zeros((D, D)), np.zeros((D, D))
        for r0 in range(0, N, rows):
            s = s + a[r0:r0 + rows].T @ b[r0:r0 + rows]
            if bounds:
                m = m + np.abs(a[r0:r0 + rows]).T @ np.abs(b[r0:r0 + rows])
        s = np.triu(s) + np.triu(s, 1).T
        cov[k] = s / nk[k]
        cov[k][np.diag_indices(D)] += reg
        mag[k] = m / nk[k]
    return (nk, w, means, cov, mag) if bounds else (nk, w, means, cov)


# ---- factor ------------------------------------------------------------------------------------------------------------
def cholesky(C):
    """(L, fail): the right-looking loop of the kernel, the upper triangle zero; fail = -1 or the failed pivot's dimension."""
    A = np.array(C, np.float64)
    D = A.shape[0]
    for j in range(D):
        piv = A[j, j]
        if not (piv > 0.0) or not np.isfinite(piv):
            return np.full((D, D), np.nan), j
        l = np.sqrt(piv)
        A[j, j] = l
        A[j + 1:, j] = A[j + 1:, j] / l
        if j + 1 < D:
            col = A[j + 1:, j]
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.tril(np.outer(col, col))
    return np.tril(A), -1


def tri_inverse(L):
    D = L.shape[0]
    X = np.eye(D)
    for k in range(D):
        X[k, :k + 1] = X[k, :k + 1] / L[k, k]
        if k + 1 < D:
            X[k + 1:, :k + 1] = X[k + 1:, :k + 1] - np.outer(L[k + 1:, k], X[k, :k + 1])
    return X


def factor(cov):
    """``(chol, linv, logdet, info)`` of covariances ``[K, D, D]``."""
    K, D = cov.shape[:2]
    chol, linv = np.empty((K, D, D)), np.empty((K, D, D))
    logdet, info = np.empty(K), np.zeros(K, np.int32)
    for k in range(K):
        L, fail = cholesky(cov[k])
        if fail >= 0:
            chol[k], linv[k], logdet[k], info[k] = np.nan, np.nan, np.nan, 1 + fail
            continue
        s = 0.0
        for d in range(D):
            s = s + np.log(L[d, d])
        chol[k], linv[k], logdet[k] = L, tri_inverse(L), 2.0 * s
    return chol, linv, logdet, info


def condition(chol, linv):
    """max_k |L_k|_2 |Linv_k|_2."""
    return max(np.linalg.norm(chol[k], 2) * np.linalg.norm(linv[k], 2) for k in range(len(chol)))


# ---- E-step ------------------------------------------------------------------------------------------------------------
def logp(x, w, means, linv, logdet, bounds=False):
    """``lp [N, K]``; ``bounds``: also ``(ay, q)`` with ay[n, k, i] = sum_j |Linv[i][j]| |x[n][j] - m[j]| and q = |y|^2."""
    x = np.asarray(x, np.float64)
    N, D = x.shape
    K = len(w)
    lp, qs = np.empty((N, K)), np.empty((N, K))
    ays = np.empty((N, K, D)) if bounds else None
    for k in range(K):
        xc = x - means[k]
        if np.array_equal(linv[k], np.eye(D)):
            y = xc                                            # products with 0 and 1 are exact in any order
        else:
            y = xc @ np.tril(linv[k]).T
        q = np.zeros(N)
        for i in range(D):
            q = q + y[:, i] * y[:, i]
        qs[:, k] = q
        lp[:, k] = np.log(w[k]) - 0.5 * ((D * LOG2PI + logdet[k]) + q)
        if bounds:
            ays[:, k] = np.abs(xc) @ np.abs(np.tril(linv[k])).T
    return (lp, ays, qs) if bounds else lp


def block_sums(v):
    """The kernel's sum of ``v [N]``: per block of 256 rows the xor butterfly of each wave of 64, the four waves in order;
    the blocks folded ascending."""
    N = len(v)
    nb = cdiv(N, 256)
    pad = np.zeros(nb * 256)
    pad[:N] = v
    lanes = pad.reshape(nb, 4, 64)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, :, idx ^ o]
    total = 0.0
    for b in range(nb):
        r = 0.0
        for wv in range(4):
            r = r + lanes[b, wv, 0]
        total = total + r
    return total


def estep(x, w, means, linv, logdet, hard=False):
    """``(lp, resp, loglik, sum_loglik)``."""
    lp = logp(x, w, means, linv, logdet)
    N, K = lp.shape
    am = np.argmax(lp, axis=1)                                # the first of equal maxima, as the kernel's strict >
    m = lp[np.arange(N), am]
    if hard:
        resp = np.zeros((N, K))
        resp[np.arange(N), am] = 1.0
        lse = m
    else:
        s = np.zeros(N)
        for k in range(K):
            s = s + np.exp(lp[:, k] - m)
        lse = m + np.log(s)
        resp = np.exp(lp - lse[:, None])
    return lp, resp, lse, block_sums(lse)


# ---- Lloyd, fit ----------------------------------------------------------------------------------------------------------
def lloyd(x, K, iters, seed=0, reg=1e-6):
    """``dict(weights, means, covariances, centres, resp, gaps, history)``: the k-means initialisation of
    ``hipvae.density.kmeans_init``.  ``gaps``: per hard E-step the smallest relative gap between a row's two smallest
    distances (inf for K = 1); ``history``: the centres and assignments after every iteration."""
    x64 = np.asarray(x, np.float64)
    N, D = x64.shape
    seeds = np.random.RandomState(seed).choice(N, K, replace=False)
    centres = x64[seeds].copy()
    ones, zeros, eye = np.ones(K), np.zeros(K), np.broadcast_to(np.eye(D), (K, D, D))
    gaps, history = [], []

    def assign():
        resp = estep(x64, ones, centres, eye, zeros, hard=True)[1]
        if K > 1:
            q = np.sort(logp(x64, ones, centres, eye, zeros, bounds=True)[2], axis=1)[:, :2]
            gaps.append(float(np.min((q[:, 1] - q[:, 0]) / np.maximum(q[:, 1], 1e-300))))
        else:
            gaps.append(np.inf)
        return resp

    for _ in range(iters):
        resp = assign()
        nk, _, mean, _ = mstep(x64, resp, with_cov=False)
        centres = np.where((nk > 0.5)[:, None], mean, centres)
        history.append((centres.copy(), resp.argmax(1)))
    resp = assign()
    nk, w, mean, cov = mstep(x64, resp, reg)
    return dict(weights=w, means=mean, covariances=cov, centres=centres, resp=resp, gaps=gaps, history=history, nk=nk)


def fit(x, init, max_iter=100, tol=1e-3, reg=1e-6):
    """The EM iteration of ``hipvae.density.fit_gmm`` from ``init = (weights, means, covariances)``: a dict with the final
    parameters, ``history``, ``n_iter``, ``converged``, and per iteration the smallest ``nk`` and the largest condition."""
    x64 = np.asarray(x, np.float64)
    N = x64.shape[0]
    w, means, cov = (np.array(t, np.float64) for t in init)
    chol, linv, logdet, info = factor(cov)
    if info.any():
        raise ValueError(f"pivot {info}")
    history, prev, converged, nks, conds = [], -np.inf, False, [], [condition(chol, linv)]
    for _ in range(max_iter):
        _, resp, _, total = estep(x64, w, means, linv, logdet)
        nk, w, means, cov = mstep(x64, resp, reg)
        chol, linv, logdet, info = factor(cov)
        if info.any():
            raise ValueError(f"pivot {info}")
        nks.append(float(nk.min()))
        conds.append(condition(chol, linv))
        bound = total / N
        history.append(bound)
        if abs(bound - prev) < tol:
            converged = True
            break
        prev = bound
    return dict(weights=w, means=means, covariances=cov, chol=chol, linv=linv, logdet=logdet, history=history,
                n_iter=len(history), converged=converged, nk_min=nks, cond=conds)


def log_prob(params, x):
    return estep(x, params["weights"], params["means"], params["linv"], params["logdet"])[2]


@functools.lru_cache(maxsize=None)
def reference(N, D, K):
    """What the tests of one shape of FIT_SHAPES share, computed once and never written to: ``x``, ``seed``, ``lloyd`` (the
    k-means initialisation), ``fit`` (from it, tol = 1e-3) and ``fit_eye`` (from its weights and means with identity
    covariances, tol = FIT_EYE_TOL: more iterations)."""
    x, seed = shape_input(N, D, K)
    ll = lloyd(x, K, KMEANS_ITERS, seed)
    eye = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    return dict(x=x, seed=seed, lloyd=ll,
                fit=fit(x, (ll["weights"], ll["means"], ll["covariances"]), FIT_ITERS),
                fit_eye=fit(x, (ll["weights"], ll["means"], eye), FIT_ITERS, tol=FIT_EYE_TOL))


def rel_diff(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


# ---- sampler -----------------------------------------------------------------------------------------------------------
def sample(means, chol, comp, eps):
    """fp32 ``z [R, D]`` = (float)(m_c + sum_{j <= i} L_c[i][j] eps[j]), the sum in ascending j."""
    eps = np.asarray(eps, np.float64)
    R, D = eps.shape
    z = np.empty((R, D), np.float32)
    for c in np.unique(comp):
        rows = np.nonzero(comp == c)[0]
        L, e = chol[c], eps[rows]
        s = np.zeros((len(rows), D))
        for j in range(D):
            s[:, j:] = s[:, j:] + L[j:, j][None, :] * e[:, j:j + 1]
        z[rows] = (means[c][None, :] + s).astype(np.float32)
    return z
