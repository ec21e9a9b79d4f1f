"""The numpy fp64 restatement of the sample-quality rules of include/itcv_hip.h (csrc/quality.hip), shared by
tests/test_quality_ref_host.py (which pins it) and tests/test_hip_quality.py (which holds the kernels to it), and the
recipes of their inputs.  Free of torch."""
import functools

import numpy as np


def d2_matrix(a, b):
    """d2[i][j] = sum_d (a[i][d] - b[j][d])^2, accumulated over d in ascending order (the kernels' order)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.zeros((a.shape[0], b.shape[0]))
    for d in range(a.shape[1]):
        t = a[:, d][:, None] - b[:, d][None, :]
        out += t * t
    return out


def ref_radii(x, k, d2=None):
    """The (k + 1)-th smallest of every row of the full distance matrix, the row's own 0 included: a full sort."""
    d2 = d2_matrix(x, x) if d2 is None else d2
    return np.sort(d2, axis=1)[:, k].copy()


def ref_prdc(real, fake, k):
    """Everything itcv_prdc_counts writes, the four counts and the four scores (Python fractions of integers)."""
    drr, dff, drf = d2_matrix(real, real), d2_matrix(fake, fake), d2_matrix(real, fake)
    r2r, r2f = ref_radii(real, k, drr), ref_radii(fake, k, dff)
    inside = drf < r2r[:, None]
    hits = inside.sum(0).astype(np.int32)
    covered = (drf < r2f[None, :]).any(1).astype(np.int32)
    rmin = drf.min(1)
    N, M = drf.shape
    counts = (int((hits > 0).sum()), int(covered.sum()), int(hits.sum()), int((rmin < r2r).sum()))
    return dict(d2=drf, d2_real=drr, d2_fake=dff, r2_real=r2r, r2_fake=r2f, fake_hits=hits, real_covered=covered,
                real_min=rmin, counts=counts, precision=counts[0] / M, recall=counts[1] / N,
                density=counts[2] / (k * M), coverage=counts[3] / N)


def ref_poly(x, y, degree=3, gamma=None, coef0=1.0):
    """The three sums of the polynomial-kernel MMD from matmul, the unbiased estimate, and sum |kappa| of each sum."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    g = 1.0 / x.shape[1] if not gamma else float(gamma)
    N, M = x.shape[0], y.shape[0]
    kxx, kyy, kxy = ((g * (a @ b.T) + coef0) ** degree for a, b in ((x, x), (y, y), (x, y)))
    # the diagonal is left out BEFORE the sum: K.sum() - trace(K) would round at the size of the (larger) diagonal
    off = lambda K: K[~np.eye(len(K), dtype=bool)].sum()                           # noqa: E731
    aoff = lambda K: np.abs(K[~np.eye(len(K), dtype=bool)]).sum()                  # noqa: E731
    sxx, syy, sxy = off(kxx), off(kyy), kxy.sum()
    return dict(Sxx=sxx, Syy=syy, Sxy=sxy, mmd2=sxx / (N * (N - 1.0)) + syy / (M * (M - 1.0)) - 2.0 * sxy / (N * M),
                abs=(aoff(kxx), aoff(kyy), np.abs(kxy).sum()))


def ref_frechet(m1, c1, m2, c2, eps=0.0):
    """np.linalg.cholesky + eigvalsh: M = L^T (C2 + eps I) L with L L^T = C1 + eps I; raises LinAlgError when the first is
    not positive definite."""
    m1, m2, c1, c2 = (np.asarray(v, dtype=np.float64) for v in (m1, m2, c1, c2))
    D = len(m1)
    A, B = c1 + eps * np.eye(D), c2 + eps * np.eye(D)
    L = np.linalg.cholesky(A)
    M = L.T @ B @ L
    M = np.triu(M) + np.triu(M, 1).T
    eig = np.linalg.eigvalsh(M)
    trs = float(np.sqrt(np.maximum(eig, 0.0)).sum())
    dm = float(((m1 - m2) ** 2).sum())
    return dict(frechet=dm + np.trace(A) + np.trace(B) - 2.0 * trs, mean_term=dm, trace_real=float(np.trace(A)),
                trace_fake=float(np.trace(B)), trace_sqrt=trs, eig=eig, M=M)


def ref_cov(x):
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(0)
    xc = x - mean
    return mean, xc.T @ xc / (x.shape[0] - 1)


def frechet_bound(r, c1=None, c2=None):
    """The bound on tr sqrt of a result ``r`` of ref_frechet.  The Jacobi iteration leaves every eigenvalue within
    e = 1e-12 |M|_F (it stops at off_F <= 1e-14 |M|_F; the products that form M carry D 2^-53 |M|_F, far below), and
    |sqrt(max(l + d, 0)) - sqrt(max(l, 0))| <= min(|d| / sqrt(l), sqrt(|d|)), summed over the eigenvalues: for a positive
    definite M this is at most D e / sqrt(l_min), and it stays finite for the zero eigenvalue of a singular second
    covariance.  With ``c1, c2`` the covariances came from itcv_unsup_cov, whose stated error is 1e-12 sqrt(C_ii C_jj)
    per entry, so |dC|_F <= 1e-12 tr C; the eigenvalues of M are those of C1^1/2 C2 C1^1/2 and of C2^1/2 C1 C2^1/2, so
    they move by at most 1e-12 (l_max(C1) tr C2 + l_max(C2) tr C1), which is carried through the same way."""
    e = 1e-12 * np.linalg.norm(r["M"])
    if c1 is not None:
        e += 1e-12 * (np.linalg.eigvalsh(c1).max() * np.trace(c2) + np.linalg.eigvalsh(c2).max() * np.trace(c1))
    lam = np.maximum(r["eig"], 0.0)
    return float(np.minimum(e / np.sqrt(np.maximum(lam, 1e-300)), np.sqrt(e)).sum())


# ---- inputs --------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 2, 1, 1), (5, 9, 1, 1), (67, 45, 7, 3), (130, 131, 33, 5), (600, 515, 131, 5), (1100, 67, 512, 16),
          (100, 200, 64, 2)]
# the shapes at which the integer recipe is asserted to exercise every comparison (test_quality_ref_host.py)
RICH = [(130, 131, 33, 5), (600, 515, 131, 5), (1100, 67, 512, 16)]


def integer_features(N, M, D, seed=0):
    """Integer-valued fp32 rows on a 4-dimensional lattice: rint(4 randn(N, 4)) @ A, A in {-1, 0, 1}^(4 x D), the fakes from
    1.3 randn + 0.5.  Every d2 is an exact integer in any order of summation (|x| <= ~100, D <= 512: far below 2^53, and
    every entry is exact in fp32)."""
    rs = np.random.RandomState(1000 * D + N + seed)
    A = rs.randint(-1, 2, size=(4, D)).astype(np.float64)
    real = np.rint(4.0 * rs.randn(N, 4)) @ A
    fake = np.rint(4.0 * (1.3 * rs.randn(M, 4) + 0.5)) @ A
    return real.astype(np.float32), fake.astype(np.float32)


def gaussian_features(N, M, D, seed=0):
    """fp32 Gaussian rows; the fakes are wider and shifted so that the four scores are neither 0 nor 1 at small D."""
    rs = np.random.RandomState(77 * D + N + seed)
    real = rs.randn(N, D)
    fake = 1.1 * rs.randn(M, D) + 0.2
    return real.astype(np.float32), fake.astype(np.float32)


@functools.lru_cache(maxsize=None)
def restated(kind, N, M, D, k):
    """(real, fake, ref_prdc) of one recipe and shape: computed once, shared by the tests, never written to."""
    real, fake = (integer_features if kind == "integer" else gaussian_features)(N, M, D)
    return real, fake, ref_prdc(real, fake, k)


def near_boundary(r, rel=1e-12):
    """Number of (real, fake) pairs whose d2 lies within rel * r2 of one of the two radii it is compared with."""
    a = np.abs(r["d2"] - r["r2_real"][:, None]) <= rel * r["r2_real"][:, None]
    b = np.abs(r["d2"] - r["r2_fake"][None, :]) <= rel * r["r2_fake"][None, :]
    return int(a.sum() + b.sum())


def spd(D, seed):
    """tests/test_hip_unsup_scores.py's recipe: a covariance with eigenvalues in [1, 3]."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.randn(D, D))
    C = (Q * rs.uniform(1.0, 3.0, size=D)) @ Q.T
    return np.triu(C) + np.triu(C, 1).T
