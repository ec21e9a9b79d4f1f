"""Inputs, references and bounds for the three primitives of csrc/dense.h (block_cholesky, block_jacobi, the f64-MFMA
covariance pass), shared by tests/test_dense_cases_host.py (which proves that every input is what it claims to be and that
the restatements alone meet every bound with room) and tests/test_hip_dense.py (which holds the five launches to them).
numpy and mpmath only; free of torch.

No reference here is plain fp64 LAPACK.  Each is one of

* an exactly known answer: a symmetric matrix Q Lambda Q^T whose every entry is exact in fp64 (``exact_sym``), a circulant
  matrix whose eigenvalues are a cosine sum (``circulant``), a covariance of rows that are small integers after a
  per-column shift and power-of-two scale, taken in rationals (``cov_exact``);
* extended precision: mpmath at 200 bits (``mp_eigs``, D <= 48), np.longdouble for residuals and weighted sums; every such
  bound states the reference's own error and adds it.

u = 2^-53, gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1)."""
import functools
from fractions import Fraction

import mpmath
import numpy as np

import gmm_ref
import unsup_ref

U = 2.0 ** -53
UL = 2.0 ** -63                                   # half an ulp of np.longdouble's 64-bit mantissa, relative
LDS_DIM = 128                                     # kLdsMatrixDim: above it the matrix lies in global memory
MAX_DIM = 512                                     # kMatrixMaxDim
MAX_SWEEPS = unsup_ref.JACOBI_MAX_SWEEPS
assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble must carry a 64-bit mantissa here"


def gamma(n):
    return n * U / (1.0 - n * U)


def ld(a):
    return np.asarray(a, dtype=np.longdouble)


# ---- exactly representable symmetric matrices ------------------------------------------------------------------------------
def hadamard(n):
    """The Sylvester-Hadamard matrix of order n = 2^b, entries +-1 (int64); H H^T = n I."""
    H = np.ones((1, 1), dtype=np.int64)
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n
    return H


def block_sizes(D):
    """The powers of two of the binary expansion of D, descending."""
    return [1 << b for b in range(D.bit_length() - 1, -1, -1) if (D >> b) & 1]


def reflector(D):
    """v in {0, +-1}^D of the Householder reflector I - 2 v v^T / v^T v that ties the blocks of a D that is no power of
    two together (None for a power of two): support m = the largest power of two below D, spread evenly from index 0 to
    index D - 1, signs alternating."""
    m = 1 << (D.bit_length() - 1)
    if m == D:
        return None
    v = np.zeros(D, dtype=np.int64)
    v[(np.arange(m) * (D - 1)) // (m - 1)] = (-1) ** np.arange(m)
    assert np.abs(v).sum() == m
    return v


def basis(D):
    """(Qu int64 [D, D], col_scale [D], lm): Q = Qu diag(col_scale)^1/2 2^-lm is orthogonal.  Qu = (m I - 2 v v^T) Hb with Hb
    the block-diagonal of Sylvester-Hadamard matrices of block_sizes(D), col_scale = 1 / (the block's order), m = 2^lm the
    support of the reflector (lm = 0 and no reflector for a power of two)."""
    Hb = np.zeros((D, D), dtype=np.int64)
    scale = np.empty(D)
    o = 0
    for n in block_sizes(D):
        Hb[o:o + n, o:o + n] = hadamard(n)
        scale[o:o + n] = 1.0 / n
        o += n
    v = reflector(D)
    if v is None:
        return Hb, scale, 0
    m = int(np.abs(v).sum())
    return (m * np.eye(D, dtype=np.int64) - 2 * np.outer(v, v)) @ Hb, scale, m.bit_length() - 1


def exact_sym(D, num, s):
    """C = Q diag(num 2^-s) Q^T (fp64 [D, D]) in integer arithmetic, or None when an entry is not representable in fp64.
    Q = basis(D); the block of order n contributes H diag(lambda) H^T / n, the reflector the rank-two update
    C - (2 / m) (v w^T + w v^T) + (4 v^T w / m^2) v v^T with w = C v.  Every intermediate is an int64 in units of
    2^-(s + log2(largest block) + 2 log2 m), asserted to stay below 2^62."""
    num = np.asarray(num, dtype=np.int64)
    assert num.shape == (D,)
    sizes = block_sizes(D)
    l0 = sizes[0].bit_length() - 1
    v = reflector(D)
    lm = 0 if v is None else int(np.abs(v).sum()).bit_length() - 1
    if 8 * int(np.abs(num).max()) * sizes[0] * 4 ** lm >= 2 ** 62:
        return None
    A = np.zeros((D, D), dtype=np.int64)
    o = 0
    for n in sizes:
        H = hadamard(n)
        A[o:o + n, o:o + n] = (H @ (num[o:o + n, None] * H.T)) << (l0 - (n.bit_length() - 1))
        o += n
    E = s + l0
    if v is not None:
        w = A @ v
        a = int(v @ w)
        A = (A << (2 * lm)) - ((np.outer(v, w) + np.outer(w, v)) << (lm + 1)) + 4 * a * np.outer(v, v)
        E += 2 * lm
    C = np.ldexp(A.astype(np.float64), -E)
    if not np.array_equal(np.ldexp(C, E).astype(np.int64), A) or not np.isfinite(C).all():
        return None
    assert np.array_equal(C, C.T)
    return C


def span_bits(num):
    """Exponent of the highest set bit of any value minus the exponent of the lowest set bit of any non-zero value."""
    nz = [int(abs(v)) for v in np.asarray(num).tolist() if v]
    return max(v.bit_length() - 1 for v in nz) - min((v & -v).bit_length() - 1 for v in nz)


# spectra: (num int64 [D], s) with lambda = num 2^-s, as a function of D and a bit budget q
def spec_clusters(D, q=1):
    """Two clusters 1/2 and 3/2 of multiplicity D / 2 each: the mean of an even D is 1 (a unit diagonal at a power-of-two
    D); D = 1: the value 1."""
    if D == 1:
        return np.array([2], dtype=np.int64), 1
    return np.where(np.arange(D) % 2 == 0, 1, 3).astype(np.int64), 1


def spec_near(D, q=40):
    """Nearly equal: 1 + k 2^-q, k = +-1 .. +-D / 2 (and 0 for an odd D): the mean is exactly 1."""
    h = D // 2
    k = np.concatenate([np.arange(1, h + 1), -np.arange(1, h + 1), np.zeros(D - 2 * h, dtype=np.int64)])
    return (1 << q) + np.sort(k).astype(np.int64), q


def spec_graded(D, q=32):
    """Graded over 2^-q: 2^-(k mod (q + 1))."""
    return (1 << (q - np.arange(D) % (q + 1))).astype(np.int64), q


def spec_zeros(D, q=2):
    """min(5, D - 1) exact zeros, the rest (1 + k mod 7) / 4: rank deficiency."""
    nz = min(5, D - 1)
    num = 1 + np.arange(D) % 7
    num[(np.arange(nz) * (D - 1)) // max(nz - 1, 1)] = 0             # spread from index 0 to index D - 1
    assert (num == 0).sum() == nz
    return num.astype(np.int64), 2


SPECTRA = {"clusters": (spec_clusters, (1,)), "near": (spec_near, (40, 36, 32, 28, 24, 20, 16)),
           "graded": (spec_graded, (32, 28, 24, 20, 16, 12, 8)), "zeros": (spec_zeros, (2,))}


@functools.lru_cache(maxsize=None)
def exact_case(D, kind):
    """``dict(C, lam (ascending fp64, exact), num, s, q)`` of spectrum ``kind`` at the largest bit budget q at which every
    entry of C is exact in fp64 (the budgets of SPECTRA, descending; tests/test_dense_cases_host.py pins the q taken)."""
    fn, budgets = SPECTRA[kind]
    perm = np.random.RandomState(D).permutation(D)                # which column of Q takes which value: no pattern
    for q in budgets:
        num, s = fn(D, q)
        num = num[perm]
        C = exact_sym(D, num, s)
        if C is not None:
            lam = np.sort(np.ldexp(num.astype(np.float64), -s))
            C.setflags(write=False)
            return dict(C=C, lam=lam, num=num, s=s, q=q)
    raise AssertionError(f"no exact {kind} matrix at D = {D}")


def exact_product(D, num, s, rational=False):
    """Q diag(lambda) Q^T formed independently of exact_sym: as one product Qu diag(lambda col_scale) Qu^T 4^-lm in
    np.longdouble, or (``rational``) in Python integers.  Returns it as fp64 together with a flag: every entry converted
    without rounding."""
    Qu, scale, lm = basis(D)
    if rational:
        inv = np.rint(1.0 / scale).astype(np.int64)
        big = int(inv.max())
        Qo = Qu.astype(object)
        Lw = np.array([int(n) * (big // int(i)) for n, i in zip(num.tolist(), inv.tolist())], dtype=object)
        P = (Qo * Lw[None, :]).dot(Qo.T)                          # in units of 2^-s / (big 4^lm)
        den = (1 << s) * big * 4 ** lm
        C = np.array([[p / den for p in row] for row in P.tolist()], dtype=np.float64)
        back = all(Fraction(c) == Fraction(p, den) for rc, rp in zip(C.tolist(), P.tolist()) for c, p in zip(rc, rp))
        return C, back
    lam = np.ldexp(ld(num), -s) * ld(scale)
    P = np.ldexp((ld(Qu) * lam[None, :]) @ ld(Qu).T, -2 * lm)
    C = P.astype(np.float64)
    return C, bool(np.array_equal(ld(C), P))


def circulant(D):
    """(C, lam ascending fp64, err): the symmetric circulant matrix with first row c_0 = 1, c_j = c_{D - j} = ((7 j) mod 5 +
    1) 2^-e, e chosen so that the off-diagonal row sum is at most 1/2.  Unit diagonal, every entry non-zero and exact,
    eigenvalues lambda_t = sum_j c_j cos(2 pi j t / D) in [1/2, 3/2], equal in pairs (t and D - t).  The cosines come from
    mpmath at 200 bits rounded to np.longdouble and the sum is taken there: ``err`` = (D + 2) 2^-63 sum |c_j| bounds what
    that leaves."""
    assert D >= 3
    e = int(np.ceil(np.log2(5 * D))) + 1
    j = np.arange(D)
    jj = np.minimum(j, D - j)
    row = np.ldexp(((7 * jj) % 5 + 1).astype(np.float64), -e)
    row[0] = 1.0
    assert row[1:].sum() <= 0.5
    C = row[(j[:, None] - j[None, :]) % D]
    assert np.array_equal(C, C.T)
    with mpmath.workprec(200):
        cos = np.array([np.longdouble(mpmath.nstr(mpmath.cos(2 * mpmath.pi * r / D), 25)) for r in range(D)])
    lam = (ld(row)[None, :] * cos[(j[:, None] * j[None, :]) % D]).sum(1)
    err = (D + 2) * UL * float(row.sum())
    C.setflags(write=False)
    return C, np.sort(lam.astype(np.float64)), err + U * 1.5      # + the rounding of lambda to fp64


def generic_q(D, seed):
    rs = np.random.RandomState(1000 * D + seed)
    Q, _ = np.linalg.qr(rs.randn(D, D))
    return Q, rs


def mp_eigs(S):
    """Ascending eigenvalues of the symmetric fp64 S by mpmath.eigsy at 200 bits, rounded to fp64."""
    with mpmath.workprec(200):
        E = mpmath.eigsy(mpmath.matrix(S.tolist()), eigvals_only=True)
        return np.sort(np.array([float(v) for v in E]))


# ---- 1. Cholesky -------------------------------------------------------------------------------------------------------------
CHOL_DIMS = [1, 2, 3, 31, 32, 33, 127, 128, 129, 255, 511, 512]
SCALE_MAX_DIM = 129                                # the power-of-two scaling is sent along up to here
SCALE_EXP = 20                                     # |e_i| <= 20: (2^20)^2 cond 1e10 is far from over- and underflow


def sym(C):
    return np.tril(C) + np.tril(C, -1).T


def chol_ill(D):
    """A generic orthogonal Q with the spectrum logspace(-10, 0): cond 1e10 (D = 1: the value 0.37)."""
    Q, _ = generic_q(D, 1)
    lam = np.logspace(-10, 0, D) if D > 1 else np.array([0.37])
    return sym((Q * lam) @ Q.T)


def chol_well(D):
    Q, rs = generic_q(D, 2)
    return sym((Q * rs.uniform(1.0, 3.0, D)) @ Q.T)


def scale_exponents(D):
    return np.random.RandomState(77 + D).randint(-SCALE_EXP, SCALE_EXP + 1, D)


def scaled(C, e):
    """S C S with S = diag(2^e): exact."""
    return np.ldexp(C, e[:, None] + e[None, :])


@functools.lru_cache(maxsize=None)
def chol_batch(D):
    """[K, D, D]: the ill-conditioned matrix, the well-conditioned one, and up to SCALE_MAX_DIM the scaled ill-conditioned
    one."""
    mats = [chol_ill(D), chol_well(D)]
    if D <= SCALE_MAX_DIM:
        mats.append(scaled(mats[0], scale_exponents(D)))
    out = np.stack(mats)
    out.setflags(write=False)
    return out


def lower_product(L, X, transposed, bs=64):
    """The lower triangle of L X^T (``transposed``) or L X in np.longdouble for lower triangular L and X, block by block: the
    blocks that are zero are not multiplied (a sixth of the work of the full product at D = 512)."""
    D = L.shape[0]
    Ll, Xl = ld(L), ld(X)
    out = np.zeros((D, D), dtype=np.longdouble)
    cuts = list(range(0, D, bs)) + [D]
    nb = len(cuts) - 1
    for i in range(nb):
        ri = slice(cuts[i], cuts[i + 1])
        for j in range(i + 1):
            rj = slice(cuts[j], cuts[j + 1])
            ks = range(j + 1) if transposed else range(j, i + 1)
            acc = np.zeros((ri.stop - ri.start, rj.stop - rj.start), dtype=np.longdouble)
            for k in ks:
                rk = slice(cuts[k], cuts[k + 1])
                acc += Ll[ri, rk] @ (Xl[rj, rk].T if transposed else Xl[rk, rj])
            out[ri, rj] = acc
    return np.tril(out)


def chol_residual(C, L):
    """max over the lower triangle of |C - L L^T|_ij / (|L||L^T|)_ij, the product in np.longdouble; its own error, at most
    D 2^-63 (|L||L^T|)_ij, is ADDED to the ratio (so the figure is an upper bound on the true one)."""
    D = C.shape[0]
    R = np.abs(np.tril(ld(C)) - lower_product(L, L, True)).astype(np.float64)
    mag = np.abs(L) @ np.abs(L).T
    il = np.tril_indices(D)
    return float(np.max(R[il] / mag[il])) + D * UL


def inverse_residual(L, X):
    """max over the lower triangle of |L X - I|_ij / (|L||X|)_ij, likewise."""
    D = L.shape[0]
    R = np.abs(lower_product(L, X, False) - np.eye(D)).astype(np.float64)
    mag = np.abs(L) @ np.abs(X)
    il = np.tril_indices(D)
    return float(np.max(R[il] / mag[il])) + D * UL


def logdet_of(L):
    """(2 sum log L_ii in np.longdouble, the bound 4 D u sum |log L_ii| + 4 u of a fp64 sum of fp64 logarithms)."""
    dg = np.diag(L)
    lg = np.log(ld(dg))
    return float(2.0 * lg.sum()), 4 * len(dg) * U * float(np.abs(lg).sum()) + 4 * U


# failing pivots: (name, how the matrix is spoilt); j_in = an inner dimension past the first 32 x 32 update
def fail_matrix(C, kind):
    """A copy of the SPD ``C`` whose factorisation fails: ``neg0`` / ``neglast`` / ``neginner`` take twice the pivot off the
    diagonal element of dimension 0 / D - 1 / an inner one (the columns before it are untouched by a right-looking
    factorisation), ``inf`` puts +inf on the inner diagonal element, ``nan`` plants a NaN symmetrically below it: the first
    pivot it reaches fails."""
    D = C.shape[0]
    A = np.array(C)
    j = (2 * D) // 3
    if kind.startswith("neg"):
        L, fail = gmm_ref.cholesky(C)
        assert fail == -1
        k = {"neg0": 0, "neglast": D - 1, "neginner": j}[kind]
        A[k, k] -= 2.0 * L[k, k] ** 2
    elif kind == "inf":
        A[j, j] = np.inf
    elif kind == "nan":
        A[j, j // 2] = A[j // 2, j] = np.nan
    else:
        raise KeyError(kind)
    return A


FAIL_KINDS = ["neg0", "neglast", "neginner", "inf", "nan"]
FAIL_DIMS = [129, 512]


@functools.lru_cache(maxsize=None)
def fail_batch(D):
    """([5, D, D] of FAIL_KINDS on chol_well(D), the dimension unsup_ref.ref_cholesky_logdet reports for each)."""
    mats = np.stack([fail_matrix(chol_well(D), k) for k in FAIL_KINDS])
    dims = [unsup_ref.ref_cholesky_logdet(m)[1] for m in mats]
    mats.setflags(write=False)
    return mats, dims


MANY_K, MANY_D = 64, 129


@functools.lru_cache(maxsize=None)
def many_batch():
    """([64, 129, 129], fail dims [64]): component k is the well- (even k) or ill-conditioned (odd k) matrix under its own
    power-of-two scaling; every third one (k mod 3 == 1) fails, at dimension 0, D - 1 or an inner one in turn."""
    D = MANY_D
    base = [chol_well(D), chol_ill(D)]
    mats, dims = [], []
    for k in range(MANY_K):
        C = scaled(base[k % 2], np.random.RandomState(500 + k).randint(-8, 9, D))
        if k % 3 == 1:
            C = fail_matrix(C, ("neg0", "neglast", "neginner")[(k // 3) % 3])
        mats.append(C)
        dims.append(gmm_ref.cholesky(C)[1])
    out = np.stack(mats)
    out.setflags(write=False)
    return out, dims


# ---- 2. Jacobi ---------------------------------------------------------------------------------------------------------------
JACOBI_DIMS = [1, 2, 3, 4, 5, 127, 128, 129, 130, 255, 256, 511, 512]
RESTATED_MAX_DIM = 130                             # unsup_ref.ref_jacobi runs up to here (D = 512 would take a minute)
# K of the eigenvalue bound (1e-14 + K D u) |A|_F: 16 x the largest error of unsup_ref.ref_jacobi over every case of
# D <= 130 in units of D u |A|_F.  Measured by tests/test_dense_cases_host.py::test_jacobi_restatement_pins_k: 0.2 (one
# ulp of an eigenvalue at D = 4 and 5, frechet-zeros-D5 the largest; the largest at D >= 127 is 0.049, frechet-zeros-D129).
K_MEASURED = 0.2
K_JACOBI = 16 * K_MEASURED
A_PRIORI_SWEEPS = 8                                # the ceiling K D u <= 8 sweeps (D - 1) u: one rounding a rotation touched


def eig_bound(D, fro):
    """|sorted eigenvalue - exact| <= (1e-14 + K D u) |A|_F: the first term is the stopping rule (a diagonal is within off_F
    of the spectrum, Weyl), the second the rotations' rounding."""
    return (unsup_ref.JACOBI_TOL + K_JACOBI * D * U) * fro


def sqrt_sum_bound(lam, e):
    """sum over the eigenvalues of |sqrt(max(l + d, 0)) - sqrt(l)| for |d| <= e: min(e / sqrt(l), sqrt(e)) each."""
    lam = np.maximum(np.asarray(lam, np.float64), 0.0)
    return float(np.minimum(e / np.sqrt(np.maximum(lam, 1e-300)), np.sqrt(e)).sum())


# (kernel, D, kind).  gauss needs an exactly unit diagonal (then S = D^1/2 C D^1/2 = C exactly): the exact matrices at a
# power-of-two D with a spectrum of mean 1, the circulant matrix at every other D >= 3.  frechet runs C1 = 4 I (L = 2 I and
# M = 4 C2 exactly), which leaves C2 free.  From D = 255 on: one spectrum per kernel and D.
JACOBI_CASES = (
    [("gauss", D, k) for D in (1, 2, 4, 128) for k in ("clusters", "near")]
    + [("gauss", D, "circulant") for D in (3, 5, 127, 129, 130)]
    + [("gauss", D, "generic") for D in (2, 3, 4, 5, 48)]
    + [("gauss", 5, "diagonal"), ("gauss", 129, "diagonal")]
    + [("frechet", D, k) for D in (1, 2, 3, 4, 5) for k in ("clusters", "near", "graded", "zeros")]
    + [("frechet", 127, "zeros"), ("frechet", 127, "clusters"), ("frechet", 128, "graded"), ("frechet", 128, "near"),
       ("frechet", 129, "near"), ("frechet", 129, "zeros"), ("frechet", 130, "clusters"), ("frechet", 130, "graded")]
    + [("frechet", D, "generic") for D in (2, 3, 4, 5, 48)]
    + [("frechet", 5, "diagonal"), ("frechet", 129, "diagonal")]
)
BIG_JACOBI_CASES = [("gauss", 255, "circulant"), ("gauss", 256, "clusters"), ("gauss", 511, "circulant"),
                    ("gauss", 512, "near"), ("frechet", 255, "zeros"), ("frechet", 256, "graded"),
                    ("frechet", 511, "clusters"), ("frechet", 512, "zeros")]


def case_id(c):
    return f"{c[0]}-{c[2]}-D{c[1]}"


@functools.lru_cache(maxsize=None)
def jacobi_case(kernel, D, kind):
    """``dict(C, A, lam, ref_err, nzero, diag)``: ``C`` the matrix handed to the kernel (gauss: the covariance; frechet: the
    second covariance, the first is 4 I), ``A`` the matrix the sweep runs on (C, or 4 C: exact either way), ``lam`` its
    eigenvalues ascending, ``ref_err`` the absolute error of ``lam`` itself."""
    ref_err, diag = 0.0, False
    if kind == "circulant":
        C, lam, ref_err = circulant(D)
    elif kind == "generic":
        Q, rs = generic_q(D, 3)
        C = sym((Q * rs.uniform(0.5, 2.0, D)) @ Q.T)
        if kernel == "gauss":
            lam = mp_eigs(unsup_ref.ref_scaled(C))
        else:
            lam = mp_eigs(C)
        ref_err = U * float(np.abs(lam).max())                       # 200 bits rounded to fp64
    elif kind == "diagonal":
        d = np.ldexp(1.0, 2 * ((np.arange(D) * 5) % 7 - 3))           # powers of 4: sqrt(d) d sqrt(d) = d^2 exactly
        C, lam, diag = np.diag(d), np.sort(d * d if kernel == "gauss" else d), True
    else:
        ec = exact_case(D, kind)
        C, lam = ec["C"], ec["lam"]
    if kernel == "gauss":
        A = unsup_ref.ref_scaled(C)
        if not diag and kind != "generic":
            assert np.array_equal(np.diag(C), np.ones(D)) and np.array_equal(A, C), (D, kind)
    else:
        A, lam, ref_err = 4.0 * C, 4.0 * lam, 4.0 * ref_err
    return dict(C=C, A=A, lam=lam, ref_err=ref_err, nzero=int((lam == 0.0).sum()), diag=diag)


@functools.lru_cache(maxsize=None)
def jacobi_restated(kernel, D, kind):
    """(eigenvalues ascending, sweeps, converged) of unsup_ref.ref_jacobi on the case's A."""
    eig, sweeps, conv = unsup_ref.ref_jacobi(jacobi_case(kernel, D, kind)["A"])
    return np.sort(eig), sweeps, conv


def gauss_closed(case):
    """The closed forms of a unit-diagonal (or diagonal) gauss case: dict(tc, w, logdet, trace) from the eigenvalues of C.
    With a unit diagonal sum log C_ii = 0 and tr C = D exactly; a diagonal C = diag(d) has S = diag(d^2), so tc = w = 0."""
    C, lam = case["C"], ld(case["lam"])
    D = C.shape[0]
    if case["diag"]:
        d = ld(np.diag(C))
        logdet, sumlog, tr, ws = np.log(d).sum(), np.log(d).sum(), d.sum(), d.sum()
    else:
        logdet, sumlog, tr, ws = np.log(lam).sum(), ld(0.0), ld(D), np.sqrt(lam).sum()
    return dict(tc=float(0.5 * (sumlog - logdet)), w=float(2 * tr - 2 * ws), logdet=float(logdet), trace=float(tr))


def logdet_bound(C, lam):
    """|logdet from the computed Cholesky factor - sum log lambda|: the factor is exact for C + dC, |dC| <= gamma(D + 1)
    |L||L^T| (Higham Thm 10.3), | |L||L^T| |_F <= | |L| |_F^2 = tr C, and logdet moves by tr(C^-1 dC) <= |C^-1|_F |dC|_F
    to first order (1.01 for the rest); then the fp64 sum of logarithms, 4 D u sum |log L_ii| + 4 u."""
    D = C.shape[0]
    L, fail = gmm_ref.cholesky(C)
    assert fail == -1
    return 1.01 * gamma(D + 1) * float(np.trace(C)) * float(np.sqrt((1.0 / lam ** 2).sum())) + logdet_of(L)[1]


# ---- 3. covariance pass ------------------------------------------------------------------------------------------------------
COV_N = [2, 3, 4, 5, 511, 512, 513, 2049, 32769, 70001]
COV_D = [1, 15, 16, 17, 63, 64, 65]
COV_KINDS = ["offset", "scales", "integer"]
WIDE = (67, 512)                                   # 32 x 33 / 2 = 528 tile pairs
SLICES = {2049: (412, 5), 32769: (516, 64), 70001: (1096, 64)}   # N: (rows a slice, slices) by hand from cov_slice_rows


@functools.lru_cache(maxsize=None)
def cov_input(kind, N, D):
    """``dict(x fp32 [N, D], y, c, e)`` with x[n][d] = (c + y[n][d]) 2^e[d] exactly, y integer-valued (fp64), c an integer:
    offset   fp32 rows of mean 1000 and sd 0.01 (one ulp is 2^-14 there: c = 1000 2^14, e = -14);
    scales   small dyadic values (|y| <= 2^11, e = -8) under column scales that differ by up to 2^40;
    integer  integers |y| <= 1000 around 37 whose column sums are multiples of N: an exactly integer mean."""
    rs = np.random.RandomState(31 * N + D + 7 * COV_KINDS.index(kind))
    if kind == "offset":
        x = (1000.0 + 0.01 * rs.randn(N, D)).astype(np.float32)
        c, e = 1000 << 14, np.full(D, -14)
        y = np.ldexp(x.astype(np.float64), 14) - c
    elif kind == "scales":
        y = np.clip(np.rint(256.0 * rs.randn(N, D)), -2048, 2048)
        c, e = 0, -8 + (13 * np.arange(D)) % 41
        if D > 1:
            e[-1] = 32
        x = np.ldexp(y, e[None, :]).astype(np.float32)
    else:
        y = rs.randint(-999, 1000, (N, D)).astype(np.float64)
        r = (y.sum(0) % N).astype(np.int64)                           # take 1 off the first r rows of each column
        y -= (np.arange(N)[:, None] < r[None, :])
        c, e = 37, np.zeros(D, dtype=np.int64)
        x = (y + c).astype(np.float32)
    assert np.array_equal(y, np.rint(y)) and np.array_equal(np.ldexp(y + c, e[None, :]), x.astype(np.float64))
    x.setflags(write=False)
    return dict(x=x, y=y, c=c, e=e)


def cov_exact(inp):
    """(mean [D], C [D, D]): the ddof = 1 covariance of the EXACT fp32 values, each entry the correctly rounded fp64 of the
    rational (N sum y_i y_j - sum y_i sum y_j) / (N (N - 1)) 2^(e_i + e_j).  The two sums are integers below 2^53 (asserted),
    so fp64 adds them exactly in any order; the rest is Python integers, whose true division rounds correctly."""
    y, c, e = inp["y"], inp["c"], inp["e"]
    N, D = y.shape
    assert N * float(np.abs(y).max()) ** 2 < 2.0 ** 53
    S1 = [int(v) for v in y.sum(0)]
    S2 = [[int(v) for v in row] for row in (y.T @ y)]
    den = N * (N - 1)
    C = np.array([[(N * S2[i][j] - S1[i] * S1[j]) / den for j in range(D)] for i in range(D)])
    mean = np.array([(c * N + S1[i]) / N for i in range(D)])
    return np.ldexp(mean, e), np.ldexp(C, e[:, None] + e[None, :])


def cov_bounds(x, mean, C, w=None, nk=None):
    """(dmean [D], dC [D, D]) for a computed mean and covariance of fp32 rows x against an exact reference (mean, C):
    |dmean_i| <= gamma(N + 2) sum_n |r x_i| / nk, |dC_ij| <= gamma(N + 3) mag_ij + dm_i B_j + dm_j B_i, with b = x - mean,
    mag_ij = sum_n |r b_i| |b_j| / nk, B_j = sum_n r |b_j| / nk (tests/test_hip_gmm.py), r = 1 and nk = N (mean), N - 1
    (covariance) in the unweighted pass.  Weighted, the divisor nk is itself a sum of N roundings: + gamma(N) |m_i| and
    + gamma(N) |C_ij|.  Both carry one rounding of the reference (u |m_i|, u |C_ij|).  The sums of magnitudes are taken in
    fp64: sums of non-negative terms, right to N u relative, which the bound ignores."""
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    if w is None:
        r, n_mean, n_cov, extra = np.ones((N, 1)), float(N), float(N - 1), 0.0
    else:
        r, n_mean, n_cov, extra = w.reshape(N, 1), nk, nk, gamma(N)
    dm = gamma(N + 2) * (r * np.abs(x)).sum(0) / n_mean + (extra + U) * np.abs(mean) + 1e-300
    b = np.abs(x - mean)
    mag = (r * b).T @ b / n_cov
    B = (r * b).sum(0) / n_cov
    dC = gamma(N + 3) * mag + np.outer(dm, B) + np.outer(B, dm) + (extra + U) * np.abs(C) + 1e-300
    return dm, dC


# the weighted pass: (N, D, K).  (513, 17, 64) is the largest K; D + 1 crosses the 64-column tile of the column sums at 63 / 64
MSTEP_SHAPES = [(2, 1, 1), (5, 15, 2), (511, 16, 3), (513, 17, 64), (512, 63, 2), (2049, 64, 3), (2049, 65, 2),
                (32769, 17, 2), (70001, 16, 2)]
MSTEP_REG = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def mstep_input(N, D, K):
    """(x fp32 [N, D] of mean 1000 and sd 0.01, resp fp64 [N, K]): uniform responsibilities with a third of them exactly 0
    and a tenth 1e-300; the last component has its whole mass, 1.0, on one row."""
    x = cov_input("offset", N, D)["x"]
    rs = np.random.RandomState(17 * N + D + K)
    resp = rs.uniform(0.0, 1.0, (N, K))
    pick = rs.randint(0, 30, (N, K))
    resp[pick < 10] = 0.0
    resp[(pick >= 10) & (pick < 13)] = 1e-300
    resp[0, 0] = 0.75                                                 # no component is empty
    if K > 1 or N == 2:
        resp[:, K - 1] = 0.0
        resp[N // 2, K - 1] = 1.0
    resp.setflags(write=False)
    return x, resp


@functools.lru_cache(maxsize=None)
def mstep_exact(N, D, K):
    """(nk [K], means [K, D], cov [K, D, D], ref_dmean, ref_dcov) of the M-step rule on the exact fp32 values in
    np.longdouble, two passes; ``ref_d*`` bound the reference's own error: (N + 4) 2^-63 times the sum of magnitudes."""
    x, resp = mstep_input(N, D, K)
    xl, x64 = ld(x), x.astype(np.float64)
    nk, means, cov = np.empty(K), np.empty((K, D)), np.empty((K, D, D))
    rdm, rdc = np.empty((K, D)), np.empty((K, D, D))
    for k in range(K):
        r = ld(resp[:, k:k + 1])
        n = r.sum() + ld(gmm_ref.NK_GUARD)
        m = (r * xl).sum(0) / n
        b = xl - m
        c = (r * b).T @ b / n
        c[np.diag_indices(D)] += ld(MSTEP_REG)
        nk[k], means[k], cov[k] = float(n), m.astype(np.float64), c.astype(np.float64)
        b64 = np.abs(x64 - means[k])
        rdm[k] = (N + 4) * UL * (resp[:, k:k + 1] * np.abs(x64)).sum(0) / nk[k]
        rdc[k] = (N + 4) * UL * ((resp[:, k:k + 1] * b64).T @ b64 / nk[k]) + UL * MSTEP_REG * np.eye(D)
    return nk, means, cov, rdm, rdc


def mstep_bounds(N, D, K, k):
    """(dnk, dmean [D], dC [D, D]) of component k: cov_bounds weighted, plus the reference's own error."""
    x, resp = mstep_input(N, D, K)
    nk, means, cov, rdm, rdc = mstep_exact(N, D, K)
    dm, dC = cov_bounds(x, means[k], cov[k], w=resp[:, k], nk=nk[k])
    return gamma(N) * nk[k] + U * nk[k], dm + rdm[k], dC + rdc[k]
