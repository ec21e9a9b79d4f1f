"""The three primitives of csrc/dense.h on the device, through the five launches that reach them (itcv_gmm_factor,
itcv_unsup_gauss, itcv_frechet, itcv_unsup_cov, itcv_gmm_mstep), up to D = 512, against the references of
tests/dense_cases.py: exactly known answers, mpmath, np.longdouble; never fp64 LAPACK.  tests/test_dense_cases_host.py
shows on the CPU that every input is what it claims to be and that the numpy restatements meet every bound below with room.
u = 2^-53, gamma(n) = n u / (1 - n u).  Every test prints error / bound.

1. block_cholesky, through gmm_factor (L and X = L^-1), D in CHOL_DIMS (31 .. 33 cross the 32 x 32 update, 128 / 129 the LDS
   limit), a cond-1e10 matrix, a well-conditioned one and up to D = 129 a power-of-two scaling, several in one call:
   |C - L L^T|_ij <= gamma(D + 1) (|L||L^T|)_ij and |L X - I|_ij <= gamma(D) (|L||X|)_ij on the lower triangle (Higham,
   Accuracy and Stability, Thm 10.3 and 8.5: whatever the order and the conditioning), exact zeros above it, logdet against
   2 sum log L_ii of the returned L within 4 D u sum |log L_ii| + 4 u; factor(S C S) = S factor(C) byte for byte; the same
   logdet bytes from unsup_gauss; the spectrum of L^T L through frechet; K = 64 components of which every third fails; failing
   pivots at dimension 0, D - 1 and inside, an inf, a NaN, at D = 129 and 512 through all three callers.
2. block_jacobi, through unsup_gauss and frechet, D in JACOBI_DIMS, spectra: two clusters of multiplicity D / 2, 1 + k 2^-40,
   graded over 2^-32, five exact zeros, diagonal, circulant (equal pairs), generic (mpmath):  sorted eigenvalues within
   (1e-14 + K D u) |A|_F of the exact ones (K = dense_cases.K_JACOBI, 16 x what the restatement leaves); tc, w, logdet and
   tr sqrt against closed forms with that bound carried through; info[2] = 0; the sweeps of the restatement up to D = 130;
   scaling by 2^k scales every eigenvalue exactly; a second run gives the same bytes.  The unconverged branch is entered
   with a NaN in the second covariance.
3. The covariance pass, through unsup_cov and gmm_mstep: N in COV_N x D in COV_D, D = 512 at N = 67, rows of mean 1000 and sd
   0.01, column scales 2^40 apart, integers with an integer mean (bitwise); against the exact rational covariance of the
   fp32 values, |dC_ij| <= gamma(N + 3) mag_ij + dm_i B_j + dm_j B_i and |dmean| <= gamma(N + 2) sum |x| / N
   (dense_cases.cov_bounds); weighted with zeros, 1e-300 and a one-row component, K up to 64, against np.longdouble.

Largest error / bound seen on an MI355X: see DESIGN, "What the score kernels share"."""
import numpy as np
import pytest
import torch

import dense_cases as C
import gmm_ref

pytestmark = pytest.mark.gpu

U = C.U


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())              # a copy: the shared inputs are read-only


def N_(t):
    return t.detach().cpu().numpy()


def strided(a, pad=3):
    """The same values as the right part of a wider NaN-padded tensor (row stride > D)."""
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=a.dtype)
    wide[:, pad:] = a
    t = G(wide)[:, pad:]
    assert t.stride() == (a.shape[1] + pad, 1)
    return t


def HF():
    from hipvae import functional
    return functional


def same_bytes(a, b):
    return a.tobytes() == b.tobytes()


def report(what, err, bound):
    r = float(np.max(np.asarray(err) / np.asarray(bound)))
    print(f"{what}: error / bound = {r:.3g}")
    return r


# ---- 1. Cholesky -------------------------------------------------------------------------------------------------------------
def check_factor(cov, L, X, logdet, tag):
    D = cov.shape[0]
    assert (np.diag(L) > 0).all() and not np.triu(L, 1).any() and not np.triu(X, 1).any()
    assert not np.signbit(np.triu(L, 1)).any()
    r = report(f"{tag} |C - L L^T| / gamma(D + 1) |L||L^T|", C.chol_residual(cov, L), C.gamma(D + 1))
    ri = report(f"{tag} |L X - I| / gamma(D) |L||X|", C.inverse_residual(L, X), C.gamma(D))
    want, tol = C.logdet_of(L)
    rl = report(f"{tag} logdet", abs(logdet - want), tol)
    assert r <= 1 and ri <= 1 and rl <= 1, (tag, r, ri, rl)


@pytest.mark.parametrize("D", C.CHOL_DIMS)
def test_factor(D):
    batch = C.chol_batch(D)
    cov_t = G(batch)
    chol, linv, logdet, info = (N_(t) for t in HF().gmm_factor(cov_t))
    assert torch.equal(cov_t, G(batch)) and info.tolist() == [0] * len(batch)
    for k in range(len(batch)):
        check_factor(batch[k], chol[k], linv[k], logdet[k], f"D {D} k {k}")
    if D <= C.SCALE_MAX_DIM:                       # every operation of the algorithm commutes with a power-of-two scaling
        e = C.scale_exponents(D)
        assert same_bytes(chol[2], np.ldexp(chol[0], e[:, None])) and same_bytes(linv[2], np.ldexp(linv[0], -e[None, :]))
    again = HF().gmm_factor(cov_t)
    assert all(same_bytes(N_(a), b) for a, b in zip(again, (chol, linv, logdet, info)))


def test_many_components_do_not_disturb_each_other():
    """K = 64 at D = 129 (in place in global memory), every third component with a failing pivot."""
    mats, dims = C.many_batch()
    chol, linv, logdet, info = (N_(t) for t in HF().gmm_factor(G(mats)))
    assert info.tolist() == [d + 1 for d in dims]
    good = [k for k in range(C.MANY_K) if dims[k] < 0]
    for k in range(C.MANY_K):
        if dims[k] >= 0:
            assert np.isnan(chol[k]).all() and np.isnan(linv[k]).all() and np.isnan(logdet[k])
    for k in good[::7]:
        check_factor(mats[k], chol[k], linv[k], logdet[k], f"k {k}")
    alone = [N_(t) for t in HF().gmm_factor(G(mats[good]))]
    assert same_bytes(alone[0], chol[good]) and same_bytes(alone[1], linv[good]) and same_bytes(alone[2], logdet[good])


@pytest.mark.parametrize("D", C.FAIL_DIMS)
def test_failing_pivots_through_every_caller(D):
    """Both D work in global memory.  Each caller reports the dimension unsup_ref.ref_cholesky_logdet reports."""
    mats, dims = C.fail_batch(D)
    chol, linv, logdet, info = (N_(t) for t in HF().gmm_factor(G(mats)))
    assert info.tolist() == [d + 1 for d in dims]
    assert np.isnan(chol).all() and np.isnan(linv).all() and np.isnan(logdet).all()
    zero, other = G(np.zeros(D)), G(C.chol_well(D))
    for kind, m, d in zip(C.FAIL_KINDS, mats, dims):
        res, eig, inf = (N_(t) for t in HF().unsup_gauss(G(m)))
        assert inf.tolist() == [1, d, 0, 0] and np.isnan(res).all() and np.isnan(eig).all(), kind
        res, eig, inf = (N_(t) for t in HF().frechet(zero, G(m), zero, other))
        assert inf.tolist() == [1, d, 0, 0, 0] and np.isnan(res).all() and np.isnan(eig).all(), kind


@pytest.mark.parametrize("D", [33, 128, 129])
def test_logdet_bytes_are_the_same_across_callers(D):
    """Both are 2 x the ascending sum of log L_ii over the same block_cholesky, on both sides of the LDS limit."""
    cov = C.chol_well(D)
    a = N_(HF().unsup_gauss(G(cov))[0])[4:5]
    b = N_(HF().gmm_factor(G(cov[None]))[2])
    assert same_bytes(a, b), (a, b)


@pytest.mark.parametrize("D", [33, 129])
def test_cholesky_through_frechet(D):
    """C2 = I: T = L exactly (products with 0 and 1), M = L^T L has the spectrum of L L^T = C1 + dC1 with |dC1| <=
    gamma(D + 1) |L||L^T|, and | |L||L^T| |_F <= tr(L L^T).  C1 is exact with the graded spectrum (cond 4e9).  Bound: the
    Jacobi bound on |M|_F = |lambda|_2, plus 1.01 (gamma(D + 1) + gamma(D)) tr C1 for the factor and the product."""
    ec = C.exact_case(D, "graded")
    zero = G(np.zeros(D))
    res, eig, info = (N_(t) for t in HF().frechet(zero, G(ec["C"]), zero, G(np.eye(D))))
    assert info[:3].tolist() == [0, -1, 0] and 1 <= info[3] < C.MAX_SWEEPS and info[4] == 0
    e = C.eig_bound(D, np.linalg.norm(ec["lam"])) + 1.01 * (C.gamma(D + 1) + C.gamma(D)) * float(ec["lam"].sum())
    assert report(f"D {D} eigenvalues of L^T L", np.abs(np.sort(eig) - ec["lam"]).max(), e) <= 1
    trs = float(np.sqrt(C.ld(ec["lam"])).sum())
    assert report(f"D {D} tr sqrt", abs(res[4] - trs), C.sqrt_sum_bound(ec["lam"], e) + 4 * D * U * trs) <= 1


# ---- 2. Jacobi ---------------------------------------------------------------------------------------------------------------
def run_jacobi(kernel, Cm):
    """(res, eig, info) as numpy; frechet runs C1 = 4 I, so that L = 2 I and M = 4 C2 exactly."""
    D = Cm.shape[0]
    if kernel == "gauss":
        out = HF().unsup_gauss(G(Cm))
    else:
        zero = G(np.zeros(D))
        out = HF().frechet(zero, G(4.0 * np.eye(D)), zero, G(Cm))
    return [N_(t) for t in out]


def check_jacobi(case, rerun):
    kernel, D, kind = case
    jc = C.jacobi_case(*case)
    res, eig, info = run_jacobi(kernel, np.array(jc["C"]))
    tag = C.case_id(case)
    print(f"{tag}: sweeps {info[3]}")
    assert info[:3].tolist() == [0, -1, 0]
    if jc["diag"] or D == 1:
        assert info[3] == 0
    else:
        assert 1 <= info[3] < C.MAX_SWEEPS
    if D <= C.RESTATED_MAX_DIM:
        assert info[3] == C.jacobi_restated(*case)[1]
    fro = np.linalg.norm(jc["A"])
    e = C.eig_bound(D, fro) + jc["ref_err"]
    assert report(f"{tag} eigenvalues", np.abs(np.sort(eig) - jc["lam"]).max(), e) <= 1
    if kernel == "gauss":
        if kind != "generic":
            want = C.gauss_closed(jc)
            lam_c = jc["lam"] if not jc["diag"] else np.sort(np.diag(jc["C"]))
            ld_tol = C.logdet_bound(np.array(jc["C"]), lam_c)
            assert res[3] == want["trace"]
            assert report(f"{tag} logdet", abs(res[4] - want["logdet"]), ld_tol) <= 1
            assert report(f"{tag} tc", abs(res[0] - want["tc"]), 0.5 * ld_tol + 4 * D * U * (1 + abs(want["logdet"]))) <= 1
            w_tol = 2 * C.sqrt_sum_bound(jc["lam"], e) + 8 * D * U * want["trace"]
            assert report(f"{tag} w", abs(res[1] - want["w"]), w_tol) <= 1
            assert abs(res[2] - want["w"] / want["trace"]) <= w_tol / want["trace"] + 4 * U
    else:
        trs = float(np.sqrt(C.ld(jc["lam"])).sum())
        t_tol = C.sqrt_sum_bound(jc["lam"], e) + 4 * D * U * trs
        tr2 = float(C.ld(np.diag(jc["C"])).sum())
        assert info[4] <= jc["nzero"]
        assert res[1] == 0.0 and res[2] == 4.0 * D and abs(res[3] - tr2) <= D * U * tr2
        assert report(f"{tag} tr sqrt", abs(res[4] - trs), t_tol) <= 1
        assert abs(res[0] - (4.0 * D + tr2 - 2 * trs)) <= 2 * t_tol + 8 * D * U * (4.0 * D + tr2)
    if rerun:
        again = run_jacobi(kernel, np.array(jc["C"]))
        assert all(same_bytes(a, b) for a, b in zip(again, (res, eig, info)))
        k = 10                                     # gauss: sqrt(2^10 C_ii) = 2^5 sqrt(C_ii), so S scales by 2^20 exactly
        _, eig2, info2 = run_jacobi(kernel, np.ldexp(np.array(jc["C"]), k))
        assert same_bytes(eig2, np.ldexp(eig, 2 * k if kernel == "gauss" else k)) and info2[3] == info[3]
    return info


@pytest.mark.parametrize("case", C.JACOBI_CASES, ids=C.case_id)
def test_jacobi(case):
    check_jacobi(case, rerun=True)


@pytest.mark.parametrize("case", C.BIG_JACOBI_CASES, ids=C.case_id)
def test_jacobi_large(case):
    """One spectrum per kernel and D: the one-block sweep in global memory is the slow case.  511 and 512 are the only sizes
    that fill JacobiScratch (256 pairs)."""
    check_jacobi(case, rerun=False)


def test_commuting_pair_through_frechet():
    """C1 = Q A Q^T (two clusters), C2 = Q B Q^T (five zeros) at D = 33: the eigenvalues of M = L^T C2 L are a_k b_k.  The
    computed factor is exact for C1 + dC1, |dC1|_F <= gamma(D + 1) tr C1, and the eigenvalues of L^T C2 L are those of
    C2^1/2 (C1 + dC1) C2^1/2: they move by at most |C2|_2 |dC1|_F.  The two products that form M add 2.02 gamma(D) |L^T||C2||L|,
    at most 2.02 gamma(D) tr C1 |C2|_F in norm."""
    D = 33
    a, b = C.exact_case(D, "clusters"), C.exact_case(D, "zeros")
    lam = np.sort(np.ldexp(a["num"].astype(np.float64), -a["s"]) * np.ldexp(b["num"].astype(np.float64), -b["s"]))
    zero = G(np.zeros(D))
    res, eig, info = (N_(t) for t in HF().frechet(zero, G(a["C"]), zero, G(b["C"])))
    assert info[:3].tolist() == [0, -1, 0] and 1 <= info[3] < C.MAX_SWEEPS and info[4] <= 5
    tr1 = float(a["lam"].sum())
    e = (C.eig_bound(D, np.linalg.norm(lam)) + 1.01 * C.gamma(D + 1) * tr1 * float(b["lam"].max())
         + 2.02 * C.gamma(D) * tr1 * float(np.linalg.norm(b["lam"])))
    assert report("eigenvalues a_k b_k", np.abs(np.sort(eig) - lam).max(), e) <= 1
    trs = float(np.sqrt(C.ld(lam)).sum())
    assert report("tr sqrt", abs(res[4] - trs), C.sqrt_sum_bound(lam, e) + 4 * D * U * trs) <= 1


def test_the_unconverged_branch(monkeypatch):
    """A finite SPD c1 and a NaN planted symmetrically in c2 pass the Cholesky of c1; the sweep loop is bounded by
    kJacobiMaxSweeps and reports info[2].  hipvae.quality.frechet_distance raises its RuntimeError on that info; it cannot
    get there from features, because it refuses non-finite features first and a covariance of finite fp32 rows is finite, so
    the covariances are handed to it here in place of HF.unsup_cov's.  disentangle's raise path is fed the same info."""
    from hipvae import disentangle, quality
    D = 6
    c1, c2 = C.chol_well(D), np.array(C.chol_well(D))
    c2[1, 4] = c2[4, 1] = np.nan
    zero = G(np.zeros(D))
    res, eig, info = HF().frechet(zero, G(c1), zero, G(c2))
    assert N_(info)[:4].tolist() == [0, -1, 1, C.MAX_SWEEPS]
    served = iter([(zero, G(c1)), (zero, G(c2))])
    monkeypatch.setattr(quality.HF, "unsup_cov", lambda x, flags: next(served))
    feats = torch.zeros((8, D), dtype=torch.float32, device=dev())
    with pytest.raises(RuntimeError, match="frechet_distance: the Jacobi iteration did not converge in 60 sweeps"):
        quality.frechet_distance(feats, feats)
    with pytest.raises(RuntimeError, match="unsupervised scores: the Jacobi iteration did not converge in 60 sweeps"):
        disentangle._raise_on_gauss(N_(info)[:4].tolist())


# ---- 3. covariance pass ------------------------------------------------------------------------------------------------------
def check_cov(kind, N, D):
    inp = C.cov_input(kind, N, D)
    mean, cov = C.cov_exact(inp)
    dm, dc = C.cov_bounds(inp["x"], mean, cov)
    got = []
    for view in (G, strided):
        flags = HF().disent_flags(dev())
        gm, gc = HF().unsup_cov(view(np.array(inp["x"])), flags)
        assert N_(flags).tolist() == [0, 0] and torch.equal(gc, gc.t())
        got.append((N_(gm), N_(gc)))
    assert same_bytes(got[0][0], got[1][0]) and same_bytes(got[0][1], got[1][1])
    gm, gc = got[0]
    if kind == "integer":                           # every centred product and every sum is an exact integer
        assert same_bytes(gm, mean) and same_bytes(gc, cov)
    return max(float(np.max(np.abs(gm - mean) / dm)), float(np.max(np.abs(gc - cov) / dc)))


@pytest.mark.parametrize("N", C.COV_N)
@pytest.mark.parametrize("kind", C.COV_KINDS)
def test_covariance(kind, N):
    for D in C.COV_D:
        r = check_cov(kind, N, D)
        print(f"{kind} N {N} D {D}: error / bound = {r:.3g}")
        assert r <= 1, (kind, N, D, r)


def test_covariance_of_512_columns():
    r = check_cov("offset", *C.WIDE)
    print(f"offset N {C.WIDE[0]} D {C.WIDE[1]}: error / bound = {r:.3g}")
    assert r <= 1


@pytest.mark.parametrize("N,D,K", C.MSTEP_SHAPES)
def test_weighted_pass(N, D, K):
    x, resp = C.mstep_input(N, D, K)
    nk, means, cov, _, _ = C.mstep_exact(N, D, K)
    got = []
    for view in (G, strided):
        flags = HF().disent_flags(dev())
        out = HF().gmm_mstep(view(np.array(x)), G(np.array(resp)), flags, reg=C.MSTEP_REG)
        assert N_(flags).tolist() == [0, 0] and torch.equal(out[3], out[3].transpose(1, 2))
        got.append([N_(t) for t in out])
    assert all(same_bytes(a, b) for a, b in zip(*got))
    gnk, gw, gm, gc = got[0]
    worst = 0.0
    dnks = np.array([C.mstep_bounds(N, D, K, k)[0] for k in range(K)])
    w = nk / nk.sum()
    assert (np.abs(gw - w) <= 1.01 * (dnks / nk.sum() + w * dnks.sum() / nk.sum() + 2 * U)).all()
    for k in range(K):
        dnk, dm, dc = C.mstep_bounds(N, D, K, k)
        errs = (abs(gnk[k] - nk[k]) / dnk, np.max(np.abs(gm[k] - means[k]) / dm), np.max(np.abs(gc[k] - cov[k]) / dc))
        worst = max(worst, *map(float, errs))
        assert max(errs) <= 1, (N, D, K, k, errs)
    # the component whose whole mass sits on one row: reg on the diagonal, up to the square of x - x / nk (the guard's shift
    # and one rounding of the mean)
    assert np.abs(gc[K - 1] - C.MSTEP_REG * np.eye(D)).max() <= (1000.1 * (gmm_ref.NK_GUARD + 2 * U)) ** 2 * 1.01 \
        + U * C.MSTEP_REG
    print(f"N {N} D {D} K {K}: error / bound = {worst:.3g}")
