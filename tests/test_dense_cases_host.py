"""CPU-only proof that tests/dense_cases.py holds what it claims: every constructed matrix is exact and has the spectrum
it names, every reference is independent of LAPACK, the project's own restatements (gmm_ref.cholesky / tri_inverse,
unsup_ref.ref_jacobi / ref_cov, gmm_ref.mstep) meet every bound of tests/test_hip_dense.py with room, the constant K of the
eigenvalue bound is the measured one, and four deliberately wrong variants of the restatements each break a bound of the
new file while passing the tolerances the suite had before."""
import numpy as np
import pytest

import dense_cases as C
import gmm_ref
import quality_ref
import unsup_ref

U = C.U


def small_cases():
    return [c for c in C.JACOBI_CASES if c[1] <= C.RESTATED_MAX_DIM]


# ---- the constructed matrices ----------------------------------------------------------------------------------------------
EXACT_USED = sorted({(c[1], c[2]) for c in C.JACOBI_CASES + C.BIG_JACOBI_CASES if c[2] in C.SPECTRA}
                    | {(33, "graded"), (33, "clusters"), (129, "graded")})
# the bit budget every spectrum takes: the largest of SPECTRA at which the reflector's 2 log2 m extra bits still fit
Q_TAKEN = {(129, "near"): 32, (130, "near"): 32, (255, "near"): 36, (511, "near"): 32}


def test_basis_is_orthogonal_and_dyadic():
    for D in sorted(set(C.JACOBI_DIMS) | {33, 48}):
        Qu, scale, lm = C.basis(D)
        inv = np.rint(1.0 / scale).astype(np.int64)
        assert np.array_equal(1.0 / inv, scale) and all(int(n) & (int(n) - 1) == 0 for n in inv)
        big = int(inv.max())
        G = (Qu * (big // inv)[None, :]) @ Qu.T                            # Qu diag(1 / n) Qu^T in units of 1 / big
        assert np.array_equal(G, big * 4 ** lm * np.eye(D, dtype=np.int64)), D
        v = C.reflector(D)
        assert (v is None) == (D & (D - 1) == 0)
        if v is not None:
            m = int(np.abs(v).sum())
            assert m & (m - 1) == 0 and v[0] != 0 and v[-1] != 0          # a power-of-two support that spans the blocks


@pytest.mark.parametrize("D,kind", EXACT_USED)
def test_exact_matrix_is_exact(D, kind):
    ec = C.exact_case(D, kind)
    assert ec["q"] == Q_TAKEN.get((D, kind), C.SPECTRA[kind][1][0])
    assert C.span_bits(ec["num"]) <= 40
    P, exact = C.exact_product(D, ec["num"], ec["s"], rational=D <= 48)
    assert exact and np.array_equal(P, ec["C"])
    assert np.array_equal(ec["lam"], np.sort(ec["num"] * 2.0 ** -ec["s"]))
    if D >= 5:
        off = ec["C"][~np.eye(D, dtype=bool)]
        assert (off != 0).mean() >= 0.5
    if kind in ("clusters", "near") and D & (D - 1) == 0:
        assert np.array_equal(np.diag(ec["C"]), np.ones(D))               # what itcv_unsup_gauss needs: S = C exactly
    if kind == "zeros":
        assert (ec["lam"] == 0).sum() == min(5, D - 1)
    if kind == "clusters" and D > 1:
        assert (ec["lam"] == 0.5).sum() == (D + 1) // 2 and (ec["lam"] == 1.5).sum() == D // 2
    if kind == "near" and D > 1:
        assert np.all(np.diff(ec["lam"]) > 0) and ec["lam"][-1] - ec["lam"][0] <= 2 * D * 2.0 ** -ec["q"]
    if kind == "graded" and D > 33:
        assert ec["lam"][0] == 2.0 ** -32 and ec["lam"][-1] == 1.0


def test_a_grading_over_64_bits_is_refused():
    """What the 40-bit rule is for: 2^-k over 64 values does not fit fp64 entries."""
    assert C.exact_sym(64, (1 << (62 - np.arange(64))).astype(np.int64) >> 0, 62) is None


def test_circulant_against_mpmath():
    for D in (3, 5, 33):
        Cm, lam, err = C.circulant(D)
        assert np.array_equal(np.diag(Cm), np.ones(D)) and (Cm != 0).all()
        assert np.abs(lam - C.mp_eigs(np.array(Cm))).max() <= err + 2 * U * 1.5
        assert lam[0] >= 0.5 and lam[-1] <= 1.5
        pairs = np.sort(lam)[::-1][1:]                                     # all but the largest come in equal pairs
        assert np.abs(pairs[0::2] - pairs[1::2]).max() <= 2 * err
    for D in (255, 511):
        Cm, lam, err = C.circulant(D)
        assert err < 2.5 * U and abs(lam.sum() - D) < 1e-12                # the trace


# ---- 1. Cholesky -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", C.CHOL_DIMS)
def test_cholesky_restatement_meets_the_bounds(D):
    batch = C.chol_batch(D)
    assert len(batch) == (3 if D <= C.SCALE_MAX_DIM else 2)
    if D > 1:
        lam = np.linalg.eigvalsh(batch[0])
        assert 1e9 < lam[-1] / lam[0] < 1e11 and np.linalg.cond(batch[1]) < 3.5
    chol, linv, logdet, info = gmm_ref.factor(batch)
    assert not info.any()
    for k in range(len(batch)):
        r, ri = C.chol_residual(batch[k], chol[k]), C.inverse_residual(chol[k], linv[k])
        want, tol = C.logdet_of(chol[k])
        print(f"D {D} k {k}: |C - L L^T| / gamma(D + 1)|L||L^T| = {r / C.gamma(D + 1):.3f}, "
              f"|L X - I| / gamma(D)|L||X| = {ri / C.gamma(D):.3f}, logdet err / tol = {abs(logdet[k] - want) / tol:.3f}")
        room = 0.5 if D > 1 else 1.0                                       # D = 1 is one sqrt and one division: no room in 2 u
        assert r <= room * C.gamma(D + 1) and ri <= room * C.gamma(D) and abs(logdet[k] - want) <= 0.5 * tol
        assert (np.diag(chol[k]) > 0).all() and not np.triu(chol[k], 1).any() and not np.triu(linv[k], 1).any()
    if D <= C.SCALE_MAX_DIM:                                               # a power-of-two scaling commutes with every step
        e = C.scale_exponents(D)
        assert np.abs(e).max() <= C.SCALE_EXP and (D < 3 or len(set(e.tolist())) > 1)
        assert np.array_equal(chol[2], np.ldexp(chol[0], e[:, None]))
        assert np.array_equal(linv[2], np.ldexp(linv[0], -e[None, :]))


def test_failing_pivots_fail_where_they_should():
    for D in C.FAIL_DIMS:
        mats, dims = C.fail_batch(D)
        j = (2 * D) // 3
        assert dims == [0, D - 1, j, j, j] and D > C.LDS_DIM
        assert np.isinf(mats[3]).sum() == 1 and np.isnan(mats[4]).sum() == 2
        assert gmm_ref.factor(np.array(mats))[3].tolist() == [d + 1 for d in dims]
    mats, dims = C.many_batch()
    assert mats.shape == (64, 129, 129)
    bad = [k for k in range(64) if dims[k] >= 0]
    assert bad == list(range(1, 64, 3)) and {dims[k] for k in bad} == {0, 128, 86}


# ---- 2. Jacobi ---------------------------------------------------------------------------------------------------------------
def test_jacobi_case_table():
    ids = [C.case_id(c) for c in C.JACOBI_CASES + C.BIG_JACOBI_CASES]
    assert len(set(ids)) == len(ids)
    for kernel in ("gauss", "frechet"):
        dims = {c[1] for c in C.JACOBI_CASES + C.BIG_JACOBI_CASES if c[0] == kernel}
        assert set(C.JACOBI_DIMS) <= dims
        big = [c for c in C.BIG_JACOBI_CASES if c[0] == kernel]
        assert sorted(c[1] for c in big) == [255, 256, 511, 512]          # one spectrum per kernel and D
    kinds = {c[2] for c in C.JACOBI_CASES}
    assert kinds == {"clusters", "near", "graded", "zeros", "diagonal", "generic", "circulant"}
    assert all(c[1] <= 48 for c in C.JACOBI_CASES if c[2] == "generic")


def test_jacobi_restatement_pins_k():
    """unsup_ref.ref_jacobi on every case of D <= 130: converged in 1..59 sweeps (0 on a diagonal matrix), and its largest
    eigenvalue error in units of D u |A|_F is the figure beside K_JACOBI."""
    worst, worst_big, where = 0.0, 0.0, None
    for c in small_cases():
        case = C.jacobi_case(*c)
        eig, sweeps, conv = C.jacobi_restated(*c)
        D = c[1]
        fro = np.linalg.norm(case["A"])
        err = max(float(np.abs(eig - case["lam"]).max()) - case["ref_err"], 0.0)
        units = err / (D * U * fro)
        assert conv and sweeps < C.MAX_SWEEPS
        assert sweeps == 0 if (case["diag"] or D == 1) else sweeps >= 1, c
        assert (eig < 0).sum() <= case["nzero"]
        if units > worst:
            worst, where = units, C.case_id(c)
        if D >= 127:
            worst_big = max(worst_big, units)
    print("largest error of the restatement:", worst, "D u |A|_F at", where, "; at D >= 127:", worst_big)
    assert 0.5 * C.K_MEASURED <= worst <= C.K_MEASURED * (1 + 1e-9) and worst_big <= 0.05
    assert C.K_JACOBI == 16 * C.K_MEASURED
    for D in C.JACOBI_DIMS[1:]:
        assert C.K_JACOBI * D * U <= C.A_PRIORI_SWEEPS * (D - 1) * U


@pytest.mark.parametrize("case", [c for c in C.JACOBI_CASES if c[0] == "gauss" and c[2] != "generic"], ids=C.case_id)
def test_gauss_closed_forms(case):
    """unsup_ref.ref_gauss against the closed forms, within half of the bounds test_hip_dense.py uses."""
    jc = C.jacobi_case(*case)
    D = case[1]
    want = C.gauss_closed(jc)
    got = unsup_ref.ref_gauss(jc["C"])
    e = C.eig_bound(D, np.linalg.norm(jc["A"])) + jc["ref_err"]
    lam_c = jc["lam"] if not jc["diag"] else np.sort(np.diag(jc["C"]))
    ld_tol = C.logdet_bound(jc["C"], lam_c)
    w_tol = 2 * C.sqrt_sum_bound(jc["lam"], e) + 8 * D * U * want["trace"]
    assert got["fail_dim"] == -1 and got["converged"]
    assert abs(got["logdet"] - want["logdet"]) <= 0.5 * ld_tol
    assert abs(got["tc"] - want["tc"]) <= 0.5 * (0.5 * ld_tol + 4 * D * U * (1 + abs(want["logdet"])))
    assert abs(got["w"] - want["w"]) <= 0.5 * w_tol and got["trace"] == want["trace"]


# ---- 3. covariance -------------------------------------------------------------------------------------------------------------
def test_slice_counts():
    for N, (rows, ns) in C.SLICES.items():
        assert gmm_ref.slice_rows(N) == rows and gmm_ref.cdiv(N, rows) == ns
    assert gmm_ref.slice_rows(32768) == 512 and gmm_ref.slice_rows(32769) > 512   # the first N whose 64 slices exceed 512
    assert 70001 - 63 * 1096 == 953                                                # a ragged last slice
    assert all(gmm_ref.cdiv(N, gmm_ref.slice_rows(N)) == 1 for N in C.COV_N if N <= 512)
    nt = gmm_ref.cdiv(C.WIDE[1], 16)
    assert nt * (nt + 1) // 2 == 528


def cov_cases():
    return [(k, N, D) for k in C.COV_KINDS for N in C.COV_N for D in C.COV_D] + [("offset",) + C.WIDE]


def test_covariance_inputs_and_restatement():
    worst = 0.0
    for kind, N, D in cov_cases():
        inp = C.cov_input(kind, N, D)
        x = inp["x"].astype(np.float64)
        assert N * np.abs(inp["y"]).max() ** 2 < 2.0 ** 53
        mean, cov = C.cov_exact(inp)
        if kind == "offset" and N >= 511:
            assert np.abs(mean - 1000).max() < 2e-3 and np.abs(np.sqrt(np.diag(cov)) - 0.01).max() < 2e-3
        if kind == "scales" and D > 1:
            sd = np.sqrt(np.diag(cov))
            assert inp["e"].max() - inp["e"].min() == 40 and sd.max() / sd.min() >= 2.0 ** 38
        rm, rc = unsup_ref.ref_cov(inp["x"])
        if kind == "integer":
            assert np.array_equal(mean, np.rint(mean)) and np.array_equal(x, np.rint(x))
            assert N * np.abs(x).max() ** 2 < 2.0 ** 53
            assert np.array_equal(rm, mean) and np.array_equal(rc, cov)    # every sum is an exact integer
        dm, dc = C.cov_bounds(inp["x"], mean, cov)
        worst = max(worst, float(np.max(np.abs(rc - cov) / dc)), float(np.max(np.abs(rm - mean) / dm)))
        assert (np.abs(rm - mean) <= 0.5 * dm).all() and (np.abs(rc - cov) <= 0.5 * dc).all(), (kind, N, D)
    print("restatement: largest error / bound", worst)


def test_weighted_inputs_and_restatement():
    worst = 0.0
    assert max(s[2] for s in C.MSTEP_SHAPES) == 64
    for N, D, K in C.MSTEP_SHAPES:
        x, resp = C.mstep_input(N, D, K)
        assert (resp == 0).any() and (N < 100 or (resp == 1e-300).any())
        assert (resp[:, K - 1] != 0).sum() == 1 and resp[:, K - 1].sum() == 1.0
        nk, means, cov, rdm, rdc = C.mstep_exact(N, D, K)
        got = gmm_ref.mstep(x, np.array(resp), C.MSTEP_REG)
        # the whole mass on one row: reg on the diagonal, up to the square of the guard's shift of the mean
        assert np.abs(cov[K - 1] - C.MSTEP_REG * np.eye(D)).max() <= (1000.1 * gmm_ref.NK_GUARD) ** 2 * 1.01
        for k in range(K):
            dnk, dm, dc = C.mstep_bounds(N, D, K, k)
            assert (rdm[k] <= 0.01 * dm).all() and (rdc[k] <= 0.01 * dc).all()     # the reference's own error is small
            errs = (abs(got[0][k] - nk[k]) / dnk, np.max(np.abs(got[2][k] - means[k]) / dm),
                    np.max(np.abs(got[3][k] - cov[k]) / dc))
            worst = max(worst, *map(float, errs))
            assert max(errs) <= 0.5, (N, D, K, k, errs)
    print("restatement: largest error / bound", worst)


# ---- mutations -----------------------------------------------------------------------------------------------------------------
def old_cov_inputs():
    """The recipe and shapes of tests/test_hip_unsup_scores.py::test_covariance."""
    for N, D in [(2, 5), (67, 1), (67, 16), (600, 131), (1100, 33)]:
        rs = np.random.RandomState(N * 1000 + D)
        x = (rs.randn(N, D) * rs.uniform(0.2, 2.0, size=D) + rs.uniform(-1, 1, size=D)).astype(np.float32)
        if D > 2:
            x[:, 2] = 0.5 * x[:, 0] - x[:, 1]
        yield x


def refused_by_old_cov(fn):
    """The shapes of the old test whose tolerances (1e-13 max(1, |x|) on the mean, 1e-12 sd_i sd_j) refuse ``fn``."""
    out = []
    for x in old_cov_inputs():
        mean, cov = unsup_ref.ref_cov(x)
        gm, gc = fn(x)
        sd = np.sqrt(np.diag(cov))
        r = max(np.abs(gm - mean).max() / (1e-13 * max(1.0, np.abs(x).max())),
                np.max(np.abs(gc - cov) / (1e-12 * sd[:, None] * sd[None, :])))
        print(f"old {x.shape}: error / tolerance {r:.3g}")
        if r > 1:
            out.append(x.shape)
    return out


def refused_by_new_cov(fn):
    """The N of COV_N at which the new bounds refuse ``fn`` (mean 1000, sd 0.01, D = 17)."""
    out = []
    for N in C.COV_N:
        inp = C.cov_input("offset", N, 17)
        mean, cov = C.cov_exact(inp)
        dm, dc = C.cov_bounds(inp["x"], mean, cov)
        gm, gc = fn(inp["x"])
        r = max(np.max(np.abs(gm - mean) / dm), np.max(np.abs(gc - cov) / dc))
        print(f"new N {N}: error / bound {r:.3g}")
        if r > 1:
            out.append(N)
    return out


def one_pass_cov(x):
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    m = x.sum(0) / N
    return m, (x.T @ x - N * np.outer(m, m)) / (N - 1)


def fp32_mean_cov(x):
    """The covariance centred on a mean that was rounded to fp32; the mean it returns is the fp64 one."""
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    m = x.sum(0) / N
    xc = x - m.astype(np.float32).astype(np.float64)
    return m, xc.T @ xc / (N - 1)


def test_mutation_one_pass_covariance():
    """Passes every old tolerance (at most 0.05 of it); refused at every new N but 2 and 4, where the few bits of fp32 rows
    leave the one-pass formula exact."""
    assert refused_by_old_cov(one_pass_cov) == []
    assert refused_by_new_cov(one_pass_cov) == [N for N in C.COV_N if N not in (2, 4)]


def test_mutation_fp32_mean():
    """Refused at every new N.  Of the old shapes the four with N >= 67 let it through (at most 0.011 of the tolerance); its
    N = 2 shape refuses it, at 5 x the tolerance, because a column of two rows there has a standard deviation of 0.003."""
    assert refused_by_old_cov(fp32_mean_cov) == [(2, 5)]
    assert refused_by_new_cov(fp32_mean_cov) == C.COV_N


def fp32_update_cholesky(Cm):
    """gmm_ref.cholesky with the product of the rank-one update rounded through fp32."""
    A = np.array(Cm, np.float64)
    D = A.shape[0]
    for j in range(D):
        l = np.sqrt(A[j, j])
        A[j, j] = l
        A[j + 1:, j] = A[j + 1:, j] / l
        if j + 1 < D:
            col = A[j + 1:, j]
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - np.tril(np.outer(col, col)).astype(np.float32).astype(np.float64)
    return np.tril(A)


def test_mutation_fp32_cholesky_update():
    """At the one shape the old test ran above D = 131, (D, K) = (512, 1), its tolerance lets the mutant through; the
    componentwise residual refuses it at every D >= 2 of the new file."""
    D, K = 512, 1
    cov = gmm_ref.make_params(D, K)[2]
    chol = gmm_ref.factor(cov)[0]
    tol_L = 2 * gmm_ref.COND_MAX ** 2 * D * (D + 1) * U * np.linalg.norm(chol[0], 2)
    err = np.abs(fp32_update_cholesky(cov[0]) - chol[0]).max()
    print("old: |dL| / tol_L =", err / tol_L)
    assert err <= tol_L
    for D in (2, 33, 129, 512):
        Cm = C.chol_batch(D)[1]
        r = C.chol_residual(Cm, fp32_update_cholesky(Cm)) / C.gamma(D + 1)
        print(f"new: D {D} residual / gamma(D + 1) = {r:.3g}")
        assert r > 1.0


def loose_jacobi(S, tol=1e-10):
    saved = unsup_ref.JACOBI_TOL
    unsup_ref.JACOBI_TOL = tol
    try:
        return np.sort(unsup_ref.ref_jacobi(S)[0])
    finally:
        unsup_ref.JACOBI_TOL = saved


def test_mutation_loose_jacobi_stop():
    """Stopped at off_F <= 1e-10 |A|_F the eigenvalues of a matrix with separated eigenvalues are still right to the square
    of that, so the old 1e-12 |S|_F passes; inside a cluster the error is of first order, and the new bound refuses it."""
    for D, seed in ((5, 1), (33, 2), (131, 3)):
        S = quality_ref.spd(D, seed)
        assert np.abs(loose_jacobi(S) - np.linalg.eigvalsh(S)).max() <= 1e-12 * np.linalg.norm(S)
    broken = []
    for c in small_cases():
        if c[2] in ("clusters", "near", "circulant") and 4 <= c[1]:
            case = C.jacobi_case(*c)
            err = np.abs(loose_jacobi(case["A"]) - case["lam"]).max()
            if err > C.eig_bound(c[1], np.linalg.norm(case["A"])) + case["ref_err"]:
                broken.append(C.case_id(c))
    print("refused by the new bound:", broken)
    assert len(broken) >= 1
