"""GPU tests of the sample-quality kernels (csrc/quality.hip, hipvae/quality.py) against the numpy fp64 restatement of
tests/quality_ref.py, whose own correctness and the conditions on the inputs are pinned by tests/test_quality_ref_host.py.

Shapes (N, M, D, k) and what they cross.  The pair kernel owns 32 query rows, streams 64 candidate rows a tile and 32
columns a chunk (4 at a time), and cuts the candidates into `splits` slices:
  (2, 2, 1, 1), (5, 9, 1, 1)   one partial query tile, one partial candidate tile, one column (three padded);
  (67, 45, 7, 3)               three query tiles (the last 3 rows), two candidate tiles for the 67, D = 7 pads one column;
  (130, 131, 33, 5)            a second chunk of ONE column; three candidate tiles, the last 2 / 3 rows; splits = 3 gives
                               slices of 44, 44, 42 (ragged, and not a multiple of the tile);
  (600, 515, 131, 5)           five chunks, the last 3 columns; splits = 0 chooses 10 slices of the 600, 9 of the 515;
  (1100, 67, 512, 16)          sixteen full chunks, the longest lists (17 entries); splits = 0 chooses 18 / 2 slices;
  (100, 200, 64, 2)            exactly two full chunks, N below M.
Each is run dense and as the right part of a wider NaN-padded tensor, at splits 0, 1 and 3.  The KID kernel works on
64 x 64 tiles of 32-column chunks, 1024 partials a sum: the shapes above cross its tile and chunk edges, (2100, 70, 3)
has 33 x 33 = 1089 tiles of x on x, so 65 blocks take a second tile.

Bounds.  Integer-valued features: every d^2 is an exact integer whatever the order, so radii, counts, minima and scores
equal the restatement BITWISE.  Gaussian features: a radius is a sum of D non-negative rounded squares of exactly
representable differences, so it is within (D + 2) 2^-53 relative in any order (the kernel's order is the restatement's, so
it is in fact equal); the host test asserts that no pair lies within 1e-12 r^2 of a radius it is compared with, so the
counts must be EQUAL.  KID: a sum of R <= rows^2 terms folded in any order carries at most (depth) 2^-53 sum|kappa| with
depth <= rows here (16 per lane, 6 butterfly steps, 3 waves, at most 2 tiles a block, at most 1024 partials: below the
larger row count of every shape used); a dot product of D terms carries D 2^-53 sum_d |a_d b_d| / D, which kappa's power
passes on as about D 2^-53 |kappa| for features of unit scale; hence (D + rows) 2^-53 sum|kappa| per sum, with sum|kappa|
from the restatement.  mmd2 cancels, so its bound is the three bounds divided as the sums are, plus 4 roundings of the
terms.  Frechet: tests/quality_ref.py frechet_bound, computed from the restatement's own M."""
import numpy as np
import pytest
import torch

import quality_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
SPLITS = (0, 1, 3)


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def strided(a, pad=3):
    """The same values as the right part of a wider tensor (row stride > D); the left part must not be read."""
    a = np.asarray(a)
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=a.dtype)
    wide[:, pad:] = a
    t = G(wide)[:, pad:]
    assert t.stride() == (a.shape[1] + pad, 1)
    return t


def N_(t):
    return t.cpu().numpy()


VIEWS = {"dense": G, "strided": strided}


# ---- radii and counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,M,D,k", R.SHAPES)
def test_integer_features_are_bitwise(N, M, D, k, view):
    from hipvae import quality as Q
    real, fake, r = R.restated("integer", N, M, D, k)
    xr, xf = VIEWS[view](real), VIEWS[view](fake)
    for s in SPLITS:
        r2r, r2f = Q.knn_radius(xr, k, splits=s), Q.knn_radius(xf, k, splits=s)
        assert r2r.dtype == torch.float64 and r2r.shape == (N,) and r2r.is_cuda
        assert np.array_equal(N_(r2r), r["r2_real"]) and np.array_equal(N_(r2f), r["r2_fake"]), s
        got = Q.prdc_counts(xr, xf, k, splits=s)
        assert np.array_equal(N_(got["fake_hits"]), r["fake_hits"]) and got["fake_hits"].dtype == torch.int32
        assert np.array_equal(N_(got["real_covered"]), r["real_covered"])
        assert np.array_equal(N_(got["real_min"]), r["real_min"])
        assert tuple(got["counts"].tolist()[:4]) == r["counts"]
    sc = Q.prdc(xr, xf, k)
    print((N, M, D, k), sc)
    assert sc == {n: r[n] for n in ("precision", "recall", "density", "coverage")}
    c = r["counts"]
    assert sc == dict(precision=c[0] / M, recall=c[1] / N, density=c[2] / (k * M), coverage=c[3] / N)


@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,M,D,k", R.SHAPES)
def test_gaussian_features(N, M, D, k, view):
    from hipvae import quality as Q
    real, fake, r = R.restated("gaussian", N, M, D, k)
    xr, xf = VIEWS[view](real), VIEWS[view](fake)
    first = None
    for s in SPLITS:
        r2r, r2f = N_(Q.knn_radius(xr, k, splits=s)), N_(Q.knn_radius(xf, k, splits=s))
        err = max(np.abs(r2r / r["r2_real"] - 1).max(), np.abs(r2f / r["r2_fake"] - 1).max())
        print((N, M, D, k), "splits", s, "radius error / bound", err / ((D + 2) * U))
        assert err <= (D + 2) * U
        got = Q.prdc_counts(xr, xf, k, splits=s)
        assert np.array_equal(N_(got["fake_hits"]), r["fake_hits"])
        assert np.array_equal(N_(got["real_covered"]), r["real_covered"])
        assert np.abs(N_(got["real_min"]) / r["real_min"] - 1).max() <= (D + 2) * U
        assert tuple(got["counts"].tolist()[:4]) == r["counts"]
        bits = (r2r, r2f, N_(got["real_min"]))
        first = first or bits
        assert all(np.array_equal(a, b) for a, b in zip(first, bits))          # the same bits for every `splits`
    assert Q.prdc(xr, xf, k) == {n: r[n] for n in ("precision", "recall", "density", "coverage")}


def test_duplicated_rows_have_radius_zero():
    from hipvae import quality as Q
    real = np.repeat(np.arange(40, dtype=np.float32)[:, None] * np.ones((1, 5), np.float32), 2, axis=0)
    x = G(real)
    assert torch.equal(Q.knn_radius(x, 1), torch.zeros(80, dtype=torch.float64, device=dev()))
    assert Q.prdc(x, x.clone(), 1) == dict(precision=0.0, recall=0.0, density=0.0, coverage=0.0)
    got = Q.prdc_counts(x, x.clone(), 1)
    assert not got["fake_hits"].any() and not got["real_covered"].any() and not got["real_min"].any()


# ---- KID -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,M,D", [s[:3] for s in R.SHAPES] + [(2100, 70, 3)])
def test_poly_mmd(N, M, D, view):
    from hipvae import functional as HF
    from hipvae import quality as Q
    x, y = R.gaussian_features(N, M, D, seed=5)
    xt, yt = VIEWS[view](x), VIEWS[view](y)
    rows = max(N, M)
    for p, gamma, coef0 in ((1, None, 1.0), (2, None, 1.0), (3, None, 1.0), (4, None, 1.0), (2, 0.5, 0.25)):
        r = R.ref_poly(x, y, degree=p, gamma=gamma, coef0=coef0)
        flags = HF.disent_flags(dev())
        res = HF.poly_mmd(xt, yt, flags, degree=p, gamma=gamma or 0.0, coef0=coef0)
        got = N_(res)
        bounds = [(D + rows) * U * a for a in r["abs"]]
        for name, g, b in zip(("Sxx", "Syy", "Sxy"), got[:3], bounds):
            print((N, M, D, p), name, "error / bound", abs(g - r[name]) / max(b, 1e-300))
            assert abs(g - r[name]) <= b
        nn, mm, nm = N * (N - 1.0), M * (M - 1.0), float(N * M)
        b2 = bounds[0] / nn + bounds[1] / mm + 2 * bounds[2] / nm \
            + 4 * U * (abs(r["Sxx"]) / nn + abs(r["Syy"]) / mm + 2 * abs(r["Sxy"]) / nm)
        assert abs(got[3] - r["mmd2"]) <= b2
        assert got[3] == (got[0] / nn + got[1] / mm) - (2.0 * got[2]) / nm
        assert torch.equal(res, HF.poly_mmd(xt, yt, flags, degree=p, gamma=gamma or 0.0, coef0=coef0))
        assert flags.tolist() == [0, 0]
        if gamma:
            assert Q.kernel_distance(xt, yt, degree=p, gamma=gamma, coef0=coef0)["kid"] == got[3]
    kd = Q.kernel_distance(xt, yt)
    assert kd == dict(kid=float(N_(HF.poly_mmd(xt, yt, HF.disent_flags(dev())))[3]), kid_std=0.0)


def test_kid_subsets():
    from hipvae import quality as Q
    x, y = (G(a) for a in R.gaussian_features(300, 280, 20, seed=9))
    rs = np.random.RandomState(4)
    ir, jf = rs.choice(300, 100, replace=False), rs.choice(280, 100, replace=False)
    one = Q.kernel_distance(x, y, subset_size=100, num_subsets=1, seed=4)
    full = Q.kernel_distance(x.index_select(0, G(ir)), y.index_select(0, G(jf)))
    assert one == full and one["kid_std"] == 0.0                            # the same kernel on the same rows: bitwise
    many = Q.kernel_distance(x, y, subset_size=100, num_subsets=7, seed=4)
    assert many == Q.kernel_distance(x, y, subset_size=100, num_subsets=7, seed=4) and many["kid_std"] > 0.0
    vals = []
    rs = np.random.RandomState(4)
    for _ in range(7):
        ir, jf = rs.choice(300, 100, replace=False), rs.choice(280, 100, replace=False)
        vals.append(Q.kernel_distance(x.index_select(0, G(ir)), y.index_select(0, G(jf)))["kid"])
    assert abs(many["kid"] - np.mean(vals)) <= 1e-15 + 4 * U * np.abs(vals).max()
    assert abs(many["kid_std"] - np.std(vals)) <= 1e-15 + 1e-9 * np.std(vals)
    with pytest.raises(ValueError, match="subset_size"):
        Q.kernel_distance(x, y, subset_size=281)


# ---- Frechet ---------------------------------------------------------------------------------------------------------------
def _frechet(m1, c1, m2, c2, eps=0.0):
    from hipvae import functional as HF
    res, eig, info = HF.frechet(G(m1), G(c1), G(m2), G(c2), eps)
    return N_(res), N_(eig), info.tolist()


@pytest.mark.parametrize("D", [1, 2, 16, 33, 128, 131])
def test_frechet_kernel(D):
    """D = 128 is the largest matrix kept in LDS, 131 the first in the workspace (and odd: a padded rotation pair)."""
    from hipvae import functional as HF
    assert HF.unsup_gauss_lds_dim() == 128
    rs = np.random.RandomState(D)
    c1, c2, m1, m2 = R.spd(D, 10 + D), R.spd(D, 20 + D), rs.randn(D), rs.randn(D)
    r = R.ref_frechet(m1, c1, m2, c2)
    b = R.frechet_bound(r)
    res, eig, info = _frechet(m1, c1, m2, c2)
    tr = np.trace(c1) + np.trace(c2)
    print("D", D, "tr sqrt error / bound", abs(res[4] - r["trace_sqrt"]) / b, "sweeps", info[3])
    assert info[:3] == [0, -1, 0] and info[3] <= 60 and info[4] == 0 and (info[3] >= 1 or D == 1)
    assert abs(res[4] - r["trace_sqrt"]) <= b
    assert abs(res[0] - r["frechet"]) <= 2 * b + 4 * D * U * (tr + r["mean_term"])
    assert abs(res[1] - r["mean_term"]) <= D * U * r["mean_term"] and abs(res[2] - np.trace(c1)) <= D * U * tr
    assert abs(res[3] - np.trace(c2)) <= D * U * tr
    assert np.abs(np.sort(eig) - r["eig"]).max() <= 1e-12 * np.linalg.norm(r["M"])
    assert res[0] == ((res[1] + res[2]) + res[3]) - 2.0 * res[4]
    res2, eig2, info2 = _frechet(m1, c1, m2, c2)
    assert np.array_equal(res, res2) and np.array_equal(eig, eig2) and info == info2
    # identical Gaussians: 0 within the bound
    same, _, _ = _frechet(m1, c1, m1, c1)
    assert abs(same[0]) <= 2 * R.frechet_bound(R.ref_frechet(m1, c1, m1, c1)) + 4 * D * U * tr
    # eps equals the restatement with the same eps
    e = R.ref_frechet(m1, c1, m2, c2, eps=0.125)
    rese, _, _ = _frechet(m1, c1, m2, c2, eps=0.125)
    assert abs(rese[4] - e["trace_sqrt"]) <= R.frechet_bound(e)
    assert abs(rese[2] - e["trace_real"]) <= D * U * e["trace_real"]


def test_frechet_diagonal_closed_form():
    rs = np.random.RandomState(3)
    for D in (5, 40):
        a, b, m1, m2 = rs.uniform(0.5, 3, D), rs.uniform(0.5, 3, D), rs.randn(D), rs.randn(D)
        res, eig, info = _frechet(m1, np.diag(a), m2, np.diag(b))
        want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
        assert info == [0, -1, 0, 0, 0]                                     # already diagonal: no sweep
        bound = R.frechet_bound(R.ref_frechet(m1, np.diag(a), m2, np.diag(b)))
        assert abs(res[0] - want) <= 2 * bound + 8 * D * U * (a.sum() + b.sum())
        assert np.abs(eig - a * b).max() <= 4 * U * (a * b).max()


def _features_with(cov_seed, N, D, const=None, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(N, D) @ np.linalg.cholesky(R.spd(D, cov_seed)).T + rs.randn(D)
    if const is not None:
        x[:, const] = 0.75
    return x.astype(np.float32)


@pytest.mark.parametrize("view", ["dense", "strided"])
def test_frechet_distance_of_features(view):
    from hipvae import quality as Q
    D = 12
    real, fake = _features_with(1, 400, D, seed=1), _features_with(2, 333, D, seed=2)

    def want_of(a, b, eps=0.0):
        (m1, c1), (m2, c2) = R.ref_cov(a), R.ref_cov(b)
        r = R.ref_frechet(m1, c1, m2, c2, eps)
        e = np.eye(D) * eps
        return r, R.frechet_bound(r, c1 + e, c2 + e), np.trace(c1) + np.trace(c2) + 2 * D * eps

    def check(got, a, b, eps=0.0, swapped=False):
        r, bound, tr = want_of(b, a, eps) if swapped else want_of(a, b, eps)
        print("fd", got["frechet"], "error / bound", abs(got["frechet"] - r["frechet"]) / (2 * bound + 2e-12 * tr))
        assert abs(got["trace_sqrt"] - r["trace_sqrt"]) <= bound
        assert abs(got["frechet"] - r["frechet"]) <= 2 * bound + 2e-12 * tr
        rt, ft = (r["trace_fake"], r["trace_real"]) if swapped else (r["trace_real"], r["trace_fake"])
        assert abs(got["trace_real"] - rt) <= 1e-12 * tr and abs(got["trace_fake"] - ft) <= 1e-12 * tr

    V = VIEWS[view]
    got = Q.frechet_distance(V(real), V(fake))
    assert sorted(got) == sorted(["frechet", "mean_term", "trace_real", "trace_fake", "trace_sqrt", "eigenvalues"])
    check(got, real, fake)
    again = Q.frechet_distance(V(real), V(fake))
    assert all(again[k] == got[k] for k in got if k != "eigenvalues") and torch.equal(again["eigenvalues"], got["eigenvalues"])
    same = Q.frechet_distance(V(real), V(real))
    _, bound, tr = want_of(real, real)
    assert abs(same["frechet"]) <= 2 * bound + 2e-12 * tr
    # a constant column in the fakes: the second covariance may be singular
    fake_c, real_c = _features_with(2, 333, D, const=4, seed=2), _features_with(1, 400, D, const=4, seed=1)
    check(Q.frechet_distance(V(real), V(fake_c)), real, fake_c)
    # a constant column in the reals: the roles are exchanged, the traces keep their names
    check(Q.frechet_distance(V(real_c), V(fake)), real_c, fake, swapped=True)
    # in both: refused, naming both dimensions and the way out; eps > 0 then equals the restatement with that eps
    with pytest.raises(ValueError, match=r"dimension 4 of the real features and of dimension 4 of the fake.*eps > 0"):
        Q.frechet_distance(V(real_c), V(fake_c))
    check(Q.frechet_distance(V(real_c), V(fake_c), eps=1e-6), real_c, fake_c, eps=1e-6)


# ---- all four: refusals ----------------------------------------------------------------------------------------------------
def test_refusals():
    from hipvae import abi
    from hipvae import functional as HF
    from hipvae import quality as Q
    x = torch.randn((40, 6), device=dev())
    bad = x.clone()
    bad[7, 2] = float("nan")
    inf = x.clone()
    inf[39, 5] = float("inf")
    for b in (bad, inf):
        for call in (lambda: Q.knn_radius(b, 3), lambda: Q.prdc(x, b, 3), lambda: Q.prdc(b, x, 3),
                     lambda: Q.kernel_distance(x, b), lambda: Q.kernel_distance(b, x), lambda: Q.frechet_distance(b, x)):
            with pytest.raises(ValueError, match="non-finite"):
                call()
    with pytest.raises(ValueError, match="limit of 512"):
        Q.frechet_distance(torch.zeros((4, 513), device=dev()), torch.zeros((4, 513), device=dev()))
    c = x.cpu()
    for call in (lambda: Q.knn_radius(c, 3), lambda: Q.prdc(c, c, 3), lambda: Q.kernel_distance(c, c),
                 lambda: Q.frechet_distance(c, c)):
        with pytest.raises(abi.HipExtensionError, match="HIP kernels need device tensors"):
            call()
    # every out-of-range argument returns non-zero before a launch: the outputs keep their fill
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=dev())          # noqa: E731
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=dev())              # noqa: E731
    p = lambda t: t.data_ptr()                                                      # noqa: E731
    y = torch.randn((30, 6), device=dev())
    r2, r2y, hits, cov, rmin, res, flags = f64(40), f64(30), i32(30), i32(40), f64(40), f64(5), i32(2)
    eig, info, m, C = f64(6), i32(5), f64(6), f64(6, 6)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    st, W = abi.stream(), ws.numel()
    big = 1 << 20
    calls = [
        ("itcv_knn_radius", p(x), 6, 1, 6, 1, 0, p(r2), p(flags), p(ws), W, st),              # N = 1
        ("itcv_knn_radius", p(x), 6, big + 1, 6, 1, 0, p(r2), p(flags), p(ws), W, st),
        ("itcv_knn_radius", p(x), 6, 40, 0, 1, 0, p(r2), p(flags), p(ws), W, st),             # D = 0
        ("itcv_knn_radius", p(x), 2049, 40, 2049, 1, 0, p(r2), p(flags), p(ws), W, st),
        ("itcv_knn_radius", p(x), 6, 40, 6, 0, 0, p(r2), p(flags), p(ws), W, st),             # k = 0
        ("itcv_knn_radius", p(x), 6, 40, 6, 17, 0, p(r2), p(flags), p(ws), W, st),
        ("itcv_knn_radius", p(x), 6, 5, 6, 5, 0, p(r2), p(flags), p(ws), W, st),              # k = N
        ("itcv_knn_radius", p(x), 6, 40, 6, 3, -1, p(r2), p(flags), p(ws), W, st),            # splits < 0
        ("itcv_knn_radius", p(x), 5, 40, 6, 3, 0, p(r2), p(flags), p(ws), W, st),             # stride below D
        ("itcv_knn_radius", None, 6, 40, 6, 3, 0, p(r2), p(flags), p(ws), W, st),
        ("itcv_knn_radius", p(x), 6, 40, 6, 3, 0, p(r2), p(flags), p(ws), 8, st),             # short workspace
        ("itcv_prdc_counts", p(x), 6, p(y), 6, 1, 30, 6, p(r2), p(r2y), 0, p(hits), p(cov), p(rmin), p(flags), st),
        ("itcv_prdc_counts", p(x), 6, p(y), 6, 40, big + 1, 6, p(r2), p(r2y), 0, p(hits), p(cov), p(rmin), p(flags), st),
        ("itcv_prdc_counts", p(x), 6, p(y), 6, 40, 30, 2049, p(r2), p(r2y), 0, p(hits), p(cov), p(rmin), p(flags), st),
        ("itcv_prdc_counts", p(x), 6, p(y), 5, 40, 30, 6, p(r2), p(r2y), 0, p(hits), p(cov), p(rmin), p(flags), st),
        ("itcv_prdc_counts", p(x), 6, p(y), 6, 40, 30, 6, p(r2), p(r2y), -2, p(hits), p(cov), p(rmin), p(flags), st),
        ("itcv_prdc_counts", p(x), 6, p(y), 6, 40, 30, 6, None, p(r2y), 0, p(hits), p(cov), p(rmin), p(flags), st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 1, 30, 6, 3, 0.0, 1.0, p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 1, 6, 3, 0.0, 1.0, p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 30, 2049, 3, 0.0, 1.0, p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 30, 6, 0, 0.0, 1.0, p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 30, 6, 5, 0.0, 1.0, p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 30, 6, 3, -1.0, 1.0, p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 30, 6, 3, 0.0, float("nan"), p(res), p(flags), p(ws), W, st),
        ("itcv_poly_mmd", p(x), 6, p(y), 6, 40, 30, 6, 3, 0.0, 1.0, p(res), p(flags), p(ws), 64, st),
        ("itcv_frechet", p(m), p(C), p(m), p(C), 0, 0.0, p(res), p(eig), p(info), p(ws), W, st),
        ("itcv_frechet", p(m), p(C), p(m), p(C), 513, 0.0, p(res), p(eig), p(info), p(ws), 1 << 30, st),
        ("itcv_frechet", p(m), p(C), p(m), p(C), 6, -1e-9, p(res), p(eig), p(info), p(ws), W, st),
        ("itcv_frechet", p(m), p(C), p(m), p(C), 6, float("inf"), p(res), p(eig), p(info), p(ws), W, st),
        ("itcv_frechet", p(m), None, p(m), p(C), 6, 0.0, p(res), p(eig), p(info), p(ws), W, st),
        ("itcv_frechet", p(m), p(C), p(m), p(C), 6, 0.0, p(res), p(eig), p(info), p(ws), 16, st),
    ]
    for name, *args in calls:
        assert getattr(abi.lib, name)(*args) != 0, (name, args)
        assert abi.last_error().startswith(name), abi.last_error()
    torch.cuda.synchronize()
    for t in (r2, r2y, rmin, res, eig, m, C):
        assert (t == 7.0).all()
    for t in (hits, cov, flags, info):
        assert (t == 7).all()
    assert abi.lib.itcv_knn_radius_workspace(1, 6, 1, 0) == 0 and abi.lib.itcv_poly_mmd_workspace(40, 1, 6) == 0
    assert abi.lib.itcv_frechet_workspace(513) == 0 and abi.lib.itcv_knn_radius_workspace(40, 6, 3, -1) == 0
    # the workspace does not grow with N^2: s * N * (k + 1) doubles, s <= 256
    assert abi.lib.itcv_knn_radius_workspace(10000, 128, 5, 0) == 4 * 10000 * 6 * 8
    assert abi.lib.itcv_knn_radius_workspace(big, 128, 16, 0) == big * 17 * 8
    assert abi.lib.itcv_poly_mmd_workspace(big, big, 2048) == 3 * 1024 * 8
    assert HF.unsup_gauss_lds_dim() == 128


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_model():
    import models
    torch.manual_seed(0)
    return models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()


@pytest.fixture(scope="module")
def images():
    return torch.from_numpy(np.random.default_rng(4).random((96, 3, 32, 32), dtype=np.float32))


class _Images:
    def __init__(self, t):
        self.t = t

    def __len__(self):
        return len(self.t)

    def __getitem__(self, i):
        return self.t[i]


class _Recorder:
    def __init__(self):
        self.log = {}

    def add_scalar(self, tag, value, global_step=None):
        self.log[tag] = (float(value), global_step)

    def add_scalars(self, tag, values, global_step=None):
        self.log[tag] = ({k: float(v) for k, v in values.items()}, global_step)

    def flush(self):
        pass


SIX = ("frechet", "kid", "precision", "recall", "density", "coverage")


def test_compute_sample_quality(tiny_model, images):
    from hipvae import quality as Q
    model, ds = tiny_model, _Images(images)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    a = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3)
    assert sorted(a) == sorted(SIX + ("kid_std", "features", "indices"))
    real, fake = a["features"]["real"], a["features"]["fake"]
    assert real.shape == (96, 10) and fake.shape == (64, 10) and real.is_cuda and real.dtype == torch.float32
    assert a["indices"].tolist() == list(range(96))
    print({k: a[k] for k in SIX})
    assert all(isinstance(a[k], float) and np.isfinite(a[k]) for k in SIX)
    # each equals the public function applied to the returned features, bitwise
    assert a["frechet"] == Q.frechet_distance(real, fake)["frechet"]
    assert a["kid"] == Q.kernel_distance(real, fake)["kid"] and a["kid_std"] == 0.0
    assert {k: a[k] for k in SIX[2:]} == Q.prdc(real, fake, 5)
    assert torch.equal(real, Q.real_features(ds, model, np.arange(96), batch_size=40))
    assert torch.equal(fake, Q.generated_features(model, 64, batch_size=40, seed=3))
    b = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3)
    assert all(a[k] == b[k] for k in SIX) and torch.equal(b["features"]["fake"], fake)
    c = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=4)
    assert not torch.equal(c["features"]["fake"], fake) and torch.equal(c["features"]["real"], real)
    # the flag and every buffer as found; torch's generators untouched
    assert model.training and all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state(dev()))
    # a subset of the scores, a subsample of the images, a callable feature
    sub = Q.compute_sample_quality(ds, model, num_real=50, num_fake=None, seed=1, scores=("prdc",), nearest_k=3)
    assert sorted(sub) == sorted(SIX[2:] + ("features", "indices")) and sub["features"]["fake"].shape == (50, 10)
    assert sub["indices"].tolist() == np.sort(np.random.RandomState(1).choice(96, 50, replace=False)).tolist()
    pix = Q.compute_sample_quality(ds, model, num_fake=64, scores=("kid",),
                                   feature=lambda im: im.flatten(1)[:, ::97].double())
    assert pix["features"]["real"].shape == (96, 32) and pix["features"]["real"].dtype == torch.float32
    assert torch.equal(pix["features"]["real"], images.flatten(1)[:, ::97].to(dev()))
    with pytest.raises(ValueError, match="unknown score"):
        Q.compute_sample_quality(ds, model, scores=("fid",))
    with pytest.raises(ValueError, match="feature"):
        Q.compute_sample_quality(ds, model, feature="inception")
    assert model.training


def test_solver_writes_the_sample_quality_record(tiny_model, images):
    from hipvae import quality as Q
    from hipvae.dataset import DeviceImageTable
    from solvers import VAESolver
    model = tiny_model
    u8 = (images.permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)
    table = DeviceImageTable.from_arrays(u8, None, dev())

    def solver_of(dataset):
        return VAESolver(dataset=dataset, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                         optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                         beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=_Recorder(), test_iter=5,
                         clip=100.0)

    solver = solver_of(table)
    assert solver.quality_params is None
    solver.extra_scores, solver.quality_params = ("sample_quality",), dict(num_fake=64, seed=2)
    solver.write_disentanglemnt_scores(3)
    assert not solver.writer.log                                      # cur_iter % test_iter != 0: nothing
    solver.write_disentanglemnt_scores(10)
    assert list(solver.writer.log) == ["sample_quality"]
    rec, step = solver.writer.log["sample_quality"]
    want = Q.compute_sample_quality(table, model, num_fake=64, seed=2, batch_size=16)
    assert step == 10 and list(rec) == list(SIX) and rec == {k: want[k] for k in SIX} and model.training
    solver.extra_scores = ("sample_quality", "nope")
    with pytest.raises(ValueError, match=r"unknown score\(s\) \['nope'\].*'log_likelihood', 'sample_quality'\)"):
        solver.write_disentanglemnt_scores(10)
