"""CPU tests that pin tests/quality_ref.py, the numpy restatement tests/test_hip_quality.py holds the kernels to, and
that assert what the GPU tests rely on in their inputs: the integer recipe exercises every comparison (counts strictly
inside their ranges, pairs exactly ON a radius, tied neighbours), and the Gaussian recipe has no pair near a radius."""
import inspect
import os

import numpy as np
import pytest

import quality_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Frechet ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 16, 33])
def test_frechet_against_sqrtm(D):
    scipy_linalg = pytest.importorskip("scipy.linalg")
    rs = np.random.RandomState(D)
    c1, c2, m1, m2 = R.spd(D, 1), R.spd(D, 2), rs.randn(D), rs.randn(D)
    r = R.ref_frechet(m1, c1, m2, c2)
    root = scipy_linalg.sqrtm(c1 @ c2)
    want = ((m1 - m2) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(root).real
    assert abs(r["frechet"] - want) <= 1e-10 * (np.trace(c1) + np.trace(c2))
    assert abs(R.ref_frechet(m1, c1, m1, c1)["frechet"]) <= 2 * R.frechet_bound(R.ref_frechet(m1, c1, m1, c1)) + 1e-13 * D
    # eps: the same as adding it to both diagonals
    e = R.ref_frechet(m1, c1, m2, c2, eps=0.25)
    assert e["frechet"] == R.ref_frechet(m1, c1 + 0.25 * np.eye(D), m2, c2 + 0.25 * np.eye(D))["frechet"]


def test_frechet_closed_form_for_diagonal_covariances():
    rs = np.random.RandomState(0)
    a, b, m1, m2 = rs.uniform(0.5, 3, 12), rs.uniform(0.5, 3, 12), rs.randn(12), rs.randn(12)
    r = R.ref_frechet(m1, np.diag(a), m2, np.diag(b))
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(r["frechet"] - want) <= 1e-12 * (a.sum() + b.sum())
    with pytest.raises(np.linalg.LinAlgError):
        R.ref_frechet(m1, np.diag(np.r_[a[:-1], 0.0]), m2, np.diag(b))
    # a singular SECOND covariance is fine
    s = R.ref_frechet(m1, np.diag(a), m2, np.diag(np.r_[b[:-1], 0.0]))
    assert abs(s["trace_sqrt"] - np.sqrt(a[:-1] * b[:-1]).sum()) <= 1e-12 * a.sum()


# ---- KID -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_poly_against_a_double_loop(p):
    rs = np.random.RandomState(p)
    x, y = rs.randn(5, 3).astype(np.float32), rs.randn(4, 3).astype(np.float32)
    r = R.ref_poly(x, y, degree=p)
    kap = lambda a, b: (float(np.dot(a.astype(np.float64), b.astype(np.float64))) / 3.0 + 1.0) ** p      # noqa: E731
    sxx = sum(kap(x[i], x[j]) for i in range(5) for j in range(5) if i != j)
    syy = sum(kap(y[i], y[j]) for i in range(4) for j in range(4) if i != j)
    sxy = sum(kap(x[i], y[j]) for i in range(5) for j in range(4))
    for got, want in ((r["Sxx"], sxx), (r["Syy"], syy), (r["Sxy"], sxy)):
        assert abs(got - want) <= 1e-13 * max(r["abs"])
    assert abs(r["mmd2"] - (sxx / 20.0 + syy / 12.0 - 2.0 * sxy / 20.0)) <= 1e-13
    assert R.ref_poly(x, y, degree=p, gamma=0.5)["Sxy"] != r["Sxy"]


# ---- PRDC ------------------------------------------------------------------------------------------------------------------
def test_prdc_against_brute_force():
    real, fake = R.integer_features(23, 17, 5, seed=3)
    k = 2
    r = R.ref_prdc(real, fake, k)
    dist = lambda a, b: sum((float(u) - float(v)) ** 2 for u, v in zip(a, b))                            # noqa: E731
    rad = lambda rows, i: sorted(dist(rows[i], o) for o in rows)[k]                                      # noqa: E731
    r2r, r2f = [rad(real, i) for i in range(23)], [rad(fake, j) for j in range(17)]
    assert r["r2_real"].tolist() == r2r and r["r2_fake"].tolist() == r2f
    hits = [sum(dist(real[i], fake[j]) < r2r[i] for i in range(23)) for j in range(17)]
    cov = [int(any(dist(real[i], fake[j]) < r2f[j] for j in range(17))) for i in range(23)]
    mins = [min(dist(real[i], fake[j]) for j in range(17)) for i in range(23)]
    assert r["fake_hits"].tolist() == hits and r["real_covered"].tolist() == cov and r["real_min"].tolist() == mins
    assert r["precision"] == sum(h > 0 for h in hits) / 17 and r["recall"] == sum(cov) / 23
    assert r["density"] == sum(hits) / (k * 17) and r["coverage"] == sum(m < q for m, q in zip(mins, r2r)) / 23


@pytest.mark.parametrize("N,M,D,k", R.RICH)
def test_integer_recipe_exercises_every_comparison(N, M, D, k):
    real, fake, r = R.restated("integer", N, M, D, k)
    assert np.array_equal(real, np.rint(real)) and np.abs(real).max() < 2 ** 20 and np.abs(fake).max() < 2 ** 20
    assert np.array_equal(r["d2"], np.rint(r["d2"])) and r["d2"].max() < 2.0 ** 50          # exact in any order
    c = r["counts"]
    print((N, M, D, k), "scores", r["precision"], r["recall"], r["density"], r["coverage"])
    assert 0 < c[0] < M and 0 < c[2] < N * M and 0 < c[3] < N
    on = int((r["d2"] == r["r2_real"][:, None]).sum() + (r["d2"] == r["r2_fake"][None, :]).sum())
    print("pairs exactly on a radius:", on)
    assert on >= 1                                                     # `<` against `<=` would change a count
    srt = np.sort(r["d2_real"], axis=1)
    assert (srt[:, k] == srt[:, k + 1]).any()                          # the (k+1)-th and (k+2)-th values tie in some row


@pytest.mark.parametrize("N,M,D,k", R.SHAPES)
def test_gaussian_recipe_has_no_pair_near_a_radius(N, M, D, k):
    _, _, r = R.restated("gaussian", N, M, D, k)
    assert R.near_boundary(r) == 0
    assert (r["r2_real"] > 0).all() and (r["r2_fake"] > 0).all()


def test_duplicated_rows_have_radius_zero():
    real = np.repeat(np.arange(6, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32), 2, axis=0)
    r = R.ref_prdc(real, real.copy(), 1)
    assert (r["r2_real"] == 0).all() and r["counts"] == (0, 0, 0, 0)   # nothing is STRICTLY inside a radius of 0


# ---- the sources say what the tests assume -------------------------------------------------------------------------------
def test_sources_state_the_rules():
    hip = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "quality.hip")).read()
    assert "#pragma clang fp contract(off)" in hip and "mfma_f64_16x16x4f64" in hip
    assert "atomicAdd(&chits" in hip
    for line in hip.splitlines():                                      # no floating-point atomic
        if "atomic" in line and "(" in line and not line.lstrip().startswith("//"):
            assert any(t in line for t in ("chits", "qcov", "qmin", "flags")), line
    mk = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "Makefile")).read()
    assert "quality.hip" in mk
    hdr = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    for fn in ("itcv_knn_radius_workspace", "itcv_knn_radius", "itcv_prdc_counts", "itcv_poly_mmd_workspace",
               "itcv_poly_mmd", "itcv_frechet_workspace", "itcv_frechet"):
        assert fn + "(" in hdr
    assert "#define ITCV_ABI_VERSION 4" in hdr
    src = open(os.path.join(ROOT, "intro-tc-vae_amd", "solvers", "vae.py")).read()
    assert "self.quality_params = None" in src
    from solvers import scores
    assert scores.TABLE["sample_quality"].params == "quality_params" and not scores.TABLE["sample_quality"].factors


def test_restatement_accumulates_in_ascending_order():
    assert "for d in range(a.shape[1])" in inspect.getsource(R.d2_matrix)
    a = np.array([[1e8, 1.0, -1.0]], dtype=np.float32)
    b = np.zeros((1, 3), dtype=np.float32)
    assert R.d2_matrix(a, b)[0, 0] == (1e16 + 1.0) + 1.0
