"""CPU only: pins the numpy restatement of the Gaussian-mixture kernels (tests/gmm_ref.py) and the conditions on the inputs
that tests/test_hip_gmm.py relies on.

Against sklearn (skipped where it is not installed).  ``sklearn.mixture.GaussianMixture(covariance_type="full")`` from
``weights_init``, ``means_init``, ``precisions_init = I`` with ``tol = 0``, ``max_iter = n`` against the restatement's fit from
the same triple for n iterations: weights, means, covariances, ``score_samples`` and ``lower_bound_``.  Cases (N, D, K, n)
= (300, 5, 3, 5), (2000, 33, 4, 8), (4000, 128, 5, 6); every component keeps Nk >= 2 D in each.  Measured with sklearn
1.7.2 (largest relative difference, max |a - b| / max |b|, over the five quantities): 5.2e-16, 1.9e-15, 3.0e-13 (the last
on ``score_samples``; 4.5e-14 on the covariances).  Asserted with a margin of 1000 over the largest, 3e-10: BLAS sums in
another order on another machine.

Conditions, asserted on the restatement alone for every shape of ``gmm_ref.FIT_SHAPES``: at every hard E-step of the
k-means initialisation no row's two smallest distances lie within 1e-9 relative of each other, so the hard assignments do
not depend on the rounding order; every component keeps Nk >= 2 D at every EM iteration; every Cholesky succeeds;
|L_k|_2 |Linv_k|_2 stays below ``gmm_ref.COND_MAX``.

Order sensitivity of the fit.  The restatement's fit on the rows in reverse order (every sum over rows then runs the other
way) against the fit on the rows as they are, from the same initial parameters: the largest relative difference over the
weights, means, covariances and ``history`` of both fits of every shape was 1.2e-15 (measured here); it is pinned, with
room for another BLAS, as ``gmm_ref.ORDER_SENSITIVITY`` = 4e-15, the yardstick of the device fit's tolerance."""
import numpy as np
import pytest

import gmm_ref as R


def _clusters(N, D, K, seed):
    x = R.make_data(N, D, K, seed=seed, sep=2.5).astype(np.float64)
    ll = R.lloyd(x, K, 3, seed=1)
    return x, ll


@pytest.mark.parametrize("N,D,K,n", [(300, 5, 3, 5), (2000, 33, 4, 8), (4000, 128, 5, 6)])
def test_fit_against_sklearn(N, D, K, n):
    mixture = pytest.importorskip("sklearn.mixture")
    import warnings
    x, ll = _clusters(N, D, K, 11)
    eye = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    got = R.fit(x, (ll["weights"], ll["means"], eye), max_iter=n, tol=0.0)
    assert got["n_iter"] == n and min(got["nk_min"]) >= 2 * D
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = mixture.GaussianMixture(K, covariance_type="full", weights_init=ll["weights"], means_init=ll["means"],
                                     precisions_init=eye, tol=0.0, max_iter=n, reg_covar=1e-6).fit(x)
    diffs = dict(weights=R.rel_diff(got["weights"], sk.weights_), means=R.rel_diff(got["means"], sk.means_),
                 covariances=R.rel_diff(got["covariances"], sk.covariances_),
                 score_samples=R.rel_diff(R.log_prob(got, x), sk.score_samples(x)),
                 lower_bound=R.rel_diff(got["history"][-1], sk.lower_bound_))
    print((N, D, K, n), diffs)
    assert max(diffs.values()) <= 3e-10, diffs


@pytest.mark.parametrize("N,D,K", R.FIT_SHAPES)
def test_conditions_on_the_inputs(N, D, K):
    ref = R.reference(N, D, K)
    ll = ref["lloyd"]
    assert len(ll["gaps"]) == R.KMEANS_ITERS + 1 and min(ll["gaps"]) > 1e-9, ll["gaps"]
    assert ll["resp"].sum(0).min() >= 2 * D
    for name in ("fit", "fit_eye"):
        f = ref[name]                                               # a failed pivot would have raised in the restatement
        print((N, D, K), name, "n_iter", f["n_iter"], "converged", f["converged"], "nk_min", min(f["nk_min"]), "cond",
              max(f["cond"]))
        assert 2 <= f["n_iter"] <= R.FIT_ITERS
        assert min(f["nk_min"]) >= 2 * D
        assert max(f["cond"]) < R.COND_MAX and np.isfinite(f["history"]).all()
    w, means, cov = R.make_params(D, K)
    chol, linv, _, info = R.factor(cov)
    assert not info.any() and R.condition(chol, linv) < R.COND_MAX
    assert any(ref[name]["n_iter"] > 2 for name in ("fit", "fit_eye")) or K == 1


def test_some_fit_takes_several_iterations():
    assert max(R.reference(*s)["fit"]["n_iter"] for s in R.FIT_SHAPES[:4]) >= 5


@pytest.mark.parametrize("N,D,K", R.FIT_SHAPES)
def test_order_sensitivity_of_the_fit(N, D, K):
    ref = R.reference(N, D, K)
    ll = ref["lloyd"]
    eye = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    worst = 0.0
    for name, init, tol in (("fit", (ll["weights"], ll["means"], ll["covariances"]), 1e-3),
                            ("fit_eye", (ll["weights"], ll["means"], eye), R.FIT_EYE_TOL)):
        fwd = ref[name]
        rev = R.fit(ref["x"][::-1], init, R.FIT_ITERS, tol=tol)
        assert rev["n_iter"] == fwd["n_iter"] and rev["converged"] == fwd["converged"]
        worst = max([worst] + [R.rel_diff(rev[k], fwd[k]) for k in ("weights", "means", "covariances", "history")])
    print((N, D, K), "order sensitivity", worst)
    assert worst <= R.ORDER_SENSITIVITY


def test_pieces_of_the_restatement():
    rng = np.random.default_rng(5)
    # the factor: L L^T = C, Linv L = I, logdet
    _, _, cov = R.make_params(33, 2)
    chol, linv, logdet, info = R.factor(cov)
    for k in range(2):
        assert np.allclose(chol[k] @ chol[k].T, cov[k], rtol=0, atol=1e-13) and np.array_equal(chol[k], np.tril(chol[k]))
        assert np.allclose(linv[k] @ chol[k], np.eye(33), rtol=0, atol=1e-13)
        assert abs(logdet[k] - np.linalg.slogdet(cov[k])[1]) < 1e-12
    bad = cov.copy()
    bad[1][:, 7] = bad[1][:, 3]
    bad[1][7, :] = bad[1][3, :]
    info = R.factor(bad)[3]
    assert info[0] == 0 and info[1] >= 8          # dimension 7 or, past a pivot of rounding noise, a later one
    # the row sum is a sum; integers are exact
    v = rng.integers(-50, 50, (1300, 3)).astype(np.float64)
    assert np.array_equal(R.row_sum(v), v.sum(0))
    assert R.block_sums(v[:, 0]) == v[:, 0].sum()
    # E-step against the textbook density
    x = rng.standard_normal((50, 33)).astype(np.float32)
    w, means, _ = R.make_params(33, 2)
    lp, resp, lse, total = R.estep(x, w, means, linv, logdet)
    for k in range(2):
        d = x.astype(np.float64) - means[k]
        want = np.log(w[k]) - 0.5 * (33 * np.log(2 * np.pi) + np.linalg.slogdet(cov[k])[1]
                                     + np.einsum("ni,ij,nj->n", d, np.linalg.inv(cov[k]), d))
        assert np.allclose(lp[:, k], want, rtol=1e-12)
    assert np.allclose(resp.sum(1), 1.0) and abs(total - lse.sum()) < 1e-10
    hard = R.estep(x, w, means, linv, logdet, hard=True)
    assert np.array_equal(hard[1].argmax(1), lp.argmax(1)) and np.array_equal(hard[1].sum(1), np.ones(50))
    # M-step with unit responsibilities is the biased covariance
    nk, w1, m1, c1 = R.mstep(x, np.ones((50, 1)), reg=0.5)
    assert nk[0] == 50.0 and w1[0] == 1.0 and np.allclose(m1[0], x.astype(np.float64).mean(0), rtol=1e-14)
    assert np.allclose(c1[0], np.cov(x.astype(np.float64).T, bias=True) + 0.5 * np.eye(33), rtol=0, atol=1e-13)
    assert np.array_equal(c1[0], c1[0].T)
    # the sampler
    comp = rng.integers(0, 2, 20).astype(np.int32)
    eps = rng.standard_normal((20, 33)).astype(np.float32)
    z = R.sample(means, chol, comp, eps)
    assert z.dtype == np.float32
    assert np.allclose(z, means[comp] + np.einsum("nij,nj->ni", chol[comp], eps.astype(np.float64)), rtol=1e-6)
    assert abs(R.LOG2PI - np.log(2 * np.pi)) < 1e-15


def test_abi_and_makefile():
    import os
    import re
    from hipvae import abi
    for name in ("itcv_gmm_factor", "itcv_gmm_estep_workspace", "itcv_gmm_estep", "itcv_gmm_mstep_workspace",
                 "itcv_gmm_mstep", "itcv_gmm_sample"):
        assert name in abi.SIGNATURES and hasattr(abi.lib, name), name
    assert abi.ABI_VERSION == 4
    with open(os.path.join(abi.CSRC, "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\bgmm\.hip\b", f.read(), re.M)
    lib = abi.lib
    assert lib.itcv_gmm_estep_workspace(5, 3, 6) == 0 and lib.itcv_gmm_estep_workspace(10, 513, 2) == 0
    assert lib.itcv_gmm_mstep_workspace(100, 3, 65, 1) == 0 and lib.itcv_gmm_mstep_workspace(100, 3, 2, 1) > 0
    assert lib.itcv_gmm_mstep_workspace(100, 3, 2, 0) < lib.itcv_gmm_mstep_workspace(100, 3, 2, 1)
