"""The Gaussian-mixture kernels (csrc/gmm.hip) and their host path (hipvae/density.py) against the numpy restatement
tests/gmm_ref.py, which adds in the kernels' order wherever that order is documented.

Shapes (N, D, K) of ``gmm_ref.SHAPES``, each run dense and as the right part of a wider NaN-padded tensor:
  (7, 1, 1)      one partial 16-row MFMA tile, one padded 4-column MFMA step, the smallest everything;
  (40, 3, 2)     a partial 64-row block with a partial last wave, D < 4;
  (600, 5, 3)    several 64-row blocks and 256-row blocks of the log-likelihood sum, two row slices in the M-step, a fit that
                 takes many iterations;
  (130, 17, 3)   a second 16-column tile holding one column (the first off-diagonal tile of Linv is skipped, the diagonal
                 one masked); the last row tile ragged;
  (300, 33, 4)   three column tiles, six tile pairs in the covariance;
  (1100, 128, 5) the LDS limit of the factor kernel; three row slices in the M-step (single launches only: a component has
                 220 rows < 2 D);
  (700, 131, 2)  the factor kernel working in global memory; D + 1 = 132 columns: three 64-column tiles of the column sums;
  (1200, 512, 1) the largest D; with K = 1 one iteration is itcv_unsup_cov's mean and its covariance times (N - 1) / N + reg.

Bounds.  u = 2^-53, g(n) = 1.01 n u.  Any two ways of adding n rounded products differ by at most 2 g(n) sum |terms|.
* Factor.  The computed factor of C is the exact factor of C + dC with |dC| <= g(D + 1) |L||L^T| (Higham, Accuracy and
  Stability, Thm 10.3), |L||L^T| <= D |C|_2 in norm, and the factor moves by at most cond(C) |dC|_F / |C|_2 |L|_2 / sqrt 2
  to first order (Sun 1991).  Two computations therefore differ by less than tol_L = 2 cond(C) D (D + 1) u |L|_2 with
  cond(C) = (|L|_2 |Linv|_2)^2 < COND_MAX^2, the figure tests/test_gmm_ref_host.py pins.  Forward substitution gives Linv
  to g(D) D cond(L) |Linv|_2 and follows L as |Linv|_2^2 tol_L: tol_Linv = |Linv|_2 (2 D^2 u COND_MAX + |Linv|_2 tol_L).
  logdet = 2 sum log L_ii: 2 D tol_L max(1 / L_ii) + 4 D u sum |log L_ii| + 4 u.
* E-step.  y_i = sum_j Linv_ij (x_j - m_j) has the terms ay_i = sum_j |Linv_ij| |x_j - m_j| (from the restatement):
  dy_i <= 2 g(D + 2) ay_i, |y_i| <= ay_i; q = sum y_i^2 in one order on both sides: dq <= 4 g(D + 2) sum ay_i^2 + 2 g(D + 1) q;
  dlp = dq / 2 + 4 u (|log w| + |D log 2 pi + logdet| + q + |lp|).  The log-sum-exp is 1-Lipschitz in the max norm: dlse =
  max_k dlp + (K + 8) u (1 + |lse|); resp = exp(lp - lse): dresp = 1.01 resp (dlp + dlse + 4 u (1 + |lp| + |lse|));
  sum_loglik: sum dlse + 2 g(N) sum |lse|.
* M-step.  nk: 2 g(N) nk.  mean: dm_i = 1.01 (2 g(N + 2) sum_n |r x_i| / nk + |m_i| dnk / nk).  Covariance, with b = x - m,
  mag_ij = sum_n |r b_i| |b_j| / nk and B_j = sum_n r |b_j| / nk: 2 g(N + 3) mag_ij + dm_i B_j + dm_j B_i + |C_ij| dnk / nk.
  (The restatement adds the column sums in the kernel's order, so nk and the means come out equal bit for bit in practice.)
* Identity factors: products with 0 and 1 are exact whatever the order inside a matrix-core product, so the hard E-step of
  the k-means initialisation is compared bit for bit on integer-valued rows, and its assignments and centres are equal on
  the real-valued test inputs (no near ties: tests/test_gmm_ref_host.py).
* Fit.  n_iter, converged equal; history, weights, means, covariances within 100 x ORDER_SENSITIVITY = 4e-13 relative
  (max |a - b| / max |b|): ORDER_SENSITIVITY = 4e-15 is what reversing the row order of every sum does to the restatement's
  own fit (measured 1.2e-15, pinned in tests/test_gmm_ref_host.py); the margin of 100 is for the ill-conditioning that
  compounds over up to 20 iterations and for exp / log differing by an ulp between the two libraries."""
import numpy as np
import pytest
import torch

import gmm_ref as R

pytestmark = pytest.mark.gpu

U = R.U
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
FIT_RTOL = 100 * R.ORDER_SENSITIVITY


def g(n):
    return 1.01 * n * U


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


def HFD():
    from hipvae import density, functional
    return functional, density


def within(got, want, tol, what):
    err = np.abs(N_(got) - want)
    bad = err > tol
    print(what, "max err", float(err.max()), "max err / tol", float(np.max(err / np.maximum(tol, 1e-300))))
    assert not bad.any(), (what, float(err.max()), float(np.max(err / np.maximum(tol, 1e-300))))


def record(params):
    """A GaussianMixture on the device from restatement parameters (weights, means, covariances)."""
    _, Dn = HFD()
    w, means, cov = params
    chol, linv, logdet, info = R.factor(cov)
    assert not info.any()
    return Dn.GaussianMixture(G(w), G(means), G(cov), G(chol), G(linv), G(logdet)), (chol, linv, logdet)


# ---- single launches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", sorted({(s[1], s[2]) for s in R.SHAPES}))
def test_factor(D, K):
    HF, _ = HFD()
    _, _, cov = R.make_params(D, K)
    chol, linv, logdet, info = R.factor(cov)
    assert not info.any() and R.condition(chol, linv) < R.COND_MAX
    cov_t = G(cov)
    got = HF.gmm_factor(cov_t)
    assert torch.equal(cov_t, G(cov)) and N_(got[3]).tolist() == [0] * K
    for k in range(K):
        nL, nX = np.linalg.norm(chol[k], 2), np.linalg.norm(linv[k], 2)
        tol_L = 2 * R.COND_MAX ** 2 * D * (D + 1) * U * nL
        tol_X = nX * (2 * D * D * U * R.COND_MAX + nX * tol_L)
        dg = np.diag(chol[k])
        tol_ld = 2 * D * tol_L * np.max(1 / dg) + 4 * D * U * np.abs(np.log(dg)).sum() + 4 * U
        within(got[0][k], chol[k], tol_L, f"chol[{k}]")
        within(got[1][k], linv[k], tol_X, f"linv[{k}]")
        within(got[2][k], logdet[k], tol_ld, f"logdet[{k}]")
        assert np.array_equal(N_(got[0][k]), np.tril(N_(got[0][k])))        # a clean lower triangle


def test_factor_reports_the_first_failed_pivot():
    HF, _ = HFD()
    _, _, cov = R.make_params(17, 3)
    cov[1] = np.diag([4.0] * 5 + [-1.0] + [4.0] * 11)
    cov[2] = np.diag([9.0] * 16 + [0.0])
    chol, linv, logdet, info = HF.gmm_factor(G(cov))
    assert N_(info).tolist() == [0, 6, 17] == R.factor(cov)[3].tolist()
    assert np.isnan(N_(logdet)[1:]).all() and np.isfinite(N_(logdet)[0]) and np.isfinite(N_(linv[0])).all()


def _estep_bounds(x, w, means, linv, logdet):
    N, D = x.shape
    K = len(w)
    lp, ay, q = R.logp(x, w, means, linv, logdet, bounds=True)
    _, resp, lse, total = R.estep(x, w, means, linv, logdet)
    dq = 4 * g(D + 2) * (ay * ay).sum(2) + 2 * g(D + 1) * q
    dlp = 0.5 * dq + 4 * U * (np.abs(np.log(w)) + np.abs(D * R.LOG2PI + logdet) + q + np.abs(lp))
    dlse = dlp.max(1) + (K + 8) * U * (1 + np.abs(lse))
    dresp = 1.01 * resp * (dlp + dlse[:, None] + 4 * U * (1 + np.abs(lp) + np.abs(lse)[:, None])) + 1e-300
    dsum = dlse.sum() + 2 * g(N) * np.abs(lse).sum()
    return (lp, resp, lse, total), (dlp, dresp, dlse, dsum)


@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,D,K", R.SHAPES)
def test_estep_and_log_prob(N, D, K, view):
    HF, Dn = HFD()
    x = R.shape_input(N, D, K)[0]
    params = R.make_params(D, K)
    gmm, (chol, linv, logdet) = record(params)
    want, tol = _estep_bounds(x, params[0], params[1], linv, logdet)
    xt = VIEWS[view](x)
    flags = HF.disent_flags(dev())
    got = HF.gmm_estep(xt, gmm.weights, gmm.means, gmm.prec_chol, gmm.log_det, flags)
    assert N_(flags).tolist() == [0, 0]
    for name, a, b, t in zip(("lp", "resp", "loglik", "sum_loglik"), got, want, tol):
        within(a, b, t, name)
    assert torch.equal(Dn.gmm_log_prob(gmm, xt), got[2]) and torch.equal(Dn.gmm_responsibilities(gmm, xt), got[1])
    hard = HF.gmm_estep(xt, gmm.weights, gmm.means, gmm.prec_chol, gmm.log_det, flags, hard=True)
    # a row whose two largest lp are closer than their bounds may go either way; every other row is the restatement's
    srt = np.sort(want[0], axis=1)
    sure = np.ones(N, bool) if K == 1 else (srt[:, -1] - srt[:, -2]) > 2 * tol[0].max(1)
    assert sure.mean() > 0.9
    assert np.array_equal(N_(hard[1]).argmax(1)[sure], want[0].argmax(1)[sure])
    assert np.array_equal(N_(hard[1]).sum(1), np.ones(N)) and set(np.unique(N_(hard[1]))) <= {0.0, 1.0}
    assert torch.equal(hard[2], hard[0].max(1).values) and torch.equal(hard[0], got[0])


@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,D,K", R.SHAPES)
def test_hard_estep_on_integers_is_bitwise(N, D, K, view):
    HF, _ = HFD()
    rng = np.random.default_rng([N, D, K])
    x = rng.integers(-8, 9, (N, D)).astype(np.float32)
    centres = rng.integers(-4, 5, (K, D)).astype(np.float64)
    centres[-1] = centres[0]                                            # a tie in every row: the lowest k wins
    ones, zeros = np.ones(K), np.zeros(K)
    eye = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    want = R.estep(x, ones, centres, eye, zeros, hard=True)
    flags = HF.disent_flags(dev())
    got = HF.gmm_estep(VIEWS[view](x), G(ones), G(centres), G(eye), G(zeros), flags, hard=True)
    assert N_(flags).tolist() == [0, 0]
    for name, a, b in zip(("lp", "resp", "loglik"), got, want):
        assert np.array_equal(N_(a), b), name
    assert K == 1 or not N_(got[1])[:, -1].any()
    assert abs(N_(got[3])[0] - want[3]) <= 2 * g(N) * np.abs(want[2]).sum()
    # the centre update of Lloyd's iteration from these assignments: sums of small integers are exact
    nk, _, mean, cov = HF.gmm_mstep(VIEWS[view](x), got[1], flags, with_cov=False)
    rnk, _, rmean, _ = R.mstep(x, want[1], with_cov=False)
    assert cov is None and np.array_equal(N_(nk), rnk) and np.array_equal(N_(mean), rmean)


@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,D,K", R.SHAPES)
def test_mstep(N, D, K, view):
    HF, _ = HFD()
    x = R.shape_input(N, D, K)[0]
    w, means, cov = R.make_params(D, K)
    _, linv, logdet, _ = R.factor(cov)
    resp = R.estep(x, w, means * 0.0, linv, logdet)[1]                   # soft responsibilities of some mixture
    reg = 1e-3
    nk, w2, m2, c2, mag = R.mstep(x, resp, reg, bounds=True)
    x64 = x.astype(np.float64)
    flags = HF.disent_flags(dev())
    got = HF.gmm_mstep(VIEWS[view](x), G(resp), flags, reg=reg)
    assert N_(flags).tolist() == [0, 0]
    dnk = 2 * g(N) * nk
    within(got[0], nk, dnk, "nk")
    within(got[1], w2, 1.01 * (dnk / nk.sum() + w2 * dnk.sum() / nk.sum() + 2 * U), "weights")
    for k in range(K):
        r = resp[:, k:k + 1]
        dm = 1.01 * (2 * g(N + 2) * (r * np.abs(x64)).sum(0) / nk[k] + np.abs(m2[k]) * dnk[k] / nk[k]) + 1e-300
        b = np.abs(x64 - m2[k])
        B = (r * b).sum(0) / nk[k]
        dc = 2 * g(N + 3) * mag[k] + np.outer(dm, B) + np.outer(B, dm) + np.abs(c2[k]) * dnk[k] / nk[k] + 1e-300
        within(got[2][k], m2[k], dm, f"mean[{k}]")
        within(got[3][k], c2[k], dc, f"cov[{k}]")
        assert torch.equal(got[3][k], got[3][k].t())
    print("nk and means bitwise:", np.array_equal(N_(got[0]), nk), np.array_equal(N_(got[2]), m2))


def test_one_iteration_with_one_component_is_the_covariance():
    HF, Dn = HFD()
    N, D, K = 1200, 512, 1
    x = G(R.shape_input(N, D, K)[0])
    flags = HF.disent_flags(dev())
    mean, cov = HF.unsup_cov(x, flags)
    eye = torch.eye(D, dtype=torch.float64, device=dev())[None]
    reg = 1e-6
    gmm = Dn.fit_gmm(x, init=(torch.ones(1, dtype=torch.float64), torch.zeros((1, D), dtype=torch.float64), eye), max_iter=1,
                     reg_covar=reg)
    assert gmm.n_iter == 1 and not gmm.converged and N_(gmm.weights).tolist() == [1.0]
    assert torch.equal(gmm.means[0], mean)
    want = N_(cov) * ((N - 1) / N) + reg * np.eye(D)
    within(gmm.covariances[0], want, 8 * U * (np.abs(N_(cov)) + reg) + 1e-300, "covariance")


# ---- the k-means initialisation and the fit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,D,K", R.FIT_SHAPES)
def test_kmeans_init_and_fit(N, D, K, view):
    _, Dn = HFD()
    ref = R.reference(N, D, K)
    xt = VIEWS[view](ref["x"])
    ll = ref["lloyd"]
    w, mean, cov, centres, resp, flags = Dn.kmeans_init(xt, K, R.KMEANS_ITERS, ref["seed"])
    assert N_(flags).tolist() == [0, 0]
    assert np.array_equal(N_(resp), ll["resp"]) and np.array_equal(N_(centres), ll["centres"])
    assert np.array_equal(N_(w), ll["weights"]) and np.array_equal(N_(mean), ll["means"])
    eye = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    for name, kw in (("fit", dict(init="kmeans", kmeans_iters=R.KMEANS_ITERS, seed=ref["seed"])),
                     ("fit_eye", dict(init=(ll["weights"], ll["means"], eye), tol=R.FIT_EYE_TOL))):
        want = ref[name]
        got = Dn.fit_gmm(xt, n_components=K, max_iter=R.FIT_ITERS, **kw)
        diffs = dict(history=R.rel_diff(got.history, want["history"]) if got.n_iter == want["n_iter"] else np.inf,
                     weights=R.rel_diff(N_(got.weights), want["weights"]), means=R.rel_diff(N_(got.means), want["means"]),
                     covariances=R.rel_diff(N_(got.covariances), want["covariances"]))
        print((N, D, K), name, "n_iter", got.n_iter, want["n_iter"], diffs)
        assert (got.n_iter, got.converged) == (want["n_iter"], want["converged"])
        assert got.lower_bound == got.history[-1] and len(got.history) == got.n_iter
        assert max(diffs.values()) <= FIT_RTOL, diffs
        # the record is consistent: the factors are those of the covariances
        chol, linv, logdet, _ = Dn.HF.gmm_factor(got.covariances)
        assert torch.equal(chol, got.chol) and torch.equal(linv, got.prec_chol) and torch.equal(logdet, got.log_det)


@pytest.mark.parametrize("N,D,K", [(130, 17, 3), (700, 131, 2)])
def test_fit_is_deterministic(N, D, K):
    _, Dn = HFD()
    ref = R.reference(N, D, K)
    kw = dict(n_components=K, max_iter=R.FIT_ITERS, kmeans_iters=R.KMEANS_ITERS, seed=ref["seed"])
    a, b, c = Dn.fit_gmm(G(ref["x"]), **kw), Dn.fit_gmm(G(ref["x"]), **kw), Dn.fit_gmm(strided(ref["x"]), **kw)
    for other in (b, c):
        assert a.history == other.history and a.n_iter == other.n_iter
        for f in ("weights", "means", "covariances", "chol", "prec_chol", "log_det"):
            assert torch.equal(getattr(a, f), getattr(other, f)), f
    r = Dn.fit_gmm(G(ref["x"]), init="random", **{k: v for k, v in kw.items() if k != "kmeans_iters"})
    w0 = Dn.kmeans_init(G(ref["x"]), K, 0, ref["seed"])
    assert np.isfinite(r.history).all() and r.n_iter >= 1
    assert np.array_equal(N_(w0[3]), ref["x"][np.random.RandomState(ref["seed"]).choice(N, K, replace=False)].astype(np.float64))


# ---- sampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", [(1, 1), (3, 2), (33, 4), (131, 2), (512, 1)])
def test_sampler(D, K):
    _, Dn = HFD()
    params = R.make_params(D, K)
    gmm, (chol, _, _) = record(params)
    num, seed = 37, 5
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    z = Dn.gmm_sample(gmm, num, seed)
    assert torch.equal(z, Dn.gmm_sample(gmm, num, seed)) and not torch.equal(z, Dn.gmm_sample(gmm, num, seed + 1))
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state(dev()))
    gen = torch.Generator().manual_seed(seed)
    comp = torch.multinomial(gmm.weights.cpu(), num, replacement=True, generator=gen).numpy()
    eps = torch.randn((num, D), generator=gen).numpy()
    assert z.dtype == torch.float32 and z.shape == (num, D)
    assert np.array_equal(N_(z), R.sample(params[1], chol, comp, eps))
    assert K == 1 or len(np.unique(comp)) > 1


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    HF, Dn = HFD()
    from hipvae.abi import HipExtensionError
    x = G(R.make_data(40, 3, 2))
    with pytest.raises(ValueError, match="fewer than n_components"):
        Dn.fit_gmm(x, n_components=41)
    with pytest.raises(ValueError, match=r"outside 1\.\.64"):
        Dn.fit_gmm(G(R.make_data(80, 3, 2)), n_components=65)
    with pytest.raises(ValueError, match=r"outside 1\.\.512"):
        Dn.fit_gmm(G(np.zeros((600, 513), np.float32)), n_components=1)
    # the library itself refuses them too, before a launch
    flags = HF.disent_flags(dev())
    for N, D, K, msg in ((5, 3, 6, "rows is outside"), (80, 3, 65, "components is outside"), (600, 513, 1, "D = 513")):
        xs = G(np.zeros((N, D), np.float32))
        eye = torch.eye(D, dtype=torch.float64, device=dev()).expand(K, D, D).contiguous()
        w, m, z = G(np.ones(K)), G(np.zeros((K, D))), G(np.zeros(K))
        with pytest.raises(HipExtensionError, match=msg):
            HF.gmm_estep(xs, w, m, eye, z, flags)
        with pytest.raises(HipExtensionError, match=msg):
            HF.gmm_mstep(xs, G(np.ones((N, K))), flags)
    with pytest.raises(HipExtensionError, match="outside"):
        HF.gmm_factor(G(np.zeros((1, 513, 513))))
    bad = R.make_data(40, 3, 2)
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        Dn.fit_gmm(G(bad), n_components=2)
    gmm = Dn.fit_gmm(x, n_components=2, max_iter=2)
    with pytest.raises(ValueError, match="non-finite"):
        Dn.gmm_log_prob(gmm, G(bad))
    # duplicated columns, no regularisation: C = [[4, 0, 4], [0, 1, 0], [4, 0, 4]] exactly, whose third pivot is exactly 0
    a = np.tile(np.array([[2, 1], [2, -1], [-2, 1], [-2, -1]], np.float32), (16, 1))
    dup = np.concatenate([a, a[:, :1]], 1)
    assert R.factor(R.mstep(dup, np.ones((64, 1)))[3])[3].tolist() == [3]
    with pytest.raises(ValueError, match=r"component 0 .*dimension 2 .*reg_covar"):
        Dn.fit_gmm(G(dup), n_components=1, reg_covar=0.0, init="random")
    with pytest.raises(ValueError, match="init must be"):
        Dn.fit_gmm(x, n_components=2, init="kmeans++")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
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


def test_sample_quality_under_the_mixture(tiny_model, images):
    from hipvae import quality as Q
    _, Dn = HFD()
    model, ds = tiny_model, _Images(images)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    a = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3, prior="gmm",
                                 gmm_params=dict(n_components=2))
    assert sorted(a) == sorted(SIX + ("kid_std", "features", "indices", "gmm"))
    assert all(isinstance(a[k], float) and np.isfinite(a[k]) for k in SIX)
    real, fake, gmm = a["features"]["real"], a["features"]["fake"], a["gmm"]
    assert isinstance(gmm, Dn.GaussianMixture) and gmm.n_components == 2 and gmm.dim == 10
    again = Dn.fit_gmm(real, n_components=2, seed=3)
    assert torch.equal(again.weights, gmm.weights) and torch.equal(again.covariances, gmm.covariances)
    # the fakes are the decoded samples of the mixture, recomputed by hand
    z = Dn.gmm_sample(gmm, 64, 3)
    model.eval()
    with torch.no_grad():
        by_hand = torch.cat([model.encode(model.decode(z[s:s + 40]))[0] for s in (0, 40)], 0)
    model.train()
    assert torch.equal(fake, by_hand) and torch.equal(fake, Q.generated_features(model, 64, 40, 3, prior=gmm))
    # a given mixture is used as it is; with a callable feature the fit still takes the encoder's latents
    b = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3, prior=gmm)
    assert b["gmm"] is gmm and torch.equal(b["features"]["fake"], fake) and all(a[k] == b[k] for k in SIX)
    pix = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3, scores=("kid",), prior="gmm",
                                   gmm_params=dict(n_components=2), feature=lambda im: im.flatten(1)[:, ::97])
    assert torch.equal(pix["gmm"].means, gmm.means) and pix["features"]["fake"].shape == (64, 32)
    # the default path: the same bits with and without the argument, and no ``gmm``
    c = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3)
    d = Q.compute_sample_quality(ds, model, num_fake=64, batch_size=40, seed=3, prior="normal")
    assert "gmm" not in c and sorted(c) == sorted(d) and all(c[k] == d[k] for k in SIX)
    assert torch.equal(c["features"]["fake"], d["features"]["fake"]) and not torch.equal(c["features"]["fake"], fake)
    assert torch.equal(c["features"]["fake"], Q.generated_features(model, 64, batch_size=40, seed=3))
    with pytest.raises(ValueError, match="prior must be"):
        Q.compute_sample_quality(ds, model, prior="vamp")
    assert model.training and all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state(dev()))


def test_compute_latent_density(tiny_model, images):
    _, Dn = HFD()
    model, ds = tiny_model, _Images(images)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    got = Dn.compute_latent_density(ds, model, num_fit=60, num_eval=30, batch_size=40, seed=2, n_components=2)
    fit_idx, held_idx = got["indices"]["fit"], got["indices"]["heldout"]
    assert len(fit_idx) == 60 and len(held_idx) == 30 and not set(fit_idx.tolist()) & set(held_idx.tolist())
    drawn = np.random.RandomState(2).choice(96, 90, replace=False)
    assert fit_idx.tolist() == np.sort(drawn[:60]).tolist() and held_idx.tolist() == np.sort(drawn[60:]).tolist()
    print({k: got[k] for k in ("loglik_fit", "loglik_heldout", "loglik_prior", "gap", "n_iter", "converged")})
    assert all(np.isfinite(got[k]) for k in ("loglik_fit", "loglik_heldout", "loglik_prior", "gap"))
    assert got["gap"] == got["loglik_heldout"] - got["loglik_prior"] and got["n_iter"] == got["gmm"].n_iter >= 1
    zf, zh = got["latents"]["fit"], got["latents"]["heldout"]
    assert zf.shape == (60, 10) and zh.shape == (30, 10) and zh.dtype == torch.float32
    z64 = N_(zh).astype(np.float64)
    closed = np.mean(-0.5 * (10 * np.log(2 * np.pi) + (z64 * z64).sum(1)))
    assert abs(got["loglik_prior"] - closed) <= 1e-13 * abs(closed)
    assert got["loglik_heldout"] == float(Dn.gmm_log_prob(got["gmm"], zh).mean())
    assert got["loglik_fit"] == float(Dn.gmm_log_prob(got["gmm"], zf).mean())
    # num_eval None: what is left, at most num_fit; sampled latents are reproducible and differ from the means
    rest = Dn.compute_latent_density(ds, model, num_fit=70, batch_size=40, seed=2, n_components=1, max_iter=3)
    assert len(rest["indices"]["heldout"]) == 26
    s1 = Dn.compute_latent_density(ds, model, num_fit=60, num_eval=30, latent="sample", seed=2, n_components=1, max_iter=3)
    s2 = Dn.compute_latent_density(ds, model, num_fit=60, num_eval=30, latent="sample", seed=2, n_components=1, max_iter=3)
    assert torch.equal(s1["latents"]["fit"], s2["latents"]["fit"]) and not torch.equal(s1["latents"]["fit"], zf)
    with pytest.raises(ValueError, match="latent must be"):
        Dn.compute_latent_density(ds, model, latent="mode")
    assert model.training and all(torch.equal(before[k], v) for k, v in model.state_dict().items())


def test_solver_writes_the_latent_density_record(tiny_model, images):
    _, Dn = HFD()
    from hipvae.dataset import DeviceImageTable
    from solvers import VAESolver
    model = tiny_model
    u8 = (images.permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)
    table = DeviceImageTable.from_arrays(u8, None, dev())
    solver = VAESolver(dataset=table, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                       optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                       beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=_Recorder(), test_iter=5,
                       clip=100.0)
    assert solver.density_params is None
    params = dict(num_fit=60, num_eval=30, seed=2, n_components=2)
    solver.extra_scores, solver.density_params = ("latent_density",), params
    solver.write_disentanglemnt_scores(3)
    assert not solver.writer.log                                      # cur_iter % test_iter != 0: nothing
    solver.write_disentanglemnt_scores(10)
    assert list(solver.writer.log) == ["latent_density"]
    rec, step = solver.writer.log["latent_density"]
    want = Dn.compute_latent_density(table, model, batch_size=16, **params)
    four = ("loglik_heldout", "loglik_prior", "gap", "n_iter")
    assert step == 10 and list(rec) == list(four) and rec == {k: float(want[k]) for k in four} and model.training
    # sample quality under the mixture through the solver
    solver.writer.log.clear()
    solver.extra_scores = ("sample_quality",)
    solver.quality_params = dict(num_fake=64, seed=2, prior="gmm", gmm_params=dict(n_components=2))
    solver.write_disentanglemnt_scores(10)
    assert list(solver.writer.log["sample_quality"][0]) == list(SIX)
    solver.extra_scores = ("latent_density", "nope")
    with pytest.raises(ValueError, match=r"unknown score\(s\) \['nope'\].*'latent_density', 'log_likelihood', 'sample_quality'\)"):
        solver.write_disentanglemnt_scores(10)
