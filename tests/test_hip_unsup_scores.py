"""GPU tests of the device-side unsupervised scores and IRS (csrc/unsup_scores.hip, hipvae/disentangle.py) against the numpy
fp64 restatement of tests/unsup_ref.py and the values recorded in golden/unsup_scores.npz.

Bounds.  Covariance: |dC_ij| <= 1e-12 sqrt(C_ii C_jj) -- two fp64 sums of at most 1100 O(1) terms carry about 1100 * 2^-53 =
1.2e-13 each in any order.  Total correlation 1e-9 absolute, Wasserstein correlation 1e-9 tr C: cond(S) <= 100 on every
matrix used here (asserted by the host tests for the fixture, by construction for the others), so an input error of 1e-13
grows to about 1e-11.  Eigenvalues: 1e-12 |S|_F against LAPACK's.  Mutual information: 1e-12 (integer tables, sums of at
most 400 terms below 1).  IRS on the fixture: 1e-12 (group means of at most 600 O(1) terms; the order statistics are exact).
IRS on integer-valued groups that are symmetric about 0: every group mean is exactly 0 in any order, every |x - e| an exact
integer, so cum, the matrix and the score must equal the restatement BITWISE."""
import os

import numpy as np
import pytest
import torch

import unsup_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py


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


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "unsup_scores.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement of the fixture, computed once and left unchanged."""
    g = golden
    x = np.ascontiguousarray(g["mu"][:, g["active"]])
    mean, C = R.ref_cov(x)
    mi, mis = R.ref_mi_matrix(x)
    return dict(x=x, mean=mean, cov=C, gauss=R.ref_gauss(C), mi=mi, mi_score=mis,
                irs=R.ref_irs(g["mu"], g["factors"], [int(s) for s in g["sizes"]]))


def spd(D, seed):
    """A covariance with eigenvalues in [1, 3], so with a diagonal in [1, 3] too: cond(S) <= 27."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.randn(D, D))
    C = (Q * rs.uniform(1.0, 3.0, size=D)) @ Q.T
    return np.triu(C) + np.triu(C, 1).T


# ---- covariance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["dense", "strided"])
@pytest.mark.parametrize("N,D", [(2, 5), (67, 1), (67, 16), (600, 131), (1100, 33)])
def test_covariance(N, D, view):
    """N = 2 (one product, three padded rows), 67 (16 products and 3 rows), 600 and 1100 (2 and 3 row slices); D = 1, 16
    (one full tile), 33, 131 (9 tiles, 45 tile pairs, the last tile 3 columns wide)."""
    from hipvae import disentangle as DS
    rs = np.random.RandomState(N * 1000 + D)
    x = (rs.randn(N, D) * rs.uniform(0.2, 2.0, size=D) + rs.uniform(-1, 1, size=D)).astype(np.float32)
    if D > 2:
        x[:, 2] = 0.5 * x[:, 0] - x[:, 1]
    mean, C = R.ref_cov(x)
    xt = G(x) if view == "dense" else strided(x)
    gm, gc = DS.covariance(xt)
    assert gm.dtype == gc.dtype == torch.float64 and gm.shape == (D,) and gc.shape == (D, D) and gc.is_cuda
    gm, gcn = gm.cpu().numpy(), gc.cpu().numpy()
    sd = np.sqrt(np.diag(C))
    err = np.abs(gcn - C) / np.maximum(sd[:, None] * sd[None, :], 1e-300)
    print("max |dC_ij| / sqrt(C_ii C_jj)", err.max(), "max |dmean|", np.abs(gm - mean).max())
    assert np.abs(gm - mean).max() <= 1e-13 * max(1.0, np.abs(x).max())
    assert (np.abs(gcn - C) <= 1e-12 * sd[:, None] * sd[None, :]).all()
    assert torch.equal(gc, gc.t())                                     # bitwise
    gm2, gc2 = DS.covariance(xt)
    assert torch.equal(gc, gc2) and np.array_equal(gm, gm2.cpu().numpy())


def test_covariance_refusals():
    from hipvae import disentangle as DS
    x = torch.zeros((4, 3), device=dev())
    with pytest.raises(ValueError, match="at least 2 rows"):
        DS.covariance(x[:1])
    bad = x.clone()
    bad[2, 1] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        DS.covariance(bad)
    with pytest.raises(RuntimeError, match="D = 513"):
        DS.covariance(torch.zeros((4, 513), device=dev()))
    torch.cuda.synchronize()


# ---- Cholesky and Jacobi -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["dense", "strided"])
def test_unsupervised_scores_on_the_fixture(golden, restated, view):
    from hipvae import disentangle as DS
    g, r = golden, restated
    x = G(r["x"]) if view == "dense" else strided(r["x"])
    got = DS.unsupervised_scores(x)
    assert sorted(got) == sorted(["gaussian_total_correlation", "gaussian_wasserstein_correlation",
                                  "gaussian_wasserstein_correlation_norm", "mutual_info_score", "covariance", "eigenvalues",
                                  "mutual_info_matrix"])
    tc, w, wn, mis = (got[k] for k in ("gaussian_total_correlation", "gaussian_wasserstein_correlation",
                                       "gaussian_wasserstein_correlation_norm", "mutual_info_score"))
    assert all(isinstance(v, float) for v in (tc, w, wn, mis))
    tr = r["gauss"]["trace"]
    S = R.ref_scaled(r["cov"])
    eig = got["eigenvalues"].cpu().numpy()
    print("tc", tc, "err", abs(tc - r["gauss"]["tc"]), "w", w, "err / trC", abs(w - r["gauss"]["w"]) / tr,
          "eig err / |S|_F", np.abs(eig - np.linalg.eigvalsh(S)).max() / np.linalg.norm(S),
          "mi err", np.abs(got["mutual_info_matrix"].cpu().numpy() - r["mi"]).max())
    assert abs(tc - r["gauss"]["tc"]) <= 1e-9 and abs(tc - float(g["tc"])) <= 1e-9 and abs(tc - float(g["lib_tc"])) <= 1e-9
    assert abs(w - r["gauss"]["w"]) <= 1e-9 * tr and abs(w - float(g["lib_w"])) <= 1e-9 * tr
    assert abs(wn - r["gauss"]["w_norm"]) <= 1e-9 and abs(wn - w / np.trace(got["covariance"].cpu().numpy())) <= 1e-15
    assert np.abs(eig - np.linalg.eigvalsh(S)).max() <= 1e-12 * np.linalg.norm(S) and (np.diff(eig) >= 0).all()
    mi = got["mutual_info_matrix"]
    assert mi.dtype == torch.float64 and torch.equal(mi, mi.t())
    assert np.abs(mi.cpu().numpy() - r["mi"]).max() <= 1e-12 and abs(mis - r["mi_score"]) <= 1e-12
    assert abs(mis - float(g["mi_score"])) <= 1e-12
    again = DS.unsupervised_scores(x)
    assert all(again[k] == got[k] for k in ("gaussian_total_correlation", "gaussian_wasserstein_correlation",
                                            "gaussian_wasserstein_correlation_norm", "mutual_info_score"))
    assert all(torch.equal(again[k], got[k]) for k in ("covariance", "eigenvalues", "mutual_info_matrix"))


def test_gaussian_scores_analytic_cases():
    from hipvae import disentangle as DS
    tc, w, wn, eig = DS.gaussian_scores(G(np.array([[2.5]])))
    assert abs(tc) <= 1e-14 and abs(w) <= 1e-14 and abs(wn) <= 1e-14 and eig.shape == (1,)
    for rho in (0.6, -0.95):
        tc, w, _, _ = DS.gaussian_scores(G(np.array([[1.0, rho], [rho, 1.0]])))
        want = R.ref_gauss(np.array([[1.0, rho], [rho, 1.0]]))
        assert abs(tc + 0.5 * np.log(1 - rho * rho)) <= 1e-14 and abs(w - want["w"]) <= 1e-14
        assert abs(w - (4.0 - 2.0 * (np.sqrt(1 + rho) + np.sqrt(1 - rho)))) <= 1e-14      # lambda = 1 +- rho
    d = np.array([0.5, 2.0, 1.25, 3.0, 0.75, 1.0, 4.0])
    tc, w, wn, eig = DS.gaussian_scores(G(np.diag(d)))
    assert abs(tc) <= 1e-14 and abs(w) <= 1e-14 and np.abs(eig.cpu().numpy() - d * d).max() <= 1e-14


def test_gaussian_scores_on_both_sides_of_the_lds_limit():
    """D = the LDS limit (the matrix in LDS, D even) and the limit + 9 (the global workspace, D odd: one index sits out of
    every round).  Eigenvalues of C in [1, 3]: cond(S) <= 27 by Ostrowski's theorem."""
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    lim = HF.unsup_gauss_lds_dim()
    assert lim == 128
    for D in (lim, lim + 9):
        C = spd(D, D)
        S = R.ref_scaled(C)
        lam = np.linalg.eigvalsh(S)
        assert lam[-1] / lam[0] <= 100.0
        res, eig, info = HF.unsup_gauss(G(C))
        res2, eig2, info2 = HF.unsup_gauss(G(C))
        assert torch.equal(res, res2) and torch.equal(eig, eig2) and torch.equal(info, info2)      # bitwise
        res, eig, info = res.cpu().numpy(), np.sort(eig.cpu().numpy()), info.cpu().tolist()
        tr = np.trace(C)
        want_tc = 0.5 * (np.log(np.diag(C)).sum() - np.linalg.slogdet(C)[1])
        want_w = 2.0 * tr - 2.0 * np.sqrt(lam).sum()
        print("D", D, "sweeps", info[3], "tc err", abs(res[0] - want_tc), "w err / trC", abs(res[1] - want_w) / tr,
              "eig err / |S|_F", np.abs(eig - lam).max() / np.linalg.norm(S))
        assert info[:3] == [0, -1, 0] and 1 <= info[3] <= 20
        assert abs(res[0] - want_tc) <= 1e-9 and abs(res[1] - want_w) <= 1e-9 * tr and abs(res[3] - tr) <= 1e-12 * tr
        assert np.abs(eig - lam).max() <= 1e-12 * np.linalg.norm(S)


def test_singular_covariance_raises_and_names_the_dimension():
    """Columns 0 and 1 are identical with variance exactly 1 (32 times +1, 32 times -1 and one 0 in 65 rows): the second
    pivot is 1 - 1 * 1 = 0 in any arithmetic.  A finite input that errors is not a fault."""
    from hipvae import disentangle as DS
    rs = np.random.RandomState(5)
    x = rs.randn(65, 4).astype(np.float32)
    x[:, 0] = np.concatenate([np.ones(32), -np.ones(32), [0.0]]).astype(np.float32)[rs.permutation(65)]
    x[:, 1] = x[:, 0]
    assert R.ref_gauss(R.ref_cov(x)[1])["fail_dim"] == 1
    with pytest.raises(ValueError, match="dimension 1 "):
        DS.unsupervised_scores(G(x))
    const = x.copy()
    const[:, 2] = 0.25
    with pytest.raises(ValueError, match="not positive definite"):
        DS.unsupervised_scores(G(const[:, 2:]))
    torch.cuda.synchronize()
    assert np.isfinite(DS.unsupervised_scores(G(x[:, 1:]))["gaussian_total_correlation"])


# ---- mutual information ------------------------------------------------------------------------------------------------
def test_mutual_info_score_with_two_factor_chunks():
    """D = 17: the columns go through the histogram kernel as 16 + 1 "factors"."""
    from hipvae import disentangle as DS
    rs = np.random.RandomState(17)
    x = rs.randn(300, 17)
    x[:, 16] = x[:, 0] + 0.3 * rs.randn(300)
    x[:, 5] = -x[:, 4] ** 2 + 0.1 * rs.randn(300)
    x = x.astype(np.float32)
    want, score = R.ref_mi_matrix(x)
    got = DS.unsupervised_scores(strided(x))
    mi = got["mutual_info_matrix"]
    print("max |MI - ref|", np.abs(mi.cpu().numpy() - want).max(), "score", got["mutual_info_score"], score)
    assert mi.shape == (17, 17) and torch.equal(mi, mi.t())
    assert np.abs(mi.cpu().numpy() - want).max() <= 1e-12 and abs(got["mutual_info_score"] - score) <= 1e-12
    assert want[0, 16] > 2 * np.median(want[0, 1:16])                 # the planted dependence stands out of the 20-bin bias
    one = DS.unsupervised_scores(G(x[:, :1]))
    assert np.isnan(one["mutual_info_score"]) and abs(one["gaussian_total_correlation"]) <= 1e-14


# ---- IRS ---------------------------------------------------------------------------------------------------------------
GROUPS = (1, 2, 3, 64, 65, 101, 201, 1100)


def exact_case():
    """Integer-valued latents [1537, 131].  The rows come in units: a pair (u, -u) of integer vectors or a single zero row;
    every factor gives both rows of a pair the same value, so every group of every factor is symmetric about 0.  Factor 0
    (size 9, value 4 absent) has the groups of GROUPS; factor 1 (size 4) deals the units out at random.  Column 0 takes
    the values 0 / +-1 only (heavy duplicates: a[lo] == a[hi]), column 1 only 0 / +-7, column 130 is constant 0."""
    rs = np.random.RandomState(9)
    D = 131
    rows, f0, f1 = [], [], []
    values = [0, 1, 2, 3, 5, 6, 7, 8]                                   # 4 never occurs
    for n, v in zip(GROUPS, values):
        if n % 2:
            rows.append(np.zeros((1, D)))
            f0.append(v), f1.append(rs.randint(4))
        for _ in range(n // 2):
            u = rs.randint(-40, 41, size=D).astype(np.float64)
            u[0] = rs.randint(0, 2)
            u[1] = 7 * rs.randint(0, 2)
            u[2] = rs.randint(0, 3) * 1000
            rows += [u[None], -u[None]]
            k1 = rs.randint(4)
            f0 += [v, v]
            f1 += [k1, k1]
    x = np.concatenate(rows, 0)
    x[:, 130] = 0.0
    f = np.stack([f0, f1], 1).astype(np.int32)
    perm = rs.permutation(len(x))
    return x[perm].astype(np.float32), f[perm], [9, 4]


@pytest.mark.parametrize("view", ["dense", "strided"])
def test_irs_quantile_selection_is_exact(view):
    from hipvae import disentangle as DS
    x, f, sizes = exact_case()
    assert x.shape == (sum(GROUPS), 131) and sorted(np.bincount(f[:, 0], minlength=9)) == sorted(GROUPS + (0,))
    assert np.array_equal(x, np.round(x))
    want = R.ref_irs(x, f, sizes)
    act = want["active"]
    assert act.sum() == 130 and not act[130]
    # both branches of the interpolation, and a[lo] == a[hi] next to a[lo] < a[hi]
    ts = [(n - 1) * 0.99 - np.floor((n - 1) * 0.99) for n in GROUPS]
    assert min(ts) < 0.5 <= max(ts)
    got = DS.irs_score_matrix(G(x) if view == "dense" else strided(x), G(f), sizes)
    assert got["num_active_dims"] == 130 and np.array_equal(got["active_dims"].cpu().numpy(), np.nonzero(act)[0])
    assert np.array_equal(got["max_deviations"].cpu().numpy(), want["max_deviations"][act])
    assert np.array_equal(got["cum_deviations"].cpu().numpy(), want["cum"][act])               # bitwise
    assert np.array_equal(got["IRS_matrix"].cpu().numpy(), want["IRS_matrix"][act])
    assert np.array_equal(got["disentanglement_scores"].cpu().numpy(), want["scores"][act])
    assert got["avg_score"] == want["avg_score"]
    assert got["parents"].dtype == torch.int64 and np.array_equal(got["parents"].cpu().numpy(), want["parents"][act])
    assert DS.irs_score(G(x), G(f), sizes) == want["avg_score"]
    # another quantile: the median takes the other branch in other groups, q = 1 and 0 take the ends
    for q in (0.5, 1.0, 0.0, 0.37):
        w2 = R.ref_irs(x, f, sizes, q)
        g2 = DS.irs_score_matrix(G(x), G(f), sizes, q)
        assert np.array_equal(g2["cum_deviations"].cpu().numpy(), w2["cum"][act]) and g2["avg_score"] == w2["avg_score"]


def test_irs_on_the_fixture(golden, restated):
    from hipvae import disentangle as DS
    g, want = golden, restated["irs"]
    sizes = [int(s) for s in g["sizes"]]
    act = want["active"]
    for x in (G(g["mu"]), strided(g["mu"])):
        got = DS.irs_score_matrix(x, G(g["factors"]), sizes)
        M = got["IRS_matrix"].cpu().numpy()
        print("max |M - ref|", np.abs(M - want["IRS_matrix"][act]).max(), "|avg - ref|", abs(got["avg_score"] - want["avg_score"]))
        assert sorted(got) == sorted(["avg_score", "disentanglement_scores", "parents", "IRS_matrix", "max_deviations",
                                      "num_active_dims", "cum_deviations", "active_dims"])
        assert M.shape == (9, 4) and got["num_active_dims"] == 9 and 8 not in got["active_dims"].cpu().tolist()
        assert np.abs(M - want["IRS_matrix"][act]).max() <= 1e-12 and np.abs(M - g["lib_irs_matrix"]).max() <= 1e-12
        assert abs(got["avg_score"] - want["avg_score"]) <= 1e-12 and abs(got["avg_score"] - float(g["lib_irs_avg"])) <= 1e-12
        assert np.array_equal(got["parents"].cpu().numpy(), want["parents"][act])
        assert np.array_equal(got["parents"].cpu().numpy(), g["lib_irs_parents"])
        assert np.abs(got["max_deviations"].cpu().numpy() - want["max_deviations"][act]).max() <= 1e-13
        again = DS.irs_score_matrix(x, G(g["factors"]), sizes)
        assert again["avg_score"] == got["avg_score"] and all(
            torch.equal(again[k], got[k]) for k in got if isinstance(got[k], torch.Tensor))
    # numpy arrays as factors, and an int64 tensor
    assert DS.irs_score(G(g["mu"]), g["factors"], sizes) == got["avg_score"]
    assert DS.irs_score(G(g["mu"]), G(g["factors"]).long(), sizes) == got["avg_score"]


def test_irs_degenerate_inputs_and_refusals(golden):
    from hipvae import disentangle as DS
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    mu, f = G(g["mu"]), G(g["factors"])
    const = torch.full((600, 3), 0.25, device=dev())
    got = DS.irs_score_matrix(const, f, sizes)
    assert got["avg_score"] == 0.0 and got["num_active_dims"] == 0 and got["IRS_matrix"].shape == (0, 4)
    bad = mu.clone()
    bad[17, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        DS.irs_score(bad, f, sizes)
    for value in (7, -1):
        fb = f.clone()
        fb[11, 3] = value
        with pytest.raises(ValueError, match="outside"):
            DS.irs_score(mu, fb, sizes)
    with pytest.raises(RuntimeError, match="257 values"):
        DS.irs_score(mu, f, sizes[:-1] + [257])
    with pytest.raises(RuntimeError, match="quantile"):
        DS.irs_score(mu, f, sizes, diff_quantile=1.5)
    torch.cuda.synchronize()                                          # no fault behind any of them
    assert abs(DS.irs_score(mu, f, sizes) - float(g["irs_avg"])) <= 1e-12


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_model():
    import models
    torch.manual_seed(0)
    return models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()


def test_compute_scores_end_to_end(tiny_model):
    from hipvae import aggregate
    from hipvae import disentangle as DS
    from test_hip_disent import make_dataset
    model, ds = tiny_model, make_dataset()
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    got = DS.compute_unsupervised_scores(ds, model, num_train=16, batch_size=5, seed=3)
    idx = np.sort(np.random.RandomState(3).choice(20, 16, replace=False))
    mu, _ = aggregate.dataset_posteriors(ds, model, idx, 5)
    direct = DS.unsupervised_scores(mu)
    keys = ("gaussian_total_correlation", "gaussian_wasserstein_correlation", "gaussian_wasserstein_correlation_norm",
            "mutual_info_score")
    print({k: got[k] for k in keys})
    assert all(got[k] == direct[k] and np.isfinite(got[k]) for k in keys)
    everything = DS.compute_unsupervised_scores(ds, model, num_train=50, batch_size=8)
    assert everything["covariance"].shape == (10, 10)
    irs = DS.compute_irs_score(DS.FactorSampler(ds, dev(), seed=42), model, params=dict(num_train=96, batch_size=16))
    twin_mu, twin_v = DS.factor_representations(DS.FactorSampler(ds, dev(), seed=42), model, 96, 16)
    want = R.ref_irs(twin_mu.cpu().numpy(), twin_v.cpu().numpy(), [4, 5])
    print("irs", irs["avg_score"], want["avg_score"], "active", irs["num_active_dims"])
    assert irs["num_active_dims"] == want["num_active_dims"] and abs(irs["avg_score"] - want["avg_score"]) <= 1e-12
    assert model.training and before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)


def test_solver_writes_irs_and_unsupervised(tiny_model):
    from solvers import VAESolver
    from test_hip_disent import StubWriter, make_dataset
    from hipvae.disentangle import FactorSampler
    model, ds = tiny_model, make_dataset()

    class Plain:
        def __len__(self):
            return len(ds)

        def __getitem__(self, i):
            return ds[i]

    def solver_of(dataset, w):
        return VAESolver(dataset=dataset, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                         optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                         beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)

    w = StubWriter()
    solver = solver_of(ds, w)
    assert solver.extra_scores == () and solver.irs_params is None and solver.unsupervised_params is None
    solver.latent_generator = FactorSampler(ds, dev(), seed=42)
    solver.device_scores = False
    solver.write_disentanglemnt_scores(0)
    assert w.calls == []                                              # extra_scores = (): neither record
    solver.extra_scores = ("irs", "unsupervised")
    solver.irs_params, solver.unsupervised_params = dict(num_train=96, batch_size=16), dict(num_train=18, seed=1)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    solver.write_disentanglemnt_scores(0)
    assert [(c[0], c[1], c[3]) for c in w.calls] == [("add_scalars", "irs", 0), ("add_scalars", "unsupervised", 0)]
    irs, unsup = w.calls[0][2], w.calls[1][2]
    print(irs, unsup)
    assert list(irs) == ["IRS", "num_active_dims"] and list(unsup) == [
        "gaussian_total_correlation", "gaussian_wasserstein_correlation", "gaussian_wasserstein_correlation_norm",
        "mutual_info_score"]
    assert all(np.isfinite(v) for v in list(irs.values()) + list(unsup.values())) and 1 <= irs["num_active_dims"] <= 10
    assert model.training and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    # off the test iteration: nothing; an unknown name is still refused
    solver.test_iter = 2
    w.calls.clear()
    solver.write_disentanglemnt_scores(1)
    assert w.calls == []
    solver.test_iter, solver.extra_scores = 1, ("irs", "mig")
    with pytest.raises(ValueError, match="unknown"):
        solver.write_disentanglemnt_scores(0)
    # a dataset without factors still gets the unsupervised record, and only that one
    w2 = StubWriter()
    plain = solver_of(Plain(), w2)
    plain.extra_scores, plain.unsupervised_params = ("irs", "unsupervised"), dict(num_train=18, seed=1)
    plain.write_disentanglemnt_scores(0)
    assert [(c[0], c[1]) for c in w2.calls] == [("add_scalars", "unsupervised")]
    assert w2.calls[0][2] == unsup
    # after use_device_dataset the images come from the device table: the same record as from the dataset
    from test_hip_dataset import make_factor_dataset
    fds, recs = make_factor_dataset((3, 32, 32)), []
    for use_table in (False, True):
        w3 = StubWriter()
        s3 = solver_of(fds, w3)
        s3.device_scores, s3.extra_scores, s3.unsupervised_params = False, ("unsupervised",), dict(num_train=20, seed=2)
        if use_table:
            s3.use_device_dataset()
        s3.write_disentanglemnt_scores(0)
        assert [(c[0], c[1]) for c in w3.calls] == [("add_scalars", "unsupervised")]
        recs.append(w3.calls[0][2])
    assert recs[0] == recs[1]
    assert model.training
