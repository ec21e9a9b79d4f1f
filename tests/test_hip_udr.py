"""GPU tests of the device-side Unsupervised Disentanglement Ranking (csrc/udr.hip, hipvae/disentangle.py) against the
numpy fp64 restatement of tests/udr_ref.py on the fixture golden/udr.npz and on synthetic shapes.

Bounds.  Ranks: integers, so BITWISE.  Spearman: 1e-12 (the covariance of integer columns of 600 rows carries about 600 *
2^-53 relative error in any order; a quotient of O(1) values follows).  Lasso: 1e-9 and the same zero pattern -- the host
tests assert for the fixture that lambda_min(G_live) >= 0.005, that every zero coordinate keeps its gradient 1e-6 inside
alpha and every nonzero is at least 1e-6, so two points that meet the stop test (v <= 1e-12) differ by at most 2e-12 /
lambda_min = 4e-10; the synthetic matrices have lambda_min(G) >= 1/3 by construction.  The sweep count may differ by 2
from the restatement's: v is summed in another order.  Relative strength and the scores: 1e-12 on equal matrices, the
matrix bound through sums of at most 10 terms otherwise (1e-9 Lasso, 1e-12 Spearman)."""
import os

import numpy as np
import pytest
import torch

import udr_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
FLT_MAX = np.finfo(np.float32).max


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def strided(a, pad=3):
    """The same values as the right part of a wider tensor (row stride > D); the left part is nan and must not be read."""
    a = np.asarray(a)
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=a.dtype)
    wide[:, pad:] = a
    t = G(wide)[:, pad:]
    assert t.stride() == (a.shape[1] + pad, 1)
    return t


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "udr.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def pairs(golden):
    return [tuple(int(v) for v in p) for p in golden["pairs"]]


@pytest.fixture(scope="module")
def restated(golden, pairs):
    """The restatement of the fixture, computed once and left unchanged."""
    g = golden
    mus, lvs = [g[f"mu{m}"] for m in range(3)], [g[f"logvar{m}"] for m in range(3)]
    return dict(mus=mus, lvs=lvs, spearman={p: R.ref_spearman(mus[p[0]], mus[p[1]]) for p in pairs},
                lasso={p: R.ref_lasso(mus[p[0]], mus[p[1]], details=True) for p in pairs},
                udr={c: R.ref_udr(mus, lvs, c) for c in ("spearman", "lasso")})


# ---- ranks -------------------------------------------------------------------------------------------------------------
KINDS = 11


def column(kind, N, rs):
    """One column of every kind the rule names."""
    if kind == 0:
        return rs.randn(N)
    if kind == 1:
        return np.full(N, -1.25)                                       # all equal
    if kind == 2:
        return rs.choice([0.5, -3.0], size=N)                          # two distinct values
    if kind == 3:
        return rs.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=N)           # +-0 tie
    if kind == 4:
        return -np.abs(rs.randn(N)) - 0.1                              # negative values
    if kind == 5:
        return rs.randint(-20, 21, size=N) * np.float32(1e-45)         # denormals and +-0 around them
    if kind == 6:
        return rs.choice([FLT_MAX, -FLT_MAX, 0.0, 1.0], size=N)
    if kind == 7:
        return np.sort(rs.randn(N))                                    # already sorted
    if kind == 8:
        return np.sort(rs.randn(N))[::-1]                              # reverse sorted
    if kind == 9:
        return np.round(rs.randn(N) * 4) / 4                           # many ties
    return rs.randn(N) * 1e30                                          # large magnitudes of both signs


def rank_case(N, D, first):
    rs = np.random.RandomState(N * 31 + D)
    return np.stack([column((first + d) % KINDS, N, rs) for d in range(D)], 1).astype(np.float32)


def check_ranks(x):
    from hipvae import functional as HF
    want = R.ref_ranks2(x)
    for xt in (G(x), strided(x)):
        flags = HF.disent_flags(dev())
        got = HF.udr_ranks(xt, flags)
        assert got.dtype == torch.float32 and got.shape == x.shape and got.is_contiguous()
        assert flags.tolist() == [0, 0]
        assert np.array_equal(got.cpu().numpy(), want)                 # bitwise: integers
        assert torch.equal(HF.udr_ranks(xt, flags), got)
    return want


def test_ranks_of_two_rows():
    assert np.array_equal(check_ranks(np.array([[0.5], [0.5]], np.float32)), [[3.0], [3.0]])
    assert np.array_equal(check_ranks(np.array([[0.5], [-0.5]], np.float32)), [[4.0], [2.0]])
    assert np.array_equal(check_ranks(np.array([[0.0], [-0.0]], np.float32)), [[3.0], [3.0]])


@pytest.mark.parametrize("N,D,first", [(64, 3, 0), (64, 3, 3), (67, 16, 0), (1100, 131, 0)])
def test_ranks(N, D, first):
    """N = 64 and 67: a power of two and not, one key per thread at most; 1100: two keys for some threads; D = 131 blocks."""
    x = rank_case(N, D, first)
    want = check_ranks(x)
    assert np.array_equal(want.astype(np.float64).sum(0), np.full(D, float(N) * (N + 1)))


def test_ranks_on_both_sides_of_the_lds_limit():
    """The last N whose sorted keys sit in LDS and the first that sorts in the workspace (and is no power of two)."""
    from hipvae import functional as HF
    rows = HF.udr_rank_lds_rows()
    assert rows == 32768
    check_ranks(rank_case(rows, 2, 9))                                 # ties, large magnitudes
    check_ranks(rank_case(rows + 5, 3, 3))                             # +-0, negative, denormals


def test_ranks_flag_non_finite_values(golden):
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    a, b = golden["mu0"], golden["mu1"]
    for value in (float("nan"), float("inf"), float("-inf")):
        bad = a.copy()
        bad[17, 3] = value
        flags = HF.disent_flags(dev())
        HF.udr_ranks(G(bad), flags)
        assert flags.tolist() == [1, 0]
        with pytest.raises(ValueError, match="non-finite"):
            DS.spearman_matrix(G(bad), G(b))
        with pytest.raises(ValueError, match="non-finite"):
            DS.spearman_matrix(G(b), G(bad))
    with pytest.raises(RuntimeError, match="D = 513"):
        HF.udr_ranks(torch.zeros((4, 513), device=dev()), HF.disent_flags(dev()))
    torch.cuda.synchronize()


# ---- Spearman ----------------------------------------------------------------------------------------------------------
def test_spearman_matrix_on_the_fixture(golden, pairs, restated):
    from hipvae import disentangle as DS
    g, r = golden, restated
    got = {}
    for n, (i, j) in enumerate(pairs):
        got[i, j] = DS.spearman_matrix(G(r["mus"][i]) if n % 2 else strided(r["mus"][i]), G(r["mus"][j]))
        m = got[i, j]
        assert m.dtype == torch.float64 and m.shape == (10, 10) and m.is_cuda
        err = np.abs(m.cpu().numpy() - r["spearman"][i, j]).max()
        print((i, j), "max |rho - ref|", err)
        assert err <= 1e-12 and np.abs(m.cpu().numpy() - g["lib_spearman"][n]).max() <= 1e-12
        const = int(g[f"perm{i}"][5])
        assert not m[const].any() and not m[:, int(g[f"perm{j}"][5])].any()        # exact zeros
        assert torch.equal(DS.spearman_matrix(G(r["mus"][i]), G(r["mus"][j])), m)
    for i, j in pairs:
        assert torch.equal(got[j, i], got[i, j].t())                   # bitwise transpose


# ---- Lasso -------------------------------------------------------------------------------------------------------------
def test_lasso_on_the_fixture(golden, pairs, restated):
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    g, r = golden, restated
    for n, (i, j) in enumerate(pairs):
        want, _, sweeps, conv, _, _ = r["lasso"][i, j]
        a, b = G(r["mus"][i]), G(r["mus"][j])
        flags = HF.disent_flags(dev())
        _, cov = HF.unsup_cov(torch.cat([a, b], 1), flags)
        W, info = HF.udr_lasso(cov, 10, 10)
        assert W.dtype == torch.float64 and W.shape == (10, 10) and info.dtype == torch.int32
        Wn, info = W.cpu().numpy(), info.tolist()
        print((i, j), "max |W - ref|", np.abs(Wn - want).max(), "vs sklearn", np.abs(Wn - g["lib_lasso"][n]).max(),
              "sweeps", info[2], "ref", sweeps.max())
        assert np.abs(Wn - want).max() <= 1e-9 and np.array_equal(Wn == 0, want == 0)
        assert np.abs(Wn - g["lib_lasso"][n]).max() <= 1e-9
        assert info[:2] == [0, 0] and abs(info[2] - int(sweeps.max())) <= 2
        W2, info2 = HF.udr_lasso(cov, 10, 10)
        assert torch.equal(W2, W) and info2.tolist() == info            # bitwise
        assert torch.equal(DS.lasso_matrix(strided(r["mus"][i]), b), W)
        # the blocks swapped: the Lasso of (j, i) from the same covariance
        Ws, _ = HF.udr_lasso(cov.roll((10, 10), (0, 1)).contiguous(), 10, 10)
        assert np.abs(Ws.cpu().numpy() - r["lasso"][j, i][0]).max() <= 1e-9


def test_lasso_large_alpha_gives_exact_zeros_after_one_sweep(restated):
    from hipvae import functional as HF
    a, b = G(restated["mus"][2]), G(restated["mus"][0])
    _, cov = HF.unsup_cov(torch.cat([a, b], 1), HF.disent_flags(dev()))
    W, info = HF.udr_lasso(cov, 10, 10, alpha=1.5)                      # |c_k| <= 1 < alpha
    assert not W.any() and info.tolist() == [0, 0, 1]
    assert R.ref_lasso(restated["mus"][2], restated["mus"][0], alpha=1.5, details=True)[2].max() == 1


def test_lasso_of_single_columns():
    """Da = Db = 1: w = S(rho, alpha) in one sweep."""
    from hipvae import disentangle as DS
    rs = np.random.RandomState(4)
    a = rs.randn(300, 1)
    for mix, alpha in ((0.8, 0.1), (0.05, 0.1), (-0.9, 0.25)):
        b = mix * a + (1 - abs(mix)) * rs.randn(300, 1)
        a32, b32 = a.astype(np.float32), b.astype(np.float32)
        want = R.ref_lasso(a32, b32, alpha)
        rho = np.corrcoef(a32[:, 0].astype(np.float64), b32[:, 0].astype(np.float64))[0, 1]
        got = DS.lasso_matrix(G(a32), G(b32), alpha=alpha).cpu().numpy()
        assert got.shape == (1, 1) and abs(got[0, 0] - want[0, 0]) <= 1e-9
        assert abs(got[0, 0] - max(abs(rho) - alpha, 0.0)) <= 1e-9 and (got[0, 0] == 0) == (abs(rho) <= alpha)


def spd(D, seed):
    """A covariance with eigenvalues in [1, 3], so with a diagonal in [1, 3] too: the correlation matrix has eigenvalues in
    [1/3, 3] and so has every principal block G of it (interlacing): cond(G) <= 9 <= 30."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.randn(D, D))
    C = (Q * rs.uniform(1.0, 3.0, size=D)) @ Q.T
    return np.triu(C) + np.triu(C, 1).T


@pytest.mark.parametrize("Da", [128, 129])
def test_lasso_on_both_sides_of_the_lds_limit(Da):
    """Da = 128: the last G kept in LDS; 129: its rows are read from the workspace and a lane owns three coordinates.
    alpha = 0.01, below the typical |R_kl| of these matrices (about 0.05), so that many coordinates are nonzero."""
    from hipvae import functional as HF
    Db = 3
    C = spd(Da + Db, Da)
    want, w, sweeps, conv, Gm, _ = R.ref_lasso_cov(C, Da, Db, alpha=0.01, details=True)
    ev = np.linalg.eigvalsh(Gm)
    assert ev[-1] / ev[0] <= 30.0 and conv.all() and (w != 0).sum() >= Da
    W, info = HF.udr_lasso(G(C), Da, Db, alpha=0.01)
    Wn, info = W.cpu().numpy(), info.tolist()
    print("Da", Da, "max |W - ref|", np.abs(Wn - want).max(), "nonzeros", (Wn != 0).sum(), "sweeps", info[2], sweeps.max())
    assert Wn.shape == (Da, Db) and np.abs(Wn - want).max() <= 1e-9
    assert info[:2] == [0, 0] and abs(info[2] - int(sweeps.max())) <= 2
    W2, info2 = HF.udr_lasso(G(C), Da, Db, alpha=0.01)
    assert torch.equal(W2, W) and info2.tolist() == info


def test_lasso_that_runs_out_of_sweeps_raises(restated):
    """One sweep is not enough on the cond = 100 model."""
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    a, b = G(restated["mus"][2]), G(restated["mus"][0])
    assert restated["lasso"][2, 0][2].max() > 10
    _, cov = HF.unsup_cov(torch.cat([a, b], 1), HF.disent_flags(dev()))
    _, info = HF.udr_lasso(cov, 10, 10, max_sweeps=1)
    info = info.tolist()
    assert info[0] == 1 and 1 <= info[1] <= 10 and info[2] == 1
    with pytest.raises(RuntimeError, match="did not converge"):
        DS.lasso_matrix(a, b, max_sweeps=1)
    with pytest.raises(RuntimeError, match="Da \\+ Db = 513"):
        HF.udr_lasso(torch.eye(513, dtype=torch.float64, device=dev()), 500, 13)
    torch.cuda.synchronize()
    assert DS.lasso_matrix(a, b).shape == (10, 10)


# ---- relative strength and the ranking ---------------------------------------------------------------------------------
def test_relative_strength(restated, pairs):
    from hipvae import disentangle as DS
    mats = [restated["spearman"][p] for p in pairs] + [restated["lasso"][p][0] for p in pairs]
    mats += [np.array([[0.9, 0.0, 0.1], [0.0, 0.0, 0.0], [0.2, 0.0, 0.6]]), np.array([[0.7]]), np.eye(4),
             np.random.RandomState(1).rand(7, 3)]
    for c in mats:
        got = DS.relative_strength(G(c))
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        assert abs(float(got) - R.ref_relative_strength(c)) <= 1e-12
        assert torch.equal(DS.relative_strength(G(c)), got)
    assert float(DS.relative_strength(G(np.eye(4)))) == 1.0
    for shape in ((0, 3), (3, 0), (0, 0)):
        assert np.isnan(float(DS.relative_strength(torch.zeros(shape, dtype=torch.float64, device=dev()))))
    assert float(DS.relative_strength(torch.zeros((2, 2), dtype=torch.float64, device=dev()))) == 0.0


@pytest.mark.parametrize("form,tol", [("spearman", 1e-12), ("lasso", 1e-9)])
def test_udr_scores_on_the_fixture(golden, restated, form, tol):
    from hipvae import disentangle as DS
    g, r = golden, restated
    want = r["udr"][form]
    mus, lvs = [G(m) for m in r["mus"]], [G(lv) for lv in r["lvs"]]
    got = DS.udr_scores(mus, lvs, correlation=form)
    assert sorted(got) == sorted(["model_scores", "pairwise_disentanglement_scores", "raw_correlations", "kl_masks",
                                  "kl_divergence"])
    pw = got["pairwise_disentanglement_scores"]
    off = ~np.eye(3, dtype=bool)
    print(form, "scores", got["model_scores"], "max pairwise err", np.abs(pw[off] - want["pairwise"][off]).max())
    assert pw.shape == (3, 3) and np.isnan(np.diag(pw)).all()
    assert np.abs(pw[off] - want["pairwise"][off]).max() <= tol
    assert all(isinstance(s, float) for s in got["model_scores"])
    assert np.abs(np.array(got["model_scores"]) - np.array(want["model_scores"])).max() <= tol
    assert np.abs(np.array(got["model_scores"]) - g[f"lib_scores_{form}"]).max() <= tol
    for m in range(3):
        assert np.array_equal(got["kl_masks"][m], want["kl_masks"][m]) and got["kl_masks"][m].sum() == 6
        assert np.abs(got["kl_divergence"][m] - want["kl_divergence"][m]).max() <= 1e-12
    assert sorted(got["raw_correlations"]) == sorted(want["raw"])
    for key, mat in got["raw_correlations"].items():
        assert mat.is_cuda and mat.dtype == torch.float64 and mat.shape == (10, 10)
        assert np.abs(mat.cpu().numpy() - want["raw"][key]).max() <= tol
        if form == "spearman":
            assert torch.equal(got["raw_correlations"][key[1], key[0]], mat.t())
    again = DS.udr_scores(mus, lvs, correlation=form)
    assert again["model_scores"] == got["model_scores"]
    assert np.array_equal(again["pairwise_disentanglement_scores"], pw, equal_nan=True)
    # two models; no logvars: every dimension is kept
    two = DS.udr_scores(mus[:2], lvs[:2], correlation=form)
    assert two["pairwise_disentanglement_scores"].shape == (2, 2)
    assert abs(two["model_scores"][0] - want["pairwise"][1, 0]) <= tol
    assert abs(two["model_scores"][1] - want["pairwise"][0, 1]) <= tol
    full = DS.udr_scores(mus, correlation=form)
    wfull = R.ref_udr(r["mus"], None, form)
    assert full["kl_divergence"] is None and all(m.all() and len(m) == 10 for m in full["kl_masks"])
    assert np.abs(np.array(full["model_scores"]) - np.array(wfull["model_scores"])).max() <= tol
    # a model without an informative dimension: its pairs are nan and the median skips them
    dead_mu, dead_lv = r["mus"][1] * np.float32(1e-3), np.zeros_like(r["lvs"][1])
    wdead = R.ref_udr([r["mus"][0], dead_mu, r["mus"][2]], [r["lvs"][0], dead_lv, r["lvs"][2]], form)
    dead = DS.udr_scores([mus[0], G(dead_mu), mus[2]], [lvs[0], G(dead_lv), lvs[2]], correlation=form)
    dpw = dead["pairwise_disentanglement_scores"]
    assert not dead["kl_masks"][1].any() and np.isnan(dpw[1]).all() and np.isnan(dpw[:, 1]).all()
    assert np.array_equal(np.isnan(dpw), np.isnan(wdead["pairwise"]))
    assert np.isnan(dead["model_scores"][1]) and np.isnan(wdead["model_scores"][1])
    assert abs(dead["model_scores"][0] - want["pairwise"][2, 0]) <= tol
    assert abs(dead["model_scores"][2] - want["pairwise"][0, 2]) <= tol


def test_udr_scores_refusals(restated):
    from hipvae import disentangle as DS
    mus = [G(m) for m in restated["mus"]]
    with pytest.raises(ValueError, match="at least two"):
        DS.udr_scores(mus[:1])
    with pytest.raises(ValueError, match="same N"):
        DS.udr_scores([mus[0], mus[1][:500]])
    with pytest.raises(ValueError, match="logvars"):
        DS.udr_scores(mus, [mus[0]])
    bad = mus[1].clone()
    bad[5, 5] = float("nan")
    for form in ("lasso", "spearman"):
        with pytest.raises(ValueError, match="non-finite"):
            DS.udr_scores([mus[0], bad], correlation=form)
    torch.cuda.synchronize()


# ---- end to end --------------------------------------------------------------------------------------------------------
class Images:
    """96 random 32 x 32 images as a plain dataset: no factors."""

    def __init__(self):
        self.x = torch.rand((96, 3, 32, 32), generator=torch.Generator().manual_seed(7))

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i]


@pytest.fixture(scope="module")
def tiny_models():
    import models
    out = []
    for seed in (0, 1, 2):
        torch.manual_seed(seed)
        out.append(models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train())
    return out


def buffers(models_):
    return [{k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k} for m in models_]


def test_compute_udr_score_end_to_end(tiny_models):
    from hipvae import aggregate
    from hipvae import disentangle as DS
    ds = Images()
    before = buffers(tiny_models)
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    for form in ("lasso", "spearman"):
        got = DS.compute_udr_score(ds, tiny_models, num_train=80, batch_size=32, seed=3,
                                   params=dict(correlation=form, kl_filter_threshold=0.0))
        idx = np.sort(np.random.RandomState(3).choice(96, 80, replace=False))
        post = [aggregate.dataset_posteriors(ds, m, idx, 32) for m in tiny_models]
        direct = DS.udr_scores([p[0] for p in post], [p[1] for p in post], form, 0.0)
        print(form, got["model_scores"])
        assert got["model_scores"] == direct["model_scores"] and len(got["model_scores"]) == 3
        assert np.array_equal(got["pairwise_disentanglement_scores"], direct["pairwise_disentanglement_scores"],
                              equal_nan=True)
        want = R.ref_udr([p[0].cpu().numpy() for p in post], [p[1].cpu().numpy() for p in post], form, 0.0)
        assert np.array_equal(np.isnan(np.array(got["model_scores"])), np.isnan(np.array(want["model_scores"])))
        assert all(np.array_equal(a, b) for a, b in zip(got["kl_masks"], want["kl_masks"]))
    everything = DS.compute_udr_score(ds, tiny_models[:2], num_train=500, batch_size=48, params=dict(num_train=200))
    assert everything["raw_correlations"][0, 1].shape == (10, 10)
    assert all(m.training for m in tiny_models)
    assert all(torch.equal(v, m.state_dict()[k]) for m, b in zip(tiny_models, before) for k, v in b.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)


def test_solver_writes_udr(tiny_models):
    from solvers import VAESolver
    from test_hip_disent import StubWriter
    from hipvae import disentangle as DS
    model, ds = tiny_models[0], Images()

    def solver_of(w):
        return VAESolver(dataset=ds, model=model, batch_size=32, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                         optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                         beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)

    w = StubWriter()
    solver = solver_of(w)
    assert solver.extra_scores == () and solver.udr_peers is None and solver.udr_params is None
    solver.write_disentanglemnt_scores(0)
    assert w.calls == []                                              # extra_scores = (): nothing
    solver.extra_scores = ("udr",)
    with pytest.raises(ValueError, match="udr_peers"):
        solver.write_disentanglemnt_scores(0)
    assert w.calls == []
    solver.udr_peers = tiny_models[1:]
    solver.udr_params = dict(num_train=80, kl_filter_threshold=0.0, correlation="spearman")
    before = buffers(tiny_models)
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    solver.write_disentanglemnt_scores(0)
    assert [(c[0], c[1], c[3]) for c in w.calls] == [("add_scalars", "udr", 0)]
    rec = w.calls[0][2]
    print(rec)
    assert list(rec) == ["model_score", "mean_pairwise"]
    want = DS.compute_udr_score(ds, tiny_models, batch_size=32, params=solver.udr_params)
    col = [v for v in want["pairwise_disentanglement_scores"][1:, 0] if v == v]
    assert rec["model_score"] == want["model_scores"][0] and rec["mean_pairwise"] == sum(col) / len(col)
    assert np.isfinite(rec["model_score"]) and 0.0 < rec["mean_pairwise"] <= 1.0
    assert all(m.training for m in tiny_models)
    assert all(torch.equal(v, m.state_dict()[k]) for m, b in zip(tiny_models, before) for k, v in b.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    solver.test_iter = 2                                              # off the test iteration: nothing
    w.calls.clear()
    solver.write_disentanglemnt_scores(1)
    assert w.calls == []
