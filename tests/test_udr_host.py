"""CPU-only tests of the Unsupervised Disentanglement Ranking: the numpy restatement (tests/udr_ref.py) of the rules in
include/itcv_hip.h against the library values recorded in golden/udr.npz (scipy.stats.spearmanr, sklearn's Lasso after
StandardScaler, disentanglement_lib's relative strength), the conditions of the fixture that the bounds of
tests/test_hip_udr.py rest on, and what the new entry points refuse before any launch."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import udr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["itcv_udr_rank_lds_rows", "itcv_udr_ranks_workspace", "itcv_udr_ranks", "itcv_udr_lasso_workspace", "itcv_udr_lasso"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "udr.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def pairs(golden):
    return [tuple(int(v) for v in p) for p in golden["pairs"]]


@pytest.fixture(scope="module")
def restated(golden, pairs):
    """The restatement of the fixture, computed once: per ordered pair the Spearman matrix and the Lasso with its details,
    and the ranking of both forms."""
    g = golden
    mus, lvs = [g[f"mu{m}"] for m in range(3)], [g[f"logvar{m}"] for m in range(3)]
    return dict(spearman={p: R.ref_spearman(mus[p[0]], mus[p[1]]) for p in pairs},
                lasso={p: R.ref_lasso(mus[p[0]], mus[p[1]], details=True) for p in pairs},
                udr={c: R.ref_udr(mus, lvs, c) for c in ("spearman", "lasso")})


def test_fixture_shape(golden, pairs):
    g = golden
    assert pairs == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    for m in range(3):
        mu, lv, perm = g[f"mu{m}"], g[f"logvar{m}"], g[f"perm{m}"]
        assert mu.shape == lv.shape == (600, 10) and mu.dtype == lv.dtype == np.float32
        col = {k: int(perm[k]) for k in range(10)}                     # position in the generator -> column
        assert (mu[:, col[5]] == mu[0, col[5]]).all()                  # exactly constant
        q = mu[:, col[1]]
        assert np.array_equal(q * 4, np.round(q * 4)) and len(np.unique(q)) < 40       # quantised: many ties
        kl = R.ref_kl(mu, lv)
        assert sorted(np.nonzero(kl > 0.01)[0]) == sorted(col[k] for k in range(6))    # informative + the constant one
        assert all(kl[col[k]] < 0.01 for k in range(6, 10))


def test_doubled_ranks_small_cases():
    x = np.array([[1.0, 5.0], [1.0, -2.0]], dtype=np.float32)
    assert np.array_equal(R.ref_ranks2(x), np.array([[3.0, 4.0], [3.0, 2.0]], dtype=np.float32))
    z = np.array([[0.0], [-0.0], [1e-45], [-1e-45]], dtype=np.float32)            # +-0 tie, denormals are values
    assert np.array_equal(R.ref_ranks2(z)[:, 0], np.array([5.0, 5.0, 8.0, 2.0], dtype=np.float32))
    rs = np.random.RandomState(0)
    v = rs.randint(0, 7, size=(101, 3)).astype(np.float32)
    r = R.ref_ranks2(v)
    assert np.array_equal(r.sum(0), np.full(3, 101.0 * 102.0, dtype=np.float32))   # twice 1 + 2 + ... + N


def test_restatement_reproduces_the_recorded_library_values(golden, pairs, restated):
    g, r = golden, restated
    for n, p in enumerate(pairs):
        es = np.abs(r["spearman"][p] - g["lib_spearman"][n]).max()
        el = np.abs(r["lasso"][p][0] - g["lib_lasso"][n]).max()
        print(p, "spearman err", es, "lasso err", el, "sweeps <=", r["lasso"][p][2].max())
        assert es <= 1e-12 and el <= 1e-10
        assert r["lasso"][p][3].all()
    for m in range(3):
        assert np.abs(R.ref_kl(g[f"mu{m}"], g[f"logvar{m}"]) - g["lib_kl"][m]).max() <= 1e-14
    for form in ("spearman", "lasso"):
        u = r["udr"][form]
        off = ~np.eye(3, dtype=bool)
        assert np.isnan(np.diag(u["pairwise"])).all()
        assert np.abs(u["pairwise"][off] - g[f"lib_pairwise_{form}"][off]).max() <= 1e-10
        assert np.abs(np.array(u["model_scores"]) - g[f"lib_scores_{form}"]).max() <= 1e-10
        assert all(np.array_equal(u["kl_masks"][m], g["lib_kl"][m] > 0.01) for m in range(3))
    # the transpose rule of the Spearman form, and the block-swap rule of the Lasso form
    for i, j in pairs:
        assert np.array_equal(r["spearman"][i, j], r["spearman"][j, i].T)
    a, b = g["mu0"], g["mu2"]
    C = R.ref_cov(np.concatenate([a, b], 1))
    # (BLAS fixes no summation order, so the two numpy products agree to rounding only)
    assert np.abs(np.roll(C, (10, 10), (0, 1)) - R.ref_cov(np.concatenate([b, a], 1))).max() <= 1e-14


def test_fixture_meets_the_conditions_of_the_gpu_bounds(pairs, restated):
    """What the GPU tolerances rest on.  A constant column has G_kk = 0, stays at 0 by rule and drops out of the problem,
    so the strong convexity is that of the live columns: lambda_min(G_live) >= 0.005.  Every coordinate the restatement
    leaves at 0 keeps |g_k| at least 1e-6 below alpha and every nonzero has |w_k| >= 1e-6.  Two points with v <= 1e-12 then
    share the zero pattern, and on it their gradients differ by at most 2e-12, so they differ by at most 2e-12 / lambda_min
    <= 4e-10."""
    conds = []
    for p in pairs:
        _, w, sweeps, conv, G, cs = restated["lasso"][p]
        live = np.diag(G) != 0
        assert live.sum() == 9 and np.array_equal(np.diag(G)[live], np.ones(9))
        ev = np.linalg.eigvalsh(G[live][:, live])
        conds.append(ev[-1] / ev[0])
        grad = G @ w - cs
        zero = (w == 0) & live[:, None]
        margin = (0.1 - np.abs(grad[zero])).min()
        small = np.abs(w[w != 0]).min()
        print(p, "lambda_min", ev[0], "cond", conds[-1], "zero margin", margin, "smallest |w|", small, "sweeps", sweeps)
        assert ev[0] >= 0.005 and margin >= 1e-6 and small >= 1e-6 and conv.all() and sweeps.max() <= 1000
        assert not w[~live].any()
    assert 60.0 <= max(conds) <= 200.0                                 # model 2: cond(G) about 100
    assert min(conds) <= 10.0


def test_relative_strength_restatement():
    assert R.ref_relative_strength(np.eye(4)) == 1.0
    assert R.ref_relative_strength(np.full((3, 3), 0.5)) == pytest.approx(1.0 / 6.0 * 1.0, abs=1e-15)
    assert R.ref_relative_strength(np.array([[0.7]])) == pytest.approx(0.7, abs=1e-16)
    c = np.array([[0.9, 0.0, 0.1], [0.0, 0.0, 0.0], [0.2, 0.0, 0.6]])          # a zero row and a zero column count as 0
    sx = (0.81 / 1.1 + 0.0 + 0.36 / 0.7) / 3
    sy = (0.81 / 1.0 + 0.0 + 0.36 / 0.8) / 3
    assert R.ref_relative_strength(c) == pytest.approx((sx + sy) / 2, abs=1e-15)
    assert np.isnan(R.ref_relative_strength(np.zeros((0, 3)))) and np.isnan(R.ref_relative_strength(np.zeros((3, 0))))
    assert R.ref_median([3.0, 1.0]) == 2.0 and R.ref_median([5.0, 1.0, 2.0]) == 2.0 and np.isnan(R.ref_median([]))


def test_entry_points_declared_bound_and_exported():
    from hipvae import abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "itcv_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/itcv_hip.h"
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert abi.ABI_VERSION == 4
    assert "udr.hip" in open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "Makefile")).read()
    hip = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "udr.hip")).read()
    assert "#pragma clang fp contract(off)" in hip and "asm" not in hip


def test_library_refuses_before_any_launch():
    from hipvae import abi
    L = abi.lib
    rows = L.itcv_udr_rank_lds_rows()
    assert 1024 <= rows and rows * 4 <= 160 * 1024                     # the sorted keys of the last LDS size fit the CU
    assert L.itcv_udr_ranks(None, 10, 1, 10, None, None, None, 0, None) != 0
    assert "N = 1" in abi.last_error()
    assert L.itcv_udr_ranks(None, 10, (1 << 24) + 1, 10, None, None, None, 0, None) != 0
    assert L.itcv_udr_ranks(None, 600, 100, 513, None, None, None, 0, None) != 0
    assert "D = 513" in abi.last_error()
    assert L.itcv_udr_ranks(None, 10, 100, 0, None, None, None, 0, None) != 0
    assert "D = 0" in abi.last_error()
    assert L.itcv_udr_ranks(None, 10, 100, 10, None, None, None, 0, None) != 0                  # NULL pointers
    assert "requirement failed" in abi.last_error()
    assert L.itcv_udr_ranks(None, 3, rows + 5, 3, None, None, None, (rows + 5) * 3 * 4 - 1, None) != 0
    assert "workspace" in abi.last_error()
    assert L.itcv_udr_ranks_workspace(1, 10) == 0 and L.itcv_udr_ranks_workspace(100, 513) == 0
    assert L.itcv_udr_ranks_workspace(rows, 7) == 0 and L.itcv_udr_ranks_workspace(rows + 5, 3) == (rows + 5) * 3 * 4

    def lasso(Da, Db, alpha=0.1, gtol=1e-12, sweeps=1000, ws=0):
        return L.itcv_udr_lasso(None, Da, Db, alpha, gtol, sweeps, None, None, None, ws, None)

    assert lasso(0, 5) != 0 and "Da = 0" in abi.last_error()
    assert lasso(5, 0) != 0 and "Db = 0" in abi.last_error()
    assert lasso(500, 13) != 0 and "Da + Db = 513" in abi.last_error()
    assert lasso(5, 5, alpha=-0.1) != 0 and "alpha" in abi.last_error()
    assert lasso(5, 5, alpha=float("nan")) != 0 and "alpha" in abi.last_error()
    assert lasso(5, 5, gtol=-1.0) != 0 and "gtol" in abi.last_error()
    assert lasso(5, 5, sweeps=0) != 0 and "max_sweeps = 0" in abi.last_error()
    assert lasso(5, 5) != 0 and "workspace" in abi.last_error()                                # NULL, too small
    need = L.itcv_udr_lasso_workspace(5, 7)
    assert need == 12 * 12 * 8 + 7 * 2 * 4
    buf = ctypes.create_string_buffer(need)
    assert L.itcv_udr_lasso(None, 5, 7, 0.1, 1e-12, 1000, None, None, buf, need - 1, None) != 0
    assert "workspace" in abi.last_error()
    assert L.itcv_udr_lasso(None, 5, 7, 0.1, 1e-12, 1000, None, None, buf, need, None) != 0      # NULL pointers
    assert "requirement failed: cov" in abi.last_error()
    assert L.itcv_udr_lasso_workspace(0, 5) == 0 and L.itcv_udr_lasso_workspace(5, 0) == 0
    assert L.itcv_udr_lasso_workspace(500, 13) == 0 and L.itcv_udr_lasso_workspace(511, 1) == 512 * 512 * 8 + 8


def test_wrappers_refuse_cpu_tensors(golden):
    from hipvae import abi
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    g = golden
    a, b = torch.from_numpy(g["mu0"]), torch.from_numpy(g["mu1"])
    for name in ("spearman_matrix", "lasso_matrix", "relative_strength", "udr_scores", "compute_udr_score"):
        assert name in DS.__all__ and callable(getattr(DS, name))
    assert HF.udr_rank_lds_rows() == abi.lib.itcv_udr_rank_lds_rows()
    flags = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        HF.udr_ranks(a, flags)
    with pytest.raises(ValueError, match="at least 2 rows"):
        HF.udr_ranks(a[:1], flags)
    with pytest.raises(abi.HipExtensionError, match="no CPU path"):
        HF.udr_lasso(torch.eye(20, dtype=torch.float64), 10, 10)
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.spearman_matrix(a, b)
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.lasso_matrix(a, b)
    with pytest.raises(abi.HipExtensionError, match="no CPU path"):
        DS.relative_strength(torch.eye(3, dtype=torch.float64))
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.udr_scores([a, b])
    with pytest.raises(ValueError, match="same N"):
        DS.spearman_matrix(a, b[:500])
    with pytest.raises(ValueError, match="correlation"):
        DS.udr_scores([a, b], correlation="pearson")


def test_solver_attributes_default_to_nothing():
    import inspect
    from solvers import VAESolver
    src = inspect.getsource(VAESolver.__init__)
    assert "self.extra_scores = ()" in src and "self.udr_peers = None" in src and "self.udr_params = None" in src
    from solvers import scores
    udr = scores.TABLE["udr"]                                  # a record of the score table, which reads the peers
    assert not udr.factors and udr.params == "udr_params" and udr.tag == "udr"
    assert "udr_peers" in inspect.getsource(udr.compute)


def test_udr_without_peers_is_refused_on_the_cpu():
    """The writer itself, with a stub writer: the refusal comes before any device call."""
    import score_writer_cases as C
    for attrs in ({}, dict(udr_peers=[]), dict(udr_peers=())):
        log = C.run_case(C.case("udr without peers", extras=("udr",), attrs=attrs))
        assert log[:-1] == [["raised", "ValueError", 'extra_scores: "udr" compares this model with models trained from '
                             "other seeds: set udr_peers to a sequence of them"]]
    log = C.run_case(C.case("udr with a peer", extras=("udr",), peers=1))
    assert [e[:2] for e in log[:-1]] == [["compute", "disentangle.compute_udr_score"], ["add_scalars", "udr"]]
    assert log[0][2] == ["Plain", "list"] and log[1][2] == [["model_score", 0.625], ["mean_pairwise", 0.25]]


def test_scipy_values_still_agree(golden, pairs):
    """The recorded library values recomputed where scipy is installed: ranks and Spearman's rho."""
    stats = pytest.importorskip("scipy.stats")
    g = golden
    for m in range(3):
        x = g[f"mu{m}"]
        assert np.array_equal(R.ref_ranks2(x), (2.0 * stats.rankdata(x, axis=0)).astype(np.float32))
    for n, (i, j) in enumerate(pairs):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rho = stats.spearmanr(g[f"mu{i}"].astype(np.float64), g[f"mu{j}"].astype(np.float64))[0]
        assert np.abs(np.nan_to_num(np.abs(rho[:10, 10:]), nan=0.0) - g["lib_spearman"][n]).max() <= 1e-12


def test_sklearn_values_still_agree(golden, pairs, restated):
    """The recorded Lasso recomputed where sklearn is installed (tol = 1e-14: sklearn's default tolerance stops early,
    up to 1.3e-3 away on the cond = 100 pair)."""
    pytest.importorskip("sklearn")
    from sklearn.linear_model import Lasso
    from sklearn.preprocessing import StandardScaler
    g = golden
    for n, (i, j) in enumerate(pairs):
        a = StandardScaler().fit_transform(g[f"mu{i}"].astype(np.float64))
        b = StandardScaler().fit_transform(g[f"mu{j}"].astype(np.float64))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tight = np.abs(Lasso(alpha=0.1, tol=1e-14, max_iter=100000).fit(a, b).coef_).T
        assert np.abs(tight - g["lib_lasso"][n]).max() <= 1e-12
        assert np.abs(tight - restated["lasso"][i, j][0]).max() <= 1e-10
