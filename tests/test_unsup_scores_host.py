"""CPU-only tests of the unsupervised scores and IRS: the numpy restatement (tests/unsup_ref.py) of the rules in
include/itcv_hip.h against the literal library formulas recorded in golden/unsup_scores.npz (np.cov, np.linalg.slogdet,
scipy.linalg.sqrtm, np.percentile) and against its own recorded values, the conditions of the fixture that the bounds of
tests/test_hip_unsup_scores.py rest on, and what the new entry points refuse before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import unsup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ["itcv_unsup_cov_workspace", "itcv_unsup_cov", "itcv_unsup_gauss_lds_dim", "itcv_unsup_gauss_workspace",
       "itcv_unsup_gauss", "itcv_irs_workspace", "itcv_irs"]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "unsup_scores.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def restated(golden):
    """The restatement of the fixture, computed once."""
    g = golden
    x = g["mu"][:, g["active"]]
    mean, C = R.ref_cov(x)
    mi, mis = R.ref_mi_matrix(x)
    return dict(x=x, mean=mean, cov=C, gauss=R.ref_gauss(C), mi=mi, mi_score=mis,
                irs=R.ref_irs(g["mu"], g["factors"], [int(s) for s in g["sizes"]]))


def test_fixture_shape(golden):
    g = golden
    assert g["mu"].shape == (600, 10) and g["mu"].dtype == np.float32 and g["factors"].shape == (600, 4)
    assert tuple(g["sizes"]) == (3, 5, 4, 7) and all(g["factors"][:, k].max() < s for k, s in enumerate(g["sizes"]))
    assert (g["mu"][:, 8] == g["mu"][0, 8]).all() and list(g["active"]) == [0, 1, 2, 3, 4, 5, 6, 7, 9]
    corr = np.corrcoef(g["mu"][:, g["active"]].astype(np.float64).T)
    assert np.abs(corr - np.eye(9)).max() > 0.3                        # correlated columns


def test_restatement_equals_the_library_formulas(golden, restated):
    g, r = golden, restated
    C = r["cov"]
    assert np.array_equal(C, C.T)
    assert np.abs(C - g["lib_cov"]).max() <= 1e-13 * np.abs(C).max()
    assert abs(r["gauss"]["tc"] - float(g["lib_tc"])) <= 1e-12
    assert abs(r["gauss"]["w"] - float(g["lib_w"])) <= 1e-12 * abs(float(g["lib_w"]))
    assert abs(r["gauss"]["w_norm"] - float(g["lib_w_norm"])) <= 1e-12 * abs(float(g["lib_w_norm"]))
    # the Cholesky log-determinant against slogdet, and the Jacobi eigenvalues against LAPACK
    assert abs(r["gauss"]["logdet"] - np.linalg.slogdet(C)[1]) <= 1e-12
    S = R.ref_scaled(C)
    assert np.abs(np.sort(r["gauss"]["eig"]) - np.linalg.eigvalsh(S)).max() <= 1e-12 * np.linalg.norm(S)
    assert r["gauss"]["converged"] and r["gauss"]["sweeps"] <= 10
    irs = r["irs"]
    keep = g["lib_irs_keep"]
    assert np.array_equal(keep, irs["active"])                         # var > 0 and min < max agree on this fixture
    assert np.abs(irs["IRS_matrix"][keep] - g["lib_irs_matrix"]).max() <= 1e-12
    assert np.abs(irs["max_deviations"][keep] - g["lib_irs_maxdev"]).max() <= 1e-13
    assert abs(irs["avg_score"] - float(g["lib_irs_avg"])) <= 1e-12
    assert np.array_equal(irs["parents"][keep], g["lib_irs_parents"])


def test_percentile_rule_is_numpys_bit_for_bit(golden):
    g = golden
    x = g["mu"].astype(np.float64)
    checked = 0
    for k, s in enumerate(g["sizes"]):
        for v in range(int(s)):
            G = x[g["factors"][:, k] == v]
            a = np.sort(np.abs(G - G.sum(0) / len(G)), axis=0)
            want = np.percentile(a, q=0.99 * 100, axis=0)
            got = np.array([R.ref_quantile(a[:, d], 0.99) for d in range(a.shape[1])])
            assert np.array_equal(got, want)
            checked += 1
    assert checked == 19
    rs = np.random.RandomState(3)
    for n in (1, 2, 3, 64, 65, 101, 201, 1100):                       # both branches of the interpolation occur
        a = np.sort(rs.rand(n))
        for q in (0.99, 0.5, 0.25, 1.0, 0.0):
            assert R.ref_quantile(a, q) == np.percentile(a, q * 100)
    ts = [(n - 1) * 0.99 - np.floor((n - 1) * 0.99) for n in (2, 3, 64, 65, 101, 201, 1100)]
    assert min(ts) < 0.5 <= max(ts)


def test_restatement_equals_golden(golden, restated):
    g, r = golden, restated
    assert np.allclose(r["mean"], g["mean"], rtol=0, atol=1e-14) and np.allclose(r["cov"], g["cov"], rtol=1e-13, atol=0)
    for key in ("tc", "w", "w_norm"):
        assert abs(r["gauss"][key] - float(g[key])) <= 1e-13
    assert np.abs(np.sort(r["gauss"]["eig"]) - g["eig"]).max() <= 1e-13
    assert np.abs(r["mi"] - g["mi_matrix"]).max() <= 1e-13 and abs(r["mi_score"] - float(g["mi_score"])) <= 1e-13
    assert np.array_equal(r["mi"], r["mi"].T)
    irs = r["irs"]
    assert np.abs(irs["IRS_matrix"] - g["irs_matrix"]).max() <= 1e-13 and np.abs(irs["cum"] - g["irs_cum"]).max() <= 1e-13
    assert abs(irs["avg_score"] - float(g["irs_avg"])) <= 1e-13 and np.array_equal(irs["parents"], g["irs_parents"])
    assert np.array_equal(irs["active"], g["irs_active"]) and irs["num_active_dims"] == 9
    assert not irs["active"][8] and not irs["IRS_matrix"][8].any()


def test_fixture_meets_the_conditions_of_the_gpu_bounds(golden, restated):
    g, r = golden, restated
    S = R.ref_scaled(r["cov"])
    cond = np.linalg.cond(S)
    top = np.sort(r["irs"]["IRS_matrix"][r["irs"]["active"]], axis=1)
    gap = (top[:, -1] - top[:, -2]).min()
    print("cond(S)", cond, "smallest gap between the two largest entries of an IRS row", gap)
    assert cond <= 100.0 and gap >= 1e-3
    assert 0.0 < r["gauss"]["tc"] and 0.0 < r["gauss"]["w"] and 0.0 < r["irs"]["avg_score"] < 1.0


def test_restatement_analytic_cases():
    assert abs(R.ref_gauss(np.array([[2.5]]))["tc"]) <= 1e-15 and abs(R.ref_gauss(np.array([[2.5]]))["w"]) <= 1e-14
    rho = 0.6
    C = np.array([[1.0, rho], [rho, 1.0]])
    assert abs(R.ref_gauss(C)["tc"] + 0.5 * np.log(1 - rho * rho)) <= 1e-15
    d = R.ref_gauss(np.diag([0.5, 2.0, 1.25, 3.0, 0.75]))
    assert abs(d["tc"]) <= 1e-14 and abs(d["w"]) <= 1e-14 and d["sweeps"] == 0
    sing = R.ref_gauss(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    assert sing["fail_dim"] == 1 and np.isnan(sing["tc"])
    assert np.isnan(R.ref_mi_matrix(np.arange(12, dtype=np.float32).reshape(12, 1))[1])
    const = R.ref_irs(np.ones((6, 3), np.float32), np.zeros((6, 1), int), [2])
    assert const["avg_score"] == 0.0 and const["num_active_dims"] == 0


def test_entry_points_declared_bound_and_exported():
    from hipvae import abi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "itcv_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/itcv_hip.h"
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert abi.ABI_VERSION == 4
    assert "unsup_scores.hip" in open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "Makefile")).read()
    hip = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "unsup_scores.hip")).read()
    dense = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "dense.h")).read()         # the covariance pass lives there
    assert "#pragma clang fp contract(off)" in hip and '#include "dense.h"' in hip and "cov_tile_rows<false>" in hip
    tile = dense.split("cov_tile_rows(")[1].split("\n}\n")[0]
    assert "#pragma clang fp contract(off)" in tile and "mfma_f64_16x16x4f64" in tile


def test_library_refuses_before_any_launch():
    from hipvae import abi
    L = abi.lib
    assert L.itcv_unsup_cov(None, 10, 1, 10, None, None, None, None, 0, None) != 0
    assert "N = 1" in abi.last_error()
    assert L.itcv_unsup_cov(None, 600, 100, 513, None, None, None, None, 0, None) != 0
    assert "D = 513" in abi.last_error()
    assert L.itcv_unsup_cov(None, 10, 100, 10, None, None, None, None, 0, None) != 0          # NULL pointers
    assert L.itcv_unsup_cov_workspace(1, 10) == 0 and L.itcv_unsup_cov_workspace(100, 513) == 0
    # 600 rows: 2 slices of 300; D = 10: one tile pair
    assert L.itcv_unsup_cov_workspace(600, 10) == (2 * 10 + 10 + 2 * 1 * 256) * 8
    assert L.itcv_unsup_gauss(None, 0, None, None, None, None, 0, None) != 0
    assert "D = 0" in abi.last_error()
    assert L.itcv_unsup_gauss(None, 513, None, None, None, None, 0, None) != 0
    assert L.itcv_unsup_gauss(None, 10, None, None, None, None, 0, None) != 0                   # NULL pointers
    assert L.itcv_unsup_gauss_workspace(200) == 200 * 200 * 8 and L.itcv_unsup_gauss_workspace(513) == 0
    lim = L.itcv_unsup_gauss_lds_dim()
    assert 64 <= lim and lim * (lim | 1) * 8 + 16 * 1024 <= 160 * 1024                        # the matrix and the tables fit LDS
    sizes = (ctypes.c_int * 2)(3, 2)
    args = [None] * 10 + [None, 0, None]
    assert L.itcv_irs(None, 8, None, None, 100, 8, 17, sizes, 0.99, *args) != 0
    assert "K = 17" in abi.last_error()
    assert L.itcv_irs(None, 8, None, None, 0, 8, 2, sizes, 0.99, *args) != 0
    assert "N = 0" in abi.last_error()
    big = (ctypes.c_int * 2)(3, 257)
    assert L.itcv_irs(None, 8, None, None, 100, 8, 2, big, 0.99, *args) != 0
    assert "257 values" in abi.last_error()
    assert L.itcv_irs(None, 8, None, None, 100, 8, 2, sizes, 1.5, *args) != 0
    assert "quantile" in abi.last_error()
    assert L.itcv_irs(None, 8, None, None, 100, 8, 2, sizes, 0.99, *args) != 0                   # NULL pointers
    assert L.itcv_irs_workspace(100, 8, 2, 5) > 0 and L.itcv_irs_workspace(100, 8, 17, 20) == 0


def test_wrappers_refuse_cpu_tensors_and_single_rows(golden):
    from hipvae import abi
    from hipvae import disentangle as DS
    g = golden
    mu, f = torch.from_numpy(g["mu"]), torch.from_numpy(g["factors"])
    for name in ("covariance", "unsupervised_scores", "gaussian_scores", "compute_unsupervised_scores", "irs_score_matrix",
                 "irs_score", "compute_irs_score"):
        assert name in DS.__all__ and callable(getattr(DS, name))
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.covariance(mu)
    with pytest.raises(ValueError, match="at least 2 rows"):
        DS.covariance(mu[:1])
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.unsupervised_scores(mu)
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.irs_score(mu, f, [3, 5, 4, 7])
    with pytest.raises(abi.HipExtensionError):
        DS.gaussian_scores(torch.eye(3, dtype=torch.float64))


def test_solver_attributes_default_to_nothing():
    import inspect
    from solvers import VAESolver
    src = inspect.getsource(VAESolver.__init__)
    assert "self.extra_scores = ()" in src and "self.irs_params = None" in src and "self.unsupervised_params = None" in src
    from solvers import scores
    assert "irs" in scores.TABLE and "unsupervised" in scores.TABLE and "mig" not in scores.TABLE
    assert scores.TABLE["irs"].factors and scores.TABLE["irs"].params == "irs_params"
    assert not scores.TABLE["unsupervised"].factors and scores.TABLE["unsupervised"].params == "unsupervised_params"


def test_mig_is_not_an_extra_score():
    """The writer itself on the CPU, with a stub writer: "mig" next to "irs" on a factored dataset is an unknown name,
    refused before anything is computed; the two names of this file are computed and written."""
    import score_writer_cases as C
    log = C.run_case(C.case("irs and mig", factored=True, extras=("irs", "mig")))
    assert log[:-1] == [["raised", "ValueError", "extra_scores: unknown score(s) ['mig'] (known: "]]
    log = C.run_case(C.case("irs and unsupervised", factored=True, extras=("unsupervised", "irs"), device_scores=False))
    assert [e[1] for e in log[:-1]] == ["disentangle.compute_irs_score", "irs", "disentangle.compute_unsupervised_scores",
                                        "unsupervised"]


def test_scipy_formula_still_agrees(golden):
    """The recorded library value recomputed where scipy is installed."""
    linalg = pytest.importorskip("scipy.linalg")
    g = golden
    lc = np.cov(g["mu"][:, g["active"]].astype(np.float64).T)
    w = 2 * np.trace(lc) - 2 * np.trace(linalg.sqrtm(lc * np.expand_dims(np.diag(lc), axis=1)))
    assert abs(float(np.real(w)) - float(g["lib_w"])) <= 1e-12 * abs(float(g["lib_w"]))
