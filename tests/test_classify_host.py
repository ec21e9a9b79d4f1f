"""CPU-only checks of the device-side beta-VAE and explicitness scores: the new entry points are declared, bound and
exported alike and refuse what lies outside their range before any launch, and a numpy fp64 restatement of the rule of
include/itcv_hip.h -- written here, shared with tests/test_hip_classify.py, free of sklearn and scipy -- reproduces what
was recorded from sklearn and the unmodified reference (tests/golden/classify.npz, made by make_golden_classify.py).

Tolerances that compare with RECORDED numbers were measured here on the CPU and carry a 10x margin:
  PROBA_GOLDEN_TOL   restatement (Newton, max|grad| <= 1e-11) against sklearn's tightly converged predict_proba
                     (lbfgs, tol = 1e-12): measured 5.1e-7 at the most (sklearn's own residual)            -> 6e-6
  LOOSE_AUC_TOL      the reference's own explicitness (saga, max_iter = 300, StandardScaler on fp32) against the
                     optimum's.  N = 777: measured 3.2e-6 (train), 2.9e-6 (test)                           -> 4e-5
                     N = 60 (label dropout): measured 7.4e-5 (train; one AUC pair of a class with 2 x 9 pairs is
                     worth 8e-3 / 7 factors / ~20 classes), 0 (test)                                       -> 8e-4
  PROBA_SOLVE_TOL    two restatement solves stopped at max|grad| <= 1e-9 and <= 1e-11: measured 4.0e-9 at the most
                     (the strong-convexity bound |dtheta| <= |grad| / lambda with lambda = 1/777 allows 1e-6) -> 5e-8
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("itcv_logreg_colstats_workspace", "itcv_logreg_colstats", "itcv_logreg_workspace", "itcv_logreg_valgrad",
       "itcv_logreg_proba", "itcv_logreg_auc", "itcv_zdiff_row")
PROBA_GOLDEN_TOL, LOOSE_AUC_TOL, PROBA_SOLVE_TOL = 6e-6, {"full": 4e-5, "small": 8e-4}, 5e-8


# ---- the rule, restated in numpy fp64 --------------------------------------------------------------------------------
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def ref_colstats(x):
    """StandardScaler: (mean, scale) with the population variance; scale = 1 where the variance is 0."""
    x = np.asarray(x, dtype=np.float64)
    m = x.mean(0)
    s = np.sqrt(((x - m) ** 2).mean(0))
    s[s == 0] = 1.0
    return m, s


def ref_prepare(x, stats=None):
    x = np.asarray(x, dtype=np.float64)
    return x if stats is None else (x - stats[0]) / stats[1]


def ref_logits(theta, X):
    return X @ theta[:-1] + theta[-1]


def ref_objective(theta, X, y, valid, C=1.0):
    """(F, grad) of ONE problem: theta [(D + 1), S], X [N, D] fp64, y [N] ints, valid [S] bools."""
    valid = np.asarray(valid, dtype=bool)
    rows = valid[y]
    n = int(rows.sum())
    Xv, yv = X[rows], y[rows]
    z = np.where(valid, ref_logits(theta, Xv), -np.inf)
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    se = e.sum(1, keepdims=True)
    lam = (2.0 if valid.sum() == 2 else 1.0) / (C * n)
    f = float(((mx + np.log(se))[:, 0] - z[np.arange(n), yv]).sum() / n + 0.5 * lam * (theta[:-1][:, valid] ** 2).sum())
    r = e / se
    r[np.arange(n), yv] -= 1.0
    g = np.zeros_like(theta)
    g[:-1] = Xv.T @ r / n + lam * theta[:-1] * valid
    g[-1] = r.sum(0) / n
    return f, g


def ref_valgrad_all(theta, X, y, sizes, cvalid, C=1.0):
    """(f [K], grad [(D + 1), csum]) of all problems at the stacked theta."""
    off = offsets(sizes)
    f, g = np.zeros(len(sizes)), np.zeros_like(theta)
    for k in range(len(sizes)):
        sl = slice(off[k], off[k + 1])
        f[k], g[:, sl] = ref_objective(theta[:, sl], X, y[:, k], cvalid[sl], C)
    return f, g


def ref_solve(X, y, valid, gtol=1e-11, C=1.0):
    """Newton's method from zero on the valid classes (minimum-norm steps: the intercepts have one flat direction, which
    the gradient never enters).  Returns theta [(D + 1), S] with zeros at the invalid classes and max|grad|."""
    valid = np.asarray(valid, dtype=bool)
    idx = np.flatnonzero(valid)
    remap = -np.ones(len(valid), dtype=int)
    remap[idx] = np.arange(len(idx))
    rows = valid[y]
    Xv, yv = X[rows], remap[y[rows]]
    n, D = Xv.shape
    S = len(idx)
    ones = np.ones(S, dtype=bool)
    Xt = np.concatenate([Xv, np.ones((n, 1))], 1)
    lam = (2.0 if S == 2 else 1.0) / (C * n)
    th = np.zeros((D + 1, S))
    f, g = ref_objective(th, Xv, yv, ones, C)
    for _ in range(200):
        if np.abs(g).max() <= gtol:
            break
        z = ref_logits(th, Xv)
        p = np.exp(z - z.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        A = (Xt[:, :, None] * p[:, None, :]).reshape(n, -1)
        H = -(A.T @ A) / n
        H4 = H.reshape(D + 1, S, D + 1, S)
        for c in range(S):
            H4[:, c, :, c] += Xt.T @ (p[:, c:c + 1] * Xt) / n
            H4[np.arange(D), c, np.arange(D), c] += lam
        step = np.linalg.lstsq(H, -g.reshape(-1), rcond=1e-13)[0].reshape(D + 1, S)
        t = 1.0
        while True:
            f2, g2 = ref_objective(th + t * step, Xv, yv, ones, C)
            if f2 <= f + 1e-4 * t * float((g * step).sum()) or np.abs(g2).max() < np.abs(g).max() or t < 1e-6:
                break
            t *= 0.5
        th, f, g = th + t * step, f2, g2
    out = np.zeros((D + 1, len(valid)))
    out[:, idx] = th
    return out, float(np.abs(g).max())


def ref_proba(theta, X, y, valid):
    """(P [N, S] with 0 for invalid classes and rows with an invalid label, pred [N] = first argmax over valid classes)."""
    valid = np.asarray(valid, dtype=bool)
    z = np.where(valid, ref_logits(theta, X), -np.inf)
    e = np.exp(z - z.max(1, keepdims=True))
    P = e / e.sum(1, keepdims=True)
    P[~valid[y]] = 0.0
    return P, z.argmax(1)


def ref_pair_counts(P, y, valid):
    """(count2, pos, neg) [S] ints over the rows with a valid label."""
    valid = np.asarray(valid, dtype=bool)
    rows = valid[y]
    Pv, yv = P[rows], y[rows]
    S = len(valid)
    c2, pos, neg = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    for c in np.flatnonzero(valid):
        a, b = Pv[yv == c, c], Pv[yv != c, c]
        c2[c] = 2 * int((a[:, None] > b[None, :]).sum()) + int((a[:, None] == b[None, :]).sum())
        pos[c], neg[c] = len(a), len(b)
    return c2, pos, neg


def ref_auc(P, y, valid):
    c2, pos, neg = ref_pair_counts(P, y, valid)
    v = np.asarray(valid, dtype=bool)
    return c2[v] / (2.0 * pos[v] * neg[v])


def ref_present(y, sizes):
    return np.concatenate([np.bincount(y[:, k], minlength=s)[:s] > 0 for k, s in enumerate(sizes)])


def ref_fit_all(X, y, sizes, cvalid, gtol=1e-11):
    off = offsets(sizes)
    theta = np.zeros((X.shape[1] + 1, off[-1]))
    for k in range(len(sizes)):
        sl = slice(off[k], off[k + 1])
        theta[:, sl], _ = ref_solve(X, y[:, k], cvalid[sl], gtol)
    return theta


def ref_explicitness(xtr, vtr, xte, vte, sizes, gtol=1e-11):
    """(train, test, theta, cvalid, stats) by the rule: statistics from train, classes present in both sets."""
    stats = ref_colstats(xtr)
    a, b = ref_prepare(xtr, stats), ref_prepare(xte, stats)
    cvalid = ref_present(vtr, sizes) & ref_present(vte, sizes)
    theta = ref_fit_all(a, vtr, sizes, cvalid, gtol)
    off = offsets(sizes)
    res = []
    for X, v in ((a, vtr), (b, vte)):
        per = []
        for k in range(len(sizes)):
            sl = slice(off[k], off[k + 1])
            per.append(ref_auc(ref_proba(theta[:, sl], X, v[:, k], cvalid[sl])[0], v[:, k], cvalid[sl]).mean())
        res.append(float(np.mean(per)))
    return res[0], res[1], theta, cvalid, stats


def ref_factor_change_accuracy(xtr, ytr, xte, yte, num_classes, scale, gtol=1e-11):
    stats = ref_colstats(xtr) if scale else None
    valid = np.bincount(ytr, minlength=num_classes) > 0
    theta, _ = ref_solve(ref_prepare(xtr, stats), ytr, valid, gtol)
    P, pred = ref_proba(theta, ref_prepare(xte, stats), yte, valid)
    return float((pred == yte).mean()), theta, P


def ref_zdiff(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)).mean(0).astype(np.float32)


# ---- fixtures --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "classify.npz"))
    return {k: g[k] for k in g.files}


_SOLVED = {}


def solved_pair(g, tag):
    """The restatement's explicitness solve of the full / label-dropout pair, computed once per process."""
    if tag not in _SOLVED:
        n = 777 if tag == "full" else 60
        sizes = [int(s) for s in g["sizes"]]
        _SOLVED[tag] = ref_explicitness(g["x_train"][:n], g["v_train"][:n], g["x_test"][:n], g["v_test"][:n], sizes)
    return _SOLVED[tag]


# ---- the boundary ----------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in abi.SIGNATURES and hasattr(lib, n), n
    assert abi.ABI_VERSION == 4


def test_refusals_before_any_launch():
    from hipvae import abi
    lib = abi.lib
    one = ctypes.c_void_p(16)          # never dereferenced: every call below is refused by the range checks

    def valgrad(N, D, sizes):
        cs = (ctypes.c_int * len(sizes))(*sizes)
        return lib.itcv_logreg_valgrad(one, D, None, None, one, N, D, len(sizes), cs, one, one, 1.0, one, one, one, one, 1 << 40,
                                       None)
    for args, what in (((10, 8, [2] * 17), "K = 17"), ((10, 8, [2, 257]), "257 classes"), ((10, 513, [3]), "D = 513"),
                       ((0, 8, [3]), "N = 0"), ((10, 8, [0]), "0 classes")):
        assert valgrad(*args) != 0
        assert what in abi.last_error(), (what, abi.last_error())
    cs = (ctypes.c_int * 1)(300)
    assert lib.itcv_logreg_proba(one, 8, None, None, one, 10, 8, 1, cs, one, one, one, one, one, None) != 0
    assert lib.itcv_logreg_auc(one, one, 10, 1, cs, one, one, one, one, one, None) != 0
    assert lib.itcv_logreg_colstats(one, 4, 10, 8, one, one, one, one, 1 << 30, None) != 0       # ld < D
    assert lib.itcv_zdiff_row(one, one, 8, 0, 8, one, None) != 0                                  # no rows
    assert lib.itcv_logreg_workspace(10, 513, 1, 3) == 0 and lib.itcv_logreg_workspace(10, 8, 17, 40) == 0
    assert lib.itcv_logreg_workspace(777, 10, 7, 100) >= 11 * 100 * 8
    from hipvae import functional as HF
    with pytest.raises(RuntimeError, match="device tensors"):
        HF.logreg_colstats(torch.zeros(4, 3), torch.zeros(2, dtype=torch.int32))


# ---- the restatement -------------------------------------------------------------------------------------------------
def test_gradient_against_central_differences(golden):
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    X = ref_prepare(g["x_train"][:60], ref_colstats(g["x_train"][:60]))
    y = g["v_train"][:60]
    cvalid = ref_present(y, sizes) & ref_present(g["v_test"][:60], sizes)
    rs = np.random.RandomState(0)
    theta = 0.3 * rs.randn(11, sum(sizes))
    f, grad = ref_valgrad_all(theta, X, y, sizes, cvalid)
    assert not grad[:, ~cvalid].any() and (~cvalid).any()
    h, worst = 1e-6, 0.0
    owner = np.repeat(np.arange(len(sizes)), sizes)
    for _ in range(60):
        d, c = rs.randint(11), rs.randint(sum(sizes))
        tp, tm = theta.copy(), theta.copy()
        tp[d, c] += h
        tm[d, c] -= h
        num = (ref_valgrad_all(tp, X, y, sizes, cvalid)[0][owner[c]] - ref_valgrad_all(tm, X, y, sizes, cvalid)[0][owner[c]]) / (2 * h)
        worst = max(worst, abs(num - grad[d, c]))
    print("max |central difference - gradient|", worst)
    assert worst <= 1e-8                 # truncation h^2 f''' / 6 ~ 1e-13, rounding of f: 2 ulp(f ~ 4) / (2 h) ~ 5e-10


def test_restatement_reproduces_sklearn_at_the_optimum(golden):
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    off = offsets(sizes)
    worst = 0.0
    for tag, n in (("small", 60), ("full", 777)):
        tr, te, theta, cvalid, stats = solved_pair(g, tag)
        for k in range(len(sizes)):
            sl = slice(off[k], off[k + 1])
            cls = g[f"classes_{tag}_{k}"]
            assert np.array_equal(np.flatnonzero(cvalid[sl]), cls)
            sets = [("test", g["x_test"][:n], g["v_test"][:n])] + ([("train", g["x_train"][:n], g["v_train"][:n])] if tag == "small" else [])
            for name, x, v in sets:
                P, _ = ref_proba(theta[:, sl], ref_prepare(x, stats), v[:, k], cvalid[sl])
                rows = cvalid[sl][v[:, k]]
                worst = max(worst, float(np.abs(P[rows][:, cls] - g[f"proba_{tag}_{name}_{k}"]).max()))
        ref = g[f"expl_{tag}"]
        print(tag, "explicitness", (tr, te), "reference (saga, 300)", ref, "distance", abs(tr - ref[0]), abs(te - ref[1]))
        assert abs(tr - ref[0]) <= LOOSE_AUC_TOL[tag] and abs(te - ref[1]) <= LOOSE_AUC_TOL[tag]
    print("max |restatement proba - sklearn tight proba|", worst)
    assert worst <= PROBA_GOLDEN_TOL


def test_factor_change_accuracy_equals_the_reference(golden):
    g = golden
    for scale in (0, 1):
        acc, _, P = ref_factor_change_accuracy(g["fc_x_train"], g["fc_y_train"].astype(int), g["fc_x_test"],
                                               g["fc_y_test"].astype(int), 5, bool(scale))
        d = float(np.abs(P - g[f"fc_proba_{scale}"]).max())
        print("scale", scale, "accuracy", acc, float(g[f"fc_acc_{scale}"]), "max |proba - sklearn|", d)
        assert acc == float(g[f"fc_acc_{scale}"]) and d <= PROBA_GOLDEN_TOL


def test_pair_count_auc_equals_roc_auc_score_with_ties(golden):
    g = golden
    got = ref_auc(g["tie_scores"], g["tie_y"], np.ones(4, dtype=bool))
    print("max |pair-count AUC - roc_auc_score|", np.abs(got - g["tie_auc"]).max())
    assert np.abs(got - g["tie_auc"]).max() <= 1e-15


def test_two_stopping_tolerances_agree(golden):
    """What stopping at max|grad| <= 1e-9 instead of 1e-11 does to the probabilities: the bound the GPU test uses."""
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    off = offsets(sizes)
    _, _, theta, cvalid, stats = solved_pair(g, "full")
    X = ref_prepare(g["x_train"], stats)
    worst = 0.0
    for k in (2, 5):
        sl = slice(off[k], off[k + 1])
        loose, gm = ref_solve(X, g["v_train"][:, k], cvalid[sl], gtol=1e-9)
        assert gm <= 1e-9
        a = ref_proba(loose, X, g["v_train"][:, k], cvalid[sl])[0]
        b = ref_proba(theta[:, sl], X, g["v_train"][:, k], cvalid[sl])[0]
        worst = max(worst, float(np.abs(a - b).max()))
    print("max |proba(gtol 1e-9) - proba(gtol 1e-11)|", worst)
    assert worst <= PROBA_SOLVE_TOL


def test_lbfgs_reaches_the_restatements_optimum_and_reports_failure(golden):
    """hipvae.logreg.minimize driven by the restatement's value/gradient on the CPU: the stopping rule holds for every
    problem, the optimum is Newton's, and too few iterations raise instead of returning."""
    from hipvae import logreg
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    off = [int(o) for o in offsets(sizes)]
    tr, te, theta, cvalid, stats = solved_pair(g, "small")
    X, y = ref_prepare(g["x_train"][:60], stats), g["v_train"][:60]

    def valgrad(t):
        f, gr = ref_valgrad_all(t.numpy(), X, y, sizes, cvalid)
        return torch.from_numpy(f), torch.from_numpy(gr)
    got, info = logreg.minimize(valgrad, theta.shape, off, torch.device("cpu"), gtol=1e-9, max_iter=2000)
    print("iterations", info["iterations"], "evaluations", info["evaluations"], "max|grad|", max(info["gmax"]))
    assert max(info["gmax"]) <= 1e-9 and len(info["gmax"]) == len(sizes)
    for k in range(len(sizes)):
        sl = slice(off[k], off[k + 1])
        a = ref_proba(got.numpy()[:, sl], X, y[:, k], cvalid[sl])[0]
        b = ref_proba(theta[:, sl], X, y[:, k], cvalid[sl])[0]
        assert np.abs(a - b).max() <= PROBA_SOLVE_TOL
    with pytest.raises(RuntimeError, match="problem"):
        logreg.minimize(valgrad, theta.shape, off, torch.device("cpu"), gtol=1e-9, max_iter=3)
