"""CPU-only checks of the device-side FactorVAE and SAP scores: the new entry points are declared, bound and exported
alike and refuse what lies outside their range before any launch, and a numpy fp64 restatement of the two rules of
include/itcv_hip.h -- written here, shared with tests/test_hip_extra_scores.py, free of sklearn and scipy -- reproduces
what was recorded in tests/golden/extra_scores.npz (made by make_golden_extra.py).

The one tolerance that compares with RECORDED numbers of another program was measured when the fixture was made and
carries a 10x margin:
  THETA_GOLDEN_TOL   restatement (damped Newton, max|grad| <= 1e-10) against sklearn's
                     LinearSVC(C=0.01, class_weight="balanced", dual=False, tol=1e-12, max_iter=10**6) coef_ / intercept_
                     on the 8 x 4 pairs of the fixture: measured 3.72e-8 at the most (liblinear's own residual: the
                     restatement's final gradient is 3.7e-15 at the most, so it sits within 1e-14 of the optimum) -> 3.8e-7
Everything else is exact: predictions, S, SAP, the vote tables, the classifier and both accuracies.  Exactness of the
predictions between two solves of the same problem needs the decision values to be away from a tie by more than the
solves can differ: both lie within sqrt(2) * gtol of the unique optimum (F is 1-strongly convex), so decision values
differ by at most 2 * 1.5e-10 * (1 + max|x|) = 3e-10 * (1 + max|x|); the fixture keeps every gap above 1e-7.

The generated cases of the GPU tests whose exactness rests on a property of the data are built here and held to it on the
CPU: the 19-class SAP case converges and keeps every test decision 1e-6 from a tie (100 x what a theta error of 1e-9
moves a decision at |x| <= 10), the wide SAP case converges, and the copied columns of the FactorVAE tie cases have
bitwise-equal variances and ratios while every other arg-min stays 1e-6 (relative) clear of the runner-up."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("itcv_fvae_gvar", "itcv_fvae_votes", "itcv_fvae_classify", "itcv_sap_svc_lds_rows", "itcv_sap_svc_workspace",
       "itcv_sap_svc_fit", "itcv_sap_svc_score")
THETA_GOLDEN_TOL = 3.8e-7
GAP_MIN = 1e-7
ARMIJO, MAX_HALVINGS = 1e-4, 50


# ---- the FactorVAE rule, restated in numpy fp64 ----------------------------------------------------------------------
def ref_gvar(mu_var):
    return np.var(np.asarray(mu_var, dtype=np.float64), axis=0, ddof=1)


def ref_group_ratios(mu, L, gvar, threshold):
    """(ratio[M][D] with inf at the inactive dimensions, lvar[M][D]): rows added in ascending order, each operation
    rounded on its own."""
    x = np.asarray(mu, dtype=np.float32).astype(np.float64)
    M, D = x.shape[0] // L, x.shape[1]
    x = x.reshape(M, L, D)
    s = np.zeros((M, D))
    for r in range(L):
        s = s + x[:, r]
    m = s / float(L)
    q = np.zeros((M, D))
    for r in range(L):
        t = x[:, r] - m
        q = q + t * t
    lvar = q / float(L - 1)
    active = np.sqrt(gvar) >= threshold
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = lvar / gvar[None, :]
    ratio[:, ~active] = np.inf
    return ratio, lvar


def ref_votes(mu, L, gvar, threshold, fidx, K):
    ratio, _ = ref_group_ratios(mu, L, gvar, threshold)
    votes = np.zeros((ratio.shape[1], K), dtype=np.int64)
    if not (np.sqrt(gvar) >= threshold).any():
        return votes
    for g, d in enumerate(np.argmin(ratio, axis=1)):                  # the first minimum: ties to the smallest d
        votes[d, fidx[g]] += 1
    return votes


def ref_factor_vae(mu_var, mu_train, fidx_train, mu_eval, fidx_eval, L, K, threshold=0.05, gvar=None):
    gvar = ref_gvar(mu_var) if gvar is None else gvar
    vt = ref_votes(mu_train, L, gvar, threshold, fidx_train, K)
    ve = ref_votes(mu_eval, L, gvar, threshold, fidx_eval, K)
    classifier = np.argmax(vt, axis=1)                                # the first maximum: ties to the smallest k
    nact = int((np.sqrt(gvar) >= threshold).sum())
    d = np.arange(vt.shape[0])
    train = float(vt[d, classifier].sum()) / len(fidx_train) if nact else 0.0
    ev = float(ve[d, classifier].sum()) / len(fidx_eval) if nact else 0.0
    return dict(gvar=gvar, votes_train=vt, votes_eval=ve, classifier=classifier.astype(np.int32), train_accuracy=train,
                eval_accuracy=ev, num_active=nact)


# ---- the SAP rule, restated in numpy fp64 ----------------------------------------------------------------------------
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def svc_eval(x, t, cw, w, b):
    """(F, gw, gb, hww, hwb, hbb) of F(w, b) = (w^2 + b^2) / 2 + sum_n cw_n max(0, 1 - t_n (w x_n + b))^2."""
    xi = 1.0 - t * (w * x + b)
    act = xi > 0.0
    xa, ta, ca, xia = x[act], t[act], cw[act], xi[act]
    a = ca * xia
    F = 0.5 * (w * w + b * b) + float(np.sum(a * xia))
    gw = w - 2.0 * float(np.sum(a * ta * xa))
    gb = b - 2.0 * float(np.sum(a * ta))
    return (F, gw, gb, 1.0 + 2.0 * float(np.sum(ca * xa * xa)), 2.0 * float(np.sum(ca * xa)),
            1.0 + 2.0 * float(np.sum(ca)))


def svc_solve(x, t, cw, gtol=1e-10, max_iter=100):
    """Damped Newton from (0, 0): (w, b, final max-norm of the gradient, Newton steps, converged)."""
    w = b = 0.0
    e = svc_eval(x, t, cw, w, b)
    gn, it = max(abs(e[1]), abs(e[2])), 0
    while not gn <= gtol and it < max_iter:
        F, gw, gb, hww, hwb, hbb = e
        det = hww * hbb - hwb * hwb
        dw, db = -((hbb * gw - hwb * gb) / det), -((hww * gb - hwb * gw) / det)
        slope = gw * dw + gb * db
        alpha, accepted = 1.0, False
        for _ in range(MAX_HALVINGS + 1):
            wt, bt = w + alpha * dw, b + alpha * db
            et = svc_eval(x, t, cw, wt, bt)
            gt = max(abs(et[1]), abs(et[2]))
            if et[0] <= F + (ARMIJO * alpha) * slope or gt <= gtol:
                w, b, e, gn, accepted = wt, bt, et, gt, True
                break
            alpha *= 0.5
        if not accepted:
            break
        it += 1
    return w, b, gn, it, gn <= gtol


def ref_sap_fit(x_train, y_train, sizes, C=0.01, gtol=1e-10, max_iter=100):
    """(theta[D][csum][2], gnorm[D][csum], iters[D][csum], cvalid[csum], converged): zeros at a slot without a problem."""
    x_train = np.asarray(x_train, dtype=np.float32).astype(np.float64)
    N, D = x_train.shape
    off = offsets(sizes)
    csum = off[-1]
    theta, gnorm = np.zeros((D, csum, 2)), np.zeros((D, csum))
    iters, cvalid, ok = np.zeros((D, csum), dtype=np.int32), np.zeros(csum, dtype=np.int32), True
    for j, s in enumerate(sizes):
        y = y_train[:, j]
        cnt = np.bincount(y, minlength=s)
        V = [c for c in range(s) if cnt[c] > 0]
        cvalid[off[j] + np.array(V)] = 1
        if len(V) < 2:
            continue
        bw = {c: float(N) / (float(len(V)) * float(cnt[c])) for c in V}
        for c in (V if len(V) >= 3 else V[1:]):
            t = np.where(y == c, 1.0, -1.0)
            cw = np.where(y == c, C * bw[c], C * bw[V[0]] if len(V) == 2 else C)
            for i in range(D):
                w, b, gn, it, conv = svc_solve(x_train[:, i], t, cw, gtol, max_iter)
                theta[i, off[j] + c] = (w, b)
                gnorm[i, off[j] + c], iters[i, off[j] + c] = gn, it
                ok = ok and conv
    return theta, gnorm, iters, cvalid, ok


def ref_sap_predict(theta, cvalid, x_test, sizes):
    """(pred[D][K][Nt] int32, the smallest distance of a decision from a tie)."""
    x = np.asarray(x_test, dtype=np.float32).astype(np.float64)
    Nt, D = x.shape
    off = offsets(sizes)
    pred, gap = np.zeros((D, len(sizes), Nt), dtype=np.int32), np.inf
    for j, s in enumerate(sizes):
        V = [c for c in range(s) if cvalid[off[j] + c]]
        for i in range(D):
            if len(V) == 1:
                pred[i, j] = V[0]
            elif len(V) == 2:
                w, b = theta[i, off[j] + V[1]]
                dec = w * x[:, i] + b
                pred[i, j] = np.where(dec > 0.0, V[1], V[0])
                # a binary problem on a constant column is symmetric under the balanced weights: its gradient at the start
                # is 0 up to rounding, no solve leaves (0, 0), the decision is exactly 0 everywhere and V[0] is predicted
                if w != 0.0 or b != 0.0:
                    gap = min(gap, float(np.abs(dec).min()))
            else:
                dec = np.stack([theta[i, off[j] + c, 0] * x[:, i] + theta[i, off[j] + c, 1] for c in V], 0)
                pred[i, j] = np.array(V)[np.argmax(dec, axis=0)]      # the first maximum: ties to the smallest class
                top = np.sort(dec, axis=0)
                gap = min(gap, float((top[-1] - top[-2]).min()))
    return pred, gap


def ref_sap_matrix(pred, y_test):
    """S[D][K] and the integer counts."""
    correct = (pred == np.asarray(y_test).T[None]).sum(2).astype(np.int64)
    return correct / float(pred.shape[2]), correct


def ref_sap(S):
    top = np.sort(S, axis=0)
    diff, tot = top[-1] - top[-2], 0.0
    for v in diff:                                                    # in factor order
        tot = tot + float(v)
    return tot / len(diff)


def ref_sap_continuous(x_train, y_train):
    x, y = np.asarray(x_train, dtype=np.float32).astype(np.float64), np.asarray(y_train, dtype=np.float64)
    xc, yc = x - x.mean(0), y - y.mean(0)
    n = x.shape[0]
    vx, vy = (xc * xc).sum(0) / (n - 1), (yc * yc).sum(0) / (n - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (xc.T @ yc / (n - 1)) ** 2 / (vx[:, None] * vy[None, :])
    S[vx <= 1e-12] = 0.0
    return S


# ---- the cases of tests/test_hip_extra_scores.py that need a condition checked on the host ---------------------------
MANY_GAP_MIN = 1e-6            # 100 x what a theta error of 1e-9 moves a decision with |x| <= 10
MANY_SEED, WIDE_SEED = 5, 0      # of seeds 0..7 the one with the widest gap (1.6e-5; the narrowest, seed 3, has 1.2e-6)


@functools.lru_cache(maxsize=None)
def sap_many_classes_case(seed=MANY_SEED):
    """More problems than the fit kernel has waves: a factor of size 21 whose classes 0 and 7 are absent (19 problems: waves
    0, 1, 2 solve three each, the others two) and a binary factor; 700 train and 300 test rows, D = 2, the latents shifted
    by their labels."""
    rs = np.random.RandomState(seed)
    n, sizes = 1000, [21, 2]
    present = np.array([c for c in range(21) if c not in (0, 7)])
    y = np.stack([present[rs.randint(19, size=n)], rs.randint(2, size=n)], 1).astype(np.int32)
    x = 0.7 * rs.randn(n, 2)
    x[:, 0] += 0.35 * y[:, 0]
    x[:, 1] += 1.2 * y[:, 1]
    x = x.astype(np.float32)
    theta, gnorm, iters, cvalid, ok = ref_sap_fit(x[:700], y[:700], sizes)
    pred, gap = ref_sap_predict(theta, cvalid, x[700:], sizes)
    return dict(sizes=sizes, x_train=x[:700], y_train=y[:700], x_test=x[700:], y_test=y[700:], theta=theta, gnorm=gnorm,
                iters=iters, cvalid=cvalid, ok=ok, pred=pred, gap=gap)


@functools.lru_cache(maxsize=None)
def sap_wide_case(seed=WIDE_SEED):
    """N = 130, D = 70, one factor of 3 classes: two 64-column tiles of the copy kernel (the second 6 wide, and without the
    label part), three 64-row tiles (the last of 2 rows), 70 x 3 problems."""
    rs = np.random.RandomState(seed)
    y = rs.randint(3, size=(130, 1)).astype(np.int32)
    x = (0.7 * rs.randn(130, 70) + y * rs.uniform(-1.5, 1.5, size=70)).astype(np.float32)
    theta, gnorm, iters, cvalid, ok = ref_sap_fit(x, y, [3])
    return dict(sizes=[3], x=x, y=y, theta=theta, gnorm=gnorm, cvalid=cvalid, ok=ok)


FVAE_TIES = {(5, 6, 69): 5, (69, 70): 69, (6, 69): 6}       # the columns that are copies of one another: who takes the vote


@functools.lru_cache(maxsize=None)
def fvae_tie_case(cols):
    """D = 131, 41 train and 9 eval groups of L = 3 rows; the columns ``cols`` are copies of cols[0] in all three inputs, and
    their group rows are shrunk so that they hold the smallest ratio of most groups.  Lane l of the vote kernel holds the
    columns l, l + 64, l + 128: (5, 69) tie inside a lane, (5, 6) and (69, 70) across lanes with the smaller index in the
    lower lane, (6, 69) across lanes with the LARGER index in the lower lane."""
    rs = np.random.RandomState(13)
    D, K, L = 131, 3, 3
    mv = rs.randn(67, D).astype(np.float32) * rs.uniform(0.5, 2.0, size=D).astype(np.float32)
    mt, me = rs.randn(41 * L, D).astype(np.float32), rs.randn(9 * L, D).astype(np.float32)
    for a in (mt, me):
        a[:, cols[0]] *= np.float32(0.01)
    for a in (mv, mt, me):
        for c in cols[1:]:
            a[:, c] = a[:, cols[0]]
    return dict(L=L, K=K, mu_var=mv, mu_train=mt, mu_eval=me, fidx_train=rs.randint(K, size=41),
                fidx_eval=rs.randint(K, size=9))


# ---- the tests -------------------------------------------------------------------------------------------------------
def test_many_classes_case_converges_and_keeps_its_decisions_off_a_tie():
    c = sap_many_classes_case()
    cnt = np.bincount(c["y_train"][:, 0], minlength=21)
    assert (cnt > 0).sum() == 19 and cnt[0] == 0 and cnt[7] == 0 and (np.bincount(c["y_train"][:, 1]) > 0).all()
    assert c["cvalid"].tolist() == [int(k not in (0, 7)) for k in range(21)] + [1, 1]
    assert c["ok"] and c["gnorm"].max() <= 1e-10 and np.abs(c["x_test"]).max() <= 10.0
    solved = c["iters"] > 0
    assert solved.sum() == 2 * (19 + 1) and not c["theta"][~solved].any()
    print("smallest decision gap", c["gap"], "newton steps at the most", c["iters"].max())
    assert c["gap"] >= MANY_GAP_MIN
    assert len(set(c["pred"][0, 0])) > 3                              # the informative latent tells classes apart


def test_wide_case_converges():
    c = sap_wide_case()
    assert c["ok"] and c["gnorm"].max() <= 1e-10 and c["cvalid"].tolist() == [1, 1, 1]
    assert (np.abs(c["theta"]).max(axis=(1, 2)) > 0).all()            # all 70 columns are fitted


@pytest.mark.parametrize("cols", sorted(FVAE_TIES), ids=lambda c: "-".join(map(str, c)))
def test_fvae_tie_case_ties_exactly_and_the_first_copy_takes_the_votes(cols):
    c = fvae_tie_case(cols)
    gvar = ref_gvar(c["mu_var"])
    assert all(gvar[k] == gvar[cols[0]] for k in cols)                # the same bits: the ratios tie exactly
    winner = FVAE_TIES[cols]
    assert winner == min(cols)
    for part in ("train", "eval"):
        ratio, _ = ref_group_ratios(c[f"mu_{part}"], c["L"], gvar, 0.05)
        assert all(np.array_equal(ratio[:, k], ratio[:, winner]) for k in cols)
        votes = ref_votes(c[f"mu_{part}"], c["L"], gvar, 0.05, c[f"fidx_{part}"], c["K"])
        taken = int(votes[winner].sum())
        print(cols, part, "groups won by the copies", taken, "of", len(c[f"fidx_{part}"]))
        assert 2 * taken > len(c[f"fidx_{part}"]) and not any(votes[k].any() for k in cols if k != winner)
        # away from the planted tie, no arg-min is close enough for a last-bit difference of gvar (1e-13) to move it
        rest = np.sort(np.delete(ratio, [k for k in cols if k != winner], axis=1), axis=1)
        assert ((rest[:, 1] - rest[:, 0]) / rest[:, 1]).min() > 1e-6


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "extra_scores.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def sap_fit(golden):
    g = golden
    sizes = [int(s) for s in g["sap_sizes"]]
    theta, gnorm, iters, cvalid, ok = ref_sap_fit(g["sap_x_train"], g["sap_y_train"], sizes)
    pred, gap = ref_sap_predict(theta, cvalid, g["sap_x_test"], sizes)
    return dict(sizes=sizes, theta=theta, gnorm=gnorm, iters=iters, cvalid=cvalid, ok=ok, pred=pred, gap=gap)


def header_text():
    return open(os.path.join(ROOT, "include", "itcv_hip.h")).read()


def test_entry_points_declared_bound_and_exported():
    from hipvae import abi
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/itcv_hip.h"
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    src = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "Makefile")).read()
    assert "extra_scores.hip" in src
    # the contraction pragma is in force wherever the order of operations is part of the rule
    hip = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "extra_scores.hip")).read()
    assert "#pragma clang fp contract(off)" in hip


def test_library_refuses_before_any_launch():
    from hipvae import abi
    L = abi.lib
    sizes = (ctypes.c_int * 2)(3, 2)
    assert L.itcv_fvae_votes(None, 10, 4, 1, 10, None, 0.05, None, 4, None, None, None) != 0
    assert "L = 1" in abi.last_error()
    assert L.itcv_fvae_votes(None, 10, 4, 5, 513, None, 0.05, None, 4, None, None, None) != 0
    assert "D = 513" in abi.last_error()
    assert L.itcv_fvae_votes(None, 10, 4, 5, 10, None, 0.05, None, 4, None, None, None) != 0      # NULL pointers
    assert L.itcv_fvae_gvar(None, 10, 1, 10, None, None, None) != 0
    assert "N = 1" in abi.last_error()
    assert L.itcv_fvae_classify(None, None, 10, 0, 3, 3, None, 0.05, None, None, None) != 0
    assert L.itcv_sap_svc_fit(None, 8, None, 100, 8, 17, sizes, 0.01, 1e-10, 100, None, None, None, None, None, None, 0,
                              None) != 0
    assert "K = 17" in abi.last_error()
    assert L.itcv_sap_svc_fit(None, 8, None, (1 << 24) + 1, 8, 2, sizes, 0.01, 1e-10, 100, None, None, None, None, None,
                              None, 0, None) != 0
    assert "N = 16777217" in abi.last_error()
    big = (ctypes.c_int * 2)(3, 257)
    assert L.itcv_sap_svc_score(None, 8, None, 100, 8, 2, big, None, None, None, None, None, None) != 0
    assert "257 classes" in abi.last_error()
    assert L.itcv_sap_svc_workspace(100, 8, 2, 5) == 8 * 100 * 4 + 208 + 5 * 4      # xt, yt (padded to 16), counts
    assert L.itcv_sap_svc_workspace(100, 600, 2, 5) == 0 and L.itcv_sap_svc_workspace((1 << 24) + 1, 8, 2, 5) == 0
    assert 10000 <= L.itcv_sap_svc_lds_rows() and 5 * L.itcv_sap_svc_lds_rows() <= 64 * 1024


def test_wrappers_refuse_cpu_tensors_short_groups_and_single_latents(golden):
    from hipvae import abi
    from hipvae import disentangle as DS
    g = golden
    mv, mt, me = (torch.from_numpy(g[k]) for k in ("fv_mu_var", "fv_mu_train5", "fv_mu_eval5"))
    ft, fe = g["fv_fidx_train"], g["fv_fidx_eval"]
    with pytest.raises(ValueError, match="L >= 2"):
        DS.factor_vae_score(mv, mt, ft, me, fe, 1, 4)
    with pytest.raises(ValueError, match="at least 2 rows"):
        DS.factor_vae_score(mv[:1], mt, ft, me, fe, 5, 4)
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.factor_vae_score(mv, mt, ft, me, fe, 5, 4)
    xtr, xte = torch.from_numpy(g["sap_x_train"]), torch.from_numpy(g["sap_x_test"])
    ytr, yte = torch.from_numpy(g["sap_y_train"]), torch.from_numpy(g["sap_y_test"])
    sizes = [int(s) for s in g["sap_sizes"]]
    for cont in (False, True):
        with pytest.raises(ValueError, match="at least two latents"):
            DS.sap_score(xtr[:, :1], ytr, xte[:, :1], yte, sizes, continuous_factors=cont)
        with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
            DS.sap_score(xtr, ytr, xte, yte, sizes, continuous_factors=cont)
    with pytest.raises(abi.HipExtensionError, match="CPU tensor"):
        DS.sap_score_matrix(xtr, ytr, xte, yte, sizes)

    class NoModel:
        training = False

    with pytest.raises(ValueError, match="L >= 2"):
        DS.compute_factor_vae_score(None, NoModel(), batch_size=1)


def test_solver_attributes_default_to_nothing():
    import inspect
    from solvers import VAESolver
    src = inspect.getsource(VAESolver.__init__)
    assert "self.extra_scores = ()" in src and "self.factor_vae_params = None" in src and "self.sap_params = None" in src


def test_sampler_fixed_factor_group():
    from hipvae.disentangle import FactorSampler

    class DS:
        factor_sizes, latent_indices = [4, 1, 5], [0, 2]

        def __getitem__(self, i):
            return torch.full((1, 2, 2), float(i)), 0

    a, b = FactorSampler(DS(), "cpu", seed=5), FactorSampler(DS(), "cpu", seed=5)
    f, obs = a.sample_fixed_factor(6, 1)
    want = b.sample_factors_of_variation(6)                           # the draws: the factors first ...
    want[:, 1] = want[0, 1]                                           # ... the fixed value is row 0's
    assert np.array_equal(f, want) and (f[:, 1] == f[0, 1]).all() and len(set(f[:, 0])) > 1
    assert torch.equal(obs, b.sample_observations_from_factors(want))
    assert obs[:, 0, 0, 0].tolist() == [float(5 * r[0] + r[1]) for r in f]


def test_restatement_reproduces_recorded_sklearn(golden, sap_fit):
    g, f = golden, sap_fit
    assert f["ok"] and f["gnorm"].max() <= 1e-10
    assert np.array_equal(f["cvalid"], g["sap_cvalid"])
    mask = g["sap_sk_mask"].astype(bool)                              # slots sklearn has a (coef_, intercept_) for
    assert mask.sum() == 8 * (3 + 1 + 5 + 1)
    err = np.abs(f["theta"] - g["sap_sk_theta"])[mask].max()
    print("max |theta - sklearn| =", err, "newton steps at the most:", f["iters"].max())
    assert err <= THETA_GOLDEN_TOL
    assert not f["theta"][~mask].any() and not f["iters"][~mask].any()
    # the recorded restatement (made on another day, another numpy): well inside what two solves may differ by
    assert np.abs(f["theta"] - g["sap_theta"]).max() <= 1e-9
    assert np.array_equal(f["pred"], g["sap_sk_pred"]) and np.array_equal(f["pred"], g["sap_pred"])
    S, correct = ref_sap_matrix(f["pred"], g["sap_y_test"])
    assert np.array_equal(correct, g["sap_correct"]) and np.array_equal(S, g["sap_S"])
    assert ref_sap(S) == float(g["sap_score"])
    assert 0.0 < ref_sap(S) < 1.0


def test_fixture_has_the_planted_cases_and_a_prediction_gap(golden, sap_fit):
    g, f = golden, sap_fit
    xtr, ytr, yte = g["sap_x_train"], g["sap_y_train"], g["sap_y_test"]
    assert xtr.dtype == np.float32 and xtr.shape == (601, 8) and g["sap_x_test"].shape == (300, 8)
    assert f["sizes"] == [3, 2, 6, 5]
    assert np.ptp(xtr[:, 6]) == 0 and np.array_equal(xtr[:, 2], xtr[:, 7])       # a constant column, two identical ones
    c6 = np.bincount(ytr[:, 2], minlength=6)
    assert (c6 == 0).sum() == 1 and (c6 == 1).sum() == 1                          # one class absent, one with a single row
    assert (np.bincount(yte[:, 2], minlength=6) > 0)[c6 == 0].all()               # the absent class occurs in the test rows
    assert (np.bincount(ytr[:, 3], minlength=5) > 0).sum() == 2                   # exactly two classes of five
    bound = 3e-10 * (1.0 + np.abs(g["sap_x_test"]).max())
    print("smallest decision gap", f["gap"], "bound", bound)
    assert f["gap"] > GAP_MIN > 10 * bound
    # the one decision that is a tie by symmetry: the binary problems of the constant column never leave the start
    off = offsets(f["sizes"])
    stuck = [(i, j) for j in (1, 3) for i in range(8) if not f["theta"][i, off[j]:off[j + 1]].any()]
    assert stuck == [(6, 1), (6, 3)] and not f["iters"][6, off[1]:off[2]].any()
    # identical columns give identical classifiers and rows of S
    assert np.array_equal(f["theta"][2], f["theta"][7]) and np.array_equal(f["pred"][2], f["pred"][7])


def test_continuous_restatement(golden):
    g = golden
    S = ref_sap_continuous(g["sap_x_train"], g["sap_y_train"])
    assert S.shape == (8, 4) and not S[6].any() and np.array_equal(S[2], S[7])
    want = np.corrcoef(g["sap_x_train"][:, 0].astype(np.float64), g["sap_y_train"][:, 0].astype(np.float64))[0, 1] ** 2
    assert abs(S[0, 0] - want) <= 1e-12 and ((S >= 0) & (S <= 1 + 1e-12)).all()


@pytest.mark.parametrize("L", [5, 64])
def test_factor_vae_restatement_reproduces_recorded(golden, L):
    g = golden
    got = ref_factor_vae(g["fv_mu_var"], g[f"fv_mu_train{L}"], g["fv_fidx_train"], g[f"fv_mu_eval{L}"], g["fv_fidx_eval"],
                         L, 4)
    assert g["fv_mu_var"].shape == (200, 10) and len(g["fv_fidx_train"]) == 37 and len(g["fv_fidx_eval"]) == 19
    assert g[f"fv_mu_train{L}"].shape == (37 * L, 10) and g[f"fv_mu_eval{L}"].shape == (19 * L, 10)
    assert np.array_equal(got["votes_train"], g[f"fv_votes_train{L}"])
    assert np.array_equal(got["votes_eval"], g[f"fv_votes_eval{L}"])
    assert np.array_equal(got["classifier"], g[f"fv_classifier{L}"])
    assert got["train_accuracy"] == float(g[f"fv_acc{L}"][0]) and got["eval_accuracy"] == float(g[f"fv_acc{L}"][1])
    assert got["votes_train"].sum() == 37 and got["votes_eval"].sum() == 19
    assert got["train_accuracy"] > 0.5                               # the planted structure is found
    # the inactive dimensions take no vote: the constant one and the one just under the threshold
    sd = np.sqrt(got["gvar"])
    assert sd[8] == 0.0 and 0.04 < sd[9] < 0.05 and got["num_active"] == 8
    assert not got["votes_train"][8:].any() and not got["votes_eval"][8:].any()
    # exact copies tie; the smaller index takes every vote
    assert np.array_equal(g["fv_mu_var"][:, 3], g["fv_mu_var"][:, 5]) and not got["votes_train"][5].any()
    assert got["votes_train"][3].any()


@pytest.mark.parametrize("L", [5, 64])
def test_factor_vae_fixture_has_no_accidental_ties(golden, L):
    """Besides the planted copy (dimension 5 of 3), the smallest and the second smallest ratio of every group are apart by
    far more than a last-bit difference of gvar (1e-13 relative) could bridge."""
    g = golden
    gvar = ref_gvar(g["fv_mu_var"])
    for part in ("train", "eval"):
        ratio, _ = ref_group_ratios(g[f"fv_mu_{part}{L}"], L, gvar, 0.05)
        ratio = np.delete(ratio, 5, axis=1)
        top = np.sort(ratio, axis=1)
        rel = ((top[:, 1] - top[:, 0]) / top[:, 1]).min()
        print(part, L, "smallest relative gap of the two best ratios", rel)
        assert rel > 1e-6


def test_all_inactive_gives_zero():
    rs = np.random.RandomState(0)
    mu = (0.01 * rs.randn(40, 3)).astype(np.float32)
    got = ref_factor_vae(mu, mu[:20], [0, 1, 0, 1], mu[20:], [1, 0, 1, 0], 5, 2)
    assert got["num_active"] == 0 and got["train_accuracy"] == 0.0 and got["eval_accuracy"] == 0.0
    assert not got["votes_train"].any()
