"""GPU tests of the device-side FactorVAE and SAP scores (csrc/extra_scores.hip, hipvae/disentangle.py) against the numpy
fp64 restatement of tests/test_extra_scores_host.py and the values recorded in golden/extra_scores.npz.

Bounds: vote tables, classifiers, accuracies, class masks, predictions, counts, S and SAP are compared EXACTLY (the
fixtures keep every arg-min / arg-max away from a tie, see the host tests).  gvar: 1e-13 relative (a two-pass fp64
variance of 200 O(1) values; each of the two sums carries at most 200 ulp = 4.4e-14 in any order).  theta: 1e-9 absolute
-- the device and the restatement both stop within sqrt(2) * gtol = 1.5e-10 of the unique optimum, and rounding of the
sums (<= 1e-13 here) is far below that.  Continuous variant: 1e-12 (ratios of fp64 sums of 601 O(1) terms).

The planted ties are the exception to "away from a tie": there the two sides are EQUAL bits (copies of a column, decisions
that are small integers), so the tie rule itself decides, and the host tests assert the equality.

What each later shape launches (conditions on the data are asserted in tests/test_extra_scores_host.py):

  test                                  shape                                   path
  vote ... exact_tie [5-6-69]           D 131, L 3, 41 + 9 groups               first minimum of a lane (5 before 69), butterfly 5 | 6
                     [69-70]                                                    butterfly, the smaller index in the lower lane
                     [6-69]                                                     butterfly, the LARGER index in the lower lane
  classifier_second_trip                D 300, K 130, tables by hand            a thread's second trip (D > 256), first of two equal
                                                                                maxima, all-zero rows, K > 4
  variances_with_empty_row_slots        N 2 and 31, D 131                       30 and 1 of the 32 row slots empty
  votes_shortest_group ...              M 5; L 2 and 197; D 70                  a short second block; L - 1 = 1; L past 64, odd
  sap_more_problems_than_waves          N 700, D 2, 19 of 21 classes + binary   waves 0, 1, 2 solve 3 problems, the others 2
  sap_wide_and_ragged_copy_tiles        N 130, D 70, 3 classes                  copy kernel 3 x 2 tiles: a 2-row tile, a 6-column tile,
                                                                                the blocks that skip the labels; 210 problems
  sap_score_tie_rules                   300 rows, D 2, sizes 4 4 3 by hand      ties of 2 and of 3 decisions, class 0 absent, dec == 0.0,
                                                                                dec < 0, dec > 0; a second block of test rows

Largest errors on the MI355X in these tests: gvar 7.7e-16 relative (0 at N = 2 and 31), theta 1.0e-15 (19 + 1 problems;
final gradient 3.2e-14, 6 Newton steps) and 3.3e-16 (the wide case; 1.0e-15, 4 steps); everything else is exact."""
import os

import numpy as np
import pytest
import torch

from test_extra_scores_host import (FVAE_TIES, GOLDEN, MANY_GAP_MIN, fvae_tie_case, offsets, ref_factor_vae, ref_gvar,
                                    ref_sap, ref_sap_continuous, ref_sap_fit, ref_sap_matrix, ref_sap_predict, ref_votes,
                                    sap_many_classes_case, sap_wide_case)

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
THETA_TOL, GTOL = 1e-9, 1e-10


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
    g = np.load(os.path.join(GOLDEN, "extra_scores.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def sap_ref(golden):
    """The restatement's fit of the fixture, computed once."""
    g = golden
    sizes = [int(s) for s in g["sap_sizes"]]
    theta, gnorm, iters, cvalid, ok = ref_sap_fit(g["sap_x_train"], g["sap_y_train"], sizes)
    assert ok
    return dict(sizes=sizes, theta=theta, cvalid=cvalid)


# ---- FactorVAE ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [5, 64])
@pytest.mark.parametrize("view", ["dense", "strided"])
def test_fvae_votes_on_the_fixture(golden, L, view):
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    g = golden
    put = G if view == "dense" else strided
    mv, mt, me = put(g["fv_mu_var"]), put(g[f"fv_mu_train{L}"]), put(g[f"fv_mu_eval{L}"])
    ft, fe = g["fv_fidx_train"], g["fv_fidx_eval"]
    want = ref_factor_vae(g["fv_mu_var"], g[f"fv_mu_train{L}"], ft, g[f"fv_mu_eval{L}"], fe, L, 4)
    got = DS.factor_vae_votes(mv, mt, ft, me, fe, L, 4)
    gv = got["gvar"].cpu().numpy()
    print("max relative |gvar - ref|", np.max(np.abs(gv - want["gvar"]) / np.maximum(want["gvar"], 1e-300)))
    assert got["gvar"].dtype == torch.float64 and (np.abs(gv - want["gvar"]) <= 1e-13 * want["gvar"]).all()
    assert got["votes_train"].dtype == torch.int64
    assert np.array_equal(got["votes_train"].cpu().numpy(), want["votes_train"])
    assert np.array_equal(got["votes_eval"].cpu().numpy(), want["votes_eval"])
    assert np.array_equal(got["votes_train"].cpu().numpy(), g[f"fv_votes_train{L}"])
    assert np.array_equal(got["classifier"].cpu().numpy(), want["classifier"])
    assert (got["train_accuracy"], got["eval_accuracy"]) == (want["train_accuracy"], want["eval_accuracy"])
    assert got["num_active"] == 8
    assert DS.factor_vae_score(mv, mt, ft, me, fe, L, 4) == tuple(float(v) for v in g[f"fv_acc{L}"])
    # the entry point alone, handed the restatement's variances
    flags = HF.extra_flags(dev())
    votes = HF.fvae_votes(mt, L, G(want["gvar"]), 0.05, ft, 4, flags)
    assert np.array_equal(votes.cpu().numpy(), ref_votes(g[f"fv_mu_train{L}"], L, want["gvar"], 0.05, ft, 4))
    assert flags.tolist() == [0, 0, 0]


def test_fvae_shapes_that_are_no_multiple_of_anything():
    """D = 131 (three lanes' worth past two full sweeps of the wave, five column tiles of the variance kernel), 7 groups
    (two blocks of the vote kernel, the second one short), L = 3, 67 variance rows (two full row sweeps and three)."""
    from hipvae import disentangle as DS
    rs = np.random.RandomState(11)
    D, K, L = 131, 3, 3
    mv = rs.randn(67, D).astype(np.float32) * rs.uniform(0.01, 2.0, size=D).astype(np.float32)
    mt, me = rs.randn(7 * L, D).astype(np.float32), rs.randn(5 * L, D).astype(np.float32)
    ft, fe = rs.randint(K, size=7), rs.randint(K, size=5)
    want = ref_factor_vae(mv, mt, ft, me, fe, L, K)
    assert 0 < want["num_active"] < D
    got = DS.factor_vae_votes(strided(mv), G(mt), ft, strided(me), fe, L, K)
    assert (np.abs(got["gvar"].cpu().numpy() - want["gvar"]) <= 1e-13 * want["gvar"]).all()
    # the votes under the DEVICE's variances: a last-bit difference of gvar may not move an arg-min here either
    again = ref_factor_vae(mv, mt, ft, me, fe, L, K, gvar=got["gvar"].cpu().numpy())
    assert np.array_equal(again["votes_train"], want["votes_train"])
    assert np.array_equal(got["votes_train"].cpu().numpy(), want["votes_train"])
    assert np.array_equal(got["votes_eval"].cpu().numpy(), want["votes_eval"])
    assert np.array_equal(got["classifier"].cpu().numpy(), want["classifier"])
    assert (got["train_accuracy"], got["eval_accuracy"], got["num_active"]) == \
        (want["train_accuracy"], want["eval_accuracy"], want["num_active"])


def test_fvae_all_inactive_and_refusals(golden):
    from hipvae import disentangle as DS
    g = golden
    rs = np.random.RandomState(0)
    small = (0.01 * rs.randn(40, 3)).astype(np.float32)
    assert DS.factor_vae_score(G(small), G(small[:20]), [0, 1, 0, 1], G(small[20:]), [1, 0, 1, 0], 5, 2) == (0.0, 0.0)
    mv, mt, me = G(g["fv_mu_var"]), G(g["fv_mu_train5"]), G(g["fv_mu_eval5"])
    ft, fe = g["fv_fidx_train"], g["fv_fidx_eval"]
    for where in ("var", "train", "eval"):
        bad = {"var": mv, "train": mt, "eval": me}[where].clone()
        bad[7, 2] = float("nan")
        args = dict(var=(bad, mt, ft, me, fe), train=(mv, bad, ft, me, fe), eval=(mv, mt, ft, bad, fe))[where]
        with pytest.raises(ValueError, match="non-finite"):
            DS.factor_vae_score(*args, 5, 4)
    fb = ft.copy()
    fb[3] = 4
    with pytest.raises(ValueError, match="outside"):
        DS.factor_vae_score(mv, mt, fb, me, fe, 5, 4)
    with pytest.raises(RuntimeError, match="K = 257"):
        DS.factor_vae_score(mv, mt, ft, me, fe, 5, 257)
    with pytest.raises(ValueError, match="L >= 2"):
        DS.factor_vae_score(mv, mt, ft, me, fe, 1, 4)
    torch.cuda.synchronize()                                          # no fault behind any of them
    assert DS.factor_vae_score(mv, mt, ft, me, fe, 5, 4) == tuple(float(v) for v in g["fv_acc5"])


@pytest.mark.parametrize("cols", sorted(FVAE_TIES), ids=lambda c: "-".join(map(str, c)))
def test_fvae_vote_goes_to_the_smallest_index_of_an_exact_tie(cols):
    """Copies of a column have bitwise-equal variances and ratios (asserted on the host): the vote goes to the smallest
    index, inside a lane (5 before 69) and in the butterfly, whichever of the two lanes holds the larger index."""
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    c, winner = fvae_tie_case(cols), FVAE_TIES[cols]
    L, K, ft, fe = c["L"], c["K"], c["fidx_train"], c["fidx_eval"]
    want = ref_factor_vae(c["mu_var"], c["mu_train"], ft, c["mu_eval"], fe, L, K)
    mv, mt, me = strided(c["mu_var"]), strided(c["mu_train"]), strided(c["mu_eval"])
    got = DS.factor_vae_votes(mv, mt, ft, me, fe, L, K)
    gv = got["gvar"].cpu().numpy()
    print("max relative |gvar - ref|", np.max(np.abs(gv - want["gvar"]) / want["gvar"]))
    assert (np.abs(gv - want["gvar"]) <= 1e-13 * want["gvar"]).all() and all(gv[k] == gv[winner] for k in cols)
    for part in ("train", "eval"):
        votes = got[f"votes_{part}"].cpu().numpy()
        assert np.array_equal(votes, want[f"votes_{part}"])
        assert 2 * votes[winner].sum() > votes.sum() and not any(votes[k].any() for k in cols if k != winner)
    assert np.array_equal(got["classifier"].cpu().numpy(), want["classifier"])
    assert (got["train_accuracy"], got["eval_accuracy"], got["num_active"]) == \
        (want["train_accuracy"], want["eval_accuracy"], want["num_active"])
    again = DS.factor_vae_votes(mv, mt, ft, me, fe, L, K)
    assert all(torch.equal(got[k], again[k]) for k in ("gvar", "votes_train", "votes_eval", "classifier"))
    # the entry point alone, handed the restatement's variances
    flags = HF.extra_flags(dev())
    votes = HF.fvae_votes(mt, L, G(want["gvar"]), 0.05, ft, K, flags)
    assert np.array_equal(votes.cpu().numpy(), want["votes_train"]) and flags.tolist() == [0, 0, 0]


def test_fvae_classifier_second_trip_tied_maxima_and_empty_rows():
    """D = 300 (the second trip of the block's 256 threads), K = 130, tables written by the test: a single maximum in most
    rows, two equal maxima in every 10th (the first k wins), no vote at all in every 17th other (class 0)."""
    from hipvae import functional as HF
    D, K = 300, 130
    rs = np.random.RandomState(2)
    vt = rs.randint(0, 3, size=(D, K)).astype(np.int64)
    ve = rs.randint(0, 4, size=(D, K)).astype(np.int64)
    want_cls, want_ht = np.zeros(D, dtype=np.int32), 0
    for d in range(D):
        k1 = (7 * d + 3) % K
        if d % 10 == 0:
            k1 = min(k1, K - 41)
            vt[d, k1] = vt[d, k1 + 40] = 5 + d % 4                  # two equal maxima: the first one
        elif d % 17 == 0:
            vt[d], k1 = 0, 0                                          # nobody voted for this dimension
        else:
            vt[d, k1] = 3 + d % 4
        want_cls[d] = k1
        want_ht += int(vt[d, k1])
    want_he = int(ve[np.arange(D), want_cls].sum())
    Mt, Me = int(vt.sum()), int(ve.sum())
    gvar = np.ones(D)
    gvar[::7] = 1e-4                                                  # sqrt = 0.01 < 0.05: inactive, counted out of res[2]
    assert np.array_equal(want_cls, np.argmax(vt, axis=1)) and len(set(want_cls)) > 100
    runs = [HF.fvae_classify(G(vt), G(ve), Mt, Me, G(gvar), 0.05) for _ in range(2)]
    cls, res = runs[0]
    assert torch.equal(cls, runs[1][0]) and torch.equal(res, runs[1][1])
    assert np.array_equal(cls.cpu().numpy(), want_cls)
    assert res.tolist() == [float(want_ht) / float(Mt), float(want_he) / float(Me), float(D - len(range(0, D, 7)))]


@pytest.mark.parametrize("N", [2, 31])
def test_fvae_variances_with_empty_row_slots(N):
    """Fewer rows than the 32 row slots of the variance kernel: the empty slots add exact zeros."""
    from hipvae import functional as HF
    rs = np.random.RandomState(40 + N)
    x = (rs.randn(N, 131) * rs.uniform(0.5, 2.0, size=131)).astype(np.float32)
    want = ref_gvar(x)
    flags = HF.extra_flags(dev())
    got = HF.fvae_gvar(strided(x), flags)
    assert torch.equal(got, HF.fvae_gvar(strided(x), flags)) and flags.tolist() == [0, 0, 0]
    print("N", N, "max relative |gvar - ref|", np.max(np.abs(got.cpu().numpy() - want) / want))
    assert (want > 0).all() and (np.abs(got.cpu().numpy() - want) <= 1e-13 * want).all()


@pytest.mark.parametrize("L", [2, 197])
def test_fvae_votes_shortest_group_and_one_past_the_wave(L):
    """M = 5 groups (a second, short block) of L = 2 and of L = 197 rows, D = 70; the variances are handed over, so both
    sides divide by the same bits and add the rows in the same order: exact."""
    from hipvae import functional as HF
    rs = np.random.RandomState(L)
    M, D, K = 5, 70, 4
    mu = (rs.randn(M * L, D) * rs.uniform(0.2, 2.0, size=(M, 1, D)).repeat(L, 1).reshape(M * L, D)).astype(np.float32)
    gvar, fidx = rs.uniform(0.5, 2.0, size=D), rs.randint(K, size=M)
    gvar[::9] = 1e-4                                                  # inactive dimensions take no vote
    want = ref_votes(mu, L, gvar, 0.05, fidx, K)
    flags = HF.extra_flags(dev())
    runs = [HF.fvae_votes(strided(mu), L, G(gvar), 0.05, fidx, K, flags) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and flags.tolist() == [0, 0, 0]
    assert np.array_equal(runs[0].cpu().numpy(), want) and want.sum() == M and not want[::9].any()


# ---- SAP ---------------------------------------------------------------------------------------------------------------
def check_fit(x, y, sizes, want_theta, want_cvalid, **kw):
    from hipvae import disentangle as DS
    theta, gnorm, iters, cvalid = DS.fit_sap_classifiers(x, y, sizes, **kw)
    assert theta.dtype == gnorm.dtype == torch.float64 and iters.dtype == cvalid.dtype == torch.int32
    err = np.abs(theta.cpu().numpy() - want_theta).max()
    print("max |theta - restatement|", err, "largest final gradient", float(gnorm.max()), "newton steps at the most",
          int(iters.max()))
    assert err <= THETA_TOL and float(gnorm.max()) <= GTOL
    assert np.array_equal(cvalid.cpu().numpy(), want_cvalid)
    return theta, gnorm, iters, cvalid


@pytest.mark.parametrize("view", ["dense", "strided"])
def test_sap_fit_and_score_on_the_fixture(golden, sap_ref, view):
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    g, r = golden, sap_ref
    put = G if view == "dense" else strided
    xtr, xte, ytr, yte = put(g["sap_x_train"]), put(g["sap_x_test"]), G(g["sap_y_train"]), G(g["sap_y_test"])
    first = check_fit(xtr, ytr, r["sizes"], r["theta"], r["cvalid"])
    second = DS.fit_sap_classifiers(xtr, ytr, r["sizes"])
    assert all(torch.equal(a, b) for a, b in zip(first, second))      # bitwise
    theta, _, iters, cvalid = first
    off = np.concatenate([[0], np.cumsum(r["sizes"])])
    assert cvalid.cpu().tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1, 0]      # class 4 of factor 2 is absent
    # slots without a problem stay zero: the absent classes and the smaller class of a binary factor
    th = theta.cpu().numpy()
    assert not th[:, off[1]].any() and not th[:, off[2] + 4].any() and not th[:, off[3]].any()
    assert not th[6, off[1] + 1].any() and int(iters[6, off[1] + 1]) == 0            # the constant column: never leaves 0
    assert torch.equal(theta[2], theta[7])                                               # identical columns
    flags = HF.extra_flags(dev())
    correct, pred = HF.sap_svc_score(xte, yte, r["sizes"], cvalid, theta, flags, with_pred=True)
    assert flags.tolist() == [0, 0, 0] and correct.dtype == torch.int64
    assert np.array_equal(pred.cpu().numpy(), g["sap_pred"]) and np.array_equal(pred.cpu().numpy(), g["sap_sk_pred"])
    assert np.array_equal(correct.cpu().numpy(), g["sap_correct"])
    S = DS.sap_score_matrix(xtr, ytr, xte, yte, r["sizes"])
    assert S.dtype == torch.float64 and S.is_cuda and np.array_equal(S.cpu().numpy(), g["sap_S"])
    assert DS.sap_score(xtr, ytr, xte, yte, r["sizes"]) == float(g["sap_score"])


def test_sap_single_class_factor_and_refusals(golden, sap_ref):
    from hipvae import disentangle as DS
    g, r = golden, sap_ref
    xtr, xte, yte = G(g["sap_x_train"]), G(g["sap_x_test"]), G(g["sap_y_test"])
    y1 = g["sap_y_train"].copy()
    y1[:, 1] = 1                                                      # a factor with a single class: nothing to solve
    theta, gnorm, iters, cvalid, ok = ref_sap_fit(g["sap_x_train"], y1, r["sizes"])
    check_fit(xtr, G(y1), r["sizes"], theta, cvalid)
    pred, gap = ref_sap_predict(theta, cvalid, g["sap_x_test"], r["sizes"])
    want_S, _ = ref_sap_matrix(pred, g["sap_y_test"])
    assert ok and gap > 1e-7 and (pred[:, 1] == 1).all()
    S = DS.sap_score_matrix(xtr, G(y1), xte, yte, r["sizes"])
    assert np.array_equal(S.cpu().numpy(), want_S)
    assert DS.sap_score(xtr, G(y1), xte, yte, r["sizes"]) == ref_sap(want_S)
    ytr = G(g["sap_y_train"])
    with pytest.raises(RuntimeError, match="did not converge"):
        DS.sap_score(xtr, ytr, xte, yte, r["sizes"], max_iter=1)
    with pytest.raises(RuntimeError, match="did not converge"):
        DS.fit_sap_classifiers(xtr, ytr, r["sizes"], max_iter=1)
    bad = xtr.clone()
    bad[5, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        DS.sap_score(bad, ytr, xte, yte, r["sizes"])
    yb = ytr.clone()
    yb[9, 2] = 6
    with pytest.raises(ValueError, match="outside"):
        DS.sap_score(xtr, yb, xte, yte, r["sizes"])
    with pytest.raises(RuntimeError, match="257 classes"):
        DS.sap_score(xtr, ytr, xte, yte, r["sizes"][:-1] + [257])
    with pytest.raises(ValueError, match="at least two latents"):
        DS.sap_score(xtr[:, :1], ytr, xte[:, :1], yte, r["sizes"])
    torch.cuda.synchronize()                                          # no fault behind any of them
    assert DS.sap_score(xtr, ytr, xte, yte, r["sizes"]) == float(g["sap_score"])


def test_sap_rows_past_the_lds_limit_are_streamed():
    """N = the LDS limit + 37: the column and the labels are read from the feature-major copies (the kernel's other path);
    D = 2 and two factors keep the restatement quick.  The seed keeps every decision 4e-5 away from a tie."""
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    N = HF.sap_svc_lds_rows() + 37
    assert N == 12837
    rs = np.random.RandomState(1)
    sizes = [3, 2]
    y = np.stack([rs.randint(s, size=N + 200) for s in sizes], 1).astype(np.int32)
    x = 0.7 * rs.randn(N + 200, 2)
    x[:, 0] += y[:, 0]
    x[:, 1] += 1.2 * y[:, 1]
    x = x.astype(np.float32)
    theta, gnorm, iters, cvalid, ok = ref_sap_fit(x[:N], y[:N], sizes)
    pred, gap = ref_sap_predict(theta, cvalid, x[N:], sizes)
    assert ok and gap > 1e-5
    xtr, ytr = strided(x[:N]), G(y[:N])
    first = check_fit(xtr, ytr, sizes, theta, cvalid)
    assert all(torch.equal(a, b) for a, b in zip(first, DS.fit_sap_classifiers(xtr, ytr, sizes)))
    S = DS.sap_score_matrix(xtr, ytr, G(x[N:]), G(y[N:]), sizes)
    assert np.array_equal(S.cpu().numpy(), ref_sap_matrix(pred, y[N:])[0])
    # the last row that still fits LDS, same data: the two paths add the same terms in the same order
    inside = DS.fit_sap_classifiers(xtr[:N - 37], ytr[:N - 37], sizes)
    want = ref_sap_fit(x[:N - 37], y[:N - 37], sizes)
    assert np.abs(inside[0].cpu().numpy() - want[0]).max() <= THETA_TOL and float(inside[1].max()) <= GTOL


def test_sap_more_problems_than_waves():
    """19 present classes of 21 and a binary factor: the 8 waves of a (latent, factor) block are dealt three problems (waves
    0, 1, 2) or two; every slot of the big factor is either solved or one of the two absent classes."""
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    c = sap_many_classes_case()
    assert c["ok"] and c["gap"] >= MANY_GAP_MIN and int(c["cvalid"][:21].sum()) == 19 > 2 * (512 // 64)
    xtr, ytr, xte, yte = strided(c["x_train"]), G(c["y_train"]), strided(c["x_test"]), G(c["y_test"])
    first = check_fit(xtr, ytr, c["sizes"], c["theta"], c["cvalid"])
    assert all(torch.equal(a, b) for a, b in zip(first, DS.fit_sap_classifiers(xtr, ytr, c["sizes"])))      # bitwise
    theta, _, iters, cvalid = first
    th, it = theta.cpu().numpy(), iters.cpu().numpy()
    for slot in (0, 7, 21):                                           # the absent classes, the binary factor's first class
        assert not th[:, slot].any() and not it[:, slot].any()
    assert (it[:, [k for k in range(23) if k not in (0, 7, 21)]] > 0).all()
    flags = HF.extra_flags(dev())
    runs = [HF.sap_svc_score(xte, yte, c["sizes"], cvalid, theta, flags, with_pred=True) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and flags.tolist() == [0, 0, 0]
    want_S, want_correct = ref_sap_matrix(c["pred"], c["y_test"])
    assert np.array_equal(runs[0][1].cpu().numpy(), c["pred"]) and np.array_equal(runs[0][0].cpu().numpy(), want_correct)
    S = DS.sap_score_matrix(xtr, ytr, xte, yte, c["sizes"])
    assert np.array_equal(S.cpu().numpy(), want_S) and DS.sap_score(xtr, ytr, xte, yte, c["sizes"]) == ref_sap(want_S)


def test_sap_wide_and_ragged_copy_tiles():
    """N = 130, D = 70: the copy kernel runs 3 x 2 tiles (the last row tile 2 rows, the second column tile 6 columns and no
    label part).  A column's problems read that column alone, so a dense 8-column slice of the same data -- one column
    tile, other row stride -- must give the same bits, on either side of the tile edge."""
    from hipvae import disentangle as DS
    c = sap_wide_case()
    assert c["ok"] and c["x"].shape == (130, 70)
    x, y = strided(c["x"]), G(c["y"])
    first = check_fit(x, y, c["sizes"], c["theta"], c["cvalid"])
    assert all(torch.equal(a, b) for a, b in zip(first, DS.fit_sap_classifiers(x, y, c["sizes"])))
    for lo in (0, 60, 62):
        part = DS.fit_sap_classifiers(G(np.ascontiguousarray(c["x"][:, lo:lo + 8])), y, c["sizes"])
        assert all(torch.equal(a[lo:lo + 8], b) for a, b in zip(first[:3], part)) and torch.equal(first[3], part[3])


def test_sap_score_tie_rules():
    """Hand-written classifiers whose decisions are small integers and quarters, exact in fp64.  Three or more present
    classes: ascending and strict, so a tie goes to the smallest present class (also when class 0 is absent); two present
    classes: the last one only on a decision > 0, the first one on 0.0 and below.  The slots of absent classes and of a
    binary factor's first class hold values that would win if they were read."""
    from hipvae import functional as HF
    sizes, present = [4, 4, 3], [[0, 2, 3], [1, 2, 3], [0, 2]]
    off = offsets(sizes)
    cvalid = np.zeros(off[-1], dtype=np.int32)
    theta = np.full((2, off[-1], 2), 1000.0)
    for j, V in enumerate(present):
        cvalid[off[j] + np.array(V)] = 1
    # latent 0.  factor 0: dec = (x, 1, 1); factor 1: three equal classifiers; factor 2: dec = x - 1
    theta[0, [0, 2, 3]] = [(1, 0), (0, 1), (0, 1)]
    theta[0, [5, 6, 7]] = [(0.5, 0.25)] * 3
    theta[0, 10] = (1, -1)
    # latent 1.  factor 0: dec = (0, -x, x); factor 1: dec = (x, x, 1); factor 2: dec = -2 x
    theta[1, [0, 2, 3]] = [(0, 0), (-1, 0), (1, 0)]
    theta[1, [5, 6, 7]] = [(1, 0), (1, 0), (0, 1)]
    theta[1, 10] = (-2, 0)
    x = np.array([[0, 0], [1, 1], [2, -1], [-1, 2], [3, -2]], dtype=np.float32)
    y = np.array([[2, 1, 0], [0, 1, 2], [3, 3, 2], [2, 1, 0], [0, 3, 2]], dtype=np.int32)
    want_pred = np.array([[[2, 0, 0, 2, 0],      # x = 0: classes 2 and 3 tie at 1; x = 1: all three tie; x = -1: 2 and 3 tie
                           [1, 1, 1, 1, 1],      # all decisions equal, class 0 absent
                           [0, 0, 2, 0, 2]],     # x = 0: -1; x = 1: exactly 0.0; x = 2: +1; x = -1: -2; x = 3: +2
                          [[0, 3, 2, 3, 2],      # x = 0: all three tie at 0
                           [3, 1, 3, 1, 3],      # x = 1: all three tie at 1; x = 2: classes 1 and 2 tie at 2
                           [0, 0, 2, 0, 2]]],    # x = 0: exactly 0.0; x = 2: -4; x = -1: +2
                         dtype=np.int32)
    want_correct = np.array([[4, 3, 4], [0, 4, 4]], dtype=np.int64)
    assert np.array_equal(ref_sap_predict(theta, cvalid, x, sizes)[0], want_pred)
    assert np.array_equal(ref_sap_matrix(want_pred, y)[1], want_correct)
    reps = 60                                                         # 300 rows: a second, short block of test rows
    xs, ys = strided(np.tile(x, (reps, 1))), G(np.tile(y, (reps, 1)))
    flags = HF.extra_flags(dev())
    runs = [HF.sap_svc_score(xs, ys, sizes, G(cvalid), G(theta), flags, with_pred=True) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and flags.tolist() == [0, 0, 0]
    correct, pred = runs[0]
    assert np.array_equal(pred.cpu().numpy(), np.tile(want_pred, (1, 1, reps)))
    assert np.array_equal(correct.cpu().numpy(), reps * want_correct)


def test_sap_continuous_factors(golden):
    from hipvae import disentangle as DS
    g = golden
    sizes = [int(s) for s in g["sap_sizes"]]
    xtr, xte, ytr, yte = strided(g["sap_x_train"]), G(g["sap_x_test"]), G(g["sap_y_train"]), G(g["sap_y_test"])
    want = ref_sap_continuous(g["sap_x_train"], g["sap_y_train"])
    S = DS.sap_score_matrix(xtr, ytr, xte, yte, sizes, continuous_factors=True)
    print("max |S - ref|", np.abs(S.cpu().numpy() - want).max())
    assert np.abs(S.cpu().numpy() - want).max() <= 1e-12 and not S[6].any()
    assert abs(DS.sap_score(xtr, ytr, xte, yte, sizes, continuous_factors=True) - ref_sap(want)) <= 1e-12


# ---- end to end --------------------------------------------------------------------------------------------------------
# the untrained tiny model spreads its means by less than the default 0.05: a threshold that keeps its dimensions active
FV = dict(num_train=8, num_eval=4, num_variance_estimate=64, batch_size=8, threshold=1e-6)
SAP = dict(num_train=64, num_test=32, batch_size=16)


@pytest.fixture(scope="module")
def tiny_model():
    import models
    torch.manual_seed(0)
    return models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()


def test_compute_scores_end_to_end(tiny_model):
    from hipvae import disentangle as DS
    from test_hip_disent import make_dataset
    model, ds = tiny_model, make_dataset()
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    runs = []
    for _ in range(2):
        sampler = DS.FactorSampler(ds, dev(), seed=42)
        fv = DS.compute_factor_vae_score(sampler, model, params=FV)
        sap = DS.compute_sap_score(sampler, model, params=SAP)
        runs.append((fv, sap))
    (train, ev), sap = runs[0]
    print("factor_vae", train, ev, "sap", sap)
    assert all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in (train, ev, sap))
    assert runs[0] == runs[1]                                         # a fixed sampler seed: the same scores
    assert model.training and before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    model.eval()
    DS.compute_factor_vae_score(DS.FactorSampler(ds, dev(), seed=1), model, params=FV)
    assert not model.training
    model.train()
    # the same draws, encoded by the test and scored by the restatement
    twin = DS.FactorSampler(ds, dev(), seed=42)
    mu_var, _ = DS.factor_representations(twin, model, 64, 8)
    model.eval()
    with torch.no_grad():
        mt, ft = DS._fixed_factor_representations(twin, model, 8, 8, 128)
        me, fe = DS._fixed_factor_representations(twin, model, 4, 8, 128)
    model.train()
    assert mt.shape == (64, 10) and me.shape == (32, 10) and ft.shape == (8,)
    got = DS.factor_vae_votes(mu_var, mt, ft, me, fe, 8, 2, threshold=FV["threshold"])
    print("active dimensions", got["num_active"], "votes", got["votes_train"].t().tolist())
    assert (got["train_accuracy"], got["eval_accuracy"]) == (train, ev)
    assert got["num_active"] > 0 and int(got["votes_train"].sum()) == 8 and int(got["votes_eval"].sum()) == 4
    assert train >= 0.5                                               # a majority vote over two factors


def test_solver_writes_the_extra_scores(tiny_model):
    from solvers import VAESolver
    from test_hip_disent import StubWriter, make_dataset
    from hipvae.disentangle import FactorSampler
    model, ds = tiny_model, make_dataset()
    w = StubWriter()
    solver = VAESolver(dataset=ds, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                       optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                       beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)
    assert solver.extra_scores == () and solver.factor_vae_params is None and solver.sap_params is None
    solver.latent_generator = FactorSampler(ds, dev(), seed=42)
    solver.write_disentanglemnt_scores(0)
    today = [(c[0], c[1]) for c in w.calls]
    assert today == [("add_scalar", "mig_score"), ("add_scalars", "mod_expl")]          # what it writes today
    solver.extra_scores, solver.factor_vae_params, solver.sap_params = ("factor_vae", "sap"), FV, SAP
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    w.calls.clear()
    solver.write_disentanglemnt_scores(0)
    assert [(c[0], c[1]) for c in w.calls] == today + [("add_scalars", "factor_vae"), ("add_scalar", "sap_score")]
    fv, sap = w.calls[-2], w.calls[-1]
    assert list(fv[2]) == ["train_accuracy", "eval_accuracy"] and fv[3] == 0 and sap[3] == 0
    assert all(0.0 <= v <= 1.0 for v in list(fv[2].values()) + [sap[2]])
    assert model.training and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    # without the device scores and without the reference's evaluation package: the two new records alone
    solver.device_scores = False
    w.calls.clear()
    solver.write_disentanglemnt_scores(0)
    assert [(c[0], c[1]) for c in w.calls] == [("add_scalars", "factor_vae"), ("add_scalar", "sap_score")]
    solver.extra_scores = ("sap",)
    w.calls.clear()
    solver.write_disentanglemnt_scores(0)
    assert [(c[0], c[1]) for c in w.calls] == [("add_scalar", "sap_score")]
    # nothing off the test iteration; an unknown name is refused; () and no device scores: nothing at all
    solver.test_iter = 2
    solver.write_disentanglemnt_scores(1)
    solver.test_iter, solver.extra_scores = 1, ("mig",)
    with pytest.raises(ValueError, match="unknown"):
        solver.write_disentanglemnt_scores(0)
    solver.extra_scores = ()
    solver.write_disentanglemnt_scores(0)
    assert len(w.calls) == 1 and model.training
