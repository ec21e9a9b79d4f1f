#!/usr/bin/env python3
"""Golden vectors for the device-side FactorVAE and SAP scores.  RUNS ONLY IN THE BUILD CONTAINER (needs numpy and
sklearn; no GPU, and nothing of the reference: it has neither score).

Writes ``extra_scores.npz``:

* SAP fixture (``sap_*``): ``x_train [601, 8]`` / ``x_test [300, 8]`` fp32, ``y_* [N, 4]`` int32, ``sizes = [3, 2, 6, 5]``.
  Columns 0-3 carry factors 0-3, column 4 mixes factors 0 and 2, column 5 is noise, column 6 is constant and column 7 an
  exact copy of column 2.  In the size-6 factor class 4 never occurs in the training labels (it does in the test labels)
  and class 5 has a single training row; of the size-5 factor the training labels hold classes 1 and 3 only.
  Recorded from sklearn, for every (latent i, factor j): ``LinearSVC(C=0.01, class_weight="balanced", dual=False,
  tol=1e-12, max_iter=10**6)`` fitted on column i alone -- ``sk_theta [8, 16, 2]`` = (coef_, intercept_) at the slot of
  the class (the binary model at the slot of the larger class value), ``sk_mask`` the slots it fills, ``sk_pred
  [8, 4, 300]`` its test predictions.  Recorded from the numpy restatement of tests/test_extra_scores_host.py: ``theta``,
  ``pred``, ``correct``, ``S``, ``score``, ``cvalid``.  The seed is the first for which every decision value of the
  restatement is further than 1e-6 from a tie (the tests ask for 1e-7) and sklearn's predictions equal the rule's.
* FactorVAE fixture (``fv_*``): D = 10, K = 4; ``mu_var [200, 10]``, 37 train / 19 eval groups at L = 5 and L = 64.
  Dimensions 0-3 carry factors 0-3, 4 / 6 / 7 are noise, 5 is an exact copy of 3 (the tie rule), 8 is constant and 9 has a
  standard deviation just under the 0.05 threshold.  Recorded from the restatement: votes, classifier, accuracies.

The file holds data only.  Prints the distance between the restatement and sklearn: tests/test_extra_scores_host.py
carries ten times that as its tolerance.

    python tests/golden/make_golden_extra.py
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(1, os.path.join(os.path.dirname(os.path.dirname(HERE)), "intro-tc-vae_amd"))

import numpy as np  # noqa: E402
from sklearn.svm import LinearSVC  # noqa: E402
import test_extra_scores_host as T  # noqa: E402  (the restatement)

SIZES = [3, 2, 6, 5]


def sap_fixture(seed):
    rs = np.random.RandomState(seed)
    out = []
    for n, train in ((601, True), (300, False)):
        y = np.stack([rs.randint(s, size=n) for s in SIZES], 1).astype(np.int32)
        if train:
            y[:, 2] = rs.randint(4, size=n)                   # classes 0..3, never 4 ...
            y[17, 2] = 5                                      # ... and a single row of class 5
            y[:, 3] = np.where(rs.rand(n) < 0.4, 1, 3)        # two classes of five
        x = 0.6 * rs.randn(n, 8)
        for d in range(4):
            x[:, d] += 1.5 * y[:, d] / (SIZES[d] - 1)
        x[:, 4] += 0.8 * y[:, 0] - 0.3 * y[:, 2]
        x[:, 6] = 0.25
        x = x.astype(np.float32)
        x[:, 7] = x[:, 2]
        out += [x, y]
    return out


def sklearn_fits(xtr, ytr, xte):
    off = T.offsets(SIZES)
    theta, mask = np.zeros((8, off[-1], 2)), np.zeros((8, off[-1]), dtype=np.uint8)
    pred = np.zeros((8, len(SIZES), len(xte)), dtype=np.int32)
    for j in range(len(SIZES)):
        for i in range(8):
            clf = LinearSVC(C=0.01, class_weight="balanced", dual=False, tol=1e-12, max_iter=10 ** 6)
            clf.fit(xtr[:, [i]].astype(np.float64), ytr[:, j])
            slots = clf.classes_[1:] if len(clf.classes_) == 2 else clf.classes_
            for r, c in enumerate(slots):
                theta[i, off[j] + c] = (clf.coef_[r, 0], clf.intercept_[r])
                mask[i, off[j] + c] = 1
            pred[i, j] = clf.predict(xte[:, [i]].astype(np.float64))
    return theta, mask, pred


def fv_fixture(seed):
    rs = np.random.RandomState(seed)
    sizes = [4, 5, 3, 6]

    def encode(f):
        n = len(f)
        mu = rs.randn(n, 10)
        for d in range(4):
            mu[:, d] = f[:, d] / sizes[d] + 0.05 * rs.randn(n)
        mu[:, 8] = 0.3
        mu[:, 9] = 0.045 * rs.randn(n)
        mu = mu.astype(np.float32)
        mu[:, 5] = mu[:, 3]
        return mu

    def factors(n):
        return np.stack([rs.randint(s, size=n) for s in sizes], 1)

    out = dict(fv_mu_var=encode(factors(200)))
    out["fv_fidx_train"] = rs.randint(4, size=37).astype(np.int32)
    out["fv_fidx_eval"] = rs.randint(4, size=19).astype(np.int32)
    for L in (5, 64):
        for part in ("train", "eval"):
            rows = []
            for k in out[f"fv_fidx_{part}"]:
                f = factors(L)
                f[:, k] = f[0, k]
                rows.append(encode(f))
            out[f"fv_mu_{part}{L}"] = np.concatenate(rows, 0)
    return out


def main():
    warnings.simplefilter("error")                            # a ConvergenceWarning of liblinear must not pass
    for seed in range(1, 200):
        xtr, ytr, xte, yte = sap_fixture(seed)
        theta, gnorm, iters, cvalid, ok = T.ref_sap_fit(xtr, ytr, SIZES)
        pred, gap = T.ref_sap_predict(theta, cvalid, xte, SIZES)
        print("seed", seed, "converged", ok, "smallest decision gap", gap)
        if not ok or gap <= 1e-6:
            continue
        sk_theta, sk_mask, sk_pred = sklearn_fits(xtr, ytr, xte)
        if np.array_equal(sk_pred, pred):
            break
    else:
        raise SystemExit("no seed keeps the decisions away from a tie")
    m = sk_mask.astype(bool)
    err = np.abs(theta - sk_theta)[m].max()
    print("max |restatement - sklearn| over coef_ / intercept_ =", err, "(the tests allow ten times that)")
    print("newton steps at the most", iters.max(), "largest final gradient", gnorm.max())
    assert not theta[~m].any()
    S, correct = T.ref_sap_matrix(pred, yte)
    out = dict(sap_seed=np.int64(seed), sap_x_train=xtr, sap_y_train=ytr, sap_x_test=xte, sap_y_test=yte,
               sap_sizes=np.array(SIZES, dtype=np.int32), sap_sk_theta=sk_theta, sap_sk_mask=sk_mask, sap_sk_pred=sk_pred,
               sap_theta=theta, sap_pred=pred, sap_correct=correct, sap_S=S, sap_score=np.float64(T.ref_sap(S)),
               sap_cvalid=cvalid, sap_sk_distance=np.float64(err))
    print("S =\n", np.round(S, 3), "\nSAP =", out["sap_score"])
    for seed in range(1, 200):
        fv = fv_fixture(seed)
        gvar, good = T.ref_gvar(fv["fv_mu_var"]), 0.04 < np.sqrt(T.ref_gvar(fv["fv_mu_var"]))[9] < 0.05
        for L in (5, 64):
            for part in ("train", "eval"):
                top = np.sort(np.delete(T.ref_group_ratios(fv[f"fv_mu_{part}{L}"], L, gvar, 0.05)[0], 5, axis=1), axis=1)
                good = good and ((top[:, 1] - top[:, 0]) / top[:, 1]).min() > 1e-5
        if good:
            break
    else:
        raise SystemExit("no seed for the FactorVAE fixture")
    out.update(fv, fv_seed=np.int64(seed))
    for L in (5, 64):
        got = T.ref_factor_vae(fv["fv_mu_var"], fv[f"fv_mu_train{L}"], fv["fv_fidx_train"], fv[f"fv_mu_eval{L}"],
                               fv["fv_fidx_eval"], L, 4)
        out[f"fv_votes_train{L}"], out[f"fv_votes_eval{L}"] = got["votes_train"], got["votes_eval"]
        out[f"fv_classifier{L}"] = got["classifier"]
        out[f"fv_acc{L}"] = np.array([got["train_accuracy"], got["eval_accuracy"]])
        print("FactorVAE L =", L, "accuracies", out[f"fv_acc{L}"], "classifier", got["classifier"], "\n", got["votes_train"].T)
    path = os.path.join(HERE, "extra_scores.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
