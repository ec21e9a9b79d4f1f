#!/usr/bin/env python3
"""Golden vectors for the device-side beta-VAE and explicitness scores.  RUNS ONLY IN THE BUILD CONTAINER (needs the
reference, numpy and sklearn; no GPU).

Imports the unmodified reference's ``evaluation.utils`` with the stand-ins of make_golden_disent.py and writes
``classify.npz``:

* ``x_train / v_train / x_test / v_test``: two draws of the make_golden_disent.py generator (N = 777, D = 10, factor
  sizes [6, 6, 2, 3, 3, 40, 40], W density 0.3 and shared by both sets, the last column constant 1.25: scale = 1).
  The label-dropout pair is the first 60 rows of each (the 40-class factors lose labels on either side).
* ``expl_full / expl_small``: the reference's ``compute_explicitness`` (train, test) on each pair with the parameters
  its writer uses (``saga``, ``max_iter=300``), on ``StandardScaler`` output as metrics.py:296-302 produces it.
* ``proba_full_test_k / proba_small_{train,test}_k``: sklearn's TIGHTLY converged ``predict_proba`` (``lbfgs``,
  ``tol=1e-12``) per factor on the valid rows, columns in ``classes_small_k / classes_full_k`` order, fitted on the fp64
  standardisation (population variance, scale 1 where it is 0).
* ``fc_*``: a synthetic factor-change set (157 x 10, 5 classes, train and test), the reference's
  ``compute_factor_change_accuracy`` for ``scale`` False / True and the tight test probabilities of both.
* ``tie_*``: ``roc_auc_score`` per class on a small score matrix full of ties, saturated 0.0 and 1.0 included.

The script asserts that at the tight optimum every factor-change test row has a top-two probability gap >= 1e-4 (the
predictions are unambiguous) and that the reference's loose-solver accuracy equals the tight one; it moves on to the
next seed otherwise.  The file holds data only.

    python tests/golden/make_golden_classify.py
"""
import os
import sys
import types
import warnings
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

xgb = types.ModuleType("xgboost")       # empty stand-in: evaluation/utils.py:7 does `from xgboost import XGBClassifier`
xgb.XGBClassifier = None
sys.modules["xgboost"] = xgb
black = types.ModuleType("black")       # models.py:2 `from black import out`
black.out = None
sys.modules["black"] = black
for name in ("torchvision", "torchvision.utils", "torchvision.transforms", "torchvision.transforms.functional",
             "torchvision.io", "torchvision.datasets", "torch.utils.tensorboard", "umap", "pandas", "PIL"):
    try:
        __import__(name)
    except Exception:  # noqa: BLE001
        sys.modules[name] = MagicMock()
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
from sklearn.linear_model import LogisticRegression  # noqa: E402
from sklearn.metrics import accuracy_score, roc_auc_score  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402
from evaluation import utils as U  # noqa: E402  (the reference's)

N, D = 777, 10
SIZES = np.array([6, 6, 2, 3, 3, 40, 40])
LOOSE = {"explicitness_lr_params": {"solver": "saga", "max_iter": 300}}
TIGHT = dict(solver="lbfgs", tol=1e-12, max_iter=200000)


def standardise(x_train, x):
    m = x_train.astype(np.float64).mean(0)
    s = np.sqrt(x_train.astype(np.float64).var(0))
    s[s == 0] = 1.0
    return (x.astype(np.float64) - m) / s


def make_pair(seed):
    rs = np.random.RandomState(seed)
    W = rs.randn(len(SIZES), D) * (rs.rand(len(SIZES), D) < 0.3)
    out = []
    for _ in range(2):
        v = np.stack([rs.randint(s, size=N) for s in SIZES], 1).astype(np.int32)
        x = ((v / SIZES) @ W + 0.3 * rs.randn(N, D)).astype(np.float32)
        x[:, -1] = np.float32(1.25)
        out += [x, v]
    return out


def tight_probas(xtr, vtr, xte, vte):
    """Per factor: (classes, proba on the valid train rows, proba on the valid test rows) at the tight optimum."""
    a, b = standardise(xtr, xtr), standardise(xtr, xte)
    res = []
    for k in range(vtr.shape[1]):
        itr, ite = U.get_valid_indices(vtr[:, k], vte[:, k])
        clf = LogisticRegression(**TIGHT).fit(a[itr], vtr[itr, k])
        res.append((clf.classes_.astype(np.int32), clf.predict_proba(a[itr]), clf.predict_proba(b[ite])))
    return res


def reference_explicitness(xtr, vtr, xte, vte):
    scl = StandardScaler()                                  # metrics.py:296-298, on the fp32 arrays as the reference has them
    a, b = scl.fit_transform(xtr), scl.transform(xte)
    return np.array(U.compute_explicitness(a, vtr.astype(np.float64), b, vte.astype(np.float64), params=LOOSE))


def make_factor_change(seed):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(2):
        y = rs.randint(5, size=157)
        x = np.abs(0.6 + 0.25 * rs.randn(157, 10))
        x[np.arange(157), 2 * y] *= 0.55                    # the fixed factor's latent moves less
        out += [x.astype(np.float32), y.astype(np.int8)]
    return out


def main():
    warnings.simplefilter("ignore")
    xtr, vtr, xte, vte = make_pair(2024)
    out = dict(x_train=xtr, v_train=vtr, x_test=xte, v_test=vte, sizes=SIZES.astype(np.int32))
    for tag, n in (("full", N), ("small", 60)):
        a, b, c, d = xtr[:n], vtr[:n], xte[:n], vte[:n]
        out[f"expl_{tag}"] = reference_explicitness(a, b, c, d)
        for k, (cls, ptr, pte) in enumerate(tight_probas(a, b, c, d)):
            out[f"classes_{tag}_{k}"] = cls
            out[f"proba_{tag}_test_{k}"] = pte
            if tag == "small":
                out[f"proba_{tag}_train_{k}"] = ptr
        print(tag, "reference explicitness (train, test):", out[f"expl_{tag}"])
    for seed in range(7, 40):
        ftr, ytr, fte, yte = make_factor_change(seed)
        good, rec = True, {}
        for scale in (False, True):
            ref = U.compute_factor_change_accuracy(ftr, ytr, fte, yte, params=dict(scale=scale))
            a, b = (standardise(ftr, ftr), standardise(ftr, fte)) if scale else (ftr.astype(np.float64), fte.astype(np.float64))
            clf = LogisticRegression(**TIGHT).fit(a, ytr)
            p = clf.predict_proba(b)
            top = np.sort(p, 1)
            gap = float((top[:, -1] - top[:, -2]).min())
            acc = accuracy_score(yte, clf.predict(b))
            print("seed", seed, "scale", scale, "reference accuracy", ref, "tight", acc, "smallest top-two gap", gap)
            good &= gap >= 1e-4 and ref == acc
            rec[f"fc_acc_{int(scale)}"], rec[f"fc_proba_{int(scale)}"] = np.float64(ref), p
        if good:
            break
    else:
        raise SystemExit("no seed gives unambiguous predictions")
    out.update(rec, fc_seed=np.int64(seed), fc_x_train=ftr, fc_y_train=ytr, fc_x_test=fte, fc_y_test=yte)
    rs = np.random.RandomState(5)
    ty = rs.randint(4, size=48)
    ts = rs.choice([0.0, 0.125, 0.25, 0.5, 0.75, 1.0], size=(48, 4))
    onehot = (ty[:, None] == np.arange(4)[None, :]).astype(int)
    out.update(tie_y=ty.astype(np.int32), tie_scores=ts, tie_auc=np.asarray(roc_auc_score(onehot, ts, average=None)))
    path = os.path.join(HERE, "classify.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
