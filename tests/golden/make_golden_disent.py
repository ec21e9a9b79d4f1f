#!/usr/bin/env python3
"""Golden vectors for the device-side disentanglement scores.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference,
numpy and sklearn; no GPU).

Imports the unmodified reference's ``evaluation.utils`` -- with an empty stand-in for ``xgboost``, which that module
imports at the top and which is absent here (the stand-in only carries the one name the import statement asks for) --
and writes ``disent.npz``: the inputs and the reference's own ``discretize`` (bins 10 and 20), ``calculate_mutual_info``,
``calculate_entropy`` and ``compute_modularity`` results (of all latents: nan, the constant column divides 0 by 0; and
of the nine informative ones), and the MIG expression of evaluation/metrics.py:213-219.

Inputs: N = 777 samples, D = 10 latents, factor sizes [6, 6, 2, 3, 3, 40, 40]; factors uniform; latents
``fp32((v / sizes) @ W + 0.3 * noise)`` with W sparse Gaussian (10 % density); the last latent column constant 1.25.

The script asserts that the fixed fp64 binning rule of include/itcv_hip.h reproduces the reference's ``discretize`` on
these inputs with ZERO differing entries, and moves on to the next seed if it does not.  The file holds data only.

    python tests/golden/make_golden_disent.py
"""
import os
import sys
import types
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
from evaluation import utils as U  # noqa: E402  (the reference's)

N, D = 777, 10
SIZES = np.array([6, 6, 2, 3, 3, 40, 40])
BINS = (10, 20)


def rule_bins(x, bins):
    """The fixed rule, restated in numpy fp64."""
    out = np.zeros(x.shape, dtype=np.int32)
    for d in range(x.shape[1]):
        col = x[:, d].astype(np.float64)
        lo, hi = col.min(), col.max()
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        w = (hi - lo) / bins
        for j in range(bins):
            out[:, d] += col >= lo + j * w
    return out


def make_inputs(seed):
    rs = np.random.RandomState(seed)
    v = np.stack([rs.randint(s, size=N) for s in SIZES], 1).astype(np.int32)
    W = rs.randn(len(SIZES), D) * (rs.rand(len(SIZES), D) < 0.1)
    x = ((v / SIZES) @ W + 0.3 * rs.randn(N, D)).astype(np.float32)
    x[:, -1] = np.float32(1.25)
    return x, v


def main():
    for seed in range(2024, 2034):
        x, v = make_inputs(seed)
        ref = {b: U.discretize(x, bins=b) for b in BINS}
        diff = {b: int((rule_bins(x, b) != ref[b]).sum()) for b in BINS}
        print("seed", seed, "entries differing from the reference's discretize:", diff)
        if not any(diff.values()):
            break
    else:
        raise SystemExit("no seed reproduces the reference's discretize exactly")
    out = dict(seed=np.int64(seed), x=x, v=v, sizes=SIZES.astype(np.int32))
    vf = v.astype(np.float64)                    # the reference hands float factor arrays to sklearn
    out["H"] = U.calculate_entropy(vf)
    for b in BINS:
        assert ref[b].min() == 1 and ref[b].max() == b
        out[f"bins{b}"] = ref[b].astype(np.int32)
        out[f"MI{b}"] = U.calculate_mutual_info(ref[b], vf)
    I_sorted = np.sort(out["MI10"], axis=0)[::-1]                      # evaluation/metrics.py:217-219
    out["mig"] = np.float64(np.mean((I_sorted[0] - I_sorted[1]) / out["H"]))
    # metrics.py:293-304.  The constant column has MI = 0 with every factor (theta = 0): the reference's 0 / 0 makes the
    # score of all ten latents nan; the score of the nine informative ones is recorded next to it.
    with np.errstate(invalid="ignore"):
        out["modularity"] = np.float64(U.compute_modularity(out["MI20"]))
    assert np.isnan(out["modularity"])
    out["modularity_informative"] = np.float64(U.compute_modularity(out["MI20"][:-1]))
    path = os.path.join(HERE, "disent.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), "mig", out["mig"], "modularity", out["modularity"],
          out["modularity_informative"])


if __name__ == "__main__":
    main()
