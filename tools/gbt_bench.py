#!/usr/bin/env python3
"""Time one default DCI fit (hipvae.gbt.fit_boosted_trees) on synthetic representations:
N = 10000, D = 128, factor sizes 3 / 6 / 40 / 32 / 32, 100 rounds, depth 6, max_bin 256.

    python tools/gbt_bench.py [--rounds 100] [--depth 6] [--n 10000] [--d 128] [--cpu-reference]

Prints one JSON line.  ``--cpu-reference`` also times sklearn's GradientBoostingClassifier (the default estimator of the
reference's fit_info_clf) on the same arrays, if sklearn is installed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))


def data(n, d, sizes, seed):
    rs = np.random.RandomState(seed)
    W = rs.randn(len(sizes), d) * (rs.rand(len(sizes), d) < 0.1)
    out = []
    for _ in range(2):
        v = np.stack([rs.randint(s, size=n) for s in sizes], 1).astype(np.int32)
        out += [((v / np.array(sizes)) @ W * 3 + 0.3 * rs.randn(n, d)).astype(np.float32), v]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--cpu-reference", action="store_true")
    a = ap.parse_args()
    sizes = [3, 6, 40, 32, 32]
    xtr, ytr, xte, yte = data(a.n, a.d, sizes, 0)
    res = dict(N=a.n, D=a.d, sizes=sizes, rounds=a.rounds, max_depth=a.depth)
    import torch
    from hipvae import gbt
    dev = torch.device("cuda:0")
    args = [torch.as_tensor(t).to(dev) for t in (xtr, ytr, xte, yte)]
    gbt.fit_boosted_trees(*args, sizes, rounds=2, max_depth=a.depth)          # warm-up: module load, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = gbt.fit_boosted_trees(*args, sizes, rounds=a.rounds, max_depth=a.depth)
    res["device_fit_s"] = time.perf_counter() - t0
    res["test_accuracy"] = fit.test_accuracy
    res["splits"] = int((fit.trees[0] >= 0).sum())
    if a.cpu_reference:
        from sklearn.ensemble import GradientBoostingClassifier
        t0 = time.perf_counter()
        acc = []
        for k in range(len(sizes)):
            clf = GradientBoostingClassifier().fit(xtr, ytr[:, k])
            acc.append(float((clf.predict(xte) == yte[:, k]).mean()))
        res["sklearn_fit_s"], res["sklearn_test_accuracy"] = time.perf_counter() - t0, acc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
