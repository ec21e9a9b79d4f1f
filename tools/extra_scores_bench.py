#!/usr/bin/env python3
"""Time the FactorVAE and SAP scores at their default sizes: D = 128, factor sizes 3 / 6 / 40 / 32 / 32;
FactorVAE 10000 variance rows, 10000 / 5000 groups of 64; SAP 10000 / 5000 rows.

    python tools/extra_scores_bench.py [--calls 5] [--encode-images 16384] [--cpu-reference]

HIP events, ``--calls`` calls after one warm-up call.  The SCORE stages run on synthetic representations (the scores do
not care where the numbers come from); the ENCODE stage is the c2 model's eval-mode ``encode`` of device-resident images
in forward calls of 1024 images, reported as images per second, from which the encode time of a default call follows
(FactorVAE: 970000 images, SAP: 15000).  ``--cpu-reference`` also times the same SAP matrix from a loop of sklearn
``LinearSVC`` fits in a pool of 16 processes over the same arrays, if sklearn is installed.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
SIZES = [3, 6, 40, 32, 32]


def representations(n, d, seed):
    rs = np.random.RandomState(seed)
    W = rs.randn(len(SIZES), d) * (rs.rand(len(SIZES), d) < 0.1)
    v = np.stack([rs.randint(s, size=n) for s in SIZES], 1).astype(np.int32)
    return ((v / np.array(SIZES)) @ W * 3 + 0.3 * rs.randn(n, d)).astype(np.float32), v


def timed(fn, calls):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return dict(ms_median=float(np.median(out)), ms_min=float(min(out)), ms_max=float(max(out)))


def _svc_column(args):
    from sklearn.svm import LinearSVC
    x, ytr, xte, yte = args
    row = []
    for j in range(ytr.shape[1]):
        clf = LinearSVC(C=0.01, class_weight="balanced", dual=False).fit(x[:, None], ytr[:, j])
        row.append(float((clf.predict(xte[:, None]) == yte[:, j]).mean()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--encode-images", type=int, default=16384)
    ap.add_argument("--cpu-reference", action="store_true")
    a = ap.parse_args()
    import torch
    import models
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    dev = torch.device("cuda:0")
    D, L = a.d, 64
    res = dict(D=D, sizes=SIZES, calls=a.calls)
    xtr, ytr = representations(10000, D, 0)
    xte, yte = representations(5000, D, 1)
    sap_args = [torch.as_tensor(t).to(dev) for t in (xtr, ytr, xte, yte)]
    res["sap_score"] = timed(lambda: DS.sap_score(*sap_args, SIZES), a.calls)
    flags = HF.extra_flags(dev)
    res["sap_svc_fit"] = timed(lambda: HF.sap_svc_fit(sap_args[0], sap_args[1], SIZES, flags), a.calls)
    theta, gnorm, iters, _ = HF.sap_svc_fit(sap_args[0], sap_args[1], SIZES, flags)
    res["sap_newton_steps_max"], res["sap_gnorm_max"] = int(iters.max()), float(gnorm.max())
    res["sap_value"] = DS.sap_score(*sap_args, SIZES)
    rs = np.random.RandomState(2)
    mu_var = torch.as_tensor(representations(10000, D, 3)[0]).to(dev)
    groups = {}
    for name, m in (("train", 10000), ("eval", 5000)):
        fidx = rs.randint(len(SIZES), size=m)
        mu = torch.randn((m, L, D), device=dev)
        mu[torch.arange(m), :, torch.as_tensor(fidx)] *= 0.05       # the fixed factor's dimension varies little
        groups[name] = (mu.reshape(m * L, D), fidx)
    fv = lambda: DS.factor_vae_score(mu_var, *groups["train"], *groups["eval"], L, len(SIZES))  # noqa: E731
    res["factor_vae_score"] = timed(fv, a.calls)
    res["factor_vae_value"] = fv()
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", cdim=3, zdim=D, channels=(64, 128, 256, 512), image_size=64).to(dev).eval()
    images = torch.rand((1024, 3, 64, 64), device=dev)

    def encode():
        with torch.no_grad():
            for _ in range(max(1, a.encode_images // 1024)):
                model.encode(images)

    t = timed(encode, a.calls)
    res["encode"] = dict(t, images=max(1, a.encode_images // 1024) * 1024)
    res["encode_images_per_s"] = res["encode"]["images"] / (t["ms_median"] * 1e-3)
    if a.cpu_reference:
        from multiprocessing import Pool
        t0 = time.perf_counter()
        with Pool(16) as pool:
            S = np.array(pool.map(_svc_column, [(xtr[:, i].astype(np.float64), ytr, xte[:, i].astype(np.float64), yte)
                                                for i in range(D)]))
        res["sklearn_sap_matrix_s"] = time.perf_counter() - t0
        top = np.sort(S, axis=0)
        res["sklearn_sap_value"] = float(np.mean(top[-1] - top[-2]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
