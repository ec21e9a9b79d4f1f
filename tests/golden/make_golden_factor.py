#!/usr/bin/env python3
"""Golden vectors for the FactorVAE objective (csrc/factor.hip, the fused discriminator layers).  Needs numpy only; no GPU.

Writes ``factor.npz``.  Stored, all values fp64 from ``factor_ref`` (tests/factor_ref.py):

* per head case ``head:<R0>:`` -- logits ``factor_ref.make_logits(R0, seed)`` [2 R0, 2]: ``seed``, ``checksum`` (the fp64
  sum of the fp32 logits), ``tc``, ``d_loss``, ``d_acc``;
* per op case ``op:<B>x<zdim>x<hidden>:`` -- ``factor_ref.make_inputs(B, zdim, seed)`` and the two-hidden-layer MLP
  ``factor_ref.make_mlp(zdim, hidden, 2, seed + 1)``, slope 0.2: ``seed``, ``checksum`` (sums of z, keys and of every
  weight and bias), ``tc``, ``d_loss``, ``d_acc``, ``gz`` = max |d tc / d z| and, for the shapes of ``FULL``, ``dz`` and
  the first layer's ``dW0``.

Every stored head case satisfies |tc| >= 1e-2 mean |l0 - l1| and 0 < d_acc < 1: conditions on the inputs (asserted here
and where the file is read) that keep relative bounds on tc and d_acc meaningful.  The file holds data only.

    python tests/golden/make_golden_factor.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import factor_ref as R  # noqa: E402

HEAD_R0 = [1, 2, 63, 64, 65, 4096]
OPS = [(8, 10, 64), (64, 128, 64), (65, 33, 64), (8, 10, 1000), (64, 128, 1000), (65, 33, 1000)]
FULL = [(8, 10, 64)]
SLOPE = 0.2


def main():
    out = {"head_r0": np.array(HEAD_R0), "ops": np.array(OPS), "slope": np.array(SLOPE)}
    for n, R0 in enumerate(HEAD_R0):
        seed = 3000 + n
        l = R.make_logits(R0, seed)
        h = R.head(l, R0)
        d = np.abs(l[:, 0].astype(np.float64) - l[:, 1]).mean()
        print(f"head:{R0}: tc / mean|d| = {abs(h['tc']) / d:.3f}  d_acc = {h['d_acc']:.3f}")
        assert abs(h["tc"]) >= 1e-2 * d and 0.0 < h["d_acc"] < 1.0, (R0, h["tc"], d, h["d_acc"])
        p = f"head:{R0}:"
        out[p + "seed"], out[p + "checksum"] = np.array(seed), np.array(l.astype(np.float64).sum())
        for k in ("tc", "d_loss", "d_acc"):
            out[p + k] = np.array(h[k])
    for n, (B, zdim, hidden) in enumerate(OPS):
        seed = 3100 + 2 * n
        z, keys = R.make_inputs(B, zdim, seed)
        Ws, bs = R.make_mlp(zdim, hidden, 2, seed + 1)
        ref = R.factor(z, R.permute_dims(z, keys), Ws, bs, SLOPE)
        p = f"op:{B}x{zdim}x{hidden}:"
        print(p, f"tc {ref['tc']:.4f} d_loss {ref['d_loss']:.4f} d_acc {ref['d_acc']:.3f} max|dz| {np.abs(ref['dz']).max():.2e}")
        out[p + "seed"] = np.array(seed)
        out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in (z, keys, *Ws, *bs)])
        for k in ("tc", "d_loss", "d_acc"):
            out[p + k] = np.array(ref[k])
        out[p + "gz"] = np.array(np.abs(ref["dz"]).max())
        if (B, zdim, hidden) in FULL:
            out[p + "dz"], out[p + "dW0"] = ref["dz"], ref["dW"][0]
    np.savez_compressed(os.path.join(HERE, "factor.npz"), **out)


if __name__ == "__main__":
    main()
