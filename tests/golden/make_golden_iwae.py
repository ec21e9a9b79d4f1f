#!/usr/bin/env python3
"""Golden vectors for the importance-weighted bound (csrc/iwae.hip).  Needs numpy only; no GPU.

Writes ``iwae.npz``.  For every case (B, K, D) of ``SHAPES`` the latent inputs come from ``iwae_ref.make_inputs(B, K, D,
seed)`` and the per-row reconstruction terms are drawn as ``rows = fp32(default_rng(seed + 1).uniform(20, 60, K B))``: the
kernels and the restatement are fed the same fp32 rows.  Stored per case ``<B>x<K>x<D>:``

* ``seed``, and ``checksum`` = the fp64 sums of the fp32 inputs (mu, logvar, eps, rows): a test that regenerates the inputs
  from the seed checks that it got the same numbers;
* the restatement's ``loss``, ``rec``, ``kl``, ``bound``, ``ess`` in fp64 for ``hp`` = (beta_rec, beta_kl) and, for cases
  of at most ``FULL`` elements, the fp32 inputs and the fp64 ``lat`` and weights ``w``.

The file holds data only.

    python tests/golden/make_golden_iwae.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import iwae_ref as R  # noqa: E402

# every edge of B (the four-rows-a-block edge), K (the 64 lanes of a wave; the limit) and D (lanes; the limit) at least once
SHAPES = [(1, 1, 1), (3, 2, 31), (4, 3, 32), (5, 63, 33), (65, 64, 64), (3, 65, 65), (4, 1024, 10), (1, 3, 512), (5, 1, 10),
          (65, 2, 1)]
BETA_REC, BETA_KL = 0.75, 0.5
FULL = 2000


def make_rows(B, K, seed):
    return np.random.default_rng(seed + 1).uniform(20.0, 60.0, size=K * B).astype(np.float32)


def main():
    out = {"shapes": np.array(SHAPES), "hp": np.array([BETA_REC, BETA_KL])}
    for n, (B, K, D) in enumerate(SHAPES):
        seed = 4000 + 2 * n
        mu, logvar, eps = R.make_inputs(B, K, D, seed)
        rows = make_rows(B, K, seed)
        _, lat = R.sample(mu, logvar, eps)
        ref = R.combine(rows, lat, B, BETA_REC, BETA_KL)
        p = f"{B}x{K}x{D}:"
        out[p + "seed"] = np.array(seed)
        out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in (mu, logvar, eps, rows)])
        for k in ("loss", "rec", "kl", "bound", "ess"):
            out[p + k] = np.array(ref[k])
        if K * B * D <= FULL:
            out[p + "mu"], out[p + "logvar"], out[p + "eps"], out[p + "rows"] = mu, logvar, eps, rows
            out[p + "lat"], out[p + "w"] = lat, ref["w"]
    np.savez_compressed(os.path.join(HERE, "iwae.npz"), **out)


if __name__ == "__main__":
    main()
