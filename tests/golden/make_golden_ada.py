#!/usr/bin/env python3
"""Golden vectors for the Ada-GVAE / Ada-ML-VAE latent op (csrc/ada.hip).  Needs numpy only; no GPU.

Writes ``ada.npz``.  For every shape (pairs, D) of ``SHAPES`` the inputs come from ``ada_ref.make_inputs(B, D, seed)``
(which moves to the next seed until the margin condition on the threshold holds), the external mask from
``ada_ref.make_mask`` and the incoming gradient from ``ada_ref.make_dz``.  Stored per shape ``<B>x<D>:``

* ``seed`` (the one ``make_inputs`` used) and ``checksum`` = the fp64 sums of the fp32 inputs (mu, logvar, eps): a test
  that regenerates the inputs from the seed checks that it got the same numbers;
* per averaging and mask mode ``<B>x<D>:<averaging>:<mask>:loss``: the restatement's loss in fp64 for ``beta = BETA``.

The file holds data only, and no tensors beyond these.

    python tests/golden/make_golden_ada.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import ada_ref as R  # noqa: E402

# the wave's 64-column edges at -1 / 0 / +1, the four-pairs-per-block tail, the register maximum, more than one grid trip
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 64), (4, 63), (5, 65), (33, 10), (7, 128), (32, 128), (9, 129), (2, 511), (3, 512),
          (1025, 10)]
BETA = 0.75


def main():
    out = {"shapes": np.array(SHAPES), "hp": np.array([BETA])}
    for n, (B, D) in enumerate(SHAPES):
        mu, lv, eps, seed = R.make_inputs(B, D, 3000 + 50 * n)
        p = f"{B}x{D}:"
        out[p + "seed"] = np.array(seed)
        out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in (mu, lv, eps)])
        for averaging in R.AVERAGINGS:
            for mask in R.MASKS:
                own = R.make_mask(B, D, seed) if mask == "external" else None
                out[p + f"{averaging}:{mask}:loss"] = np.array(R.ada(mu, lv, eps, BETA, averaging, own)["loss"])
    np.savez_compressed(os.path.join(HERE, "ada.npz"), **out)


if __name__ == "__main__":
    main()
