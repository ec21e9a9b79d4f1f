#!/usr/bin/env python3
"""Golden vectors for the label regulariser of the semi-supervised S2 objectives (csrc/sup.hip).  Needs numpy only; no GPU.

Writes ``sup.npz``.  For every shape (B_l, D, F) of ``SHAPES`` the inputs come from ``sup_ref.make_inputs(B_l, D, F, seed)``:
``mu ~ N(0, 1.5^2)`` plus a column offset, ``y`` integers uniform in ``[0, K_f)`` as fp32, the sizes
``sup_ref.default_sizes(F)``, a seeded ``default_rng``; the shapes of ``BIG`` use ``sup_ref.make_big_inputs`` (|mu| up to
80).  Stored per case ``<B>x<D>x<F>:<kind>:`` (``big:`` in front for the BIG ones)

* ``seed``, and ``checksum`` = the fp64 sums of the fp32 inputs (mu, y): a test that regenerates the inputs from the seed
  checks that it got the same numbers;
* ``sup`` and ``loss`` = gamma * sup in fp64 for ``gamma = 0.75``, ``scale = 1.25``, and ``gmax`` = max |dmu|;
* for the cases of at most ``FULL`` elements also the fp32 inputs ``mu`` / ``y`` and the fp64 ``dmu``.

The file holds data only.

    python tests/golden/make_golden_sup.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import sup_ref as R  # noqa: E402

SHAPES = [(1, 1, 1), (2, 3, 3), (5, 10, 7), (64, 128, 5), (33, 65, 64),
          (3, 63, 5), (4, 64, 64), (5, 65, 33), (65, 512, 64), (65, 64, 31), (4, 33, 32), (5, 32, 32), (3, 31, 31),
          (17, 33, 33), (16, 65, 1), (15, 63, 32), (64, 32, 31), (63, 512, 5)]
BIG = [(5, 10, 7), (65, 64, 64)]
GAMMA, SCALE = 0.75, 1.25
FULL = 1000


def main():
    out = {"shapes": np.array(SHAPES), "big": np.array(BIG), "hp": np.array([GAMMA, SCALE])}
    cases = [("", s, R.make_inputs) for s in SHAPES] + [("big:", s, R.make_big_inputs) for s in BIG]
    for n, (tag, (B, D, F), make) in enumerate(cases):
        seed = 3000 + n
        mu, y, sizes = make(B, D, F, seed)
        for kind in R.KINDS:
            p = f"{tag}{B}x{D}x{F}:{kind}:"
            ref = R.sup(mu, y, kind, sizes, GAMMA, SCALE)
            out[p + "seed"] = np.array(seed)
            out[p + "checksum"] = np.array([mu.astype(np.float64).sum(), y.astype(np.float64).sum()])
            out[p + "sup"], out[p + "loss"] = np.array(ref["sup"]), np.array(ref["loss"])
            out[p + "gmax"] = np.array(np.abs(ref["dmu"]).max())
            if B * D <= FULL:
                out[p + "mu"], out[p + "y"], out[p + "dmu"] = mu, y, ref["dmu"]
    np.savez_compressed(os.path.join(HERE, "sup.npz"), **out)


if __name__ == "__main__":
    main()
