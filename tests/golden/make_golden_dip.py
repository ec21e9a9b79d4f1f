#!/usr/bin/env python3
"""Golden vectors for the DIP-VAE KL hook (csrc/dip.hip).  Needs numpy only; no GPU.

Writes ``dip.npz``.  For every shape (Bt, D) of ``SHAPES`` and both kinds the inputs come from ``dip_ref.make_inputs(Bt, D,
seed)``: columns alternate std 0.5 / 1.6 plus a column offset ~ N(0, 2^2) (so E[mu mu^T] - m m^T cancels in fp32),
``logvar ~ N(-1.5, 0.5^2)``, a seeded ``default_rng``.  Stored per case ``<Bt>x<D>:<kind>:``

* ``seed``, and ``checksum`` = the fp64 sums of the fp32 inputs (mu, logvar): a test that regenerates the inputs from the
  seed checks that it got the same numbers;
* ``loss`` and ``terms`` (mean KL, off-diagonal term, diagonal term) in fp64 for ``lambda_od = 3``, ``lambda_d = 7``,
  ``beta = 0.5`` with every row local, and ``gmax`` = max |dmu|, max |dlogvar|;
* for the cases of at most ``FULL`` elements also the fp32 inputs ``mu`` / ``logvar`` and the fp64 ``W``, ``dmu``,
  ``dlogvar``.

The file holds data only.

    python tests/golden/make_golden_dip.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import dip_ref as R  # noqa: E402

SHAPES = [(2, 1), (2, 3), (3, 64), (35, 10), (64, 128), (33, 130), (65, 65), (512, 128), (16, 300), (7, 512),
          (63, 31), (64, 32), (65, 33), (15, 63), (16, 64), (17, 65)]
LAMBDA_OD, LAMBDA_D, BETA = 3.0, 7.0, 0.5
FULL = 1000


def main():
    out = {"shapes": np.array(SHAPES), "hp": np.array([LAMBDA_OD, LAMBDA_D, BETA])}
    for n, (Bt, D) in enumerate(SHAPES):
        seed = 1000 + n
        mu, lv = R.make_inputs(Bt, D, seed)
        for kind in R.KINDS:
            p = f"{Bt}x{D}:{kind}:"
            ref = R.dip(mu, lv, kind, LAMBDA_OD, LAMBDA_D, BETA)
            out[p + "seed"] = np.array(seed)
            out[p + "checksum"] = np.array([mu.astype(np.float64).sum(), lv.astype(np.float64).sum()])
            out[p + "loss"] = np.array(ref["loss"])
            out[p + "terms"] = ref["terms"]
            out[p + "gmax"] = np.array([np.abs(ref["dmu"]).max(), np.abs(ref["dlogvar"]).max()])
            if Bt * D <= FULL:
                out[p + "mu"], out[p + "logvar"] = mu, lv
                out[p + "W"], out[p + "dmu"], out[p + "dlogvar"] = ref["W"], ref["dmu"], ref["dlogvar"]
    np.savez_compressed(os.path.join(HERE, "dip.npz"), **out)


if __name__ == "__main__":
    main()
