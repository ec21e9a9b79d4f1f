#!/usr/bin/env python3
"""Golden vectors for the MMD KL hook (csrc/mmd.hip).  Needs numpy only; no GPU.

Writes ``mmd.npz``.  For every shape (Bt, P, D) of ``SHAPES`` and both kernels the inputs come from
``mmd_ref.make_inputs(Bt, P, D, seed)``: z columns alternate std 0.6 / 1.3 plus a column offset ~ N(0, 0.5^2),
``logvar ~ N(-1.5, 0.5^2)``, ``prior ~ N(0, 1)``, a seeded ``default_rng``.  Stored per case ``<Bt>x<P>x<D>:<kernel>:``

* ``seed``, and ``checksum`` = the fp64 sums of the fp32 inputs (z, prior, mu, logvar): a test that regenerates the
  inputs from the seed checks that it got the same numbers;
* ``loss`` and ``terms`` (mean KL, MMD^2, S_zz, S_pp, S_zp) in fp64 for ``lambda_mmd = 3``, ``beta = 0.5``, ``h = 2 D``
  with every row local, and ``gmax`` = max |dz|;
* for the shapes of ``FULL`` also the fp64 ``dz`` and ``Wt``.

Every stored case satisfies |MMD^2| >= 1e-2 max(S_zz, S_pp, S_zp): a condition on the inputs (asserted here and where
the file is read) that keeps a relative bound on MMD^2 meaningful.  The file holds data only.

    python tests/golden/make_golden_mmd.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import mmd_ref as R  # noqa: E402

# the issue's shapes, then the edges of the kernels' tiles (tests/test_hip_mmd.py names them)
SHAPES = [(2, 2, 1), (2, 3, 3), (3, 2, 64), (35, 20, 10), (64, 64, 128), (33, 65, 130), (65, 64, 65), (512, 512, 128),
          (16, 16, 300), (7, 9, 512),
          (31, 33, 63), (32, 32, 64), (33, 31, 65), (15, 17, 64), (17, 15, 65), (16, 15, 9), (16, 17, 9), (1024, 3, 2),
          (1025, 2, 3)]
FULL = [(2, 3, 3), (35, 20, 10)]
LAMBDA, BETA = 3.0, 0.5


def main():
    out = {"shapes": np.array(SHAPES), "hp": np.array([LAMBDA, BETA])}
    for n, (Bt, P, D) in enumerate(SHAPES):
        seed = 2000 + n
        z, prior, mu, lv = R.make_inputs(Bt, P, D, seed)
        for kernel in R.KERNELS:
            p = f"{Bt}x{P}x{D}:{kernel}:"
            ref = R.mmd(z, prior, mu, lv, kernel, 2.0 * D, LAMBDA, BETA)
            t = ref["terms"]
            print(p, "mmd2 / max S = %.3f" % (abs(t[1]) / t[2:].max()), "gmax %.2e" % np.abs(ref["dz"]).max())
            assert abs(t[1]) >= 1e-2 * t[2:].max(), (p, t)
            out[p + "seed"] = np.array(seed)
            out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in (z, prior, mu, lv)])
            out[p + "loss"] = np.array(ref["loss"])
            out[p + "terms"] = t
            out[p + "gmax"] = np.array(np.abs(ref["dz"]).max())
            if (Bt, P, D) in FULL:
                out[p + "dz"], out[p + "Wt"] = ref["dz"], ref["Wt"]
    np.savez_compressed(os.path.join(HERE, "mmd.npz"), **out)


if __name__ == "__main__":
    main()
