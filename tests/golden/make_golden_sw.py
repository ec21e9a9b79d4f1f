#!/usr/bin/env python3
"""Golden vectors for the sliced-Wasserstein KL hook (csrc/sw.hip).  Needs numpy only; no GPU.

Writes ``sw.npz``.  For every shape (Bt, D, L) of ``SHAPES`` the inputs come from ``sw_ref.make_inputs(Bt, D, L, seed)``:
z columns alternate std 0.6 / 1.3 plus a column offset ~ N(0, 0.5^2), ``logvar ~ N(-1.5, 0.5^2)``, ``prior`` and the
directions ``t ~ N(0, 1)``, a seeded ``default_rng``.  Stored per case ``<Bt>x<D>x<L>:``

* ``seed``, and ``checksum`` = the fp64 sums of the fp32 inputs (z, prior, t, mu, logvar): a test that regenerates the
  inputs from the seed checks that it got the same numbers;
* ``loss`` and ``terms`` (mean KL, SW^2, max_l SW_l^2) in fp64 for ``lambda_sw = 3``, ``beta = 0.5`` with every row
  local, ``gap`` = ``sw_ref.min_gap`` and ``gmax`` = max |dz|;
* for the shapes of ``FULL`` also the fp64 ``dz``, ``G`` and ``per``.

Sorting is discontinuous, so every stored case satisfies a condition on the inputs (asserted here and where the file is
read): the smallest gap between adjacent sorted projections, of u and of v, is at least 1e-11 max |u|.  An fp64 evaluation
(projection error ~1e-13 relative) then sorts as the restatement does, and G is comparable element by element.  The seed
of a case is the first one from its base that satisfies it.  The file holds data only.

    python tests/golden/make_golden_sw.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import sw_ref as R  # noqa: E402

# (Bt, D, L): the smallest; the sort network off powers of two; the staging edges of both kernels (the projection's 64
# lanes over D, the backward's 16 rows x 64 columns over chunks of 32 directions); L below, at and above the chunk and
# above the grid cap of 256; the training shapes; Bt at and above the rows whose keys sit in LDS (tests/test_hip_sw.py)
SHAPES = [(1, 1, 1), (2, 1, 1), (2, 3, 2), (3, 64, 5),
          (31, 5, 3), (32, 5, 3), (33, 5, 3), (63, 4, 3), (64, 4, 3), (65, 4, 3), (1023, 3, 3), (1024, 3, 3), (1025, 3, 3),
          (15, 63, 4), (16, 64, 4), (17, 65, 4), (9, 130, 4), (5, 512, 2), (3, 2048, 2),
          (20, 7, 1), (20, 7, 2), (12, 6, 257), (65, 130, 33),
          (64, 128, 50), (512, 128, 50),
          (4096, 8, 3), (4097, 8, 3)]
FULL = [(2, 3, 2), (33, 5, 3)]
LAMBDA, BETA = 3.0, 0.5
GAP = 1e-11


def main():
    out = {"shapes": np.array(SHAPES), "hp": np.array([LAMBDA, BETA]), "gap": np.array(GAP)}
    for n, (Bt, D, L) in enumerate(SHAPES):
        seed = 3000 + 10 * n
        while R.min_gap(*R.make_inputs(Bt, D, L, seed)[:3]) < GAP:
            seed += 1
        assert seed < 3000 + 10 * n + 10
        z, prior, t, mu, lv = R.make_inputs(Bt, D, L, seed)
        p = f"{Bt}x{D}x{L}:"
        ref = R.sw(z, prior, t, mu, lv, LAMBDA, BETA)
        gap = R.min_gap(z, prior, t)
        print(p, "seed %d gap %.2e sw2 %.4f gmax %.2e" % (seed, gap, ref["terms"][1], np.abs(ref["dz"]).max()))
        out[p + "seed"] = np.array(seed)
        out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in (z, prior, t, mu, lv)])
        out[p + "loss"] = np.array(ref["loss"])
        out[p + "terms"] = ref["terms"]
        out[p + "gap"] = np.array(gap)
        out[p + "gmax"] = np.array(np.abs(ref["dz"]).max())
        if (Bt, D, L) in FULL:
            out[p + "dz"], out[p + "G"], out[p + "per"] = ref["dz"], ref["G"], ref["per"]
    np.savez_compressed(os.path.join(HERE, "sw.npz"), **out)


if __name__ == "__main__":
    main()
