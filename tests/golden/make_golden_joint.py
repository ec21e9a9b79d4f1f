#!/usr/bin/env python3
"""Golden vectors for the JointVAE / AnnealedVAE latent op (csrc/joint.hip).  Needs numpy only; no GPU.

Writes ``joint.npz``.  For every case (B, n_cont, disc) of ``CASES`` the inputs come from
``joint_ref.make_inputs(B, n_cont, disc, seed)``, which also chooses the four pairs of capacities (one per combination of
the signs of KL_z - C_z and KL_c - C_c).  Stored per case ``<B>x<n_cont>+<K_1>.<K_2>...:``

* ``seed`` and ``checksum`` = the fp64 sums of the fp32 inputs (mu, logvar, eps, u): a test that regenerates the inputs
  from the seed checks that it got the same numbers;
* per sign combination ``<s_z><s_c>:cap`` (the two capacities) and ``<s_z><s_c>:loss``: the restatement's loss in fp64 for
  the hyper-parameters ``hp`` = (beta, gamma_z, gamma_c, tau).

The file holds data only, and no tensors beyond these.

    python tests/golden/make_golden_joint.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import joint_ref as R  # noqa: E402

# one row, one column, purely discrete, the four-rows-per-block tail; zdim 63 / 64 / 65; a group across the 64-lane edge and
# the tail; the benchmark's width; one 511-wide group; 256 + 256; 256 groups of two; more than one grid trip
CASES = [(1, 1, ()), (1, 0, (2,)), (2, 3, (2,)), (7, 6, (3,)), (33, 10, (10,)), (4, 61, (2,)), (3, 62, (2,)), (5, 60, (5,)),
         (9, 60, (3, 7, 59)), (32, 118, (10,)), (2, 0, (511,)), (3, 256, (256,)), (2, 0, (2,) * 256), (1025, 10, (3, 4))]
BETA, GAMMA_Z, GAMMA_C, TAU = 0.75, 3.0, 2.0, 0.67


def tag(B, n_cont, disc):
    """``<B>x<n_cont>+<K_1>.<K_2>...:``, four or more equal sizes as ``<K>*<G>``."""
    sizes = ".".join(map(str, disc)) if len(set(disc)) != 1 or len(disc) < 4 else f"{disc[0]}*{len(disc)}"
    return f"{B}x{n_cont}+{sizes}:"


def seed_of(n):
    """The seed of case ``n``."""
    return 5000 + 50 * n


def sign_tag(sz, sc):
    return "+-"[sz < 0] + "+-"[sc < 0]


def main():
    out = {"hp": np.array([BETA, GAMMA_Z, GAMMA_C, TAU]), "cases": np.array([tag(*c) for c in CASES])}
    for n, (B, nc, disc) in enumerate(CASES):
        seed = seed_of(n)
        mu, lv, eps, u, caps = R.make_inputs(B, nc, disc, seed)
        p = tag(B, nc, disc)
        out[p + "seed"] = np.array(seed)
        out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in (mu, lv, eps, u)])
        for (sz, sc), cap in caps.items():
            out[p + sign_tag(sz, sc) + ":cap"] = np.array(cap)
            out[p + sign_tag(sz, sc) + ":loss"] = np.array(R.joint(mu, lv, eps, u, nc, disc, cap, GAMMA_Z, GAMMA_C, BETA,
                                                                   TAU)["loss"])
    np.savez_compressed(os.path.join(HERE, "joint.npz"), **out)


if __name__ == "__main__":
    main()
