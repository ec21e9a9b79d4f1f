"""Writes tests/golden/vamp.npz: per case of vamp_ref.SHAPES the seed, the checksums of the five generated inputs and the
restatement's loss (beta = vamp_ref.BETA, "mean"), nothing else.  It asserts the two conditions the tests rely on:
|mean KL| >= 5e-2 max(|mean logq|, |mean logp|), and for K >= 2 every row's largest responsibility <= 0.9.

    python tests/golden/make_golden_vamp.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import vamp_ref as R  # noqa: E402


def main():
    out = {"beta": np.float64(R.BETA)}
    for B, K, D in R.SHAPES:
        seed = R.seed_of(B, K, D)
        ins = R.make_inputs(B, K, D, seed)
        ref = R.vamp(*ins, beta=R.BETA)
        ratio, rmax = R.conditions(ref)
        assert ratio >= 5e-2, (B, K, D, ratio)
        assert K < 2 or rmax <= 0.9, (B, K, D, rmax)
        p = f"{B}x{K}x{D}:"
        out[p + "seed"] = np.int64(seed)
        out[p + "checksum"] = np.array([a.astype(np.float64).sum() for a in ins])
        out[p + "loss"] = np.float64(ref["loss"])
        print(p, f"loss {ref['loss']:.6f} ratio {ratio:.3f} rmax {rmax:.3f}")
    np.savez(os.path.join(HERE, "vamp.npz"), **out)


if __name__ == "__main__":
    main()
