"""Writes tests/golden/resize.npz: Pillow's own ``Image.resize((Wout, Hout), Image.BICUBIC)`` bytes for the cases of
tests/resize_ref.py (``SHAPES``), next to their inputs.  Run with Pillow installed:

    python tests/golden/make_golden_resize.py

Per case ``<name>_in`` is planar uint8 ``[2, C, Hin, Win]`` (a random image holding every byte value, a 0/255 image) and
``<name>_out`` planar uint8 ``[2, C, Hout, Wout]``; ``pillow_version`` records the Pillow that made them.  Mode ``L`` for
one channel, ``RGB`` for three.  The tests read this file and never import Pillow (except the live cross-check of
tests/test_resize_host.py, which is skipped without it)."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_ref as R  # noqa: E402


def pil_resize(planar, Hout, Wout):
    """One planar uint8 image ``[C, H, W]`` through Pillow."""
    img = Image.fromarray(planar[0], "L") if planar.shape[0] == 1 else Image.fromarray(
        np.ascontiguousarray(planar.transpose(1, 2, 0)), "RGB")
    out = np.asarray(img.resize((Wout, Hout), Image.BICUBIC))
    return out[None] if out.ndim == 2 else np.ascontiguousarray(out.transpose(2, 0, 1))


def main():
    rec = {"pillow_version": np.array(PIL.__version__)}
    for Hin, Win, Hout, Wout, chans in R.SHAPES:
        for C in chans:
            name = R.case_name(Hin, Win, Hout, Wout, C)
            x = R.case_images(Hin, Win, C)
            y = np.stack([pil_resize(im, Hout, Wout) for im in x])
            assert y.shape == (2, C, Hout, Wout) and y.dtype == np.uint8
            rec[name + "_in"], rec[name + "_out"] = x, y
            print(name, "saturated low/high:", int((y == 0).sum()), int((y == 255).sum()))
    path = os.path.join(HERE, "resize.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
