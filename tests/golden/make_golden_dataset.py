#!/usr/bin/env python3
"""Golden fixture of the reference's factor datasets.  RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference).

Imports the *unmodified* reference ``dataset.py`` and builds its ``DSprites`` and ``MPI3D`` classes
(dataset.py:40-90,131-162) over 40 random uint8 images each, 8 x 8 and 8 x 8 x 3, with ``resize=8`` (the stored size:
``__getitem__`` then goes through ``Image.fromarray`` -- PIL is installed -- a same-size ``Image.resize``, which PIL
answers with a copy, and ``ToTensor``).  Recorded per class: ``imgs`` as the class stored them (its ``* 255`` included,
which wraps modulo 256 on uint8), every ``__getitem__`` image, and the labels.

torchvision is not installed here, so it is stubbed in-process the way make_golden.py stubs modules.  The ``ToTensor``
stub is the torchvision definition (torchvision/transforms/functional.py ``to_tensor`` for a PIL image of mode L / RGB):
the pixels as an ``H x W x C`` uint8 array -> ``permute(2, 0, 1).contiguous()`` -> ``.to(torch.float32).div(255)``.
Nothing from the reference is copied: the fixture holds arrays only.

    python tests/golden/make_golden_dataset.py            # rewrites tests/golden/dataset.npz
"""
import os
import sys
import types
from unittest.mock import MagicMock

sys.dont_write_bytecode = True
REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402


class ToTensor:
    def __call__(self, pic):
        a = np.array(pic, np.uint8, copy=True)
        img = torch.from_numpy(a).view(pic.size[1], pic.size[0], len(pic.getbands()))
        return img.permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


def _install_stubs():
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Compose, tr.RandomHorizontalFlip = ToTensor, Compose, MagicMock()
    tv.transforms = tr
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    for name in ("torchvision.io", "torchvision.transforms.functional"):
        sys.modules[name] = MagicMock()
    try:
        import pandas  # noqa: F401
    except ImportError:
        sys.modules["pandas"] = MagicMock()


_install_stubs()
sys.path.insert(0, REF)

import dataset as ref_dataset  # noqa: E402


def record(prefix, ds, n, out):
    items = [ds[i] for i in range(n)]
    out[prefix + "_imgs"] = np.asarray(ds.imgs)
    out[prefix + "_items"] = np.stack([x.numpy() for x, _ in items])
    out[prefix + "_labels"] = np.stack([np.asarray(y) for _, y in items])
    out[prefix + "_latents_values"] = np.asarray(ds.latents_values)
    assert out[prefix + "_imgs"].dtype == np.uint8 and out[prefix + "_items"].dtype == np.float32


def main():
    rng = np.random.RandomState(20240607)
    n, out = 40, {}
    raw = rng.randint(0, 256, size=(n, 8, 8)).astype(np.uint8)
    lat = np.stack([rng.randint(0, s, size=n) for s in (1, 3, 6, 40, 32, 32)], 1).astype(np.float64)
    out["dsprites_raw"] = raw
    record("dsprites", ref_dataset.DSprites({"imgs": raw, "latents_values": lat}, resize=8), n, out)
    raw3 = rng.randint(0, 256, size=(n, 8, 8, 3)).astype(np.uint8)
    out["mpi3d_raw"] = raw3
    record("mpi3d", ref_dataset.MPI3D({"images": raw3}, resize=8), n, out)
    path = os.path.join(HERE, "dataset.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
