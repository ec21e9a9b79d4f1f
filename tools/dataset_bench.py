#!/usr/bin/env python3
"""Time the device-resident image table (hipvae/dataset.py, csrc/dataset.hip).

    python tools/dataset_bench.py [--repeats 5] [--calls 200] [--skip-end-to-end] [--bvae-samples 10000]

GATHER: ``itcv_gather_u8`` at output shapes 1024 x 1 x 64 x 64, 1024 x 3 x 64 x 64 and 64 x 3 x 256 x 256 with random
indices into a dSprites-sized table (737 280 x 64 x 64 bytes = 3.0 GB, viewed at each image shape), next to ``itcv_hflip``
on the same output shape.  A window is ``--calls`` back-to-back launches between two HIP events; the two kernels
alternate for ``--repeats`` windows each after a warm-up window, and the median window is reported per call.  Every call
of a window uses another index vector (64 of them) and both kernels cycle through 16 output buffers -- and ``itcv_hflip``
through 16 inputs, 268 MB at the smallest shape -- so that neither reads its input from a cache the real use would not
find warm.  Rates count the bytes the algorithm needs: 5 per element for the gather (1 read, 4 written), 8 for the flip.

END TO END: default ``compute_factor_vae_score`` (970 000 images) and ``compute_bvae_score`` (2 x 10 000 x 64 x 2 =
2 560 000 images; ``--bvae-samples`` scales it) on a synthetic dSprites-shaped dataset -- factor sizes 1 / 3 / 6 / 40 /
32 / 32, 737 280 random 64 x 64 uint8 images, ``__getitem__`` restating the reference's ``Image.fromarray`` + ``/ 255``
(dataset.py:141-147) -- with ``FactorSampler`` against ``DeviceFactorSampler``, same seed, host wall clock around a call
that ends in a read-back.  The encoder is the c2 model of tools/extra_scores_bench.py, which takes three channels: the
one-channel images are repeated three times on the device in front of it, for both samplers alike.  ``encode_s`` is the
encoder's share: the same number of images from a resident batch of the score's forward size, timed alone.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
TABLE_IMAGES, SIDE = 737280, 64
SHAPES = [(1024, 1, 64, 64), (1024, 3, 64, 64), (64, 3, 256, 256)]
FACTOR_SIZES, LATENT_INDICES = [1, 3, 6, 40, 32, 32], [1, 2, 3, 4, 5]


def window(fn, calls):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(calls):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # microseconds per call


def gather_bench(raw, repeats, calls):
    import torch
    from hipvae import abi
    from hipvae.dataset import DeviceImageTable
    dev, out = raw.device, []
    for n, C, H, W in SHAPES:
        num = raw.numel() // (C * H * W)
        table = DeviceImageTable.from_device_tensor(raw.view(num, C, H, W))
        g = torch.Generator(device=dev).manual_seed(n + C)
        idx = torch.randint(0, num, (64, n), generator=g, device=dev)
        coins = (torch.rand((64, n), generator=g, device=dev) < 0.5).to(torch.uint8)
        outs = torch.empty((16, n, C, H, W), device=dev)
        ins = torch.rand((16, n, C, H, W), device=dev)
        st = abi.stream()

        # raw pointers, worked out once: a window measures the kernels, not the Python in front of them
        fn_g, fn_h = abi.lib.itcv_gather_u8, abi.lib.itcv_hflip
        tp, fl = table.images.data_ptr(), torch.zeros(1, dtype=torch.int32, device=dev)
        ip, cp = [idx[k].data_ptr() for k in range(64)], [coins[k].data_ptr() for k in range(64)]
        op, xp, flp, rows = [outs[k].data_ptr() for k in range(16)], [ins[k].data_ptr() for k in range(16)], fl.data_ptr(), C * H

        def gather(k):
            fn_g(tp, num, rows, W, ip[k % 64], n, None, op[k % 16], flp, st)

        def gather_flip(k):
            fn_g(tp, num, rows, W, ip[k % 64], n, cp[k % 64], op[k % 16], flp, st)

        def hflip(k):
            fn_h(xp[k % 16], op[(k + 1) % 16], cp[k % 64], n, rows, W, st)

        fns = dict(gather=gather, gather_flip=gather_flip, hflip=hflip)
        for fn in fns.values():
            window(fn, calls)
        us = {k: [] for k in fns}
        for _ in range(repeats):
            for k, fn in fns.items():
                us[k].append(window(fn, calls))
        assert int(fl.item()) == 0
        elems = n * C * H * W
        rec = dict(shape=[n, C, H, W])
        for k, v in us.items():
            med = float(np.median(v))
            rec[k] = dict(us_median=med, us_min=float(min(v)), us_max=float(max(v)),
                          GBps=elems * (8 if k == "hflip" else 5) / med * 1e-3)
        rec["gather_over_hflip"] = rec["gather"]["us_median"] / rec["hflip"]["us_median"]
        out.append(rec)
        del outs, ins
    return out


class SyntheticSprites:
    """dSprites-shaped: what FactorSampler and DeviceImageTable.from_dataset read of the reference's class."""
    factor_sizes, latent_indices, resize = FACTOR_SIZES, LATENT_INDICES, SIDE

    def __init__(self, imgs):
        import torch
        from PIL import Image
        self.imgs, self._torch, self._image = imgs, torch, Image

    def __len__(self):
        return len(self.imgs)

    def __getitem__(self, i):
        img = self._image.fromarray(self.imgs[i])                              # dataset.py:142
        a = np.array(img, np.uint8, copy=True)                                 # ToTensor: HWC bytes -> CHW -> / 255
        return self._torch.from_numpy(a).view(SIDE, SIDE, 1).permute(2, 0, 1).contiguous().float().div(255), 0


class ThreeChannels:
    """The encoder in front of one-channel images: repeats the channel on the device."""

    def __init__(self, model):
        self.model = model
        self.training = model.training

    def eval(self):
        self.model.eval()
        self.training = False
        return self

    def train(self, mode=True):
        self.model.train(mode)
        self.training = mode
        return self

    def encode(self, x):
        return self.model.encode(x.expand(-1, 3, -1, -1).contiguous())


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    value = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, value


def end_to_end(imgs_host, dev, bvae_samples):
    import torch
    import models
    from hipvae import disentangle as DS
    from hipvae.dataset import DeviceFactorSampler, DeviceImageTable
    ds = SyntheticSprites(imgs_host)
    t_table, table = wall(lambda: DeviceImageTable.from_dataset(ds, dev))
    torch.manual_seed(0)
    model = ThreeChannels(models.SoftIntroVAE(arch="conv", cdim=3, zdim=128, channels=(64, 128, 256, 512),
                                              image_size=64).to(dev).eval())
    res = dict(table_upload_s=t_table, table_bytes=int(table.images.numel()))
    # warm every batch shape the scores use (64, 128 and 1024 images) before anything is timed
    with torch.no_grad():
        for n in (64, 128, 1024):
            model.encode(table.gather(np.arange(n)))
    images = dict(factor_vae=10000 + (10000 + 5000) * 64, bvae=2 * bvae_samples * 64 * 2)
    calls = dict(factor_vae=lambda s: DS.compute_factor_vae_score(s, model),
                 bvae=lambda s: DS.compute_bvae_score(s, model, num_samples=bvae_samples))
    forward = dict(factor_vae=1024, bvae=128)      # images per encoder call inside each score
    for name, call in calls.items():
        rec = res[name] = dict(images=images[name], images_per_forward=forward[name])
        try:
            for kind, cls in (("device", DeviceFactorSampler), ("host", DS.FactorSampler)):
                sampler = cls(ds, dev, seed=0) if kind == "host" else cls(ds, dev, seed=0, table=table)
                rec[kind + "_s"], rec[kind + "_value"] = wall(lambda: call(sampler))
        except (RuntimeError, ValueError) as e:      # e.g. a fit that does not converge on this untrained model
            rec["error"] = f"{type(e).__name__}: {e}"
            continue
        batch, reps = table.gather(np.arange(forward[name])), images[name] // forward[name]

        def encode_only():
            with torch.no_grad():
                for _ in range(reps):
                    model.encode(batch)

        rec["encode_s"] = wall(encode_only)[0] * images[name] / (reps * forward[name])
        rec["same_value"] = bool(np.array_equal(np.asarray(rec["device_value"], dtype=np.float64),
                                                np.asarray(rec["host_value"], dtype=np.float64), equal_nan=True))
        rec["host_over_device"] = rec["host_s"] / rec["device_s"]
        rec["encode_share_of_device"] = rec["encode_s"] / rec["device_s"]
        rec["encode_share_of_host"] = rec["encode_s"] / rec["host_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--skip-gather", action="store_true")
    ap.add_argument("--bvae-samples", type=int, default=10000)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dataset_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    res = dict(repeats=a.repeats, calls=a.calls, table_images=TABLE_IMAGES)
    if not a.skip_gather:
        g = torch.Generator(device=dev).manual_seed(0)
        raw = torch.randint(0, 256, (TABLE_IMAGES * SIDE * SIDE,), generator=g, device=dev, dtype=torch.uint8)
        res["gather"] = gather_bench(raw, a.repeats, a.calls)
        del raw
        torch.cuda.empty_cache()
    if not a.skip_end_to_end:
        imgs = np.random.default_rng(0).integers(0, 256, size=(TABLE_IMAGES, SIDE, SIDE), dtype=np.uint8)
        res["end_to_end"] = end_to_end(imgs, dev, a.bvae_samples)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
