"""Pillow's 8-bit bicubic resize restated in plain Python / numpy, independent of hipvae/resize.py: the reference of the
resize tests (tests/test_resize_host.py pins it to Pillow's own bytes, recorded in golden/resize.npz and live where Pillow
is installed; tests/test_hip_resize.py pins the kernel to it).

The plan of an axis is built one output position and one tap at a time with Python floats (C doubles), in the order of
Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc``; a pass is an int64 numpy sum (it cannot overflow, which lets
``max_accumulator`` check the int32 claim instead of assuming it)."""
import math

import numpy as np

BITS = 22


def cubic(t):
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def plan(in_size, out_size):
    """``(bounds [out, 2], coef [out, ksize])`` as int64 arrays."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    coef = np.zeros((out_size, ksize), dtype=np.int64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), in_size) - xmin
        w, ww = [], 0.0
        for x in range(cnt):
            v = cubic((x + xmin - center + 0.5) / fs)
            w.append(v)
            ww += v
        for x in range(cnt):
            v = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5)     # int(): C truncation
        bounds[xx] = xmin, cnt
    return bounds, coef


def max_accumulator(coef):
    """The largest magnitude the accumulator of a pass can reach with bytes in [0, 255]."""
    return 255 * int(np.abs(coef).sum(axis=1).max()) + (1 << (BITS - 1))


def one_pass(a, out_size, axis):
    """uint8 array ``a`` resized along ``axis``."""
    bounds, coef = plan(a.shape[axis], out_size)
    src = np.moveaxis(a, axis, -1).astype(np.int64)
    out = np.empty(src.shape[:-1] + (out_size,), dtype=np.uint8)
    for xx in range(out_size):
        mn, c = bounds[xx]
        acc = (1 << (BITS - 1)) + (src[..., mn:mn + c] * coef[xx, :c]).sum(axis=-1)
        out[..., xx] = np.clip(acc >> BITS, 0, 255)
    return np.moveaxis(out, -1, axis)


def resize(planar, Hout, Wout):
    """uint8 ``[..., H, W]`` -> ``[..., Hout, Wout]``: the horizontal pass to uint8, then the vertical pass on that; an
    axis whose size does not change gets no pass."""
    a = np.asarray(planar)
    assert a.dtype == np.uint8
    if a.shape[-1] != Wout:
        a = one_pass(a, Wout, a.ndim - 1)
    if a.shape[-2] != Hout:
        a = one_pass(a, Hout, a.ndim - 2)
    return np.ascontiguousarray(a)


def unit(u8):
    """``ToTensor``'s fp32 ``byte / 255``."""
    return u8.astype(np.float32) / np.float32(255)


# Hin, Win, Hout, Wout, channel counts: the cases of golden/resize.npz and of the GPU tests
SHAPES = [
    (64, 64, 128, 128, (1, 3)), (64, 64, 32, 32, (1, 3)), (256, 256, 64, 64, (3,)), (256, 256, 128, 128, (1,)),
    (64, 64, 256, 256, (1,)), (64, 64, 96, 96, (1,)), (64, 64, 48, 48, (1,)), (8, 8, 12, 12, (3,)), (16, 16, 5, 5, (3,)),
    (5, 6, 10, 12, (3,)), (7, 9, 13, 4, (3,)), (12, 20, 12, 8, (1,)), (12, 20, 6, 20, (1,)),
]


def case_name(Hin, Win, Hout, Wout, C):
    return f"{Hin}x{Win}_{Hout}x{Wout}_c{C}"


def case_images(Hin, Win, C, seed=0):
    """The two inputs of a case, planar uint8 ``[2, C, Hin, Win]``: a random image in which every byte value occurs (as
    far as the image has room) and a 0/255 image, whose overshoot reaches both clamps."""
    rng = np.random.RandomState(seed + 7 * Hin + 131 * Win + 1009 * C)
    a = rng.randint(0, 256, size=(C, Hin, Win)).astype(np.uint8)
    flat = a.reshape(-1)
    m = min(256, flat.size)
    flat[:m] = rng.permutation(256)[:m].astype(np.uint8)
    b = (rng.randint(0, 2, size=(C, Hin, Win)) * 255).astype(np.uint8)
    return np.stack([a, b])
