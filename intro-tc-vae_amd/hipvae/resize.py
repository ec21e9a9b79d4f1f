"""Pillow's 8-bit bicubic resize as plans for ``itcv_resize_u8`` (csrc/resize.hip).

``Image.resize(size, Image.BICUBIC)`` on an ``L`` or ``RGB`` image is integer arithmetic once its per-axis coefficient
tables exist; the tables themselves come out of C doubles.  ``bicubic_plan`` makes them here in numpy fp64, operation for
operation (the weights' sum included: left to right, not numpy's pairwise sum), so the kernel has nothing left to do in
floating point and its bytes equal Pillow's.  ``ResizePlan`` holds the device copies for one pair of image sizes.
"""
import math

import numpy as np
import torch

from . import abi

__all__ = ["bicubic_plan", "ResizePlan", "PRECISION_BITS"]

PRECISION_BITS = 32 - 8 - 2          # Pillow's 8-bit fixed point: coefficients in units of 2^-22


def _bicubic(t):
    """Pillow's bicubic filter (a = -0.5) on an fp64 array."""
    a = -0.5
    t = np.abs(t)
    inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    outer = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def bicubic_plan(in_size, out_size):
    """``(bounds int32 [out_size, 2], coef int32 [out_size, ksize])`` of one axis: output ``xx`` is
    ``clamp((2^21 + sum_{t < bounds[xx, 1]} src[bounds[xx, 0] + t] * coef[xx, t]) >> 22, 0, 255)``.  Rows of ``coef`` are
    zero past their tap count.  Raises ``ValueError`` for sizes below 1 and for a plan whose accumulator could leave
    int32 (``255 * sum |coef| + 2^21 >= 2^31``: no bicubic plan met so far comes near, the sum stays at or below 1.25 * 2^22)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"bicubic_plan: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # C truncation: the operands are > -1
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    live = taps < cnt[:, None]
    w = _bicubic((taps + xmin[:, None] - center[:, None] + 0.5) / fs)
    w = np.where(live, w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):                                                    # the sum as C makes it: left to right
        ww = ww + w[:, t]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    fixed = w * float(1 << PRECISION_BITS)
    coef = np.where(w < 0, np.trunc(fixed - 0.5), np.trunc(fixed + 0.5)).astype(np.int64)
    coef = np.where(live, coef, 0)
    if 255 * int(np.abs(coef).sum(axis=1).max()) + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError(f"bicubic_plan: the {in_size} -> {out_size} plan does not fit an int32 accumulator")
    return np.stack([xmin, cnt], axis=1).astype(np.int32), coef.astype(np.int32)


class ResizePlan:
    """The device copies of the two axis plans of ``Hin x Win -> Hout x Wout``; an axis of equal size holds ``None``
    (Pillow runs no pass over it).  ``ResizePlan.get`` keeps one per (sizes, device)."""

    _cache = {}

    def __init__(self, Hin, Win, Hout, Wout, device):
        self.Hin, self.Win, self.Hout, self.Wout = (int(v) for v in (Hin, Win, Hout, Wout))
        self.device = torch.device(device)
        self.xbounds = self.xcoef = self.ybounds = self.ycoef = None
        self.kx = self.ky = 0
        if self.Wout != self.Win:
            b, c = bicubic_plan(self.Win, self.Wout)
            self.xbounds, self.xcoef, self.kx = self._up(b), self._up(c), int(c.shape[1])
        elif self.Win < 1:
            raise ValueError("ResizePlan: sizes must be positive")
        if self.Hout != self.Hin:
            b, c = bicubic_plan(self.Hin, self.Hout)
            self.ybounds, self.ycoef, self.ky = self._up(b), self._up(c), int(c.shape[1])
        elif self.Hin < 1:
            raise ValueError("ResizePlan: sizes must be positive")

    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    @property
    def identity(self):
        return self.xbounds is None and self.ybounds is None

    @classmethod
    def get(cls, Hin, Win, Hout, Wout, device):
        device = torch.device(device)
        key = (int(Hin), int(Win), int(Hout), int(Wout), device.type, device.index)
        plan = cls._cache.get(key)
        if plan is None:
            plan = cls._cache[key] = cls(Hin, Win, Hout, Wout, device)
        return plan

    def launch(self, table, num_images, planes, idx, n, flip, out, flags):
        """One ``itcv_resize_u8`` call on the current stream: ``table`` a uint8 device tensor whose images are
        ``[planes, Hin, Win]``, ``idx`` an int64 device tensor or ``None`` (images ``0..n-1``), ``out`` a dense uint8 or
        fp32 ``[n, planes, Hout, Wout]`` device tensor."""
        abi.call("itcv_resize_u8", abi.ptr(table), num_images, planes, self.Hin, self.Win, abi.ptr(idx), n, abi.ptr(flip),
                 abi.ptr(self.xbounds), abi.ptr(self.xcoef), self.kx, abi.ptr(self.ybounds), abi.ptr(self.ycoef), self.ky,
                 self.Hout, self.Wout, abi.ptr(out), int(out.dtype == torch.float32), flags.data_ptr(), abi.stream())
