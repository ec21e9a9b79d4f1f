"""The numpy fp64 restatement of the SSIM rules of include/itcv_hip.h (csrc/ssim.hip), shared by
tests/test_ssim_ref_host.py (which pins it) and tests/test_hip_ssim.py (which holds the kernels to it), with the recipes
of their inputs, their shapes, and the kernels' a-priori error bound.  Free of torch.

The windowed sums are written as the DIRECT 2-D sum over the K x K taps of g (x) g (and its transpose, the scatter of
every position back onto its K x K pixels), so the restatement shares no structure with the separable, tiled kernels.

The error bound (``ssim_bound``).  u = 2^-53.  Inputs are fp32 values in [0, 1]; x^2, y^2 and xy are exact in fp64.
* A moment (w*x, w*y, w*x^2, w*y^2, w*xy) is a sum of K^2 non-negative terms g_i g_j v.  Summed in any order, with the
  products rounded, the result is within (K^2 + 1) u of the exact sum, relatively (Higham, Accuracy and Stability,
  eq. 3.4 and 4.4).  The kernels' separable order -- K taps along a row, then K taps down the rows -- costs 2 K + 2 <=
  K^2 + 1 roundings per term for K >= 3.  Kernel and restatement each err by that much, so their moments differ by at most
  e_m |m|, e_m = 2 (K^2 + 1) u.
* Everything after the moments is a fixed expression tree that the kernels and this file evaluate alike (the formulas of
  the header, grouped as written there).  ``_E`` carries a value with a bound on |kernel - restatement| through that tree,
  the running error analysis of Higham 3.3: for c = a op b the propagated bound is exact interval arithmetic on the
  operands' bounds (|a| eb + |b| ea + ea eb for a product, (ea + |a / b| eb) / (|b| - eb) for a quotient), plus 2 u (|c| +
  propagated) for the two roundings, one on each side.  Nothing is linearised: A2 may cross zero (only its absolute
  error enters) and the denominators stay positive because B1 >= C1 and B2 >= C2 up to the same bounds, which the
  quotient's (|b| - eb) accounts for.
* A sum of n terms of either sign in any order (the tile sums, the fold of the partials, numpy's pairwise sum here) is
  within (n - 1) u sum |t| of exact on each side: 2 u n sum |t| between the two, on top of the terms' own bounds.  The
  adjoint window sums of the gradient are of this kind with the products rounded: e_m sum g_i g_j |coef| on top of
  sum g_i g_j bound(coef).
* The result is rounded to fp32 once: the tests add 2^-24 |ref| themselves, and the bound is multiplied by 1 + 2^-23 for
  the rounding of a value that is off by the bound.
For K <= 15 and inputs in [0, 1] the row bound comes to about 2e-10 P at worst, dominated by the error of A2 over C2 =
9e-4; an fp32 evaluation of the same map is off by about 4e-6 P.  tests/test_ssim_ref_host.py holds every input of the GPU
tests to 1e-9 P (rows) and 1e-9 max |dy| (gradient), so that no fp32 implementation can pass."""
import functools

import numpy as np

U = 2.0 ** -53
C1, C2 = 0.01 ** 2, 0.03 ** 2
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
TILE = 16                                    # the kernels' tile of positions (forward) and of pixels (backward)

# (B, C, H, W, K): the issue's table with its 32 replaced by the tile of 16
SHAPES = (
    (1, 1, 11, 11, 11),                      # one position
    (2, 3, 12, 17, 11),                      # 2 x 7 positions
    (2, 1, 11, 43, 11),                      # one row of positions, three tiles wide (33 columns)
    (3, 1, 27, 26, 11),                      # 17 x 16 positions: a one-row partial tile next to full ones
    (2, 3, 32, 32, 11),                      # the tiny model's images
    (1, 3, 64, 64, 11),                      # a c2 image
    (2, 2, 9, 20, 3),                        # both ends of K
    (1, 1, 40, 40, 15),
)
KINDS = ("uniform", "smooth", "binary", "constant", "same")
ALPHAS = (1.0, 0.84, 0.0)
REDUCTIONS = ("none", "sum", "mean")


def window(K=11, sigma=1.5):
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return g / g.sum()


def _grid(v, bits):
    """v rounded to multiples of 2^-bits in [0, 1], as fp32 (exact for bits <= 24)."""
    s = float(1 << bits)
    return (np.clip(np.rint(np.asarray(v, dtype=np.float64) * s), 0.0, s) / s).astype(np.float32)


def _box(a, r=2):
    """(2 r + 1)^2 box mean with edge replication: the low-pass of the smooth pairs."""
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], mode="edge")
    H, W = a.shape[-2:]
    out = np.zeros_like(a)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            out += p[..., i:i + H, j:j + W]
    return out / (2 * r + 1) ** 2


@functools.lru_cache(maxsize=None)
def make_pair(kind, shape, seed=0, bits=24):
    """(x, y) fp32 [B, C, H, W] in [0, 1], multiples of 2^-bits (torch.rand's grid for 24; y - x is then exact in fp32 too,
    and with bits = 16 four 2 x 2 means in a row are exact).  The arrays are shared: do not write to them."""
    B, C, H, W = shape
    rs = np.random.RandomState(1000 * seed + 7 * KINDS.index(kind) + H * W + B + C)
    if kind == "uniform":
        x, y = rs.rand(B, C, H, W), rs.rand(B, C, H, W)
    elif kind == "smooth":
        # a 3 x 3 low-pass and some grain: flatter pairs (a 5 x 5 mean, 2 % grain) put windows of next to no variance
        # under B2 ~ C2, where the gradient's three terms of size 1 / C2 cancel, and break the host test's gradient cap
        x = _box(rs.rand(B, C, H, W), 1)
        y = np.clip(x + 0.2 * (_box(rs.rand(B, C, H, W), 1) - 0.5) + 0.2 * (rs.rand(B, C, H, W) - 0.5), 0.0, 1.0)
    elif kind == "binary":
        # white on black as in dSprites: blobs, perforated so that no window is all white (all-black ones, whose moments
        # are exactly 0, abound) -- an all-white window is the flat case above at its worst and breaks the same cap at K = 3
        x = ((_box(rs.rand(B, C, H, W)) > 0.5) & (rs.rand(B, C, H, W) < 0.35)).astype(np.float64)
        y = np.where(rs.rand(B, C, H, W) < 0.1, 1.0 - x, x)
    elif kind == "constant":
        x = np.broadcast_to(rs.rand(B, C, 1, 1), (B, C, H, W)).copy()
        y = rs.rand(B, C, H, W)
    elif kind == "same":
        x = rs.rand(B, C, H, W)
        y = x
    else:
        raise ValueError(kind)
    x = _grid(x, bits)
    y = x.copy() if kind == "same" else _grid(y, bits)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


def upstream(B, reduction, seed=0):
    """The gradient of the loss's output that the tests feed back: fp32 [B] for "none", a scalar else."""
    rs = np.random.RandomState(77 + seed + B)
    return (0.5 + rs.rand(B if reduction == "none" else 1)).astype(np.float32)


def wsum(a, g):
    """Valid filtering of [..., H, W] with g (x) g as the direct sum over the K x K taps, rows outside columns."""
    K = len(g)
    Hp, Wp = a.shape[-2] - K + 1, a.shape[-1] - K + 1
    out = np.zeros(a.shape[:-2] + (Hp, Wp))
    for i in range(K):
        for j in range(K):
            out += (g[i] * g[j]) * a[..., i:i + Hp, j:j + Wp]
    return out


def wsum_t(c, g):
    """The adjoint of ``wsum``: every position's value back onto its K x K pixels."""
    K = len(g)
    Hp, Wp = c.shape[-2:]
    out = np.zeros(c.shape[:-2] + (Hp + K - 1, Wp + K - 1))
    for i in range(K):
        for j in range(K):
            out[..., i:i + Hp, j:j + Wp] += (g[i] * g[j]) * c
    return out


def maps(x, y, K=11, sigma=1.5):
    """Every intermediate of the definition at every position of every plane (fp64 [B, C, H', W'])."""
    g = window(K, sigma)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mx, my, ex2, ey2, exy = wsum(x, g), wsum(y, g), wsum(x * x, g), wsum(y * y, g), wsum(x * y, g)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = ex2 - mxx, ey2 - myy, exy - mxy
    A1, A2 = 2.0 * mxy + C1, 2.0 * sxy + C2
    B1, B2 = (mxx + myy) + C1, (sx + sy) + C2
    return dict(g=g, mx=mx, my=my, ex2=ex2, ey2=ey2, exy=exy, A1=A1, A2=A2, B1=B1, B2=B2, S=(A1 * A2) / (B1 * B2),
                cs=A2 / B2)


def rows(x, y, alpha=1.0, K=11, sigma=1.5):
    """rows[b] = (P alpha) (1 - SSIM_b) + (1 - alpha) sum |y - x|."""
    m = maps(x, y, K, sigma)
    B = x.shape[0]
    P, n = float(np.prod(x.shape[1:])), float(np.prod(m["S"].shape[1:]))
    l1 = np.abs(np.asarray(y, dtype=np.float64) - np.asarray(x, dtype=np.float64)).reshape(B, -1).sum(1)
    return (P * alpha) * (1.0 - m["S"].reshape(B, -1).sum(1) / n) + (1.0 - alpha) * l1


def loss(x, y, alpha=1.0, reduction="sum", scale=1.0, K=11, sigma=1.5):
    """What itcv_ssim_loss_fwd writes, before its one rounding to fp32; ``scale`` is taken as the fp32 it is passed as."""
    r, s = rows(x, y, alpha, K, sigma), float(np.float32(scale))
    if reduction == "none":
        return s * r
    return np.array(s * (r.sum() / len(r) if reduction == "mean" else r.sum()))


def grad(x, y, gup, alpha=1.0, reduction="sum", scale=1.0, K=11, sigma=1.5):
    """d loss / d y for the upstream gradient ``gup`` ([B] for "none", [1] else), before the rounding to fp32."""
    m = maps(x, y, K, sigma)
    g = m["g"]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B = x.shape[0]
    P, n = float(np.prod(x.shape[1:])), float(np.prod(m["S"].shape[1:]))
    A1, A2, B1, B2, S = m["A1"], m["A2"], m["B1"], m["B2"], m["S"]
    b12 = B1 * B2
    ca = (2.0 * m["mx"]) * (A2 - A1) / b12 + (2.0 * m["my"]) * S * (1.0 / B2 - 1.0 / B1)
    cb = -S / B2
    cc = (2.0 * A1) / b12
    inner = (wsum_t(ca, g) + (2.0 * y) * wsum_t(cb, g)) + x * wsum_t(cc, g)
    coef = float(np.float32(scale)) / B if reduction == "mean" else float(np.float32(scale))
    gb = np.asarray(gup, dtype=np.float64) * coef
    gb = (gb if reduction == "none" else np.repeat(gb, B)).reshape(B, 1, 1, 1)
    return -(gb * ((P * alpha) / n)) * inner + (gb * (1.0 - alpha)) * np.sign(y - x)


def stats(x, y, K=11, sigma=1.5):
    """fp64 [B, C, 2]: the mean of S and the mean of cs over the positions of every plane."""
    m = maps(x, y, K, sigma)
    B, C = x.shape[:2]
    n1 = float(m["S"].shape[-2] * m["S"].shape[-1])
    return np.stack([m["S"].reshape(B, C, -1).sum(2) / n1, m["cs"].reshape(B, C, -1).sum(2) / n1], 2)


def halve(a):
    """2 x 2 mean in fp32, an odd last row or column dropped (F.avg_pool2d(a, 2)); exact on a grid of 2^-22 or coarser."""
    a = np.asarray(a, dtype=np.float32)
    H2, W2 = a.shape[-2] // 2, a.shape[-1] // 2
    a = a[..., :2 * H2, :2 * W2]
    return ((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2])) * np.float32(0.25)


def levels_of(H, W, K=11):
    L = 1
    while L < 5 and (min(H, W) >> L) >= K:
        L += 1
    return L


def quality(x, y, K=11, sigma=1.5, levels=None):
    """dict of fp64 [B]: psnr, ssim, ms_ssim, mse, l1 -- hipvae.quality.reconstruction_quality's rules."""
    B = x.shape[0]
    L = levels_of(x.shape[2], x.shape[3], K) if levels is None else levels
    d = np.asarray(y, dtype=np.float64) - np.asarray(x, dtype=np.float64)
    mse, l1 = (d * d).reshape(B, -1).mean(1), np.abs(d).reshape(B, -1).mean(1)
    w = np.array(MS_WEIGHTS[:L])
    w = w / w.sum()
    ms, xl, yl, ssim = 1.0, x, y, None
    for lev in range(L):
        if lev:
            xl, yl = halve(xl), halve(yl)
        st = stats(xl, yl, K, sigma)
        if lev == 0:
            ssim = st[:, :, 0].mean(1)
        ms = ms * np.maximum(st[:, :, 0 if lev == L - 1 else 1], 0.0) ** w[lev]
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(1.0 / mse)
    return dict(psnr=psnr, ssim=ssim, ms_ssim=ms.mean(1), mse=mse, l1=l1)


# ---- the a-priori bound ---------------------------------------------------------------------------------------------------
class _E:
    """A value with a bound on |kernel - restatement| (module docstring): exact propagation plus 2 u per operation."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(a):
        return a if isinstance(a, _E) else _E(a)

    @staticmethod
    def _round(v, e):
        return _E(v, e + 2.0 * U * (np.abs(v) + e))

    def __add__(self, o):
        o = _E.of(o)
        return _E._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = _E.of(o)
        return _E._round(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = _E.of(o)
        return _E._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = _E.of(o)
        assert np.all(np.abs(o.v) > o.e), "a denominator that its own bound lets reach zero"
        q = self.v / o.v
        return _E._round(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))

    __radd__, __rmul__ = __add__, __mul__

    def __rsub__(self, o):
        return _E.of(o) - self

    def __rtruediv__(self, o):
        return _E.of(o) / self

    def __neg__(self):
        return _E(-self.v, self.e)

    def twice(self):                                   # a product with 2 is exact
        return _E(2.0 * self.v, 2.0 * self.e)

    def total(self, axis_from=1):
        """The sum over all axes from ``axis_from`` on, in any order: the terms' bounds plus 2 u n sum |t|."""
        B = self.v.shape[:axis_from]
        v, e = self.v.reshape(B + (-1,)), self.e.reshape(B + (-1,))
        n = v.shape[-1]
        return _E(v.sum(-1), e.sum(-1) + 2.0 * U * n * (np.abs(v) + e).sum(-1))


def _bound_maps(x, y, K, sigma):
    m = maps(x, y, K, sigma)
    em = 2.0 * (K * K + 1) * U
    mx, my, ex2, ey2, exy = (_E(m[k], em * np.abs(m[k])) for k in ("mx", "my", "ex2", "ey2", "exy"))
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx, sy, sxy = ex2 - mxx, ey2 - myy, exy - mxy
    A1, A2 = mxy.twice() + C1, sxy.twice() + C2
    B1, B2 = (mxx + myy) + C1, (sx + sy) + C2
    return dict(g=m["g"], em=em, mx=mx, my=my, A1=A1, A2=A2, B1=B1, B2=B2, S=(A1 * A2) / (B1 * B2), cs=A2 / B2)


def _final(e):
    return np.asarray(e) * (1.0 + 2.0 ** -23)


def ssim_bound(x, y, alpha=1.0, reduction="sum", scale=1.0, K=11, sigma=1.5, rows_only=False):
    """Bound on |kernel's fp64 value - ``loss``| per output ([B] for "none", a scalar else); ``rows_only``: on the
    unscaled rows [B]."""
    bm = _bound_maps(x, y, K, sigma)
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B = x.shape[0]
    P, n = float(np.prod(x.shape[1:])), float(np.prod(bm["S"].v.shape[1:]))
    l1 = _E(np.abs(yd - xd)).total()                                    # every term is exact
    row = _E(P * alpha, 2.0 * U * P * alpha) * (1.0 - bm["S"].total() / n) + _E(1.0 - alpha, 2.0 * U) * l1
    if rows_only:
        return _final(row.e)
    s = float(np.float32(scale))
    if reduction == "none":
        return _final((s * row).e)
    t = row.total(0)
    return _final((s * (t / float(B) if reduction == "mean" else t)).e)


def grad_bound(x, y, gup, alpha=1.0, reduction="sum", scale=1.0, K=11, sigma=1.5):
    """Bound on |kernel's fp64 dy - ``grad``| per pixel."""
    bm = _bound_maps(x, y, K, sigma)
    g, em = bm["g"], bm["em"]
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B = x.shape[0]
    P, n = float(np.prod(x.shape[1:])), float(np.prod(bm["S"].v.shape[1:]))
    A1, A2, B1, B2, S = bm["A1"], bm["A2"], bm["B1"], bm["B2"], bm["S"]
    b12 = B1 * B2
    ca = bm["mx"].twice() * (A2 - A1) / b12 + bm["my"].twice() * S * (1.0 / B2 - 1.0 / B1)
    cb = -(S / B2)
    cc = A1.twice() / b12

    def back(c):
        return _E(wsum_t(c.v, g), wsum_t(c.e, g) + em * wsum_t(np.abs(c.v) + c.e, g))

    inner = (back(ca) + _E(2.0 * yd) * back(cb)) + _E(xd) * back(cc)
    coef = _E(float(np.float32(scale))) / float(B) if reduction == "mean" else _E(float(np.float32(scale)))
    gb = _E(np.asarray(gup, dtype=np.float64)) * coef
    if reduction != "none":
        gb = _E(np.repeat(gb.v, B), np.repeat(gb.e, B))
    gb = _E(gb.v.reshape(B, 1, 1, 1), gb.e.reshape(B, 1, 1, 1))
    ratio = _E(P * alpha, 2.0 * U * P * alpha) / n
    dy = -(gb * ratio) * inner + (gb * _E(1.0 - alpha, 2.0 * U)) * _E(np.sign(yd - xd))
    return _final(dy.e)


def stats_bound(x, y, K=11, sigma=1.5):
    """Bound on |kernel - ``stats``| [B, C, 2]."""
    bm = _bound_maps(x, y, K, sigma)
    n1 = float(bm["S"].v.shape[-2] * bm["S"].v.shape[-1])
    return np.stack([(bm["S"].total(2) / n1).e, (bm["cs"].total(2) / n1).e], 2)


def quality_bound(x, y, K=11, sigma=1.5, levels=None):
    """Bounds [B] on |reconstruction_quality - ``quality``|.  ``ssim``: the statistics' bound through the mean over C
    channels (a sum of C terms and a division).  ``ms_ssim``: every factor v^w, v = max(stat, 0) >= its bound, moves by at
    most w v^(w-1) e / (1 - e / v) for a change e of v (the mean value theorem on [v - e, v + e], w <= 1) and costs 4 u of
    its own (a pow within 2 ulp on either side); the product and the channel mean go through ``_E``.  ``mse`` and ``l1``
    are means of P terms exact up to one rounding each (the difference of two fp32 values is exact in fp64, its square
    is rounded), summed in any order; ``psnr`` = 10 log10(1 / mse) moves by (10 / ln 10) e / (mse - e), plus 8 u |psnr|
    + 8 u for a log10 within 2 ulp on either side and the two other operations."""
    B, C = x.shape[:2]
    L = levels_of(x.shape[2], x.shape[3], K) if levels is None else levels
    w = np.array(MS_WEIGHTS[:L])
    w = w / w.sum()
    d = np.asarray(y, dtype=np.float64) - np.asarray(x, dtype=np.float64)
    P = float(d[0].size)
    mse = _E(d * d, 2.0 * U * d * d).total() / P
    l1 = _E(np.abs(d)).total() / P
    ms, xl, yl, ssim = None, x, y, None
    for lev in range(L):
        if lev:
            xl, yl = halve(xl), halve(yl)
        st, sb = stats(xl, yl, K, sigma), stats_bound(xl, yl, K, sigma)
        if lev == 0:
            ssim = _E(st[:, :, 0], sb[:, :, 0]).total() / float(C)
        k = 0 if lev == L - 1 else 1
        v, e = np.maximum(st[:, :, k], 0.0), sb[:, :, k]
        assert np.all(v > 2.0 * e), "a factor of MS-SSIM that its bound lets reach zero"
        f = v ** w[lev]
        f = _E(f, w[lev] * f / v * e / (1.0 - e / v) + 4.0 * U * f)
        ms = f if ms is None else ms * f
    ms = ms.total() / float(C)
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = 10.0 * np.log10(1.0 / mse.v)
        pe = np.where(mse.v > 0.0, (10.0 / np.log(10.0)) * mse.e / (mse.v - mse.e) + 8.0 * U * (np.abs(psnr) + 1.0), 0.0)
    return dict(psnr=pe, ssim=ssim.e, ms_ssim=ms.e, mse=mse.e, l1=l1.e)
