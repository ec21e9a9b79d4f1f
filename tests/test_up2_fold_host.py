"""CPU-only: where the data gradient of an upsampled conv takes the fused route (the upsample's 2x2 adjoint folded into the
band kernel's store, ``itcv_conv2d_dgrad_up2_bf16p``).

1. ``itcv_conv2d_dgrad_up2_supported`` over a grid of shapes against the rules it stands for, written out here from the
   planning code (``plan_fwd_band``, csrc/conv_band.hip): the band kernels take the launch, the plan has no K split, the
   launched kernel form has an adjoint-store instantiation (whole-row 256-pixel tiles of 16..64-wide images, two-plane
   formats, 16x16x32 products), H and W are even.
2. The gate of ``Conv2dFn.backward``: in every step configuration whose library-call sequence is pinned
   (tests/test_hip_call_trace.py: TINY and C1 at batch 8, with the batched two-group passes) the largest high-resolution
   gradient of the decoder's upsampled convs lies below the default threshold, so those steps keep their two calls."""
import pytest

F16X2 = 4


def cdiv(a, b):
    return -(-a // b)


def log2_exact(v):
    return v.bit_length() - 1 if v > 0 and not v & (v - 1) else -1


def band_plan(B, Ci, H, W, Co, KS):
    """plan_fwd_band for two planes: dict(bm, bn, rows2, mt, nt, splits), or None where the band kernels refuse."""
    lw, lh = log2_exact(W), log2_exact(H)
    if KS != 3 or lw < 3 or lw > 8 or lh < 0 or Ci % 32 or Co < 33:
        return None
    bn = 128 if lw > 6 else 256
    rows2 = lw > 6 and H >= 2
    wb = 64 if rows2 else min(W, bn)
    nr = bn // wb
    sr = min(nr, H)
    npc = cdiv((nr // sr) * (sr + 2) * (wb + 2), 64)
    if npc > 7:
        return None
    nt = cdiv(B * H * W, bn)
    bm = 64 if Co <= 64 else 128
    if bm == 128 and cdiv(Co, 128) * nt < 192 and cdiv(Co, 64) * nt >= 128:
        bm = 64
    g = 2 if (bm == 64 or bn == 128) else 1
    lds = max((3 * g * 2 * 4 * bm + 2 * 2 * 4 * npc * 64) * 16, bm * 260 * 4 if bn == 256 else 0)
    if lds > 160 * 1024:
        return None
    mt, cpt = cdiv(Co, bm), Ci // 32
    tiles = mt * nt
    if tiles < 192 and cdiv(Co, 128) * cdiv(B * H * W, 128) >= 192 and Co > 64:
        return None
    splits = 1
    if tiles < 192 and cpt >= 2:
        splits = max(1, min(256 // tiles, cpt))
    splits = cdiv(cpt, cdiv(cpt, splits))
    return dict(bm=bm, bn=bn, rows2=rows2, mt=mt, nt=nt, splits=splits)


def expected(B, Ci, H, W, Co, KS, fmt, nb):
    if min(B, Ci, H, W, Co) <= 0 or not 1 <= nb <= B or fmt not in (2, F16X2) or H % 2 or W % 2:
        return 0
    if KS not in (1, 3) or Ci % 32 or Co <= 32:           # itcv_conv2d_bf16s_supported
        return 0
    p = band_plan(B, Ci, H, W, Co, KS)
    if p is None or p["splits"] != 1:
        return 0
    return int(p["bn"] == 256 and not p["rows2"] and 4 <= log2_exact(W) <= 6)


@pytest.fixture(scope="module")
def lib():
    from hipvae import abi
    return abi.lib


GRID = [(B, Ci, S, S, Co, KS, fmt)
        for B in (1, 2, 4, 12, 17, 24, 48, 64, 96, 128)
        for Ci in (32, 64, 128, 256, 512, 48)
        for S in (4, 8, 16, 32, 64, 128, 256)
        for Co in (32, 33, 64, 96, 128, 256, 512)
        for KS in (1, 3, 5)
        for fmt in (2, 3, F16X2)
        if B * max(Ci, Co) * S * S < 1 << 27]


def test_query_follows_the_plan_rules(lib):
    assert lib.itcv_get_option(b"band_m16") == 1          # bf16 planes: the 16x16x32 form is the launched one
    ones = 0
    for B, Ci, H, W, Co, KS, fmt in GRID:
        want = expected(B, Ci, H, W, Co, KS, fmt, B)
        assert lib.itcv_conv2d_dgrad_up2_supported(B, Ci, H, W, Co, KS, fmt, B) == want, (B, Ci, H, W, Co, KS, fmt)
        ones += want
    assert 200 < ones < len(GRID) // 2


def test_query_edges(lib):
    q = lib.itcv_conv2d_dgrad_up2_supported
    assert q(128, 64, 64, 64, 64, 3, F16X2, 128) == 1 and q(128, 64, 64, 64, 64, 3, 2, 64) == 1
    assert q(128, 512, 8, 8, 512, 3, F16X2, 128) == 0                  # the c2 8x8 layer: 8-wide images have no such form
    assert q(32, 512, 8, 8, 512, 3, F16X2, 32) == 0                    # ... and with fewer images its K is split as well
    assert lib.itcv_conv2d_fwd_bf16p_workspace(32, 512, 8, 8, 512, 3, F16X2) > 0
    assert q(2, 64, 64, 64, 128, 3, F16X2, 2) == 0                     # 32 tiles, two channel groups: K split in two
    assert lib.itcv_conv2d_fwd_bf16p_workspace(2, 64, 64, 64, 128, 3, F16X2) > 0
    assert q(12, 64, 64, 64, 128, 3, F16X2, 12) == 1                   # 192 tiles: no split
    assert lib.itcv_conv2d_fwd_bf16p_workspace(12, 64, 64, 64, 128, 3, F16X2) == 0
    assert q(128, 64, 1, 64, 64, 3, F16X2, 128) == 0                   # odd H
    assert q(128, 64, 64, 64, 32, 3, F16X2, 128) == 0                  # Co < 33
    assert q(128, 64, 64, 64, 64, 3, 3, 128) == 0                      # three planes
    assert q(128, 64, 128, 128, 64, 3, F16X2, 128) == 0                # the two-row tiles of wide images
    assert q(128, 64, 64, 64, 64, 3, F16X2, 0) == 0 and q(128, 64, 64, 64, 64, 3, F16X2, 129) == 0
    assert q(0, 64, 64, 64, 64, 3, F16X2, 1) == 0
    # non-square: a 256-pixel tile of two short images
    assert q(256, 32, 8, 16, 64, 3, F16X2, 256) == expected(256, 32, 8, 16, 64, 3, F16X2, 256) == 1


def test_query_follows_the_band_m16_option(lib):
    from hipvae import functional as HF
    s = (128, 64, 64, 64, 64, 3)
    with HF.option_scope("band_m16", 0):      # bf16 planes then run the 32x32x16 form, which has no adjoint store
        assert lib.itcv_conv2d_dgrad_up2_supported(*s, 2, 128) == 0
        assert lib.itcv_conv2d_dgrad_up2_supported(*s, F16X2, 128) == 1
        assert not HF.up2_fold_route(*s, 2, 128) and HF.up2_fold_route(*s, F16X2, 128)
    assert lib.itcv_conv2d_dgrad_up2_supported(*s, 2, 128) == 1 and HF.up2_fold_route(*s, 2, 128)


def test_c2_step_layers():
    """The layers the route is for: at c2 (128-image passes, 64 live images in phase E) the 64x64 and 32x32 layers fold
    in both, the 16x16 layer in the full pass only (32 MiB exactly), the 8x8 layer never (8-wide; K split)."""
    from hipvae import functional as HF
    assert HF.UP2_FOLD_MIN_BYTES[0] == 32 << 20
    got = {(S, nb): HF.up2_fold_route(128, d, S, S, x, 3, F16X2, nb)
           for d, x, S in ((64, 64, 64), (64, 128, 32), (128, 256, 16), (256, 512, 8)) for nb in (128, 64)}
    assert got == {(64, 128): True, (64, 64): True, (32, 128): True, (32, 64): True, (16, 128): True, (16, 64): False,
                   (8, 128): False, (8, 64): False}


def test_setter_and_threshold():
    from hipvae import functional as HF
    s = (16, 64, 32, 32, 64, 3, F16X2, 16)
    assert HF.lib.itcv_conv2d_dgrad_up2_supported(*s) == expected(*s)
    prev = HF.UP2_FOLD_MIN_BYTES[0]
    try:
        HF.set_up2_fold_min_bytes(1)
        low = HF.up2_fold_route(*s)
        HF.set_up2_fold_min_bytes(16 * 64 * 32 * 32 * 4 + 1)
        assert not HF.up2_fold_route(*s)
        HF.set_up2_fold_min_bytes(16 * 64 * 32 * 32 * 4)
        assert HF.up2_fold_route(*s) == low == bool(expected(*s))
    finally:
        HF.set_up2_fold_min_bytes(prev)
    assert not HF.up2_fold_route(*s)


# ---- the gate ------------------------------------------------------------------------------------------------------------
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)          # tests/test_hip_call_trace.py
C1 = dict(cdim=3, zdim=10, channels=(64, 128, 256), image_size=32)
TRACE_BATCH, TRACE_GROUPS = 8, 2                                            # batch 8; a batched pass stacks two groups


def upsampled_convs(arch, net):
    """(dx channels, H, W) of every conv of the decoder that reads its input through the x2 upsample: H x W is the size
    of its output, which is the size of the high-resolution input gradient."""
    import models
    dec = models.Decoder(arch, net["cdim"], net["zdim"], net["channels"], net["image_size"])
    out, size = [], dec.conv_input_size[-1]
    for k, name in enumerate(dec._stages):
        if k:
            size *= 2
            blk = getattr(dec.main, name)
            out += [(m.in_channels, size, size) for m in blk.modules() if isinstance(m, models.HipConv2d)
                    and m in (getattr(blk, "conv1", None), getattr(blk, "conv_expand", None))]
    assert size == net["image_size"] and len(out) >= len(net["channels"])
    return out


@pytest.mark.parametrize("arch,net", [("conv", TINY), ("conv", C1), ("res", C1)])
def test_pinned_steps_stay_below_the_default_threshold(arch, net):
    from hipvae import functional as HF
    worst = max(TRACE_BATCH * TRACE_GROUPS * c * h * w * 4 for c, h, w in upsampled_convs(arch, net))
    assert worst < HF.UP2_FOLD_MIN_BYTES[0] == 32 << 20
    assert worst <= 8 << 20          # a quarter of the threshold
