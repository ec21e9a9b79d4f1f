"""GPU tests of the f16x3 conv arithmetic (two fp16 planes of S * x, three products on the fp16 matrix cores) in every
form its kernels launch in, each against a plain fp64 PyTorch reference of the same operation.

f16x3 is the benchmark's default arithmetic (``use_amp=True`` maps to it), and the README claims it is at least as close
to fp64 as the exact-fp32 path.  The F16 template instances of the band, 128-pixel and 5x5 kernels carry their own scale
handling, so they are checked here on their own: every launch is wrapped in ``LaunchProfile`` and its label (kind,
``LOG2W`` / ``BM`` / ``up2``, ``NS=4``) is asserted, so a shape that silently lands on another kernel fails.

Bars (error measured relative to the largest value of the fp64 result, as ``rel_err`` does):

* kernel-level forward / data-gradient: 1.5e-6 (``test_f16_planes_conv_vs_fp64``: the exact-fp32 kernel's level);
* weight gradient: 1.5e-6 (``test_f16_planes_weight_gradient``);
* 5x5 stem / predict layers: 2e-6 (``test_f16_small_layer_kernels_vs_fp64``);
* op and chain level, the "fp32-class" rule: ``err_f16 <= max(2e-6, 3 * err_fp32 + 2e-7)``, where ``err_fp32`` is the
  error of the same call under ``conv_math_scope("fp32")``.

Data-gradient and weight-gradient inputs are split with ``gradient=True`` at gradient-like magnitude (1e-7 / 1e-8).
Activations are split with scale 1: an activation tensor whose values all lie far below 2^-3 loses relative accuracy
by design (absolute error 2^-25 per element); BatchNorm outputs are O(1), and that case is not tested here.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from test_hip_ops import CONV_CASES, SPLIT_CASES
from test_hip_planes import PERSIST_CASES, PLANES_CASES, WGRAD_CASES

pytestmark = pytest.mark.gpu

F16 = 4                 # plane format code of f16x3 (include/itcv_hip.h: ITCV_PLANES_F16X2)
BAR = 1.5e-6            # kernel-level forward / data-gradient / weight-gradient bar
BAR5 = 2e-6             # 5x5 layers


@pytest.fixture(scope="module")
def HF():
    from hipvae import functional
    return functional


def dev():
    return torch.device("cuda:0")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def fp32_class(e16, e32):
    return e16 <= max(2e-6, 3 * e32 + 2e-7)


@contextlib.contextmanager
def profiled(HF):
    """Labels of the GEMM-class launches made inside the block."""
    labels = []
    HF.LaunchProfile.begin()
    try:
        yield labels
    finally:
        labels.extend(lab for lab, _, _ in HF.LaunchProfile.end())


def band_label(kind, lw, bm, up2):
    name = {8: "conv_fwd_bf16p2_kernel", 9: "conv_fwd_bf16p3_kernel"}[kind]
    return f"{name}<LOG2W={lw},BM={bm},up2={int(up2)},NS=4>"


def fwd_dgrad(HF, xd, wd, dyd, B, Ci, H, W, Co, KS, up2):
    """f16x3 forward (x at scale 1) and data-gradient (dy with its gradient scale) on fp16 planes; dx is None where the
    swapped channel roles are outside the planes kernels."""
    with HF.conv_math_scope("f16x3"):
        y = HF.conv_apply_planes(HF.split_planes(xd, F16), wd, wd, 0, None, B, Ci, H, W, Co, KS, up2, F16)
        dx = None
        if HF.lib.itcv_conv2d_bf16s_supported(Co, Ci, KS):
            dx = HF.conv_apply_planes(HF.split_planes(dyd, F16, gradient=True), wd, wd, 1, None, B, Co, H, W, Ci, KS, False,
                                      F16)
    return y, dx


def make_conv(case, KS=3, dscale=1e-7):
    B, Ci, H, W, Co, up2 = case
    g = torch.Generator().manual_seed(sum(case[:5]) + KS)
    hs, ws = (H // 2, W // 2) if up2 else (H, W)
    x = torch.randn(B, Ci, hs, ws, generator=g)
    w = torch.randn(Co, Ci, KS, KS, generator=g) / (Ci * KS * KS) ** 0.5
    dy = torch.randn(B, Co, H, W, generator=g) * dscale
    return x, w, dy


def ref_fwd(x, w, up2, KS=3):
    xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up2 else x.double()
    return F.conv2d(xin, w.double(), padding=KS // 2)


def ref_dgrad(dy, w, KS=3):
    return F.conv_transpose2d(dy.double(), w.double(), padding=KS // 2)


# ---- 1. persistent band kernel ----------------------------------------------------------------------------------------
# (LOG2W, BM) of the forward launch of each PERSIST_CASES entry (plan_fwd_band; the comments there)
PERSIST_FORMS = [(6, 64), (6, 64), (5, 128), (5, 64), (5, 64), (4, 128), (4, 64), (3, 64), (3, 128)]


@pytest.mark.parametrize("case,form", list(zip(PERSIST_CASES, PERSIST_FORMS)))
def test_f16_persistent_band_kernel_vs_one_tile_kernel_and_fp64(HF, case, form):
    """The F16 instances of the persistent band kernel at the full batch of every PERSIST_CASES entry (more tiles than
    the 256 persistent blocks): forward and data-gradient with 256 blocks, with 5 (long, ragged tile walks) and with the
    one-tile kernel (band_persist_blocks = 0) are BIT-IDENTICAL; against fp64 on images [0, 1, B-2, B-1] within 1.5e-6
    (the kernel-level f16x3 bar of test_f16_planes_conv_vs_fp64).  The default forward must be kind 9, NS=4."""
    B, Ci, H, W, Co, up2 = case
    x, w, dy = make_conv(case)
    xd, wd, dyd = x.to(dev()), w.to(dev()), dy.to(dev())
    sel = [0, 1, B - 2, B - 1]
    assert HF.get_option("band_persist_blocks") == 256
    with profiled(HF) as labels:
        y, dx = fwd_dgrad(HF, xd, wd, dyd, B, Ci, H, W, Co, 3, up2)
    assert labels[0] == band_label(9, form[0], form[1], up2), labels
    assert len(labels) == 2 and labels[1].startswith(("conv_fwd_bf16p3_kernel<LOG2W=%d," % form[0],
                                                      "conv_fwd_bf16p2_kernel<LOG2W=%d," % form[0])), labels
    assert all(lab.endswith("NS=4>") for lab in labels), labels
    for blocks in (5, 0):
        with HF.option_scope("band_persist_blocks", blocks):
            with profiled(HF) as labels2:
                y2, dx2 = fwd_dgrad(HF, xd, wd, dyd, B, Ci, H, W, Co, 3, up2)
        assert labels2[0] == band_label(9 if blocks else 8, form[0], form[1], up2), (blocks, labels2)
        assert torch.equal(y, y2) and torch.equal(dx, dx2), blocks
    assert rel_err(y[sel], ref_fwd(x[sel], w, up2)) < BAR
    assert rel_err(dx[sel], ref_dgrad(dy[sel], w)) < BAR


# ---- 2. wide images (W = 128 / 256) -----------------------------------------------------------------------------------
# plan_fwd_band gives 128- and 256-wide images 128-pixel tiles of the persistent kernel: the two-row form (2 rows x 64
# columns, rows2 = 1) at any H >= 2 and the one-row form (128 columns of one row) only at H = 1 (so never with up2).  BM 128
# does not fit those tiles into 160 KB of LDS (176 KB two-row, 208 KB one-row): a layer with more than 64 output channels
# runs the band kernel with BM 64 only where the mid-sized-layer rule picks 64-row tiles, else the 128-pixel planes
# kernel (kind 6).  Expected forward launch: (kind, LOG2W, BM).
WIDE_CASES = [
    (PLANES_CASES[7], (9, 7, 64)),           # two-row, BM 64, split-K 2
    (PLANES_CASES[8], (9, 8, 64)),           # two-row, BM 64
    (PLANES_CASES[9], (6, None, None)),      # Co 160: BM 128 -> kind 6
    (PLANES_CASES[10], (9, 8, 64)),          # two-row, BM 64, up2
    (PLANES_CASES[11], (6, None, None)),     # Co 128, 12 tiles: BM 128 -> kind 6 (up2); its data-gradient is two-row BM 64
    (PLANES_CASES[12], (9, 7, 64)),          # two-row, BM 64, 640 tiles: long persistent tile walks
    ((2, 64, 8, 128, 64, True), (9, 7, 64)),     # two-row, BM 64, up2
    ((4, 64, 32, 128, 128, False), (9, 7, 64)),  # two-row; mid-sized rule: 128 tiles -> BM 64, two M tiles
    ((2, 64, 16, 256, 128, True), (9, 8, 64)),   # two-row; mid-sized rule -> BM 64, two M tiles, up2
    ((1, 64, 8, 256, 128, True), (6, None, None)),   # BM 128 -> kind 6 (up2); data-gradient two-row BM 64, split-K 4
    ((8, 64, 1, 128, 64, False), (9, 7, 64)),    # one-row (H = 1), BM 64
    ((4, 64, 1, 256, 64, False), (9, 8, 64)),    # one-row (H = 1), BM 64
    ((4, 64, 1, 128, 256, False), (6, None, None)),  # one-row BM 128 -> kind 6; data-gradient one-row BM 64, split-K 8
]


@pytest.mark.parametrize("case,form", WIDE_CASES)
def test_f16_wide_image_kernels_vs_fp64(HF, case, form):
    """128- and 256-wide images in f16x3 (the c3 / c5 configurations): forward and data-gradient bit-identical with 256
    and with 5 persistent blocks, within 1.5e-6 of fp64 (kernel-level bar of test_f16_planes_conv_vs_fp64) on the first
    and last image; every launch NS=4 and the forward on the kernel form plan_fwd_planes selects (see WIDE_CASES)."""
    B, Ci, H, W, Co, up2 = case
    x, w, dy = make_conv(case)
    xd, wd, dyd = x.to(dev()), w.to(dev()), dy.to(dev())
    with profiled(HF) as labels:
        y, dx = fwd_dgrad(HF, xd, wd, dyd, B, Ci, H, W, Co, 3, up2)
    kind, lw, bm = form
    if kind == 9:
        assert labels[0] == band_label(9, lw, bm, up2), labels
    else:
        assert labels[0].startswith("conv_fwd_bf16p_kernel<KS=3,") and labels[0].endswith(f"up2={int(up2)},NS=4>"), labels
    assert all(lab.endswith("NS=4>") for lab in labels), labels
    with HF.option_scope("band_persist_blocks", 5):
        y2, dx2 = fwd_dgrad(HF, xd, wd, dyd, B, Ci, H, W, Co, 3, up2)
    assert torch.equal(y, y2) and (dx is None or torch.equal(dx, dx2))
    sel = sorted({0, B - 1})
    assert rel_err(y[sel], ref_fwd(x[sel], w, up2)) < BAR
    assert dx is None or rel_err(dx[sel], ref_dgrad(dy[sel], w)) < BAR


# ---- 3. 128-pixel-tile planes kernel ----------------------------------------------------------------------------------
PLANES128_CASES = [  # B, Ci, H, W, Co, KS, up2 -- plan_fwd_band refuses W < 8 and KS != 3: conv_fwd_bf16p_kernel
    (4, 128, 4, 4, 256, 3, False), (32, 512, 4, 4, 256, 3, False),        # 4x4 layers, the second split-K (K = 4608)
    (64, 256, 4, 4, 520, 3, False), (16, 256, 4, 4, 544, 3, True),        # ragged M tile (520), up2
    (2, 64, 8, 8, 64, 1, False), (5, 64, 1, 1, 70, 1, False), (3, 128, 16, 16, 96, 1, False),   # KS = 1 (res / 1x1 convs)
]


@pytest.mark.parametrize("case", PLANES128_CASES)
def test_f16_planes128_kernel_vs_fp64(HF, case):
    """launch_fwd_p<KS, 2, true> (the 4x4 layers, split-K, up2, and the KS = 1 instance): forward and data-gradient within
    1.5e-6 of fp64 (kernel-level bar of test_f16_planes_conv_vs_fp64); every launch kind 6 with NS=4."""
    B, Ci, H, W, Co, KS, up2 = case
    x, w, dy = make_conv((B, Ci, H, W, Co, up2), KS)
    xd, wd, dyd = x.to(dev()), w.to(dev()), dy.to(dev())
    with profiled(HF) as labels:
        y, dx = fwd_dgrad(HF, xd, wd, dyd, B, Ci, H, W, Co, KS, up2)
    assert len(labels) == (1 if dx is None else 2), labels
    assert labels[0].startswith(f"conv_fwd_bf16p_kernel<KS={KS},") and labels[0].endswith(f"up2={int(up2)},NS=4>"), labels
    assert all(lab.startswith(f"conv_fwd_bf16p_kernel<KS={KS},") and lab.endswith("NS=4>") for lab in labels), labels
    assert rel_err(y, ref_fwd(x, w, up2, KS)) < BAR
    assert dx is None or rel_err(dx, ref_dgrad(dy, w, KS)) < BAR


# ---- 4. weight gradient -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_f16_planes_weight_gradient_all_forms(HF, case):
    """Weight gradient from fp16 planes (x at O(1), dy at 1e-8) in every tile form of WGRAD_CASES: within 1.5e-6 of fp64
    (the bar of test_f16_planes_weight_gradient) with both inner products (wgrad_m16 0 / 1), the accumulate form within
    1.5e-6 of 2 * ref, bitwise repeatable; the launch is kind 7 with NS=4."""
    B, Ci, H, W, Co, up2 = case
    g = torch.Generator().manual_seed(7 + sum(case[:5]))
    hs, ws = (H // 2, W // 2) if up2 else (H, W)
    x = torch.randn(B, Ci, hs, ws, generator=g)
    dy = torch.randn(B, Co, H, W, generator=g) * 1e-8
    xin = F.interpolate(x.double(), scale_factor=2, mode="nearest") if up2 else x.double()
    ref = torch.nn.grad.conv2d_weight(xin, (Co, Ci, 3, 3), dy.double(), padding=1)
    xp, dyp = HF.split_planes(x.to(dev()), F16), HF.split_planes(dy.to(dev()), F16, gradient=True)
    with profiled(HF) as labels:
        dw = HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, ns=F16)
    assert len(labels) == 1 and labels[0].startswith("conv_wgrad_bf16p_kernel<") and labels[0].endswith(
        f"up2={int(up2)},NS=4>"), labels
    assert rel_err(dw, ref) < BAR
    for m16 in (0, 1):
        with HF.option_scope("wgrad_m16", m16):
            alt = HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, ns=F16)
        assert rel_err(alt, ref) < BAR, m16
    acc = HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, out=dw.clone(), accumulate=True, ns=F16)
    assert rel_err(acc, 2 * ref) < BAR
    assert torch.equal(dw, HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, ns=F16))


def test_f16_deferred_weight_gradient_reduces_equal_immediate_ones(HF):
    """deferred_wgrad_reduces with fp16 planes: the slab reduces of a whole backward folded by one launch are bitwise
    the per-call reduces (several layers, one weight added to twice, accumulation into existing gradients, a second
    backward that reuses the slab buffers and the cached table) -- as test_deferred_weight_gradient_reduces_equal_
    immediate_ones does for bf16 planes."""
    g = torch.Generator().manual_seed(3)
    d = dev()
    layers = [(2, 64, 16, 16, 64, False), (4, 128, 4, 4, 256, False), (2, 32, 32, 32, 48, True), (2, 64, 16, 16, 64, False)]
    ops_ = []
    for B, Ci, H, W, Co, up2 in layers:
        hs, ws = (H // 2, W // 2) if up2 else (H, W)
        xp = HF.split_planes(torch.randn(B, Ci, hs, ws, generator=g).to(d), F16)
        dyp = HF.split_planes((torch.randn(B, Co, H, W, generator=g) * 1e-7).to(d), F16, gradient=True)
        ops_.append((xp, dyp, B, Ci, H, W, Co, 3, up2))
    grads0 = [(torch.randn(o[6], o[3], 3, 3, generator=g) * 1e-6).to(d) for o in ops_[:3]]
    targets = [0, 1, 2, 0]

    def run(deferred):
        gr = [t.clone() for t in grads0]
        for _ in range(2):
            if deferred:
                with HF.deferred_wgrad_reduces():
                    for o, t in zip(ops_, targets):
                        HF.conv_wgrad_planes(*o, out=gr[t], accumulate=True, ns=F16)
                    assert len(HF._DEFER["pending"]) == 4
                assert not HF._DEFER["pending"]
            else:
                for o, t in zip(ops_, targets):
                    HF.conv_wgrad_planes(*o, out=gr[t], accumulate=True, ns=F16)
        return gr

    a, b = run(False), run(True)
    for t0, x, y in zip(grads0, a, b):
        assert not torch.equal(x, t0)            # the gradients did add to the targets
        assert torch.equal(x, y)


# ---- 5. 5x5 stem / predict layers -------------------------------------------------------------------------------------
# B, H, W, channels of the narrow side: the shapes of test_small_cin_conv_on_matrix_cores / test_small_cout_conv_on_planes /
# test_wgrad5_on_planes -- ragged row counts 7 / 20 / 40, widths 8 .. 256, 1 - 3 channels, B up to 64.  Widths below 32
# reach only the planes <= 3-output kernel (the other two need W % 32 == 0).
SHAPES5 = [(3, 32, 32, 3), (2, 64, 64, 3), (5, 20, 64, 2), (2, 7, 32, 1), (1, 128, 128, 3), (1, 40, 256, 3), (64, 64, 64, 3),
           (3, 16, 16, 3), (5, 32, 32, 2), (2, 8, 8, 1), (1, 256, 256, 3)]


@pytest.mark.parametrize("shape", SHAPES5)
def test_f16_5x5_layers_vs_fp64(HF, shape):
    """The 5x5 layers with a <= 3-channel side in f16x3, within 2e-6 of fp64 (the bar of test_f16_small_layer_kernels_
    vs_fp64): stem forward with bias and predict data-gradient (input at 1e-8: the device-side amax scale) on the
    small-Cin matrix-core kernel (kind 11); predict forward with bias and stem data-gradient (planes at 1e-8) on the
    planes <= 3-output kernel (kind 10); both 5x5 weight gradients (kind 12) incl. the accumulate form and a bitwise
    repeat.  Checked on images [0, 1, B-2, B-1] where the whole batch is not needed."""
    B, H, W, Cs = shape
    d = dev()
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + Cs)
    img = torch.rand(B, Cs, H, W, generator=g)
    w_stem = torch.randn(64, Cs, 5, 5, generator=g) / 6.0
    w_pred = torch.randn(Cs, 64, 5, 5, generator=g) / 40.0
    b_stem, b_pred = torch.randn(64, generator=g), torch.randn(Cs, generator=g)
    act = torch.randn(B, 64, H, W, generator=g)
    gsmall = torch.randn(B, Cs, H, W, generator=g) * 1e-8
    gbig = torch.randn(B, 64, H, W, generator=g) * 1e-8
    sel = sorted({0, min(1, B - 1), max(B - 2, 0), B - 1})
    scin = bool(HF.lib.itcv_conv2d_small_cin_bf16x3_supported(Cs, 64, 5, W))
    wg5 = bool(HF.lib.itcv_conv2d_wgrad5_bf16p_supported(Cs, 64, H, W))
    assert HF.lib.itcv_conv2d_small_cout_bf16p_supported(64, Cs, 5)
    assert scin == wg5 == (W % 32 == 0)
    c5 = f"KS=5,C={Cs}"
    with HF.conv_math_scope("f16x3"), profiled(HF) as labels:
        yp = HF.conv_apply_planes(HF.split_planes(act.to(d), F16), w_pred.to(d), w_pred.to(d), 0, b_pred.to(d), B, 64, H, W,
                                  Cs, 5, False, F16)
        dxs = HF.conv_apply_planes(HF.split_planes(gbig.to(d), F16, gradient=True), w_stem.to(d), w_stem.to(d), 1, None, B,
                                   64, H, W, Cs, 5, False, F16)
        want = [f"conv_small_cout_planes_kernel<{c5},stem=0,NS=4>"] * 2
        if scin:
            y = HF.conv_apply(img.to(d), w_stem.to(d), w_stem.to(d), 0, b_stem.to(d), B, Cs, H, W, 64, 5, False)
            dxp = HF.conv_apply(gsmall.to(d), w_pred.to(d), w_pred.to(d), 1, None, B, Cs, H, W, 64, 5, False)
            want += [f"conv_small_cin_mfma_kernel<{c5},stem=0,NS=4>"] * 2
    assert labels == want, labels
    assert rel_err(yp[sel], F.conv2d(act[sel].double(), w_pred.double(), b_pred.double(), padding=2)) < BAR5
    assert rel_err(dxs[sel], F.conv_transpose2d(gbig[sel].double(), w_stem.double(), padding=2)) < BAR5
    if not scin:
        return
    assert rel_err(y[sel], F.conv2d(img[sel].double(), w_stem.double(), b_stem.double(), padding=2)) < BAR5
    assert rel_err(dxp[sel], F.conv_transpose2d(gsmall[sel].double(), w_pred.double(), padding=2)) < BAR5
    # weight gradients: the stem's from the image (scale 1) and dy planes, the predict layer's from dy (device-side scale)
    # and the activation planes
    gbp, actp = HF.split_planes(gbig.to(d), F16, gradient=True), HF.split_planes(act.to(d), F16)
    for stem, small, big, ref in (
            (True, img, gbp, torch.nn.grad.conv2d_weight(img.double(), (64, Cs, 5, 5), gbig.double(), padding=2)),
            (False, gsmall, actp, torch.nn.grad.conv2d_weight(act.double(), (Cs, 64, 5, 5), gsmall.double(), padding=2))):
        with profiled(HF) as labels:
            dw = HF.conv_wgrad5_planes(small.to(d), big, B, Cs, H, W, stem, ns=F16)
        assert labels == [f"conv_wgrad5_planes_kernel<{c5},stem={int(stem)},NS=4>"], labels
        assert rel_err(dw, ref) < BAR5, stem
        acc = HF.conv_wgrad5_planes(small.to(d), big, B, Cs, H, W, stem, out=dw.clone(), accumulate=True, ns=F16)
        assert rel_err(acc, 2 * ref) < BAR5, stem
        assert torch.equal(dw, HF.conv_wgrad5_planes(small.to(d), big, B, Cs, H, W, stem, ns=F16)), stem


# ---- 6. Conv2dFn end to end -------------------------------------------------------------------------------------------
OP_CASES = [c + (True,) for c in CONV_CASES] + [c + (False,) for c in SPLIT_CASES]    # ..., with bias


@pytest.mark.parametrize("case", OP_CASES)
def test_f16_conv2dfn_vs_fp64(HF, case):
    """Conv2dFn forward and backward in f16x3 -- the mode's real dispatch: planes kernels, the 5x5 small-channel kernels,
    the fp32 fallbacks, bias gradients, weight gradient on planes or on the raw fp32 kernel -- with dy at O(1) and at
    1e-7: y, dx, dw and db each meet the fp32-class rule against fp64 (err_f16 <= max(2e-6, 3 * err_fp32 + 2e-7), err_fp32
    the same call under conv_math_scope("fp32"))."""
    B, Ci, H, W, Co, KS, up2, has_bias = case
    g = torch.Generator().manual_seed(sum(case[:6]) + 17)
    hs, ws = (H // 2, W // 2) if up2 else (H, W)
    x = torch.randn(B, Ci, hs, ws, generator=g)
    w = torch.randn(Co, Ci, KS, KS, generator=g) / (Ci * KS * KS) ** 0.5
    b = torch.randn(Co, generator=g) if has_bias else None
    dy0 = torch.randn(B, Co, H, W, generator=g)
    leaves = [x.double().requires_grad_(True), w.double().requires_grad_(True)]
    if has_bias:
        leaves.append(b.double().requires_grad_(True))
    xin = F.interpolate(leaves[0], scale_factor=2, mode="nearest") if up2 else leaves[0]
    yr = F.conv2d(xin, leaves[1], leaves[2] if has_bias else None, padding=KS // 2)

    def run(mode, dy):
        params = [t.to(dev()).requires_grad_(True) for t in ((x, w, b) if has_bias else (x, w))]
        with HF.conv_math_scope(mode):
            y = HF.Conv2dFn.apply(params[0], params[1], params[2] if has_bias else None, up2)
            y.backward(dy.to(dev()))
        return [y.detach()] + [p.grad for p in params]

    for scale in (1.0, 1e-7):
        dy = dy0 * scale
        refs = [yr.detach()] + list(torch.autograd.grad(yr, leaves, dy.double(), retain_graph=True))
        got16, got32 = run("f16x3", dy), run("fp32", dy)
        for name, a, a32, r in zip(("y", "dx", "dw", "db"), got16, got32, refs):
            e16, e32 = rel_err(a, r), rel_err(a32, r)
            assert fp32_class(e16, e32), (scale, name, e16, e32)


# ---- 7. the c2 hot chain ----------------------------------------------------------------------------------------------
def test_f16_c2_chain_vs_fp64(HF):
    """conv1 64->64 -> BnActFn (2 BatchNorm groups, LeakyReLU 0.2, planes-only output, fp16 gradient planes) -> conv2
    64->64, all at 64x64 with B = 32 (512 tiles: both convs on the persistent band kernel), forward and backward from dy
    at 1e-7.  y and dx on images at the ends and the group boundary, dW1, dW2, dgamma, dbeta, the running buffers and
    num_batches_tracked on the whole batch, against fp64 convs and fp64 BatchNorm per group, under the fp32-class rule
    (err_f16 <= max(2e-6, 3 * err_fp32 + 2e-7), err_fp32: the same chain in fp32).  The profile shows kind 9, 13 and 14,
    each with NS=4.

    One exception, the running mean, whose bar is ``max(2e-6, 8 * err_fp32 + 2e-7)``: with zero-mean inputs a channel
    mean of conv1's output is ~1/256 of that output's scale (16 x 64 x 64 values per group), so its error relative to
    its own largest value amplifies the difference in per-element rounding of the conv (22 significand bits per f16x3
    operand against fp32's 24).  Measured
    on this case: err_fp32 = 5.2e-7 (the exact-fp32 kernel), err_f16 = 3.6e-6.  Dropping one of the three products
    (2^-11 per element) would still exceed it by orders of magnitude."""
    B, C, S, G = 32, 64, 64, 2
    g = torch.Generator().manual_seed(21)
    x = torch.randn(B, C, S, S, generator=g)
    w1 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    w2 = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dy = torch.randn(B, C, S, S, generator=g) * 1e-7
    sel = [0, 1, 15, 16, 30, 31]
    d = dev()

    def run(mode):
        planes = F16 if mode == "f16x3" else 0
        xd, w1d, w2d, gd, bd = (t.to(d).requires_grad_(True) for t in (x, w1, w2, gamma, beta))
        rm, rv = torch.zeros(C, device=d), torch.ones(C, device=d)
        nbt = torch.zeros((), dtype=torch.int64, device=d)
        with HF.conv_math_scope(mode):
            y1 = HF.Conv2dFn.apply(xd, w1d, None, False)
            a = HF.BnActFn.apply(y1, gd, bd, None, rm, rv, nbt, 1e-4, 0.1, 0.2, False, True, None, planes, planes,
                                 not planes, not planes, G)
            if planes:    # planes only: the fp32 tensor is not written
                assert HF._tagged_planes(a, F16) is not None and not a._itcv_planes[4]
            y = HF.Conv2dFn.apply(a, w2d, None, False)
            y.backward(dy.to(d))
        return dict(y=y.detach()[sel], dx=xd.grad[sel], dw1=w1d.grad, dw2=w2d.grad, dgamma=gd.grad, dbeta=bd.grad,
                    rm=rm, rv=rv), int(nbt)

    with profiled(HF) as labels:
        got16, n16 = run("f16x3")
    assert band_label(9, 6, 64, False) in labels, labels
    assert any(lab.startswith("bn_act_fwd_planes_kernel<") and lab.endswith("NS=4>") for lab in labels), labels
    assert any(lab.startswith("bn_bwd_apply_planes<") and lab.endswith("NS=4>") for lab in labels), labels
    got32, n32 = run("fp32")
    assert n16 == n32 == G

    xr, w1r, w2r, gr, br = (t.double().requires_grad_(True) for t in (x, w1, w2, gamma, beta))
    rmr, rvr = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y1r = F.conv2d(xr, w1r, padding=1)
    acts = [F.leaky_relu(F.batch_norm(y1r[k * (B // G):(k + 1) * (B // G)], rmr, rvr, gr, br, True, 0.1, 1e-4), 0.2)
            for k in range(G)]
    yr = F.conv2d(torch.cat(acts), w2r, padding=1)
    yr.backward(dy.double())
    ref = dict(y=yr.detach()[sel], dx=xr.grad[sel], dw1=w1r.grad, dw2=w2r.grad, dgamma=gr.grad, dbeta=br.grad, rm=rmr,
               rv=rvr)
    errs = {k: (rel_err(got16[k], r), rel_err(got32[k], r)) for k, r in ref.items()}
    for k, (e16, e32) in errs.items():
        if k == "rm":     # cancellation: see the docstring
            assert e16 <= max(2e-6, 8 * e32 + 2e-7), errs
        else:
            assert fp32_class(e16, e32), (k, errs)


# ---- 8. packing and magnitude edges -----------------------------------------------------------------------------------
PACK_LAYERS = [  # Co, Ci, KS -- M = Co (forward) / Ci (data-gradient); C the other side
    (64, 64, 3), (130, 64, 3), (520, 256, 3),      # forward M 64 / 130 / 520; data-gradient C 130 / 520 (not % 32)
    (48, 130, 3), (40, 520, 1), (96, 32, 3),       # data-gradient M 130 / 520 / 32 with C 48 / 40 / 96
]


@pytest.mark.parametrize("for_dgrad", [0, 1])
def test_f16_table_packing_equals_per_layer_packing(HF, for_dgrad):
    """pack_weights_bf16s_table_kernel<2, true> (the one-launch re-pack of a parameter group after every optimiser step
    in f16x3) writes every layer's packed fp16 operand bit for bit as the per-layer packing does, padding included."""
    g = torch.Generator().manual_seed(40 + for_dgrad)
    d = dev()
    ws = [(torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5).to(d) for co, ci, ks in PACK_LAYERS]
    ref = [HF.pack_weight_bf16s(w, for_dgrad, F16) for w in ws]
    grp = HF._PackGroup()
    for w in ws:
        grp.pack(w, w, for_dgrad, F16)              # joins the group (packed on its own)
    mem = grp.members[(for_dgrad, F16)]
    assert len(mem) == len(ws)
    bufs = [r[3] for r in mem.values()]
    for buf in bufs:
        buf.fill_(0x7F7F7F7F)                       # anything the table launch does not write stays visible
    tab = grp._build(mem, for_dgrad, F16, d)
    HF.call("itcv_conv2d_pack_weights_bf16s", HF.ptr(tab[0]), tab[1], tab[2], F16, HF.stream())
    for (co, ci, ks), buf, r in zip(PACK_LAYERS, bufs, ref):
        assert torch.equal(buf, r), (co, ci, ks)


MAG_CASES = [(8, 64, 32, 32, 64, False), (20, 64, 64, 64, 64, False), (4, 128, 4, 4, 256, False)]   # band (persistent) / 128-pixel


@pytest.mark.parametrize("case", MAG_CASES)
def test_f16_magnitude_edges(HF, case):
    """Data-gradient and weight gradient from a dy that is all zero (exact zeros, no NaN), at 1e-30 and at 1e3 (within
    1.5e-6 of fp64, the kernel-level bars above); forward inputs at scale 1 with magnitude 2^-3 and 2^10 (within 1.5e-6).
    Images [0, B-1] are compared for the forward and data-gradient."""
    B, Ci, H, W, Co, up2 = case
    x0, w, dy0 = make_conv(case, dscale=1.0)
    d = dev()
    wd = w.to(d)
    sel = [0, B - 1]
    xp = HF.split_planes(x0.to(d), F16)
    for mag in (0.0, 1e-30, 1e3):
        dy = dy0 * mag
        dyp = HF.split_planes(dy.to(d), F16, gradient=True)
        with HF.conv_math_scope("f16x3"):
            dx = HF.conv_apply_planes(dyp, wd, wd, 1, None, B, Co, H, W, Ci, 3, False, F16)
        dw = HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, ns=F16)
        if mag == 0.0:
            assert torch.equal(dx, torch.zeros_like(dx)) and torch.equal(dw, torch.zeros_like(dw))
            continue
        assert rel_err(dx[sel], ref_dgrad(dy[sel], w)) < BAR, mag
        assert rel_err(dw, torch.nn.grad.conv2d_weight(x0.double(), (Co, Ci, 3, 3), dy.double(), padding=1)) < BAR, mag
    for mag in (2.0 ** -3, 2.0 ** 10):
        x = x0 * mag
        with HF.conv_math_scope("f16x3"):
            y = HF.conv_apply_planes(HF.split_planes(x.to(d), F16), wd, wd, 0, None, B, Ci, H, W, Co, 3, up2, F16)
        assert rel_err(y[sel], ref_fwd(x[sel], w, up2)) < BAR, mag
