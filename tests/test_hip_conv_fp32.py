"""The exact-fp32 gather GEMMs (conv_igemm.hip: conv_fwd_kernel, conv_wgrad_kernel and their split-K reduces), the direct
kernels (conv_small.hip) and the in-kernel-split kernels against an fp64 CPU reference, in every form they launch: the
tables of conv_cases.py, which test_conv_cases_host.py proves complete on the CPU.

Tables A and B go through the ABI wrappers (pack_weight + conv_fwd_raw, conv_wgrad_raw), so the gather GEMMs also run
the shapes conv_apply routes to the direct kernels, and are tied bit for bit to what Conv2dFn computes in fp32 mode
wherever it runs the same kernel.  Table C calls the direct kernels' entry points, table D conv_apply / conv_wgrad_raw
under bf16x3 and bf16x6.

Bars (max |err| / max |ref| per array): 2e-5 for the exact-fp32 kernels, the direct kernels and bf16x6, 5e-5 for bf16x3
(DESIGN.md section 5).  Under it every array of the exact-fp32 and direct kernels is held to max(4 * e32, 2^-22) with e32
the error of PyTorch's fp32 CPU convolution on the same inputs against the same fp64 reference (conv_cases.bound_of).
Every figure is printed before it is asserted ([conv] lines)."""
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

# (table, case id, array) held to the ceiling alone, with the reason: see DESIGN.md section 5
CEILING_ONLY = {}


@pytest.fixture(scope="module")
def HF():
    from hipvae import functional
    return functional


@pytest.fixture(autouse=True)
def fp32_mode(HF):
    HF.set_conv_math("fp32")
    yield
    HF.set_conv_math("fp32")


def dev():
    return torch.device("cuda:0")


def to_dev(*ts):
    return [None if t is None else t.to(dev()) for t in ts]


def check(table, cid, name, got, ref, e32=None, ceiling=cc.CEILING):
    err = cc.rel_err(got, ref)
    bar = ceiling if (e32 is None or (table, cid, name) in CEILING_ONLY) else min(ceiling, cc.bound_of(e32))
    ratio = err / e32 if e32 else float("nan")
    print(f"[conv] {table} {cid} {name}: err {err:.3e} e32 {e32 if e32 is not None else float('nan'):.3e} ratio {ratio:.2f} bar {bar:.3e}")
    assert tuple(got.shape) == tuple(ref.shape)
    assert err <= bar, (table, cid, name, err, e32, bar)


def conv2dfn(HF, r, c, accumulate_into=None):
    """Conv2dFn forward + backward on the case's inputs in the current mode -> (y, x.grad, w.grad); with
    ``accumulate_into`` the weight gradient is added into that preloaded .grad by the kernel (direct accumulation)."""
    x, w, b, dy = to_dev(r.x, r.w, r.b, r.dy)
    xd, wd = x.requires_grad_(True), w.requires_grad_(True)
    bd = None if b is None else b.requires_grad_(True)
    y = HF.Conv2dFn.apply(xd, wd, bd, bool(c.up2))
    if accumulate_into is not None:
        wd.grad = accumulate_into
        with HF.direct_grad_accumulation():
            y.backward(dy)
    else:
        y.backward(dy)
    return y.detach(), xd.grad, wd.grad


@pytest.mark.parametrize("cid,c", cc.cases("A"), ids=cc.ids("A"))
def test_forward_gemm(HF, cid, c):
    """itcv_conv2d_fwd in both packings: the forward Ci -> Co and the data gradient Co -> Ci on dy."""
    from hipvae import abi
    r = cc.reference(c)
    x, w, b, dy = to_dev(r.x, r.w, r.b, r.dy)
    y = HF.conv_fwd_raw(x, HF.pack_weight(w, 0), b, c.B, c.Ci, c.H, c.W, c.Co, c.KS, c.up2)
    dxu = HF.conv_fwd_raw(dy, HF.pack_weight(w, 1), None, c.B, c.Co, c.H, c.W, c.Ci, c.KS, 0)
    check("A", cid, "y", y, r.y, r.e32["y"])
    check("A", cid, "dx", dxu, r.dxu, r.e32["dxu"])
    # the path the models use: bit for bit where Conv2dFn runs the same kernel
    route = HF.conv_route(c.B, c.Ci, c.H, c.W, c.Co, c.KS, bool(c.up2), bool(c.bias), True)
    y2, dx2, _ = conv2dfn(HF, r, c)
    if route.fwd == "fp32":
        assert torch.equal(y2, y)
    else:
        assert route.fwd in ("small_cout", "small_cin") and min(c.Ci, c.Co) <= 4
    if route.dgrad == "fp32":
        if c.up2:      # Conv2dFn hands back the gradient of the low-resolution input: the adjoint of the upsampling on top
            lo = torch.empty_like(dx2)
            abi.call("itcv_upsample2_bwd", abi.ptr(dxu), abi.ptr(lo), c.B * c.Ci, c.H // 2, c.W // 2, abi.stream())
            assert torch.equal(dx2, lo)
        else:
            assert torch.equal(dx2, dxu)
    else:
        assert route.dgrad in ("small_cout", "small_cin") and min(c.Ci, c.Co) <= 4
    check("A", cid, "dx(Conv2dFn)", dx2, r.dx, None)


TAIL_CASES = [(cid, c) for cid, c in cc.cases("A") if c.B > 1 and (c.Ci & 15 or c.Co & 15)]


@pytest.mark.parametrize("cid,c", TAIL_CASES, ids=[t[0] for t in TAIL_CASES])
def test_padded_channel_rows_are_not_read(HF, cid, c):
    """Reduction channels % 16 != 0: the K tile's padded channel rows lie, in memory, on the next image's first channels.
    Their packed weights are zero, so only a value that is not finite shows a read: with every later image NaN, image 0's
    output is bit for bit what it was.  In both packings: the forward where Ci % 16 != 0, the data gradient on dy where
    Co % 16 != 0."""
    r = cc.reference(c)
    x, w, b, dy = to_dev(r.x, r.w, r.b, r.dy)
    runs = []
    if c.Ci & 15:
        runs.append((x, HF.pack_weight(w, 0), b, c.Ci, c.Co, c.up2))
    if c.Co & 15:
        runs.append((dy, HF.pack_weight(w, 1), None, c.Co, c.Ci, 0))
    assert runs
    for t, wp, bias, ci, co, up2 in runs:
        y = HF.conv_fwd_raw(t, wp, bias, c.B, ci, c.H, c.W, co, c.KS, up2)
        tn = t.clone()
        tn[1:] = float("nan")
        yn = HF.conv_fwd_raw(tn, wp, bias, c.B, ci, c.H, c.W, co, c.KS, up2)
        assert bool(torch.isfinite(yn[0]).all()) and torch.equal(yn[0], y[0])
        assert bool(torch.isnan(yn[1:]).all())


@pytest.mark.parametrize("cid,c", cc.cases("B"), ids=cc.ids("B"))
def test_weight_gradient(HF, cid, c):
    """itcv_conv2d_wgrad (conv_wgrad_kernel + either split-K reduce), fresh and added into a preloaded target."""
    r = cc.reference(c)
    x, dy, dw0 = to_dev(r.x, r.dy, r.dw0)
    dw = HF.conv_wgrad_raw(x, dy, c.B, c.Ci, c.H, c.W, c.Co, c.KS, c.up2, out=None if dw0 is None else dw0.clone(),
                           accumulate=bool(c.accumulate))
    check("B", cid, "dw", dw, r.dw, r.e32["dw"])
    # Conv2dFn's weight gradient in fp32 mode is this kernel for every shape
    assert HF.conv_route(c.B, c.Ci, c.H, c.W, c.Co, c.KS, bool(c.up2), False, True).wgrad == "raw"
    _, _, dw2 = conv2dfn(HF, r, c, accumulate_into=None if dw0 is None else dw0.clone())
    assert torch.equal(dw2, dw)


@pytest.mark.parametrize("cid,c", cc.cases("C_cout"), ids=cc.ids("C_cout"))
def test_direct_kernels_few_outputs(HF, cid, c):
    """A layer with <= 4 output channels: forward on small_cout<KS, Co>, data gradient on small_cin<KS, Co, DGRAD>."""
    from hipvae import abi
    r = cc.reference(c)
    x, w, b, dy = to_dev(r.x, r.w, r.b, r.dy)
    y, dx = torch.empty(r.y.shape, device=dev()), torch.empty(r.dxu.shape, device=dev())
    abi.call("itcv_conv2d_small_cout_fwd", abi.ptr(x), abi.ptr(w), abi.ptr(b), abi.ptr(y), c.B, c.Ci, c.H, c.W, c.Co, c.KS, 0,
             abi.stream())
    abi.call("itcv_conv2d_small_cin_fwd", abi.ptr(dy), abi.ptr(w), None, abi.ptr(dx), c.B, c.Co, c.H, c.W, c.Ci, c.KS, 1,
             abi.stream())
    check("C", cid, "y", y, r.y, r.e32["y"])
    check("C", cid, "dx", dx, r.dxu, r.e32["dxu"])
    route = HF.conv_route(c.B, c.Ci, c.H, c.W, c.Co, c.KS, False, bool(c.bias), True)
    y2, dx2, _ = conv2dfn(HF, r, c)
    assert route.fwd == "small_cout" and torch.equal(y2, y)
    if route.dgrad == "small_cin":
        assert torch.equal(dx2, dx)
    else:
        assert route.dgrad == "small_cout" and c.Ci <= 4


@pytest.mark.parametrize("cid,c", cc.cases("C_cin"), ids=cc.ids("C_cin"))
def test_direct_kernels_few_inputs(HF, cid, c):
    """A layer with <= 4 input channels: forward on small_cin<KS, Ci>, data gradient on small_cout<KS, Ci, DGRAD> (its
    reduction runs over the layer's Co channels, and the weight's inner dimension is not the template's channel count)."""
    from hipvae import abi
    r = cc.reference(c)
    x, w, b, dy = to_dev(r.x, r.w, r.b, r.dy)
    y, dx = torch.empty(r.y.shape, device=dev()), torch.empty(r.dxu.shape, device=dev())
    abi.call("itcv_conv2d_small_cin_fwd", abi.ptr(x), abi.ptr(w), abi.ptr(b), abi.ptr(y), c.B, c.Ci, c.H, c.W, c.Co, c.KS, 0,
             abi.stream())
    abi.call("itcv_conv2d_small_cout_fwd", abi.ptr(dy), abi.ptr(w), None, abi.ptr(dx), c.B, c.Co, c.H, c.W, c.Ci, c.KS, 1,
             abi.stream())
    check("C", cid, "y", y, r.y, r.e32["y"])
    check("C", cid, "dx", dx, r.dxu, r.e32["dxu"])
    route = HF.conv_route(c.B, c.Ci, c.H, c.W, c.Co, c.KS, False, bool(c.bias), True)
    y2, dx2, _ = conv2dfn(HF, r, c)
    assert route.dgrad == "small_cout" and torch.equal(dx2, dx)
    if route.fwd == "small_cin":
        assert torch.equal(y2, y)
    else:
        assert route.fwd == "small_cout" and c.Co <= 4


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x6"])
@pytest.mark.parametrize("cid,c", cc.cases("D"), ids=cc.ids("D"))
def test_in_kernel_split(HF, mode, cid, c):
    """The 'split' route of conv_apply (forward, data gradient) and of conv_wgrad_raw on the fp32 tensors."""
    r = cc.reference(c)
    x, w, b, dy, dw0 = to_dev(r.x, r.w, r.b, r.dy, r.dw0)
    HF.set_conv_math(mode)
    fmt = {"bf16x3": 2, "bf16x6": 3}[mode]
    ceiling = cc.CEILING_BF16X3 if mode == "bf16x3" else cc.CEILING
    tag = f"D/{mode}"
    assert HF._gemm_kernels(c.Ci, c.Co, c.KS, c.W, bool(c.up2), fmt, True)[1] == "split"
    y = HF.conv_apply(x, w, w, 0, b, c.B, c.Ci, c.H, c.W, c.Co, c.KS, bool(c.up2))
    check(tag, cid, "y", y, r.y, None, ceiling)
    if HF.lib.itcv_conv2d_bf16s_supported(c.Co, c.Ci, c.KS):
        assert HF._gemm_kernels(c.Co, c.Ci, c.KS, c.W, False, fmt, True)[1] == "split"
        dxu = HF.conv_apply(dy, w, w, 1, None, c.B, c.Co, c.H, c.W, c.Ci, c.KS, False)
        check(tag, cid, "dx", dxu, r.dxu, None, ceiling)
    # (a width that is no multiple of 8 leaves the weight gradient on the exact-fp32 kernel: still held to the mode's bar)
    dw = HF.conv_wgrad_raw(x, dy, c.B, c.Ci, c.H, c.W, c.Co, c.KS, c.up2, out=None if dw0 is None else dw0.clone(),
                           accumulate=bool(c.accumulate))
    check(tag, cid, "dw", dw, r.dw, None, ceiling)


# one shape per reduce kernel and the swapped shape
TWICE = [("reduce-9-slices", (6, 8, 20, 20, 16, 3, 0, 1, 1)), ("small-reduce-32-slices", (2, 3, 64, 64, 64, 5, 0, 1, 1)),
         ("swapped", (2, 64, 8, 8, 3, 5, 0, 1, 1))]


@pytest.mark.parametrize("cid,shape", TWICE, ids=[t[0] for t in TWICE])
def test_conv2dfn_backpropagates_twice_into_grad(HF, cid, shape):
    """Two backward passes add into the same preloaded .grad inside the kernels (Conv2dFn.backward's accumulate path)."""
    c = cc.Case(*shape)
    r1, r2 = cc.reference(c), cc.reference(c, 1)        # same shape, other draws
    want = r1.dw + (r2.dw - r2.dw0.double())            # dw0 + dw(x1, dy1) + dw(x2, dy2)
    db0 = torch.randn(c.Co, generator=torch.Generator().manual_seed(cc.seed_of(c, 2)))
    want_b = db0.double() + r1.dy.double().sum((0, 2, 3)) + r2.dy.double().sum((0, 2, 3))
    w = r1.w.to(dev()).requires_grad_(True)
    b = r1.b.to(dev()).requires_grad_(True)
    w.grad, b.grad = r1.dw0.to(dev()).clone(), db0.to(dev())
    grad_w, grad_b = w.grad, b.grad
    for r in (r1, r2):
        x, dy = to_dev(r.x, r.dy)
        y = HF.Conv2dFn.apply(x.requires_grad_(True), w, b, False)
        with HF.direct_grad_accumulation():
            y.backward(dy)
    assert w.grad.data_ptr() == grad_w.data_ptr() and b.grad.data_ptr() == grad_b.data_ptr()    # added in place by the kernels
    # the yardstick: the same sum by the fp32 CPU operator, dw0 + dw(x1, dy1) + dw(x2, dy2) added in fp32
    e32 = cc.rel_err(r1.dw0 + cc.dw_fp32(r1, c) + cc.dw_fp32(r2, c), want)
    check("twice", cid, "dw", w.grad, want, e32)
    check("twice", cid, "db", b.grad, want_b, None)


def test_refusals_launch_nothing(HF):
    """Bad arguments raise HipExtensionError before anything is launched: the output keeps its sentinel."""
    from hipvae import abi
    lib, call, ptr = HF.lib, abi.call, abi.ptr
    B, Ci, H, W, Co = 2, 64, 4, 4, 8
    x = torch.randn(B, Ci, H, W, device=dev())
    dy = torch.randn(B, Co, H, W, device=dev())
    wp = torch.zeros(49 * 64 * 128, device=dev())
    big = torch.empty(1 << 22, dtype=torch.uint8, device=dev())
    y = torch.full((B, Co, H, W), 7.0, device=dev())
    dw = torch.full((Co, Ci, 7, 7), 7.0, device=dev())
    w5 = torch.randn(5, 5, 5, 5, device=dev())
    st = abi.stream()
    fwd_ws, wg_ws = lib.itcv_conv2d_fwd_workspace(B, Ci, H, W, Co, 3), lib.itcv_conv2d_wgrad_workspace(B, Ci, H, W, Co, 3)
    assert fwd_ws > 0 and wg_ws > 0
    refused = [
        ("itcv_conv2d_fwd", (ptr(x), ptr(wp), None, ptr(y), B, Ci, H, W, Co, 2, 0, ptr(big), big.numel(), st)),
        ("itcv_conv2d_fwd", (ptr(x), ptr(wp), None, ptr(y), B, Ci, H, W, Co, 7, 0, ptr(big), big.numel(), st)),
        ("itcv_conv2d_wgrad", (ptr(x), ptr(dy), ptr(dw), B, Ci, H, W, Co, 2, 0, 0, ptr(big), big.numel(), st)),
        ("itcv_conv2d_wgrad", (ptr(x), ptr(dy), ptr(dw), B, Ci, H, W, Co, 7, 0, 0, ptr(big), big.numel(), st)),
        # up2 with an odd H (3 x 4 output from a 1.5-row source)
        ("itcv_conv2d_fwd", (ptr(x), ptr(wp), None, ptr(y), B, Ci, 3, W, Co, 3, 1, ptr(big), big.numel(), st)),
        ("itcv_conv2d_wgrad", (ptr(x), ptr(dy), ptr(dw), B, Ci, 3, W, Co, 3, 1, 0, ptr(big), big.numel(), st)),
        # a workspace one byte short
        ("itcv_conv2d_fwd", (ptr(x), ptr(wp), None, ptr(y), B, Ci, H, W, Co, 3, 0, ptr(big), fwd_ws - 1, st)),
        ("itcv_conv2d_wgrad", (ptr(x), ptr(dy), ptr(dw), B, Ci, H, W, Co, 3, 0, 0, ptr(big), wg_ws - 1, st)),
        # the direct kernels at 5 channels, at KS = 1
        ("itcv_conv2d_small_cout_fwd", (ptr(x), ptr(w5), None, ptr(y), B, Ci, H, W, 5, 3, 0, st)),
        ("itcv_conv2d_small_cout_fwd", (ptr(x), ptr(w5), None, ptr(y), B, Ci, H, W, 3, 1, 0, st)),
        ("itcv_conv2d_small_cin_fwd", (ptr(x), ptr(w5), None, ptr(y), B, 5, H, W, Co, 3, 0, st)),
        ("itcv_conv2d_small_cin_fwd", (ptr(x), ptr(w5), None, ptr(y), B, 3, H, W, Co, 1, 0, st)),
    ]
    for name, args in refused:
        with pytest.raises(abi.HipExtensionError):
            call(name, *args)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((dw == 7.0).all())
    # and the same calls with the right arguments go through
    call("itcv_conv2d_fwd", ptr(x), ptr(wp), None, ptr(y), B, Ci, H, W, Co, 3, 0, ptr(big), fwd_ws, st)
    call("itcv_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), B, Ci, H, W, Co, 3, 0, 0, ptr(big), wg_ws, st)
    torch.cuda.synchronize()
    assert bool((y == 0.0).all()) and not bool((dw.flatten()[:Co * Ci * 9] == 7.0).any())
