"""Sub-range ("live") forms of the backward kernels against the full calls: the computation is the same, so every comparison
is ``torch.equal`` -- no tolerance.

* ``itcv_bn_train_bwd_live`` with one live group of two against ``itcv_bn_train_bwd`` on a dy whose dead group is zero:
  the live half of dx, the live half's plane chunks, the scale record and dsums, once per backward path (pinned with
  ``itcv_bn_plan_query``), fp32 only / bf16 planes / fp16 planes, plain / pool / up2, live group 0 and 1, and one case
  whose DEAD group holds the larger |xhat| (V decides the fp16 exponent).  The dead half of dx and of the planes keeps
  the NaN / sentinel it was filled with: nothing is stored there.
* ``itcv_conv2d_fwd_bf16p_sub`` used as data gradient against the full call, live images only: the split-K planes kernel
  (512 -> 512 @ 4x4, 16 images), the 8x8 layer whose plan at 64 images differs from that at 128, the up2 band kernel, a
  range that ends inside a 256-pixel tile, both ``band_m16`` settings; the 64 -> 3 predict layer's data gradient @16x16
  through ``Conv2dFn`` 's slice form.
* whole steps, c2 network: ``skip_dead_half`` on against off, fp32 and f16x3, eager and captured, B = 8 and 64; once with
  poison on.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
F16 = 4
SLOPE = 0.2


def dev():
    return torch.device("cuda:0")


# (id, Bg, C, H, W, mode, ns, planes, path)   mode: 0 plain | 1 pool | 2 up2;  ns: 0 = no planes
BN_CASES = [
    ("one-block-f16", 4, 64, 8, 8, 0, F16, True, "OneBlock"),
    ("one-block-bf16-up2", 4, 16, 4, 4, 2, 2, True, "OneBlock"),
    ("fold-f16", 8, 8, 16, 16, 0, F16, True, "SlicedFold"),
    ("fold-f16-up2", 8, 8, 16, 16, 2, F16, True, "SlicedFold"),
    ("fold-bf16-pool", 8, 8, 16, 16, 1, 2, True, "SlicedFold"),
    ("combine-f16", 32, 8, 8, 8, 0, F16, True, "SlicedCombine"),
    ("combine-f16-pool", 32, 8, 8, 8, 1, F16, True, "SlicedCombine"),
    ("per-group-fp32", 8, 8, 16, 16, 0, 0, False, "PerGroup"),
]


def _bn_bwd(entry, x, dy, mean, rstd, gamma, beta, Bg, C, H, W, mode, ns, planes, live):
    from hipvae import abi
    G = 2
    dx = torch.full_like(x, float("nan"))
    dsums = torch.full((G, 2 * C), 7.0, dtype=torch.float64, device=dev())
    nws = abi.lib.itcv_bn_workspace(Bg, C, H * W) * G
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device=dev())
    dxp, pstride = None, 0
    if planes:
        dxp = torch.full((abi.lib.itcv_planes_bytes(G * Bg, C, H * W, ns) // 4,), 0x7fc07fc0, dtype=torch.int32, device=dev())
        pstride = G * Bg * (C // 8) * H * W
    head = (abi.ptr(x), abi.ptr(dy), abi.ptr(mean), abi.ptr(rstd), abi.ptr(gamma), abi.ptr(beta), None, abi.ptr(dsums),
            abi.ptr(dx), None, abi.ptr(dxp), ns if planes else 0, None, None, 0, Bg, C, H, W, SLOPE, int(mode == 1),
            int(mode == 2), abi.ptr(ws), nws, pstride, G)
    if entry == "full":
        abi.call("itcv_bn_train_bwd", *head, abi.stream())
    else:
        abi.call("itcv_bn_train_bwd_live", *head, live, 1, abi.stream())
    torch.cuda.synchronize()
    return dx, dxp, dsums


# V = max|xhat| only exists for fp16 planes: those cases run once more with the outlier in the dead group
BN_PARAMS = [(c, live, big) for c in BN_CASES for live in (0, 1) for big in ((False, True) if c[6] == F16 else (False,))]


@pytest.mark.parametrize("case,live,dead_big", BN_PARAMS,
                         ids=[f"{c[0]}-live{l}{'-dead-holds-V' if b else ''}" for c, l, b in BN_PARAMS])
def test_bn_bwd_live_equals_full_with_zero_dy(case, live, dead_big):
    from hipvae import abi
    _, Bg, C, H, W, mode, ns, planes, path = case
    assert abi.bn_plan_query(True, Bg, C, H, W, pool=int(mode == 1), up2=int(mode == 2), groups=2, planes=planes,
                             ns=ns if planes else 2)[0] == path
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2 * Bg, C, H, W, generator=g)
    dead = 1 - live
    if dead_big:
        x[dead * Bg, 0, 0, 0] = 40.0        # an outlier of the DEAD group: its |xhat| is the tensor's V
    shp = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[mode]
    dy = torch.randn(2 * Bg, C, *shp, generator=g)
    dy[dead * Bg:(dead + 1) * Bg] = 0.0
    xg = x.view(2, Bg, C, H * W)
    mean = xg.mean(dim=(1, 3))
    rstd = (xg.var(dim=(1, 3), unbiased=False) + 1e-4).rsqrt()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    args = [t.to(dev()).contiguous() for t in (x, dy, mean, rstd, gamma, beta)]
    full = _bn_bwd("full", *args, Bg, C, H, W, mode, ns, planes, live)
    sub = _bn_bwd("live", *args, Bg, C, H, W, mode, ns, planes, live)
    r, d = slice(live * Bg, (live + 1) * Bg), slice(dead * Bg, (dead + 1) * Bg)
    assert torch.equal(sub[0][r], full[0][r])
    assert torch.isnan(sub[0][d]).all(), "the dead group's dx was written"
    assert torch.equal(sub[2], full[2]) and bool((sub[2][dead] == 0).all())
    if planes:
        np_, chunk_ints = 2 if ns in (2, F16) else 3, (C // 8) * H * W * 4
        body = 2 * Bg * chunk_ints
        for p in range(np_):
            fp, sp = full[1][p * body:(p + 1) * body].view(2, Bg * chunk_ints), sub[1][p * body:(p + 1) * body].view(2, Bg * chunk_ints)
            assert torch.equal(sp[live], fp[live])
            assert bool((sp[dead] == 0x7fc07fc0).all()), "the dead group's planes were written"
        assert torch.equal(sub[1][np_ * body:], full[1][np_ * body:])          # the scale record (fp16), else empty
        if dead_big:
            other = x.clone()
            other[dead * Bg, 0, 0, 0] = 0.0
            ref = _bn_bwd("full", other.to(dev()), *args[1:], Bg, C, H, W, mode, ns, planes, live)
            assert not torch.equal(ref[1][np_ * body:], full[1][np_ * body:]), "the case does not make V decide the scale"


# (id, Ci(dy channels), Co(dx channels), H, W, up2, images, b0, nb)
CONV_CASES = [
    ("4x4-splitk", 512, 512, 4, 4, 0, 16, 8, 8),
    ("8x8-plan-switch", 256, 256, 8, 8, 0, 128, 64, 64),
    ("8x8-first-half", 256, 256, 8, 8, 0, 128, 0, 64),
    ("16x16-up2", 64, 64, 16, 16, 1, 8, 4, 4),
    ("8x8-inside-a-tile", 64, 64, 8, 8, 0, 8, 2, 3),
    ("16x16-64to128", 128, 64, 16, 16, 0, 8, 4, 4),
]


@pytest.mark.parametrize("m16", [1, 0])
@pytest.mark.parametrize("fmt", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_dgrad_sub_range_equals_full(case, fmt, m16):
    from hipvae import functional as HF
    _, Cy, Cx, H, W, up2, B, b0, nb = case
    g = torch.Generator().manual_seed(5)
    Hs, Ws = (H // 2, W // 2) if up2 else (H, W)
    dy = torch.randn(B, Cy, Hs, Ws, generator=g).to(dev())
    w = (torch.randn(Cy, Cx, 3, 3, generator=g) * 0.05).to(dev())          # the forward layer's OIHW weight (Cx -> Cy)
    prev = HF.get_option("band_m16")
    HF.set_option("band_m16", m16)
    try:
        with HF.conv_math_scope(fmt):
            ns = HF._NS[fmt]
            dyp = HF.split_planes(dy, ns, gradient=True)
            full = HF.conv_apply_planes(dyp, w, w, 1, None, B, Cy, H, W, Cx, 3, bool(up2), ns)
            prevp, HF._POISON[0] = HF._POISON[0], True
            try:
                sub = HF.conv_apply_planes(dyp, w, w, 1, None, B, Cy, H, W, Cx, 3, bool(up2), ns, live=(b0, nb))
            finally:
                HF._POISON[0] = prevp
    finally:
        HF.set_option("band_m16", prev)
    torch.cuda.synchronize()
    assert torch.equal(sub[b0:b0 + nb], full[b0:b0 + nb])
    rest = torch.cat([sub[:b0], sub[b0 + nb:]])
    assert torch.isnan(rest).all(), "images outside the range were written"


@pytest.mark.parametrize("fmt", ["f16x3", "bf16x3", "fp32"])
def test_predict_layer_dgrad_slice_equals_full(fmt):
    """64 -> 3 5x5 @16x16: the per-image kernels on the live slice, the fp16 scale from the live maximum."""
    from hipvae import functional as HF
    g = torch.Generator().manual_seed(6)
    B, H, W = 8, 16, 16
    dy = torch.randn(B, 3, H, W, generator=g) * 1e-3
    dy[:4] = 0.0
    dy = dy.to(dev())
    w = (torch.randn(3, 64, 5, 5, generator=g) * 0.05).to(dev())
    with HF.conv_math_scope(fmt):
        full = HF.conv_apply(dy, w, w, 1, None, B, 3, H, W, 64, 5, False)
        out = torch.full((B, 64, H, W), float("nan"), device=dev())
        HF.conv_apply(dy[4:], w, w, 1, None, 4, 3, H, W, 64, 5, False, out=out[4:])
    torch.cuda.synchronize()
    assert torch.equal(out[4:], full[4:]) and torch.isnan(out[:4]).all()


# ------------------------------------------------------------------ whole steps
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
HP = dict(beta_kl=0.5, beta_rec=0.75, beta_neg=512.0, gamma_r=1e-8, clip=100.0, lr=2e-4)


class _DS:
    def __len__(self):
        return 10000


def _run(math, B, skip, graph, steps, poison=False):
    import models
    from hipvae import functional as HF
    from solvers.intro_tc import IntroTCSovler
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev()).train()
    solver = IntroTCSovler(_DS(), model, B, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                           torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", HP["beta_kl"], HP["beta_rec"],
                           HP["beta_neg"], HP["gamma_r"], dev(), math == "f16x3", None, clip=HP["clip"])
    solver.conv_math = math
    solver.skip_dead_half = skip
    if graph:
        solver.enable_graph()
    xs = [torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(10 + s)).to(dev()) for s in range(steps)]
    torch.manual_seed(1234)
    prev, HF._POISON[0] = HF._POISON[0], poison
    try:
        res = [solver.train_step(xs[s], s) for s in range(steps)]
    finally:
        HF._POISON[0] = prev
    torch.cuda.synchronize()
    if graph:
        assert solver._graph is not None, "the captured graph was not used"
        # the switch sits between the update specs (from position 3) and the schedule key; the KL mode stays last
        from hipvae.flat import fused_update
        k = solver._graph_key
        assert k[3:5] == (fused_update(solver.optimizer_e), fused_update(solver.optimizer_d))
        assert k[5:] == (skip,) + solver._schedule_key() + (solver.kl_loss,)
    blockers = list(solver._shared_pass.live_blockers)
    return res, model.state_dict(), (solver.optimizer_e.state_dict(), solver.optimizer_d.state_dict()), blockers


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("math", ["fp32", "f16x3"])
@pytest.mark.parametrize("B", [8, 64])
def test_step_skip_on_equals_skip_off(B, math, graph):
    steps = 5 if graph else 2              # captured: three eager warm-up steps, the capture, one replay
    on, off = _run(math, B, True, graph, steps), _run(math, B, False, graph, steps)
    assert _same(on[0], off[0]) and _same(on[1], off[1]) and _same(on[2], off[2])
    # f16x3: every function of the c2 decoder pass has a sub-range form; fp32: the fp32 GEMM's K split follows the launched
    # batch, the pass as a whole keeps the full walk
    assert (on[3] == []) == (math == "f16x3"), on[3]


def test_step_skip_on_equals_skip_off_poisoned():
    on, off = _run("f16x3", 8, True, False, 2, poison=True), _run("f16x3", 8, False, False, 2, poison=True)
    assert on[3] == [] and _same(on[0], off[0]) and _same(on[1], off[1]) and _same(on[2], off[2])
    assert all(v == v for r in on[0] for v in r.values() if v is not None)
