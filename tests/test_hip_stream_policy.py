"""GPU: the ``stream_nt`` option changes no byte.  A set bit of the mask (include/itcv_hip.h: ITCV_STREAM_NT_*) makes one
kernel family load / store its once-used streams non-temporally; a cache policy cannot change a value, so every output of
every touched kernel must be byte-equal with the family's bit off and on.  Each comparison runs the same call twice inside
``functional.option_scope("stream_nt", mask)`` on the same inputs and compares all outputs as bytes (NaN fill included:
a buffer a call must not write keeps its fill in both runs).

Shapes are the smallest that reach every code path of the touched kernels:

* BatchNorm apply, forward (bit BN_FWD) and backward (bit BN_APPLY): C = 16 at 8x8 and 16x16 with 3 images (OneBlock: the
  apply kernels without the STATS / SUMS fold; at 8x8 the launch has 96 threads, so the second wave is partly filled and
  stores its planes through the scalar tail), C = 16 at 32x32 (SlicedFold, plain and pooled: STATS / SUMS on),
  6 x 24 x 12 x 20 (SlicedCombine, widths that are no powers of two) and 16 x 12 x 8 x 8 without planes (Fallback:
  ``bn_act_fwd_kernel`` / ``bn_bwd_apply_v4``; two groups: PerGroup).  Modes plain / pool / up2, one and two groups, the two
  groups also with a live range of one group (first, second), planes bf16x2 / bf16x3 / f16x2, skip given and null.
* Weight gradient (bit WGRAD_SLABS: the slab stores of a deferred call) and its deferred fold (bit FOLD:
  ``wgrad_p_reduce_many``): 32 -> 32 and 64 -> 64 at 8x8 with 2 images, up2 off and on, bf16 and fp16 planes, both MFMA
  shapes; the deferred slabs are compared as they lie in the workspace and again folded by ``itcv_wgrad_reduce_many``; the
  direct call (accumulate 0 / 1: plain stores and the plain single-layer fold under any mask) must add what the deferred
  pair adds; one table with a 70-slice (fine) and a 3-slice (wide) descriptor on random slabs.
* A whole training step of a tiny network with mask 0 and with the full mask.

The 5x5 weight-gradient pair, the single-layer fold and the optimiser kernels carry no policy (their streams are hand-offs,
or the policy did not pay: DESIGN.md section 6, round 9); bits WGRAD_OPS and OPTIM are reserved and read by no kernel.
"""
import pytest
import torch

from test_hip_bn import SLOPE, case, dev, hip_fwd, make_inputs, workspace
from test_hip_wgrad_fold_bits import build_table, make_dw, make_slab

pytestmark = pytest.mark.gpu

OB, SF, SC, FB, PG = "OneBlock", "SlicedFold", "SlicedCombine", "Fallback", "PerGroup"


@pytest.fixture(scope="module")
def HF():
    from hipvae import functional
    return functional


def bit(name):
    from hipvae import abi
    return abi.STREAM_NT[name]


def raw(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def assert_same(a, b, tag):
    """Two dicts (or lists) of tensors / None: the same keys, the same bytes."""
    items = a.items() if isinstance(a, dict) else enumerate(a)
    for k, va in items:
        vb = b[k]
        assert (va is None) == (vb is None), (tag, k)
        if va is not None:
            assert va.dtype == vb.dtype and va.shape == vb.shape and torch.equal(raw(va), raw(vb)), (tag, k)


def off_on(HF, mask, run):
    """run() under stream_nt = 0 and = mask."""
    with HF.option_scope("stream_nt", 0):
        a = run()
    with HF.option_scope("stream_nt", mask):
        assert HF.get_option("stream_nt") == mask
        b = run()
    torch.cuda.synchronize()
    return a, b


# ---- BatchNorm apply passes ---------------------------------------------------------------------------------------------
def bn_bwd(HF, c, x, dy, skip, par, mean, rstd, ns, live):
    """itcv_bn_train_bwd_live on the stacked groups (live = (first, count); (0, G) is itcv_bn_train_bwd)."""
    from hipvae import abi
    B, C, H, W = c.shape
    d, GB = dev(), c.G * B
    gamma, beta, _, _, dg0, db0 = par
    nan = float("nan")
    o = dict(dx=torch.full((GB, C, H, W), nan, device=d), dskip=None if skip is None else torch.full((GB, C, H, W), nan, device=d),
             planes=None, dgamma=dg0.clone(), dbeta=db0.clone(), dsums=torch.full((c.G, 2 * C), nan, dtype=torch.float64, device=d))
    pstride = 0
    if ns:
        o["planes"] = torch.zeros(HF.lib.itcv_planes_bytes(GB, C, H * W, ns) // 4, dtype=torch.int32, device=d)
        pstride = GB * (C // 8) * H * W
    ws, nws = workspace(HF, c, "full")
    abi.call("itcv_bn_train_bwd_live", abi.ptr(x), abi.ptr(dy), abi.ptr(mean), abi.ptr(rstd), abi.ptr(gamma), abi.ptr(beta),
             abi.ptr(skip), abi.ptr(o["dsums"]), abi.ptr(o["dx"]), abi.ptr(o["dskip"]), abi.ptr(o["planes"]), ns,
             abi.ptr(o["dgamma"]), abi.ptr(o["dbeta"]), 1, B, C, H, W, SLOPE, c.pool, c.up2, abi.ptr(ws), nws, pstride, c.G,
             live[0], live[1], abi.stream())
    return o


# name -> (shape, planes wanted, (forward path plain, forward path pooled, backward path))
BN_SHAPES = {
    "c16-8x8": ((3, 16, 8, 8), True, (OB, OB, OB)),
    "c16-16x16": ((3, 16, 16, 16), True, (OB, OB, OB)),
    "c16-32x32": ((3, 16, 32, 32), True, (SF, SF, SF)),
    "c24-12x20": ((6, 24, 12, 20), True, (SC, SC, SC)),
    "c12-8x8": ((16, 12, 8, 8), False, (FB, FB, FB)),
}


@pytest.mark.parametrize("mode", ["plain", "pool", "up2"])
@pytest.mark.parametrize("name", list(BN_SHAPES))
def test_batchnorm_apply_passes(HF, name, mode):
    from hipvae import abi
    shape, planes, paths = BN_SHAPES[name]
    pool, up2 = int(mode == "pool"), int(mode == "up2")
    assert abi.bn_plan_query(False, *shape, pool=pool, planes=planes, ns=2 if planes else 0)[0] == paths[pool]
    assert abi.bn_plan_query(True, *shape, pool=pool, up2=up2, planes=planes, ns=2 if planes else 0)[0] == paths[2]
    if name == "c16-8x8":                                   # 96 threads: a whole wave and a partly filled one
        assert shape[0] * (shape[1] // 8) * (shape[2] * shape[3] // 4) == 64 + 32
    ran = 0
    for G in (1, 2):
        for skip in (False, True):
            c = case(name, shape, G=G, pool=pool, up2=up2, planes=planes, skip=skip, acc=1)
            groups, par = make_inputs(c, "base", 1.0)
            d = dev()
            x = torch.cat([g[0] for g in groups]).to(d)
            dy = torch.cat([g[1] for g in groups]).to(d)
            sk = torch.cat([g[2] for g in groups]).to(d) if skip else None
            par = tuple(t.to(d) for t in par)
            for ns in ((2, 3, 4) if planes else (0,)):
                tag = (name, mode, G, skip, ns)
                fa, fb = off_on(HF, bit("BN_FWD"), lambda: hip_fwd(HF, c, x, sk, par, ns))
                assert_same(fa, fb, tag + ("forward",))
                assert torch.isfinite(fa["y"]).all()
                mean, rstd = fa["mean"], fa["rstd"]          # (the forward of an up2 layer is the plain one)
                lives = [(0, G)] if G == 1 else [(0, 2), (0, 1), (1, 1)]
                for live in lives:
                    ba, bb = off_on(HF, bit("BN_APPLY"), lambda: bn_bwd(HF, c, x, dy, sk, par, mean, rstd, ns, live))
                    assert_same(ba, bb, tag + ("backward", live))
                    B = shape[0]
                    assert torch.isfinite(ba["dx"][live[0] * B:(live[0] + live[1]) * B]).all(), tag
                    ran += 1
    assert ran == (2 * (1 + 3)) * (3 if planes else 1)


# ---- weight gradient and its folds ----------------------------------------------------------------------------------------
def fold_many(descs):
    from hipvae import abi
    table, n, blocks = build_table(descs)
    abi.call("itcv_wgrad_reduce_many", abi.ptr(table), n, blocks, abi.stream())


@pytest.mark.parametrize("ns", [2, 4], ids=["bf16x2", "f16x2"])
@pytest.mark.parametrize("up2", [0, 1])
@pytest.mark.parametrize("C", [32, 64])
def test_weight_gradient_slabs_and_folds(HF, C, up2, ns):
    from hipvae import abi
    B, H, W = 2, 8, 8
    assert abi.lib.itcv_conv2d_wgrad_bf16p_supported(B, C, H, W, C, 3)
    S = abi.lib.itcv_conv2d_wgrad_bf16p_slabs(B, C, H, W, C, 3)
    nws = abi.lib.itcv_conv2d_wgrad_bf16p_workspace(B, C, H, W, C, 3)
    coci = C * C
    assert S >= 1 and nws >= S * 9 * coci * 4
    gen = torch.Generator(device=dev()).manual_seed(100 * C + 10 * up2 + ns)
    x = torch.randn(B, C, H // 2 if up2 else H, W // 2 if up2 else W, generator=gen, device=dev())
    dy = torch.randn(B, C, H, W, generator=gen, device=dev()) * 1e-3
    xp, dyp = HF.split_planes(x, ns), HF.split_planes(dy, ns, gradient=True)
    dw0 = torch.randn(coci * 9, generator=gen, device=dev())

    def call(acc, ws, dw):
        abi.call("itcv_conv2d_wgrad_bf16p", abi.ptr(xp), abi.ptr(dyp), abi.ptr(dw), B, C, H, W, C, 3, up2, ns, acc, abi.ptr(ws),
                 nws, abi.stream())

    def deferred():                       # the slabs as the kernel leaves them, then folded by the table launch
        ws = torch.full((nws // 4,), float("nan"), device=dev())
        dw = dw0.clone()
        call(2, ws, dw)
        slabs = ws.clone()
        fold_many([([ws], [S], dw, C, C, 1)])
        return dict(slabs=slabs, untouched_dw=dw0.clone(), dw=dw)

    def direct():
        out = {}
        for acc in (0, 1):
            ws = torch.full((nws // 4,), float("nan"), device=dev())
            dw = dw0.clone()
            call(acc, ws, dw)
            out[f"dw{acc}"], out[f"ws{acc}"] = dw, ws
        return out

    for m16 in (0, 1):
        with HF.option_scope("wgrad_m16", m16):
            a, b = off_on(HF, bit("WGRAD_SLABS"), deferred)
            assert_same(a, b, (C, up2, ns, m16, "slab stores"))
            assert torch.isfinite(a["slabs"][:S * 9 * coci]).all() and float(a["slabs"][:S * 9 * coci].abs().max()) > 0
            assert torch.isfinite(a["dw"]).all() and not torch.equal(a["dw"], dw0)
            a2, b2 = off_on(HF, bit("FOLD"), deferred)
            assert_same(a2, b2, (C, up2, ns, m16, "fold loads"))
            assert_same(a, a2, (C, up2, ns, m16, "repeatable"))
            a3, b3 = off_on(HF, bit("WGRAD_SLABS") | bit("FOLD"), direct)
            assert_same(a3, b3, (C, up2, ns, m16, "direct call"))
            assert torch.equal(raw(a3["dw1"]), raw(a["dw"]))          # the deferred fold adds what the direct call adds


def test_fold_table_fine_and_wide(HF):
    """One launch of wgrad_p_reduce_many over a fine descriptor (70 and 2 slices, 64 x 64) and a wide one (3 slices,
    32 x 40, dw one float past 16-byte alignment, accumulate)."""
    gen = torch.Generator(device=dev()).manual_seed(9)
    specs = [(64, 64, [70, 2], 0, False), (32, 40, [3], 1, True)]
    slabs = [[make_slab(S, Co * Ci, gen) for S in splits] for Co, Ci, splits, _, _ in specs]
    dws = [make_dw(Co * Ci, mis, gen) for Co, Ci, _, _, mis in specs]
    start = [buf.clone() for buf, _, _ in dws]

    def run():
        out = []
        descs = []
        for (Co, Ci, splits, acc, mis), sl, (buf, view, st), s0 in zip(specs, slabs, dws, start):
            buf.copy_(s0)
            descs.append((sl, splits, view, Co, Ci, acc))
        fold_many(descs)
        return [buf.clone() for buf, _, _ in dws]

    a, b = off_on(HF, bit("FOLD"), run)
    assert_same(a, b, "table")
    for got, s0, (buf, view, st), (Co, Ci, _, _, _) in zip(a, start, dws, specs):
        n = Co * Ci * 9
        assert torch.isfinite(got[st:st + n]).all() and not torch.equal(got[st:st + n], s0[st:st + n])
        assert torch.equal(got[:st], s0[:st]) and torch.equal(got[st + n:], s0[st + n:])


def test_whole_mask_equals_none_on_a_training_step(HF):
    """Mask 0 against the full mask through a whole intro-TC training step of a tiny network (every family in its place in
    the step, hipGraph-free): the step's reported scalars and every parameter and buffer afterwards, byte for byte."""
    import models
    import ops
    from hipvae import abi
    from solvers.intro_tc import IntroTCSovler

    class DS:
        def __len__(self):
            return 1000

    def run():
        cfg = dict(cdim=3, zdim=16, channels=(16, 32, 64), image_size=32)
        torch.manual_seed(0)
        model = models.SoftIntroVAE(arch="conv", **cfg).to(dev()).train()
        B = 16
        solver = IntroTCSovler(DS(), model, B, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
                               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), "mse", 0.5, 0.75, 512.0, 1e-8,
                               dev(), False, None, clip=100.0)
        g = torch.Generator().manual_seed(1)
        x = torch.rand(B, 3, 32, 32, generator=g)
        out = {}
        for it in range(2):
            draws = [torch.randn(B, 16, generator=g) for _ in range(6)]
            with ops.noise_queue(draws):
                got = solver.train_step(x.to(dev()), it)
            for k, v in got.items():
                out[f"{it}:{k}"] = torch.tensor(float(v), dtype=torch.float64)
        torch.cuda.synchronize()
        for k, v in model.state_dict().items():
            out["state:" + k] = v.detach().clone()
        return out

    a, b = off_on(HF, abi.STREAM_NT["ALL"], run)
    assert len(a) > 20 and all(torch.isfinite(v.double()).all() for v in a.values())
    assert_same(a, b, "training step")
