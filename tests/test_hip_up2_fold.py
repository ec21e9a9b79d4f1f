"""GPU: the data gradient of an upsampled conv with the upsample's 2x2 adjoint folded into the band kernel's store
(``itcv_conv2d_dgrad_up2_bf16p``, the ADJ form of csrc/conv_band.hip) against the two-call path it replaces --
``itcv_conv2d_fwd_bf16p_st`` / ``_sub`` into a fresh fp32 tensor, then ``itcv_upsample2_bwd`` -- as an equality of bytes
(uint8 views: +-0 count).  Inputs are integer hashes run through the real plane-split and weight-pack calls; the fp16
planes get a gradient-sized magnitude so that their scale record is a non-trivial power of two (``oscale != 1``).

Every case names the kernel form it is there for -- one-tile (p2, profile kind 8) or persistent (p3, kind 9), 64- or
128-row tiles, log2(W) -- and both paths' launches are read back from the library's launch profile: the form that ran is
the named one.  All are 3x3; channels are dy channels -> dx channels.

Two cases are not launched at the batch they were first specified with, because their plans split K and the form
covers ``splits == 1`` only (a split launch stores partial sums in slabs; the fold has to come behind their reduction):
  * 64x64, 64 -> 128, B = 2: 32 tiles and two 32-channel groups -> two K slices.  Kept as a refusal case (query 0, the
    entry point answers with the library's error); the shape runs at B = 12, the smallest batch with 192 tiles.
  * the step-level case at B = 8 (channels (64, 128), image 32): the largest launch of that step has 64 tiles, every
    upsampled conv's data gradient splits K, and the lowered threshold changes no call.  Kept with everything else it
    asks (equal dicts, equal state, the default run's calls); the step runs at B = 24 as well, where the 32x32 layer's
    batched pass has 192 tiles and the new entry point has to appear."""
import contextlib
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16X2, F16X2 = 2, 4
FILL = 12345.0


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def HF():
    from hipvae import functional
    return functional


def _hash(n, seed):
    """n floats in [-0.5, 0.5), multiples of 2^-24: integer arithmetic only."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 69069 + 12345)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    return ((h >> np.uint64(8)).astype(np.float64) * (1.0 / (1 << 24)) - 0.5).astype(np.float32)


@contextlib.contextmanager
def profiled(HF):
    labels = []
    HF.LaunchProfile.begin()
    try:
        yield labels
    finally:
        labels.extend(lab for lab, _, _ in HF.LaunchProfile.end())


def band_label(kind, lw, bm, fmt):
    name = {8: "conv_fwd_bf16p2_kernel", 9: "conv_fwd_bf16p3_kernel"}[kind]
    return f"{name}<LOG2W={lw},BM={bm},up2=0,NS={fmt}>"


_inputs = {}


def operands(HF, B, D, H, W, X, fmt):
    """(planes of dy [B, D, H, W], weight [D, X, 3, 3]) -- made once per shape and format, never written afterwards."""
    key = (B, D, H, W, X, fmt)
    if key not in _inputs:
        _inputs.clear()                                        # one shape's tensors at a time
        dy = torch.from_numpy(_hash(B * D * H * W, 7 + B + D + H) * np.float32(2.0 ** -10)).reshape(B, D, H, W).to(dev())
        w = torch.from_numpy(_hash(D * X * 9, 11 + D + X) * np.float32(2.0 / (9 * D) ** 0.5)).reshape(D, X, 3, 3).to(dev())
        dyp = HF.split_planes(dy, fmt, gradient=True)
        if fmt == F16X2:                                       # the scale record {S, 1/S} behind the last plane
            s, inv = dyp[-4:-2].view(torch.float32).tolist()   # 16 bytes: scale, 1 / scale, padding
            assert s > 1.0 and s * inv == 1.0 and np.log2(s) == int(np.log2(s)), (s, inv)
        _inputs[key] = (dyp, w)
    return _inputs[key]


def both_paths(HF, B, D, H, W, X, fmt, live=None):
    """(two-call result, fused result, launch labels of the two-call path, of the fused call): [B, X, H/2, W/2] tensors
    that started from the same fill pattern."""
    from hipvae.abi import ptr, stream
    dyp, w = operands(HF, B, D, H, W, X, fmt)
    b0, nb = live if live is not None else (0, B)
    want = torch.full((B, X, H // 2, W // 2), FILL, device=dev())
    got = want.clone()
    with profiled(HF) as two:
        hi = HF.conv_apply_planes(dyp, w, w, 1, None, B, D, H, W, X, 3, False, fmt, live=live)
        HF.call("itcv_upsample2_bwd", ptr(hi[b0:b0 + nb]), ptr(want[b0:b0 + nb]), nb * X, H // 2, W // 2, stream())
    with profiled(HF) as one:
        HF.call("itcv_conv2d_dgrad_up2_bf16p", ptr(dyp), ptr(HF.packed_weight(w, w, 1, fmt)), ptr(got), B, D, H, W, X, 3, fmt,
                b0, nb, None, 0, stream())
    torch.cuda.synchronize()
    return want, got, two, one


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# (B, dy channels, H, W, dx channels) -> (profile kind, BM) of the launch plan_fwd_band gives the shape
FORMS = [
    ((96, 64, 16, 16, 128), (8, 64)),       # 16 wide: a tile is one image; 192 tiles of 64 rows
    ((48, 256, 16, 16, 512), (8, 128)),     # 16 wide, 128-row tiles, eight channel groups
    ((24, 64, 32, 32, 96), (8, 64)),        # 96 channels: the second 64-row tile is half empty (m < Co)
    ((48, 64, 32, 32, 96), (8, 128)),       # ... and the only 128-row tile a quarter empty
    ((24, 128, 32, 32, 256), (8, 128)),
    ((12, 64, 64, 64, 128), (8, 128)),      # 64 wide: four rows a tile (at B = 2 the plan splits K: test_refusals)
    ((6, 32, 8, 16, 64), (8, 64)),          # 8 x 16 images: a tile holds two images (two band segments)
    ((17, 64, 64, 64, 64), (9, 64)),        # persistent: 272 tiles on 256 blocks, 18 MB of output
    ((17, 64, 64, 64, 128), (9, 128)),
    ((65, 64, 32, 32, 64), (9, 64)),        # 260 tiles: the id space is padded to 264
    ((80, 64, 32, 32, 128), (9, 128)),
    ((264, 64, 16, 16, 64), (9, 64)),
    ((136, 64, 16, 16, 256), (9, 128)),
]


@pytest.mark.parametrize("fmt", [BF16X2, F16X2], ids=["bf16x2", "f16x2"])
@pytest.mark.parametrize("shape,form", FORMS, ids=[f"{s[2]}x{s[3]}-{s[1]}to{s[4]}-B{s[0]}" for s, _ in FORMS])
def test_fused_equals_two_calls(HF, shape, form, fmt):
    B, D, H, W, X = shape
    assert HF.lib.itcv_conv2d_dgrad_up2_supported(B, D, H, W, X, 3, fmt, B) == 1
    assert HF.lib.itcv_conv2d_fwd_bf16p_workspace(B, D, H, W, X, 3, fmt) == 0          # no K split
    want, got, two, one = both_paths(HF, B, D, H, W, X, fmt)
    label = band_label(form[0], int(np.log2(W)), form[1], fmt)
    assert two == [label] and one == [label], (two, one, label)
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0 and not (want == FILL).any()
    assert same_bytes(want, got), float((want - got).abs().max())


SUB = [
    ((4, 32, 64, 64, 64), (8, 64)),         # B = 4: one channel group, so 64 tiles do not split K
    ((4, 32, 32, 32, 128), (8, 128)),
]


@pytest.mark.parametrize("fmt", [BF16X2, F16X2], ids=["bf16x2", "f16x2"])
@pytest.mark.parametrize("live", [(1, 2), (2, 2)])
@pytest.mark.parametrize("shape,form", SUB, ids=[f"{s[2]}x{s[3]}-{s[1]}to{s[4]}" for s, _ in SUB])
def test_sub_range(HF, shape, form, live, fmt):
    B, D, H, W, X = shape
    assert HF.lib.itcv_conv2d_dgrad_up2_supported(B, D, H, W, X, 3, fmt, live[1]) == 1
    want, got, two, one = both_paths(HF, B, D, H, W, X, fmt, live=live)
    label = band_label(form[0], int(np.log2(W)), form[1], fmt)
    assert two == [label] and one == [label], (two, one, label)
    inside = slice(live[0], live[0] + live[1])
    outside = [b for b in range(B) if not live[0] <= b < live[0] + live[1]]
    assert (got[outside] == FILL).all() and not (got[inside] == FILL).any()
    assert same_bytes(want, got)
    full = both_paths(HF, B, D, H, W, X, fmt)[1]                 # the plan is the whole batch's: the live images' bits too
    assert same_bytes(full[inside], got[inside])


@pytest.mark.parametrize("fmt", [BF16X2, F16X2], ids=["bf16x2", "f16x2"])
def test_sub_range_persistent(HF, fmt):
    """Phase E's shape in small: the live half of a 34-image pass, both halves' launches persistent (544 / 272 tiles)."""
    B, D, H, W, X = 34, 64, 64, 64, 64
    for live in ((17, 17), (0, 17)):
        want, got, two, one = both_paths(HF, B, D, H, W, X, fmt, live=live)
        assert two == one == [band_label(9, 6, 64, fmt)]
        assert same_bytes(want, got) and (got[17 - live[0]:34 - live[0]] == FILL).all()


def test_refusals(HF):
    from hipvae import abi
    q = HF.lib.itcv_conv2d_dgrad_up2_supported
    bad = [(128, 512, 8, 8, 512),        # query only: the c2 8x8 layer
           (2, 64, 64, 64, 128),         # K split in two (32 tiles, two channel groups)
           (4, 64, 1, 16, 64),           # odd H
           (4, 64, 16, 16, 32)]          # fewer than 33 output channels
    for fmt in (BF16X2, F16X2):
        for s in bad:
            assert q(*s, 3, fmt, s[0]) == 0, s
    assert HF.lib.itcv_conv2d_fwd_bf16p_workspace(2, 64, 64, 64, 128, 3, F16X2) > 0
    dummy = torch.zeros(1024, device=dev())
    for s in bad[1:]:
        B, D, H, W, X = s
        with pytest.raises(abi.HipExtensionError, match="itcv_conv2d_dgrad_up2_bf16p"):
            HF.call("itcv_conv2d_dgrad_up2_bf16p", abi.ptr(dummy), abi.ptr(dummy), abi.ptr(dummy), B, D, H, W, X, 3, F16X2, 0,
                    B, None, 0, abi.stream())
    with pytest.raises(abi.HipExtensionError, match="image range"):
        HF.call("itcv_conv2d_dgrad_up2_bf16p", abi.ptr(dummy), abi.ptr(dummy), abi.ptr(dummy), 12, 64, 64, 64, 128, 3, F16X2,
                8, 5, None, 0, abi.stream())
    torch.cuda.synchronize()
    assert (dummy == 0).all()


# ------------------------------------------------------------------ whole steps
NET = dict(cdim=3, zdim=10, channels=(64, 128), image_size=32)
HP = dict(beta_kl=0.5, beta_rec=0.75, beta_neg=512.0, gamma_r=1e-8, clip=100.0, lr=2e-4)
NEW, OLD = "itcv_conv2d_dgrad_up2_bf16p", "itcv_upsample2_bwd"


class _DS:
    def __len__(self):
        return 1000


@contextlib.contextmanager
def call_names(log):
    from hipvae import flat, functional

    def wrap(inner):
        def call(name, *args):
            log.append(name)
            return inner(name, *args)
        return call

    saved = functional.call, flat.call
    functional.call, flat.call = wrap(saved[0]), wrap(saved[1])
    try:
        yield
    finally:
        functional.call, flat.call = saved


def run_steps(HF, B, min_bytes, graph):
    """(returned dicts, digest per state tensor, library calls) of the intro-TC solver in f16x3: eager, two steps on queued
    draws; captured, five steps on seeded device noise (three warm-up steps, the capture, one replay)."""
    import models
    import ops
    from solvers.intro_tc import IntroTCSovler
    torch.manual_seed(3)
    model = models.SoftIntroVAE(arch="conv", **NET).to(dev()).train()
    solver = IntroTCSovler(_DS(), model, B, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                           torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", HP["beta_kl"], HP["beta_rec"],
                           HP["beta_neg"], HP["gamma_r"], dev(), False, None, clip=HP["clip"])
    solver.conv_math = "f16x3"
    if graph:
        solver.enable_graph()
    g = torch.Generator().manual_seed(11)
    steps = 5 if graph else 2
    xs = [torch.rand(B, 3, 32, 32, generator=g).to(dev()) for _ in range(steps)]
    draws = [[torch.randn(B, NET["zdim"], generator=g) for _ in range(6)] for _ in range(steps)]
    torch.manual_seed(1234)
    prev, calls, dicts = HF.UP2_FOLD_MIN_BYTES[0], [], []
    HF.set_up2_fold_min_bytes(min_bytes)
    try:
        with call_names(calls):
            for s in range(steps):
                with (contextlib.nullcontext() if graph else ops.noise_queue(draws[s])):
                    dicts.append(solver.train_step(xs[s], s))
    finally:
        HF.set_up2_fold_min_bytes(prev)
    torch.cuda.synchronize()
    if graph:
        assert solver._graph is not None, "the captured graph was not used"
        assert solver._graph_key[2] == ("f16x3", min_bytes)
    state = [f"{k}:{hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}"
             for k, v in model.state_dict().items()]
    return dicts, state, calls


def folding_layers(HF, B):
    """Does any upsampled conv of NET's decoder have the fused form in a step at batch B (single or batched pass, whole
    or live half)?  Decoder: 128 -> 128 @ 8x8, 128 -> 64 @ 16x16 (upsampled), 64 -> 64 @ 32x32 (upsampled)."""
    return any(HF.lib.itcv_conv2d_dgrad_up2_supported(b, d, s, s, x, 3, F16X2, nb)
               for d, x, s in ((64, 128, 16), (64, 64, 32)) for b, nb in ((B, B), (2 * B, 2 * B), (2 * B, B)))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("B", [8, 24])
def test_step_lowered_threshold_equals_default(HF, B, graph):
    default = HF.UP2_FOLD_MIN_BYTES[0]
    assert default == 32 << 20
    low, ref = run_steps(HF, B, 1, graph), run_steps(HF, B, default, graph)
    assert low[0] == ref[0] and all(np.isfinite(v) for d in low[0] for v in d.values() if v is not None)
    assert low[1] == ref[1]
    assert OLD in ref[2] and NEW not in ref[2]
    # B = 8: every data gradient of the step splits K (at most 64 tiles a launch), which the form does not cover
    assert folding_layers(HF, B) == (B == 24)
    assert (NEW in low[2]) == (B == 24)
    if B == 24:
        assert low[2].count(OLD) < ref[2].count(OLD) and len(low[2]) < len(ref[2])
