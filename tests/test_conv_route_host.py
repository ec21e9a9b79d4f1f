"""CPU-only: the conv route record of hipvae.functional (``conv_route``) against tests/golden/conv_routes.json, which
tests/golden/make_golden_conv_routes.py recorded from the nine separate predicates the record replaced
(``_planes_ns``, ``_dgrad_sub_kind``, ``_wgrad5_mode``, ``_wgrad_planes_ok``, ``conv_input_mode``, ``conv_grad_mode``,
``conv_input_planes_ns``, ``conv_grad_planes_ns`` and the ``keep_xp`` decision of ``Conv2dFn.forward``): every conv
layer of the c2 / c3 / c5 "conv" configurations and the convs of one residual and one inception block, at the per-GPU
batch and its 2x / 3x multiples, in all four arithmetic modes, with the small-cin matrix-core form on and off, with and
without an input gradient, with and without bias.  Pure host queries: no GPU."""
import json
import os

import pytest

from test_conv_plan_host import CONFIGS, layers

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")
MODES = ("fp32", "bf16x3", "bf16x6", "f16x3")
# the 32 variants of one shape, in the order of a case's row indices: (mode, small-cin MFMA, needs_input_grad, has_bias)
VARIANTS = [(m, s, g, b) for m in MODES for s in (True, False) for g in (True, False) for b in (False, True)]
# what the recorder wrote per variant, in this order
COLUMNS = ("fwd_ns", "dgrad_ns", "dgrad_sub", "wgrad5", "wgrad_planes_ok", "input_mode", "grad_mode", "input_planes_ns",
           "grad_planes_ns", "keep_xp")


def block_layers():
    """(Ci, H, W, Co, KS, up2) of the convs of one residual block (128 -> 256: the 1x1 expand and the two 3x3) and one
    inception block (128 -> 256: expand, branch_0, the two of branch_1, the biased output conv), at 8x8 and 16x16."""
    out = []
    for s in (8, 16):
        out += [(128, s, s, 256, 1, 0), (128, s, s, 256, 3, 0), (256, s, s, 256, 3, 0)]
        out += [(128, s, s, 128, 1, 0), (256, s, s, 128, 1, 0), (256, s, s, 256, 1, 0)]
    return out


def shapes():
    """(B, Ci, H, W, Co, KS, up2) of every recorded case, in a fixed order, each once."""
    seen = []
    for cfg in sorted(CONFIGS):
        for mult in (1, 2, 3):
            seen += [(CONFIGS[cfg][2] * mult,) + lay for lay in layers(cfg)]
    for mult in (1, 2, 3):
        seen += [(CONFIGS["c2"][2] * mult,) + lay for lay in block_layers()]
    return list(dict.fromkeys(seen))


# forward / backward in different modes: a handful of c2 layers (stem, 3x3 wide and narrow, an upsampling one, predict)
MIXED_SHAPES = [(64, 3, 64, 64, 64, 5, 0), (64, 64, 32, 32, 128, 3, 0), (64, 512, 4, 4, 512, 3, 0),
                (64, 128, 32, 32, 64, 3, 1), (64, 64, 64, 64, 3, 5, 0)]
MIXED_PAIRS = [(f, b) for f in MODES for b in MODES if f != b]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _route(HF, shape, mode, scin, nig, bias):
    B, Ci, H, W, Co, KS, up2 = shape
    prev = HF._SCIN_MFMA[0]
    HF._SCIN_MFMA[0] = scin
    try:
        with HF.conv_math_scope(mode):
            return HF.conv_route(B, Ci, H, W, Co, KS, bool(up2), bias, nig)
    finally:
        HF._SCIN_MFMA[0] = prev


def _row(r):
    """The recorded columns, read off a route record."""
    return [r.fwd_ns, r.dgrad_ns, r.dgrad_sub, r.wgrad if r.wgrad in ("stem", "predict") else None, r.wgrad == "planes",
            list(r.in_mode), list(r.grad_mode), r.in_mode_keep_fp32[0], r.grad_mode_keep_fp32[0], r.keep_xp]


def test_golden_is_complete(golden):
    assert golden["columns"] == list(COLUMNS) and golden["variants"] == [list(v) for v in VARIANTS]
    assert [tuple(c[:7]) for c in golden["cases"]] == shapes()
    assert all(len(c[7]) == len(VARIANTS) for c in golden["cases"])
    assert len(shapes()) == 191             # 164 launches of the conv configurations + the block convs not among them


def test_route_reproduces_every_recorded_entry(golden):
    from hipvae import functional as HF
    rows = golden["rows"]
    n = 0
    for case in golden["cases"]:
        shape = tuple(case[:7])
        for (mode, scin, nig, bias), idx in zip(VARIANTS, case[7]):
            r = _route(HF, shape, mode, scin, nig, bias)
            assert _row(r) == rows[idx], (shape, mode, scin, nig, bias)
            # the shape-free hints are the same plane formats with the fp32 tensor always kept
            assert r.in_mode_keep_fp32 == (r.in_mode[0], True) and r.grad_mode_keep_fp32 == (r.grad_mode[0], True)
            n += 1
    assert n == len(shapes()) * len(VARIANTS)


def test_route_forward_kernels():
    """The kernel names of the c2 layers in bf16x3: what Conv2dFn runs per direction (not part of the recorded table: the
    predicates the record replaced did not name kernels; the GPU call trace pins the launches themselves)."""
    from hipvae import functional as HF
    got = {}
    for lay in layers("c2"):
        r = _route(HF, (64,) + lay, "bf16x3", True, True, False)
        got[lay] = (r.fwd, r.dgrad, r.wgrad)
    assert got[(3, 64, 64, 64, 5, 0)] == ("small_cin_mfma", "small_cout_planes", "stem")
    assert got[(64, 64, 64, 3, 5, 0)] == ("small_cout_planes", "small_cin_mfma", "predict")
    assert got[(64, 32, 32, 128, 3, 0)] == ("planes", "planes", "planes")
    r = _route(HF, (64, 3, 64, 64, 64, 5, 0), "bf16x3", False, True, False)
    assert (r.fwd, r.fwd_fp32) == ("small_cin", "small_cin")
    r = _route(HF, (64, 64, 32, 32, 128, 3, 0), "fp32", True, True, False)
    assert (r.fwd, r.dgrad, r.wgrad, r.fwd_ns, r.keep_xp) == ("fp32", "fp32", "raw", 0, False)
    r = _route(HF, (64, 64, 32, 32, 128, 3, 0), "bf16x6", True, True, False)
    assert (r.fwd, r.fwd_fp32, r.wgrad) == ("planes", "split", "raw")


def test_mode_changed_between_forward_and_backward(golden):
    """A forward in one mode and a backward in another: Conv2dFn.backward raises its two "mode changed" errors exactly
    where the backward route needs an operand the forward route did not leave (``missing_operand``)."""
    from hipvae import functional as HF
    want = golden["mixed"]
    assert [(tuple(m[0]), m[1], m[2]) for m in want] == [(s, f, b) for s in MIXED_SHAPES for f, b in MIXED_PAIRS]
    assert any(m[3] for m in want) and any(m[4] for m in want)
    for shape, fmode, bmode, x_missing, sub_missing in want:
        fwd = _route(HF, tuple(shape), fmode, True, True, False)
        bwd = _route(HF, tuple(shape), bmode, True, True, False)
        got = HF.missing_operand(fwd, bwd)
        assert (got[0], got[1]) == (x_missing, sub_missing), (shape, fmode, bmode)
