"""torch.autograd.Function wrappers around the HIP kernels of libitcv_hip.so.

Each Function forwards device pointers to one or a few C-ABI entry points (hipvae.abi) and
keeps only what its backward needs.  PyTorch provides memory, the stream and the autograd
tape; all arithmetic on activations, gradients and statistics happens in the HIP kernels.
The optional ``group`` arguments are torch.distributed process groups: they turn BatchNorm
into Sync-BN (all-reduce of the fp64 channel moments over RCCL) for data-parallel parity
with the full-batch reference.
"""
import contextlib
import ctypes
import functools
import os
import weakref
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import abi
from .abi import call, lib, ptr, stream

F32 = torch.float32


def set_option(name, value):
    """Launch-shape options of the library (include/itcv_hip.h: itcv_set_option): 'band_m16' (0/1),
    'band_persist_blocks' (0 = one tile per block, else the persistent kernel's block count), 'wgrad_m16' (0 / 1 =
    32x32x16 / 16x16x32 products in the planes weight gradient), 'planes_mfma_waves' (4 / 8), 'stream_nt' (a mask of
    abi.STREAM_NT bits: which kernel families stream their once-used tensors non-temporally; bit-identical), and the two
    test options of the sliced-Wasserstein kernels, 'sw_lds_rows' and 'sw_max_blocks' (0 = the default).  Validated by
    the library."""
    call("itcv_set_option", name.encode(), int(value))
    _up2_fold_route.cache_clear()      # the one cached host decision that reads an option ('band_m16')
    lib.forget("itcv_conv2d_dgrad_up2_supported")
    lib.forget("itcv_sw_workspace")    # 'sw_lds_rows' / 'sw_max_blocks'


def get_option(name):
    return lib.itcv_get_option(name.encode())


@contextlib.contextmanager
def option_scope(name, value):
    prev = get_option(name)
    set_option(name, value)
    try:
        yield
    finally:
        set_option(name, prev)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _f32c(t):
    if t.dtype != F32:
        raise abi.HipExtensionError(f"HIP path is fp32 only (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------ gradient accumulation mode
_DIRECT = [False]


@contextlib.contextmanager
def direct_grad_accumulation():
    """Inside this block the backward kernels add parameter gradients straight into an existing,
    contiguous ``param.grad`` (the solvers' flat gradient buffers) and hand autograd ``None``,
    instead of returning fresh tensors for autograd to add (saves one elementwise pass and one
    launch per parameter per network pass)."""
    prev, _DIRECT[0] = _DIRECT[0], True
    try:
        yield
    finally:
        _DIRECT[0] = prev


def _grad_target(param):
    g = param.grad if _DIRECT[0] else None
    return g if (g is not None and g.is_contiguous() and g.dtype == F32) else None


# ------------------------------------------------------------------ one recorded pass, two backward passes
# A network pass that two losses need with the same weights and the same input is recorded once (the intro step's
# dec(noise | z), solvers/intro.py).  What the skipped second pass would have done beyond recomputing the same tensors
# is made up for here:
#   * its BatchNorm running-buffer updates: BnActFn leaves the two floats every group blended into the buffers in a
#     persistent [2][G][C] tensor per layer and ``replay()`` repeats the updates, for all layers in one launch, at the
#     point of the stream where the second pass used to run;
#   * its parameter gradients: the pass is recorded with its parameters requiring a gradient, and ``param_grads`` tells
#     Conv2dFn / LinearFn / BnActFn.backward whether a backward pass through it may compute and accumulate them (they add
#     straight into the flat .grad buffers from inside those functions, out of autograd's sight);
#   * ``input_grad`` False: the first function of the pass does not compute the gradient of the pass's input.
#   * ``live`` = (g, G): the pass is a batch of G stacked groups and the gradient handed to this backward is exactly zero
#     outside group g (the intro step's phase E: ``fake`` of dec(noise | z) only feeds constants).  The backward functions
#     then run the sub-range forms of the kernels on group g's images alone: zero in gives zero out, so nothing is computed
#     for the other groups, and the dead part of every gradient tensor on the way is never written and never read (NaN in
#     _POISON mode).  The values of the live images are bit for bit those of the full backward.  It holds only for a
#     backward with ``param_grads`` off (a weight gradient reads every image), and only for a pass whose functions all
#     have a sub-range form: the forward calls note what stands in the way in ``live_blockers`` and the pass then runs the
#     full backward, as a whole.  The chain ends at the first pointwise function in front of a LinearFn, which writes
#     zeros for the dead rows: the Linear data gradient (a GEMM planned by its batch) runs unchanged.
_SHARED_PASS = [None]


class SharedPass:
    """Owned by a solver (the statistics buffers and the device table are persistent: a captured hipGraph bakes their
    addresses in, so they are never freed or rebuilt while this object lives)."""

    def __init__(self):
        self.param_grads = True
        self.input_grad = True
        self.live = None
        self.live_blockers = []
        self.records = []
        self._first = False
        self._pool = {}
        self._tables = {}

    @contextlib.contextmanager
    def record(self):
        """Forward calls inside this block belong to the pass: their BatchNorm layers are collected for ``replay``."""
        prev, _SHARED_PASS[0] = _SHARED_PASS[0], self
        self.records, self._first = [], True
        self.param_grads = self.input_grad = True
        self.live, self.live_blockers = None, []
        try:
            yield self
        finally:
            _SHARED_PASS[0] = prev

    def _claim_first(self):
        first, self._first = self._first, False
        return first

    def _stats(self, G, C, device):
        """[2][G][C] (mean, unbiased variance) of the next BatchNorm layer of the pass: one buffer per position."""
        k = (len(self.records), G, C, str(device))
        buf = self._pool.get(k)
        if buf is None:
            buf = self._pool[k] = torch.empty((2, G, C), dtype=F32, device=device)
        return buf

    def replay(self):
        """Repeats the running-buffer updates of every BatchNorm layer recorded by the last ``record()`` block."""
        replay_bn_running(self.records, self._tables)


def _shared_ok(ctx, what):
    sp = ctx.shared
    return sp is None or getattr(sp, what)


def _block_live(why):
    """Forward of a function inside SharedPass.record() that has no sub-range backward for this call."""
    sp = _SHARED_PASS[0]
    if sp is not None and why not in sp.live_blockers:
        sp.live_blockers.append(why)


def _live_images(ctx, B):
    """(b0, nb): the images of a B-image gradient this backward has to walk, or None for all of them (see SharedPass)."""
    sp = getattr(ctx, "shared", None)
    if sp is None or sp.live is None or sp.param_grads or sp.live_blockers:
        return None
    g, G = sp.live
    if B % G:
        raise abi.HipExtensionError(f"SharedPass.live: batch {B} is not {G} equal groups")
    return g * (B // G), B // G


def _new_grad(like_or_shape, device=None, live=None):
    """Gradient tensor of which a live range writes a part only: the rest is never read (NaN in _POISON mode)."""
    t = torch.empty_like(like_or_shape) if device is None else torch.empty(like_or_shape, dtype=F32, device=device)
    if live is not None and _POISON[0]:
        t.fill_(float("nan"))
    return t


def _desc_table(entry, desc_bytes, items, fill, device):
    """Device-resident descriptor table of a table-driven launch -> (uint8 device tensor, len(items), total blocks).
    ``fill(slot, item, blocks)`` writes one descriptor through the library's ``entry`` and returns the blocks it
    adds behind the ``blocks`` of the ones before it (<= 0: the library refused; its message is raised)."""
    host = (ctypes.c_uint8 * (desc_bytes * len(items)))()
    blocks = 0
    for i, item in enumerate(items):
        got = fill(ctypes.byref(host, i * desc_bytes), item, blocks)
        if got <= 0:
            raise abi.HipExtensionError(entry + ": " + abi.last_error())
        blocks += got
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).to(device), len(items), blocks


def replay_bn_running(records, tables=None):
    """records: (running_mean, running_var, num_batches_tracked, mean [G][C], unbiased variance [G][C], momentum) per
    BatchNorm call, as BnActFn leaves them inside ``SharedPass.record()``.  Advances every layer's buffers as a second
    forward over the same batch would: ONE launch (itcv_bn_replay_many).  ``tables``: dict that keeps the device tables
    alive, one per sequence of pointers; the caller owns it for as long as a captured graph may replay the launch.
    Without it the table lives for this (eager, stream-ordered) launch only."""
    if tables is None:
        tables = {}
    recs = [r for r in records if r[0] is not None or r[1] is not None or r[2] is not None]
    if not recs:
        return
    key = tuple((0 if r[0] is None else r[0].data_ptr(), 0 if r[1] is None else r[1].data_ptr(),
                 0 if r[2] is None else r[2].data_ptr(), r[3].data_ptr(), r[4].data_ptr(), tuple(r[3].shape), r[5])
                for r in recs)
    tab = tables.get(key)
    if tab is None:
        if len(recs) > lib.itcv_bn_replay_max_descs():
            raise abi.HipExtensionError("replay_bn_running: more BatchNorm layers than one table holds")
        def fill(slot, rec, blocks):
            rm, rv, nbt, mean, uvar, momentum = rec
            return lib.itcv_bn_replay_desc(slot, ptr(rm), ptr(rv), ptr(nbt), ptr(mean), ptr(uvar), mean.shape[1], mean.shape[0],
                                           float(momentum), blocks)

        # the records keep the tensors the table points at alive with the table
        tab = tables[key] = _desc_table("itcv_bn_replay_desc", lib.itcv_bn_replay_desc_bytes(), recs, fill,
                                        recs[0][3].device) + (recs,)
    call("itcv_bn_replay_many", ptr(tab[0]), tab[1], tab[2], stream())


# (Round 1 issued the weight-gradient GEMMs on a second HIP stream; with the batched passes of round 2 they fill the chip
# on their own and running them beside the data-gradient chain cost more than the gaps it filled -- same-box A/B of the c2
# step 18.45 vs 18.0 ms -- so the side stream is gone.)

# ------------------------------------------------------------------ convolution / linear
_WEIGHT_EPOCH = [0]
_PACK_CACHE = {}


_PARAM_EPOCH = {}


def bump_weight_epoch(params=None):
    """Call after parameters were modified through raw pointers (fused Adam): invalidates the packed-weight
    cache (torch's own in-place ops are tracked through ``tensor._version``).  ``params``: only these tensors
    changed (the optimiser step of one model half leaves the other half's packed weights valid)."""
    if params is None:
        _WEIGHT_EPOCH[0] += 1
        return
    for p in params:
        _PARAM_EPOCH[id(p)] = _PARAM_EPOCH.get(id(p), 0) + 1


# conv arithmetic -> plane format code of the C ABI (include/itcv_hip.h): 2 / 3 bf16 planes, 4 = two fp16 planes + scale
_NS = {"fp32": 0, "bf16x3": 2, "bf16x6": 3, "f16x3": 4}
F16X2 = abi.DEFINES["ITCV_PLANES_F16X2"]
_CONV_MATH = [os.environ.get("ITCV_CONV_MATH", "fp32")]   # the one documented environment override (with ITCV_DDP_GRAPH, ITCV_LIB)
assert _CONV_MATH[0] in _NS, "ITCV_CONV_MATH must be one of fp32 / bf16x3 / bf16x6 / f16x3"


def _two(ns):
    """Two-plane formats (bf16x3, f16x3): the ones the weight-gradient and 5x5 planes kernels take."""
    return ns in (2, F16X2)


# Module switch of the test matrix (never read from the environment): fill planes-only tensors with NaN (nothing may read
# an fp32 tensor that was not written).  The gather kernels the planes kernels are compared with, bit for bit, are
# reached by calling conv_apply / conv_wgrad_raw directly.
_POISON = [False]


def set_conv_math(mode):
    """Arithmetic of the conv/linear forward and data-gradient GEMMs:
    'fp32'   exact fp32 MFMA (v_mfma_f32_32x32x2_f32) -- the parity path and the default;
    'bf16x6' operands split into 3 bf16 planes, 6 bf16 MFMAs per product, fp32 accumulate: fp32-class
             accuracy (~2^-23 per product) at 2.7x the matrix-core rate;
    'bf16x3' 2 planes / 3 MFMAs: ~2^-16 per product at 5.3x the matrix-core rate;
    'f16x3'  2 FP16 planes (hi, lo of the tensor times a power-of-two scale) / the same 3 MFMAs on the fp16 matrix
             cores: 22 significand bits, ~2^-21 per product -- fp32 class at the bf16x3 rate.  Shapes outside the planes
             kernels run on the exact fp32 kernels in this mode.
    Layers the split kernel does not cover (3-channel stem/predict, KS=5) stay on the fp32 kernel."""
    assert mode in _NS, mode
    _CONV_MATH[0] = mode


def conv_math():
    return _CONV_MATH[0]


@contextlib.contextmanager
def conv_math_scope(mode):
    """Temporarily select the conv arithmetic (used by the solvers: ``use_amp`` picks the mode)."""
    if mode is None:
        yield
        return
    assert mode in _NS, mode
    prev, _CONV_MATH[0] = _CONV_MATH[0], mode
    try:
        yield
    finally:
        _CONV_MATH[0] = prev


def _pack_key(weight):
    return (weight.data_ptr(), weight._version, _WEIGHT_EPOCH[0], _PARAM_EPOCH.get(id(weight), 0))


def _pack_entry(weight, key):
    ent = _PACK_CACHE.get(id(weight))
    if ent is None:
        ent = _PACK_CACHE[id(weight)] = [key, {}]
        weakref.finalize(weight, _PACK_CACHE.pop, id(weight), None)
        weakref.finalize(weight, _PARAM_EPOCH.pop, id(weight), None)
    elif ent[0] != key:
        ent[0], ent[1] = key, {}
    return ent


def packed_weight(weight, w4, for_dgrad, ns=0):
    """Packed operand of ``weight`` (viewed as ``w4`` [Co,Ci,KS,KS]), cached until the weight changes:
    the frozen half of the model is packed once per phase instead of once per network pass.  Weights registered
    through register_pack_group() (the parameters of one optimiser) are re-packed together, one launch per
    (direction, arithmetic), when the first of them is asked for after the optimiser step."""
    ent = _pack_entry(weight, _pack_key(weight))
    wp = ent[1].get((for_dgrad, ns))
    if wp is None:
        grp = _PACK_GROUPS.get(id(weight)) if ns and _PACK_BATCH[0] else None
        if grp is not None:
            wp = grp.pack(weight, w4, for_dgrad, ns)
        else:
            wp = ent[1][(for_dgrad, ns)] = pack_weight(w4, for_dgrad) if ns == 0 else pack_weight_bf16s(w4, for_dgrad, ns)
    return wp


# One launch re-packs every split-bf16 conv weight of a parameter group (False: one launch per layer; the tests compare the two).
_PACK_BATCH = [True]
_PACK_GROUPS = {}


class _PackGroup:
    """Conv weights that change together.  Membership per (for_dgrad, ns) is learnt from the requests: a weight seen for
    the first time is packed on its own and joins; from then on a miss on any member re-packs all of them into their
    persistent buffers through one device-resident descriptor table."""

    def __init__(self):
        self.members = {}    # (for_dgrad, ns) -> {id(weight): [weakref(weight), (co, ci, ks), data_ptr, wp]}
        self.tables = {}     # (for_dgrad, ns) -> (dev_table, n, total_blocks)

    def pack(self, weight, w4, for_dgrad, ns):
        k = (for_dgrad, ns)
        mem = self.members.setdefault(k, {})
        rec = mem.get(id(weight))
        if rec is None or rec[2] != w4.data_ptr() or rec[1] != tuple(w4.shape[:3]):
            wp = pack_weight_bf16s(w4, for_dgrad, ns)
            mem[id(weight)] = [weakref.ref(weight), tuple(w4.shape[:3]), w4.data_ptr(), wp]
            self.tables.pop(k, None)
            _pack_entry(weight, _pack_key(weight))[1][k] = wp
            return wp
        # The table holds every member's raw source pointer: before a grouped launch each member must still be alive and
        # sit where it was registered (a `p.data` reassignment or a freed weight would be re-packed from stale memory).
        # Members that moved or died leave the group (and drop the table); they re-join on their next own request.
        stale = [i for i, r in mem.items()
                 if r[0]() is None or r[0]().data_ptr() != r[2] or tuple(r[0]().shape[:3]) != r[1]]
        if stale:
            for i in stale:
                del mem[i]
            self.tables.pop(k, None)
        tab = self.tables.get(k)
        if tab is None:
            tab = self.tables[k] = self._build(mem, for_dgrad, ns, weight.device)
        call("itcv_conv2d_pack_weights_bf16s", ptr(tab[0]), tab[1], tab[2], ns, stream())
        for r in mem.values():        # every remaining member was just verified: its buffer holds the fresh packing
            m = r[0]()
            _pack_entry(m, _pack_key(m))[1][k] = r[3]
        return rec[3]

    @staticmethod
    def _build(mem, for_dgrad, ns, device):
        def fill(slot, r, blocks):
            co, ci, ks = r[1]
            return lib.itcv_conv2d_pack_desc_bf16s(slot, r[2], ptr(r[3]), co, ci, ks, int(for_dgrad), ns, blocks)

        return _desc_table("itcv_conv2d_pack_desc_bf16s", lib.itcv_pack_desc_bytes(), list(mem.values()), fill, device)


def register_pack_group(params):
    """Parameters that one optimiser step changes together (hipvae.flat.FlatGroup): their packed conv operands are
    refreshed by one launch per direction."""
    grp = _PackGroup()
    for p in params:
        if p.dim() == 4:
            _PACK_GROUPS[id(p)] = grp
            weakref.finalize(p, _PACK_GROUPS.pop, id(p), None)
    return grp


def pack_weight_bf16s(w4, for_dgrad, ns):
    co, ci, ks = w4.shape[0], w4.shape[1], w4.shape[2]
    nbytes = lib.itcv_conv2d_packed_weight_bytes_bf16s(co, ci, ks, int(for_dgrad), ns)
    wp = torch.empty(nbytes // 4, dtype=torch.int32, device=w4.device)
    call("itcv_conv2d_pack_weight_bf16s", ptr(w4), ptr(wp), co, ci, ks, int(for_dgrad), ns, stream())
    return wp


# bf16x3 mode: the 3 -> 64 stem conv and the prediction layer's data-gradient on the matrix cores (False: the direct fp32
# kernel, as in the other arithmetic modes; the tests compare the two)
_SCIN_MFMA = [True]


# ---- conv routing: which kernels a conv's three GEMMs run, and in which form they read their operands ----------------
@functools.lru_cache(maxsize=None)
def _gemm_kernels(Ci, Co, KS, W, up2, fmt, scin):
    """(kernel on pre-split planes or None, kernel on the fp32 tensor) of a forward-type conv GEMM Ci -> Co (a forward, or
    a data gradient with Ci / Co exchanged) in plane format ``fmt`` (0: exact fp32).  Planes are read where a planes kernel
    exists; the second name is what conv_apply runs when it is handed the fp32 tensor."""
    if not up2 and lib.itcv_conv2d_small_cout_supported(Co, KS):
        direct = "small_cout"        # <= 4 output channels: direct fp32 conv on the vector ALUs, raw OIHW weights
    elif not up2 and lib.itcv_conv2d_small_cin_supported(Ci, KS):
        # <= 4 reduction channels: the pixel's input window lives in registers; two-plane modes: on the matrix cores
        mfma = scin and _two(fmt) and lib.itcv_conv2d_small_cin_bf16x3_supported(Ci, Co, KS, W)
        direct = "small_cin_mfma" if mfma else "small_cin"
    elif fmt in (2, 3) and lib.itcv_conv2d_bf16s_supported(Ci, Co, KS):
        direct = "split"             # gather GEMM that splits its operands in the kernel
    else:
        direct = "fp32"
    if not up2 and _two(fmt) and lib.itcv_conv2d_small_cout_bf16p_supported(Ci, Co, KS):
        return "small_cout_planes", direct      # the 5x5 predict conv / stem data-gradient on the matrix cores
    if fmt and direct in ("split", "fp32") and lib.itcv_conv2d_bf16s_supported(Ci, Co, KS):
        return "planes", direct
    return None, direct


class ConvRoute(NamedTuple):
    """Everything the host decides for one conv call (stride 1, 'same' padding) in one arithmetic mode.  Kernel names:
    'planes' (LDS-DMA GEMM on pre-split planes), 'small_cout_planes' (5x5, <= 3 outputs, matrix cores), 'small_cout' /
    'small_cin' (direct fp32), 'small_cin_mfma', 'split' (in-kernel-split gather GEMM), 'fp32' (exact fp32 GEMM)."""
    fwd: str                                # kernel of the forward
    fwd_ns: int                             # plane format in which it reads x (0: reads fp32)
    fwd_fp32: str                           # kernel conv_apply runs on an fp32 x (tests compare it with the planes kernel)
    dgrad: str                              # the same three facts for the data gradient (the Co -> Ci conv on dy)
    dgrad_ns: int
    dgrad_fp32: str
    dgrad_sub: Optional[str]                # its image sub-range form (SharedPass.live): 'planes' (the whole batch's plan,
                                            # itcv_conv2d_fwd_bf16p_sub), 'small' (per-image 5x5 kernels on a batch slice),
                                            # None (fp32 / in-kernel-split GEMMs: their K split follows the launched batch)
    wgrad: str                              # 'planes' | 'stem' | 'predict' (5x5 with a <= 3-channel side) | 'raw'
    keep_xp: bool                           # forward saves x's planes instead of fp32 x
    in_mode: Tuple[int, bool]               # (ns, fp32_needed) for the producer of x ...
    grad_mode: Tuple[int, bool]             # ... and of the output gradient
    in_mode_keep_fp32: Tuple[int, bool]     # the same formats where something else reads the fp32 tensor as well
    grad_mode_keep_fp32: Tuple[int, bool]   # (skip paths of the residual block, the encoder stem)


@functools.lru_cache(maxsize=None)
def _build_route(B, Ci, H, W, Co, KS, up2, has_bias, needs_input_grad, math, scin):
    fmt = _NS[math]
    fwd_p, fwd_d = _gemm_kernels(Ci, Co, KS, W, up2, fmt, scin)
    dg_p, dg_d = _gemm_kernels(Co, Ci, KS, W, False, fmt, scin)
    fwd_ns, dgrad_ns = (fmt if fwd_p else 0), (fmt if dg_p else 0)
    if dg_p:
        sub = "planes" if dg_p == "planes" else None
    else:
        sub = "small" if dg_d in ("small_cin", "small_cin_mfma") else None
    wg_planes = bool(_two(fmt) and lib.itcv_conv2d_wgrad_bf16p_supported(B, Ci, H, W, Co, KS))
    wgrad = "planes" if wg_planes else "raw"
    if not up2 and KS == 5 and _two(fmt):       # the 5x5 weight gradient with a 3-channel side on the matrix cores
        if Ci <= 3 and lib.itcv_conv2d_wgrad5_bf16p_supported(Ci, Co, H, W):
            wgrad = "stem"
        elif Co <= 3 and lib.itcv_conv2d_wgrad5_bf16p_supported(Co, Ci, H, W):
            wgrad = "predict"
    keep_xp = _two(fwd_ns) and (wg_planes or wgrad == "predict")
    # The format of the output gradient's planes is decided by a shape-free rule (it predates the shape-aware hints and
    # also serves the blocks that always keep fp32): the data gradient's, else the mode's for the layers whose weight
    # gradient usually runs on planes.  It is NOT wg_planes; the fp32_needed flag below is what the shapes correct.
    # Changing it changes which planes a BatchNorm backward writes.
    grad_ns = dgrad_ns if needs_input_grad else 0
    if not grad_ns and _two(fmt) and (KS == 3 or (KS == 5 and Ci <= 3 and Co == 64)):
        grad_ns = fmt
    grad_planes_only = bool(grad_ns and (not needs_input_grad or dgrad_ns == grad_ns) and wg_planes and not has_bias)
    return ConvRoute(fwd_p or fwd_d, fwd_ns, fwd_d, dg_p or dg_d, dgrad_ns, dg_d, sub, wgrad, keep_xp,
                     (fwd_ns, not keep_xp), (grad_ns, not grad_planes_only), (fwd_ns, True), (grad_ns, True))


def conv_route(B, Ci, H, W, Co, KS, up2=False, has_bias=False, needs_input_grad=True):
    """The route of a conv whose OUTPUT is [B, Co, H, W] in the current mode (memoised on the full key)."""
    return _build_route(B, Ci, H, W, Co, KS, up2, has_bias, needs_input_grad, _CONV_MATH[0], _SCIN_MFMA[0])


def conv_route_of(conv, B, H, W, up2=False, needs_input_grad=True):
    """conv_route of an nn.Conv2d-like module: what the BatchNorm passes around it ask for their out_mode / grad_mode."""
    return conv_route(B, conv.in_channels, H, W, conv.out_channels, conv.kernel_size[0], bool(up2), conv.bias is not None,
                      bool(needs_input_grad))


# Data gradient of a conv that reads its input through the fused x2 upsample: the high-resolution gradient is consumed only
# as the sum of its 2x2 blocks, and itcv_conv2d_dgrad_up2_bf16p folds that sum into the conv's store.  Taken where the
# high-resolution tensor (nb * C * H * W fp32) is at least this many bytes: below the 32 MiB of aggregate L2 the round trip
# through itcv_upsample2_bwd is served on-die and the fold buys nothing, so smaller steps keep issuing the two calls (on
# purpose: the call sequence of the small configurations is pinned).  Bitwise the same result either way.
UP2_FOLD_MIN_BYTES = [32 << 20]


def set_up2_fold_min_bytes(nbytes):
    """Threshold of the fused data-gradient + upsample-adjoint route (1: wherever the library has the form)."""
    UP2_FOLD_MIN_BYTES[0] = int(nbytes)


@functools.lru_cache(maxsize=None)
def _up2_fold_route(B, Cd, H, W, Cx, KS, fmt, nb, min_bytes):
    return bool(nb * Cx * H * W * 4 >= min_bytes and lib.itcv_conv2d_dgrad_up2_supported(B, Cd, H, W, Cx, KS, fmt, nb))


def up2_fold_route(B, Cd, H, W, Cx, KS, fmt, nb):
    """Does the data gradient dy [B, Cd, H, W] -> dx [B, Cx, H/2, W/2] of an upsampled conv, over ``nb`` live images, take
    the fused route?  Decided once per shape (memoised like conv_route; kept beside the route record, not in it)."""
    return _up2_fold_route(B, Cd, H, W, Cx, KS, fmt, nb, UP2_FOLD_MIN_BYTES[0])


def missing_operand(fwd, bwd):
    """(fp32 x, sub-range form): what a backward on route ``bwd`` needs that a forward on route ``fwd`` did not leave --
    the conv math mode changed in between."""
    return bwd.wgrad == "raw" and fwd.keep_xp, fwd.dgrad_sub is not None and bwd.dgrad_sub is None


def conv_apply(x, weight, w4, for_dgrad, bias, B, Ci, H, W, Co, KS, up2, out=None):
    """Forward-type conv GEMM (forward, or data-gradient with the roles of Ci/Co swapped by the caller) on the fp32
    tensor ``x``, on the kernel selected by set_conv_math().  ``out`` (per-image <= 4-reduction-channel kernels only):
    write there."""
    fmt = _NS[_CONV_MATH[0]]
    kernel = _gemm_kernels(Ci, Co, KS, W, bool(up2), fmt, _SCIN_MFMA[0])[1]
    if out is not None and kernel not in ("small_cin", "small_cin_mfma"):
        raise abi.HipExtensionError("conv_apply: an output tensor is taken by the small-cin kernels only")
    if kernel == "fp32":
        return conv_fwd_raw(x, packed_weight(weight, w4, for_dgrad), bias, B, Ci, H, W, Co, KS, up2)
    y = out if out is not None else torch.empty((B, Co, H, W), dtype=F32, device=x.device)
    if kernel == "small_cout":
        call("itcv_conv2d_small_cout_fwd", ptr(x), ptr(w4), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(for_dgrad),
             stream())
    elif kernel == "small_cin":
        call("itcv_conv2d_small_cin_fwd", ptr(x), ptr(w4), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(for_dgrad),
             stream())
    elif kernel == "small_cin_mfma":
        # fp16 form: the data-gradient's input is a gradient tensor -> scale from its magnitude (device side)
        amax = absmax_parts(x) if (fmt == F16X2 and for_dgrad) else None
        call("itcv_conv2d_small_cin_fwd_bf16x3", ptr(x), ptr(w4), ptr(bias), ptr(y), B, Ci, H, W, Co, KS,
             int(for_dgrad), fmt, ptr(amax), stream())
    else:
        wp = packed_weight(weight, w4, for_dgrad, fmt)
        nws = lib.itcv_conv2d_fwd_bf16s_workspace(B, Ci, H, W, Co, KS)
        ws = _ws(nws, x.device) if nws else None
        call("itcv_conv2d_fwd_bf16s", ptr(x), ptr(wp), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(up2), fmt, ptr(ws), nws,
             stream())
    return y


def absmax_parts(x):
    """256 block maxima of |x| (device side): what the fp16 split kernels derive a gradient tensor's scale from."""
    parts = torch.empty(256, dtype=F32, device=x.device)
    call("itcv_absmax", ptr(x), x.numel(), ptr(parts), stream())
    return parts


def split_planes(x, ns, gradient=False):
    """fp32 [B,C,H,W] -> pre-split planes [planes][B][C/8][H][W] x 16 B in format ``ns`` (see include/itcv_hip.h).
    fp16 planes (ns = 4): activations are split with scale 1; a ``gradient`` tensor (arbitrary magnitude) with the
    power-of-two scale that maps its largest element just under 2^15 (two launches: maxima, split)."""
    B, C, H, W = x.shape
    nbytes = lib.itcv_planes_bytes(B, C, H * W, ns)
    if not nbytes:
        raise abi.HipExtensionError(f"split_planes: unsupported shape {tuple(x.shape)} / ns={ns}")
    xp = torch.empty(nbytes // 4, dtype=torch.int32, device=x.device)
    if ns == F16X2 and gradient:
        call("itcv_split_planes_scaled", ptr(x), ptr(xp), B, C, H * W, ns, ptr(absmax_parts(x)), stream())
    else:
        call("itcv_split_planes", ptr(x), ptr(xp), B, C, H * W, ns, stream())
    return xp


# BatchNorm statistics from the conv epilogue (itcv_conv2d_fwd_bf16p_st).  OFF by default: measured, the staged epilogue
# that produces them costs the band kernel more (+8 % on the 64-channel layers) than the statistics pass it replaces
# saves -- that pass reads the conv output out of the Infinity Cache right behind the conv (4-10 us) -- see DESIGN.md.
# Kept as a tested option of the C ABI (itcv_conv2d_fwd_bf16p_st), not reachable from the environment.
_FUSE_STATS = [False]


def conv_apply_planes(xp, weight, w4, for_dgrad, bias, B, Ci, H, W, Co, KS, up2, ns, want_stats=False, live=None):
    """conv_apply with the input given as pre-split planes (LDS-DMA kernel, no gather).  ``want_stats``: where the
    kernel can, it also leaves the per-tile channel sums of its output for the BatchNorm that follows
    (attached to the result as ``_itcv_tile_stats``; BnActFn then skips its own statistics pass).
    ``live`` = (b0, nb): only these images of the B-image tensors are computed, with the whole batch's launch plan."""
    if live is None and _gemm_kernels(Ci, Co, KS, W, bool(up2), ns, _SCIN_MFMA[0])[0] == "small_cout_planes":
        y = torch.empty((B, Co, H, W), dtype=F32, device=xp.device)
        call("itcv_conv2d_small_cout_fwd_bf16p", ptr(xp), ptr(w4), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(for_dgrad),
             ns, stream())
        return y
    wp = packed_weight(weight, w4, for_dgrad, ns)
    y = _new_grad((B, Co, H, W), xp.device, live)
    nws = lib.itcv_conv2d_fwd_bf16p_workspace(B, Ci, H, W, Co, KS, ns)
    ws = _ws(nws, xp.device) if nws else None
    if live is not None:
        call("itcv_conv2d_fwd_bf16p_sub", ptr(xp), ptr(wp), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(up2), ns, live[0],
             live[1], ptr(ws), nws, stream())
        return y
    T = lib.itcv_conv2d_fwd_bf16p_stat_tiles(B, Ci, H, W, Co, KS, ns) if (want_stats and _FUSE_STATS[0]) else 0
    stats = torch.empty((2, Co, T), dtype=F32, device=xp.device) if T else None
    call("itcv_conv2d_fwd_bf16p_st", ptr(xp), ptr(wp), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(up2), ns, ptr(stats),
         ptr(ws), nws, stream())
    if stats is not None:
        y._itcv_tile_stats = (stats, T, 256, y._version, y.data_ptr())     # 256 = (image, pixel) positions per tile
    return y


def _tile_stats_of(x, B, G, HW):
    """(stats, tiles per group, pitch) when ``x`` carries the producing conv's per-tile channel sums and the BatchNorm
    groups are whole numbers of tiles, else None."""
    tag = getattr(x, "_itcv_tile_stats", None)
    if tag is None or tag[3] != x._version or tag[4] != x.data_ptr():
        return None
    stats, T, px = tag[0], tag[1], tag[2]
    if T * px != B * HW or (B // G * HW) % px:
        return None
    return stats, T // G, T


# ---- deferred slab reduces of the planes weight gradients ------------------------------------------------------------
# Inside deferred_wgrad_reduces() (the solvers wrap loss.backward() in it) a weight gradient that accumulates into an
# existing .grad leaves its split-K slabs in a persistent buffer and is folded, together with all the other layers of the
# backward pass, by ONE table-driven launch when the block ends (36 reduce launches per intro step -> 3).  Same summation
# order as the per-call reduce: bitwise equal.  Slab buffers are kept per position in the backward's call sequence and the
# device tables per sequence of (slab, target) pointers, so a steady-state step (and its hipGraph) allocates and copies
# nothing.
_DEFER = {"on": False, "pending": [], "pool": {}, "tables": {}}


@contextlib.contextmanager
def deferred_wgrad_reduces():
    prev, _DEFER["on"] = _DEFER["on"], True
    try:
        yield
    finally:
        _DEFER["on"] = prev
        if not prev:
            flush_wgrad_reduces()


def flush_wgrad_reduces():
    pend = _DEFER["pending"]
    if not pend:
        return
    # group the calls by target (a weight used by several network passes of the backward), keeping call order
    groups = {}
    for ws, dw, co, ci, slabs in pend:
        groups.setdefault(dw.data_ptr(), [dw, co, ci, []])[3].append((ws, slabs))
    key = tuple((k, tuple((w.data_ptr(), n) for w, n in g[3])) for k, g in groups.items())
    tab = _DEFER["tables"].get(key)
    if tab is None:
        descs = []
        for dw, co, ci, srcs in groups.values():
            for c0 in range(0, len(srcs), 4):          # at most four slab sources per descriptor; later ones accumulate
                descs.append((dw, co, ci, srcs[c0:c0 + 4]))
        # descriptors of one target that were split into several (> 4 sources) would race inside one launch
        if len(descs) != len(groups):
            raise abi.HipExtensionError("deferred weight-gradient reduce: more than four passes over one weight")

        def fill(slot, desc, blocks):
            dw, co, ci, part = desc
            sl = (ctypes.c_void_p * len(part))(*[w.data_ptr() for w, _ in part])
            sp = (ctypes.c_int * len(part))(*[n for _, n in part])
            return lib.itcv_wgrad_reduce_desc(slot, sl, sp, len(part), dw.data_ptr(), co, ci, 1, blocks)

        if len(_DEFER["tables"]) > 64:
            _DEFER["tables"].clear()
        tab = _DEFER["tables"][key] = _desc_table("itcv_wgrad_reduce_desc", lib.itcv_wgrad_reduce_desc_bytes(), descs, fill,
                                                  pend[0][1].device)
    call("itcv_wgrad_reduce_many", ptr(tab[0]), tab[1], tab[2], stream())
    pend.clear()


def _defer_slab_buffer(nbytes, device):
    """Persistent slab buffer for the next deferred call: one per position in the pending sequence (and size)."""
    k = (len(_DEFER["pending"]), int(nbytes), str(device))
    buf = _DEFER["pool"].get(k)
    if buf is None:
        buf = _DEFER["pool"][k] = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    return buf


def conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, KS, up2, out=None, accumulate=False, ns=2):
    """Weight gradient from the pre-split planes of x and dy (two-plane formats; transposing-LDS-read kernel)."""
    dw = out if out is not None else torch.empty((Co, Ci, KS, KS), dtype=F32, device=xp.device)
    nws = lib.itcv_conv2d_wgrad_bf16p_workspace(B, Ci, H, W, Co, KS)
    if _DEFER["on"] and out is not None and accumulate:
        same = sum(1 for p in _DEFER["pending"] if p[1].data_ptr() == dw.data_ptr())
        if same >= 4 or (same == 0 and len({p[1].data_ptr() for p in _DEFER["pending"]}) >= lib.itcv_wgrad_reduce_max_descs()):
            flush_wgrad_reduces()                      # four sources per weight, a bounded table per launch
        ws = _defer_slab_buffer(nws, xp.device)
        call("itcv_conv2d_wgrad_bf16p", ptr(xp), ptr(dyp), ptr(dw), B, Ci, H, W, Co, KS, int(up2), int(ns), 2, ptr(ws), nws,
             stream())
        _DEFER["pending"].append((ws, dw, Co, Ci, lib.itcv_conv2d_wgrad_bf16p_slabs(B, Ci, H, W, Co, KS)))
        # (flushing mid-backward, every 48 / 96 / 192 MB of slabs, so that the fold reads them out of the Infinity Cache,
        # measured slower on one box: 16.90-16.93 ms per c2 step against 16.70-16.78 with one fold per backward)
        return dw
    ws = _ws(nws, xp.device)

    call("itcv_conv2d_wgrad_bf16p", ptr(xp), ptr(dyp), ptr(dw), B, Ci, H, W, Co, KS, int(up2), int(ns), int(accumulate),
         ptr(ws), nws, stream())
    return dw


def pack_weight(w4, for_dgrad):
    """w4 [Co,Ci,KS,KS] -> packed K-major operand (see include/itcv_hip.h)."""
    co, ci, ks = w4.shape[0], w4.shape[1], w4.shape[2]
    wp = torch.empty(lib.itcv_conv2d_packed_weight_elems(co, ci, ks, for_dgrad), dtype=F32, device=w4.device)
    call("itcv_conv2d_pack_weight", ptr(w4), ptr(wp), co, ci, ks, int(for_dgrad), stream())
    return wp


class LaunchProfile:
    """Per-launch timing of the GEMM-class kernels, recorded INSIDE libitcv_hip.so: a HIP event pair on
    the launch stream around the main kernel of every conv call (bench.py's roofline leg)."""
    KINDS = {0: "conv_fwd_kernel", 1: "conv_fwd_bf16s_kernel", 2: "conv_wgrad_kernel", 3: "conv_wgrad_bf16s_kernel",
             4: "conv_small_cout_kernel", 5: "conv_small_cin_kernel", 6: "conv_fwd_bf16p_kernel",
             7: "conv_wgrad_bf16p_kernel", 8: "conv_fwd_bf16p2_kernel", 9: "conv_fwd_bf16p3_kernel",
             10: "conv_small_cout_planes_kernel", 11: "conv_small_cin_mfma_kernel", 12: "conv_wgrad5_planes_kernel",
             13: "bn_act_fwd_planes_kernel", 14: "bn_bwd_apply_planes"}
    HBM_KINDS = (13, 14)     # HBM-bound kernels: the record's "work" is algorithmic BYTES, not FLOP

    @classmethod
    def begin(cls):
        call("itcv_profile_begin")

    @classmethod
    def end(cls):
        """-> list of (kernel label, algorithmic FLOP, seconds)."""
        n = lib.itcv_profile_end()
        code, flop, ms = ctypes.c_int(), ctypes.c_double(), ctypes.c_float()
        out = []
        for i in range(n):
            call("itcv_profile_get", i, ctypes.byref(code), ctypes.byref(flop), ctypes.byref(ms))
            c = code.value
            kind, ks, bm, up2, ns = c & 15, (c >> 4) & 15, (c >> 8) & 255, (c >> 16) & 1, (c >> 20) & 15
            if kind in (0, 2):
                label = f"{cls.KINDS[kind]}<KS={ks},BM={bm},up2={up2}>"
            elif kind in (7, 8, 9):   # templates <LOG2W, ...>: the KS field carries log2(W); 9 = persistent band kernel
                label = f"{cls.KINDS[kind]}<LOG2W={ks},BM={bm},up2={up2},NS={ns}>"
            elif kind in (1, 3, 6):
                label = f"{cls.KINDS[kind]}<KS={ks},BM={bm},up2={up2},NS={ns}>"
            elif kind in cls.HBM_KINDS:    # BatchNorm apply passes: channels, image width, pool / adjoint mode, plane format
                label = f"{cls.KINDS[kind]}<C={8 * bm},W={1 << ks},mode={(c >> 16) & 15},NS={ns}>"
            elif kind in (10, 11, 12):     # the 5x5 layers on the matrix cores: C = the narrow side's channels
                label = f"{cls.KINDS[kind]}<KS={ks},C={bm},stem={up2},NS={ns}>"
            else:
                label = f"{cls.KINDS[kind]}<KS={ks},C={bm}>"
            out.append((label, flop.value, ms.value * 1e-3))
        call("itcv_profile_clear")
        return out


def conv_fwd_raw(x, wp, bias, B, Ci, H, W, Co, KS, up2):
    y = torch.empty((B, Co, H, W), dtype=F32, device=x.device)
    nws = lib.itcv_conv2d_fwd_workspace(B, Ci, H, W, Co, KS)
    ws = _ws(nws, x.device) if nws else None

    call("itcv_conv2d_fwd", ptr(x), ptr(wp), ptr(bias), ptr(y), B, Ci, H, W, Co, KS, int(up2), ptr(ws), nws, stream())
    return y


def conv_wgrad_raw(x, dy, B, Ci, H, W, Co, KS, up2, out=None, accumulate=False):
    dw = out if out is not None else torch.empty((Co, Ci, KS, KS), dtype=F32, device=x.device)
    nws = lib.itcv_conv2d_wgrad_workspace(B, Ci, H, W, Co, KS)
    ws = _ws(nws, x.device)
    ns = _NS[_CONV_MATH[0]]
    if ns in (2, 3) and lib.itcv_conv2d_wgrad_bf16s_supported(Ci, H, W, Co, KS):
        if up2:   # the split kernel reads 8-pixel chunks: materialise the x2 nearest upsampling once
            xu = torch.empty((B, Ci, H, W), dtype=F32, device=x.device)
            call("itcv_upsample2_fwd", ptr(x), ptr(xu), B * Ci, H // 2, W // 2, stream())
            x = xu

        call("itcv_conv2d_wgrad_bf16s", ptr(x), ptr(dy), ptr(dw), B, Ci, H, W, Co, KS, ns, int(accumulate), ptr(ws), nws,
             stream())
        return dw

    call("itcv_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), B, Ci, H, W, Co, KS, int(up2), int(accumulate), ptr(ws), nws,
         stream())
    return dw


def bias_grad_raw(dy, B, C, HW, target=None):
    """db = sum_{b,hw} dy; with ``target`` the sum is added into it and None is returned."""
    db = target if target is not None else torch.empty((C,), dtype=F32, device=dy.device)
    nws = lib.itcv_bias_grad_workspace(B, C, HW)
    ws = _ws(nws, dy.device)
    call("itcv_bias_grad", ptr(dy), ptr(db), B, C, HW, int(target is not None), ptr(ws), nws, stream())
    return None if target is not None else db


PLANES_STATS = [0, 0]   # conv operands taken from producer-attached planes / split on demand (diagnostic)


def _tag_planes(t, planes, ns, fp32_valid=True):
    """Attach the pre-split planes of ``t`` to the tensor object (consumed by the next conv GEMM).
    ``fp32_valid=False``: the producer did not write ``t`` itself -- only the planes carry its values."""
    t._itcv_planes = (planes, ns, t._version, t.data_ptr(), fp32_valid)


def _require_fp32(t, what):
    tag = getattr(t, "_itcv_planes", None)
    if tag is not None and not tag[4]:
        raise abi.HipExtensionError(f"{what}: this tensor was produced as planes only (fp32 values not written)")
    return t


def _tagged_planes(t, ns):
    tag = getattr(t, "_itcv_planes", None)
    if tag is None or tag[1] != ns or tag[2] != t._version or tag[3] != t.data_ptr():
        return None
    return tag[0]


def planes_of(t, ns, gradient=False):
    """Planes of ``t``: the ones its producer attached, else a split pass (``gradient``: see split_planes)."""
    p = _tagged_planes(t, ns)
    PLANES_STATS[0 if p is not None else 1] += 1
    return p if p is not None else split_planes(t, ns, gradient)


def conv_wgrad5_planes(small, big_planes, B, Cs, H, W, stem, out=None, accumulate=False, ns=2):
    """5x5 weight gradient with a <= 3-channel side from the planes of the 64-channel side.  fp16 form: the predict
    conv's small side is a gradient tensor and gets a device-side scale; the stem's is the input image (scale 1)."""
    dw = out if out is not None else torch.empty((64, Cs, 5, 5) if stem else (Cs, 64, 5, 5), dtype=F32, device=small.device)
    nws = lib.itcv_conv2d_wgrad5_bf16p_workspace(B, H)
    ws = _ws(nws, small.device)

    amax = absmax_parts(small) if (ns == F16X2 and not stem) else None
    call("itcv_conv2d_wgrad5_bf16p", ptr(small), ptr(big_planes), ptr(dw), B, Cs, H, W, int(stem), int(ns), ptr(amax),
         int(accumulate), ptr(ws), nws, stream())
    return dw


class Conv2dFn(Function):
    """nn.Conv2d(stride 1, padding KS//2) forward/backward; ``up2`` reads the input through a
    virtual nearest x2 upsampling (models.py:284-286 fused into the consumer conv).

    In the split-bf16 modes the operands travel as pre-split planes: x is split once in forward (and
    kept for the weight gradient), dy once in backward (shared by data- and weight-gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, up2):
        x, weight = _f32c(x), _f32c(weight)
        B, Ci, Hs, Ws = x.shape
        Co, KS = weight.shape[0], weight.shape[2]
        H, W = (Hs * 2, Ws * 2) if up2 else (Hs, Ws)
        b = None if bias is None else _f32c(bias)
        r = conv_route(B, Ci, H, W, Co, KS, bool(up2), bias is not None, ctx.needs_input_grad[0])
        xp = None
        if r.fwd_ns:
            xp = planes_of(x, r.fwd_ns)
            y = conv_apply_planes(xp, weight, weight, 0, b, B, Ci, H, W, Co, KS, up2, r.fwd_ns, want_stats=True)
        else:
            y = conv_apply(_require_fp32(x, "Conv2dFn.forward"), weight, weight, 0, b, B, Ci, H, W, Co, KS, up2)
        ctx.save_for_backward(None if r.keep_xp else _require_fp32(x, "Conv2dFn.forward (saved input)"), weight, bias,
                              xp if r.keep_xp else None)
        ctx.cfg = (B, Ci, H, W, Co, KS, up2, bias is not None, (Hs, Ws))
        ctx.route = r
        ctx.shared = _SHARED_PASS[0]
        ctx.shared_first = ctx.shared is not None and ctx.shared._claim_first()
        if ctx.shared is not None and r.dgrad_sub is None:
            _block_live(f"conv {Ci}->{Co} k{KS}: data gradient without a sub-range form in mode {_CONV_MATH[0]}")
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, bias, xp = ctx.saved_tensors
        B, Ci, H, W, Co, KS, up2, has_bias, (Hs, Ws) = ctx.cfg
        dy = _f32c(dy)
        dx = dw = db = None
        # a pass shared by two backward passes (SharedPass): parameter / input gradients only where this one wants them
        need_x = ctx.needs_input_grad[0] and not (ctx.shared_first and not ctx.shared.input_grad)
        need_w = ctx.needs_input_grad[1] and _shared_ok(ctx, "param_grads")
        need_b = ctx.needs_input_grad[2] and _shared_ok(ctx, "param_grads")
        r = conv_route(B, Ci, H, W, Co, KS, bool(up2), has_bias, ctx.needs_input_grad[0])    # of the mode as it is now
        no_x, no_sub = missing_operand(ctx.route, r)
        ns_d = r.dgrad_ns if need_x else 0
        wgrad = r.wgrad if need_w else None
        fmt2 = F16X2 if _NS[_CONV_MATH[0]] == F16X2 else 2       # the two-plane format of the current mode
        live = _live_images(ctx, B) if need_x else None          # (param_grads is off then: no weight / bias gradient)
        if live is not None and no_sub:
            raise abi.HipExtensionError("Conv2dFn.backward: conv math mode changed inside a shared pass")
        if wgrad is not None and no_x:
            raise abi.HipExtensionError("Conv2dFn.backward: conv math mode changed between forward and backward")
        if live is not None and ns_d and _tagged_planes(dy, ns_d) is None:
            # no planes from the producer: the split pass reads the whole tensor, so the dead images become the zeros they stand for
            full = torch.zeros_like(dy)
            full[live[0]:live[0] + live[1]] = dy[live[0]:live[0] + live[1]]
            dy = full
        dyp = planes_of(dy, ns_d if ns_d else fmt2, gradient=True) if (ns_d or wgrad == "planes") else None
        if need_x:
            b0, nb = live if live is not None else (0, B)
            fold = bool(up2 and ns_d) and up2_fold_route(B, Co, H, W, Ci, KS, ns_d, nb)
            if fold:
                # the upsample's adjoint folded into the conv's store: the H x W gradient is never written
                dx = _new_grad((B, Ci, H // 2, W // 2), dy.device, live)
                call("itcv_conv2d_dgrad_up2_bf16p", ptr(dyp), ptr(packed_weight(weight, weight, 1, ns_d)), ptr(dx), B, Co, H, W,
                     Ci, KS, ns_d, b0, nb, None, 0, stream())
            elif ns_d:
                dx = conv_apply_planes(dyp, weight, weight, 1, None, B, Co, H, W, Ci, KS, False, ns_d, live=live)
            elif live is not None:
                # the per-image 5x5 kernels on the live images (a contiguous slice; the fp16 scale comes from their maximum,
                # which is the whole tensor's: the rest is zero)
                sl = slice(live[0], live[0] + live[1])
                dx = _new_grad((B, Ci, H, W), dy.device, live)
                conv_apply(_require_fp32(dy, "Conv2dFn.backward")[sl], weight, weight, 1, None, live[1], Co, H, W, Ci, KS, False,
                           out=dx[sl])
            else:
                dx = conv_apply(_require_fp32(dy, "Conv2dFn.backward"), weight, weight, 1, None, B, Co, H, W, Ci, KS, False)
            if up2 and not fold:
                lo = _new_grad((B, Ci, H // 2, W // 2), dy.device, live)
                call("itcv_upsample2_bwd", ptr(dx[b0:b0 + nb]), ptr(lo[b0:b0 + nb]), nb * Ci, H // 2, W // 2, stream())
                dx = lo
        if wgrad is not None:
            # into .grad where the solvers' flat buffers take it (autograd then gets None), else a fresh tensor
            tgt = _grad_target(weight)
            into = dict(out=tgt, accumulate=tgt is not None)
            if wgrad == "stem":
                big = dyp if dyp is not None else planes_of(dy, fmt2, gradient=True)
                dw = conv_wgrad5_planes(_require_fp32(x, "Conv2dFn.backward (5x5 weight gradient)"), big, B, Ci, H, W, True,
                                        ns=fmt2, **into)
            elif wgrad == "predict":
                big = xp if xp is not None else split_planes(x, fmt2)
                dw = conv_wgrad5_planes(_require_fp32(dy, "Conv2dFn.backward (5x5 weight gradient)"), big, B, Co, H, W, False,
                                        ns=fmt2, **into)
            elif wgrad == "planes":
                dw = conv_wgrad_planes(xp if xp is not None else split_planes(x, fmt2), dyp, B, Ci, H, W, Co, KS, up2,
                                       ns=fmt2, **into)
            else:
                dw = conv_wgrad_raw(x, _require_fp32(dy, "Conv2dFn.backward (weight gradient)"), B, Ci, H, W, Co, KS, up2,
                                    **into)
            if tgt is not None:
                dw = None
        if has_bias and need_b:
            db = bias_grad_raw(_require_fp32(dy, "Conv2dFn.backward (bias gradient)"), B, Co, H * W, _grad_target(bias))
        return dx, dw, db, None


class LinearFn(Function):
    """nn.Linear on the skinny fp32 MFMA GEMMs (itcv_linear_*): exact fp32 in every conv-math mode."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, weight = _f32c(x), _f32c(weight)
        B, K = x.shape
        N = weight.shape[0]
        y = torch.empty((B, N), dtype=F32, device=x.device)
        nws = lib.itcv_linear_workspace(B, K, N)
        ws = _ws(nws, x.device) if nws else None
        call("itcv_linear_fwd", ptr(x), ptr(weight), ptr(None if bias is None else _f32c(bias)), ptr(y), B, K, N, ptr(ws),
             nws, stream())
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (B, K, N, bias is not None)
        ctx.shared = _SHARED_PASS[0]
        ctx.shared_first = ctx.shared is not None and ctx.shared._claim_first()
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        B, K, N, has_bias = ctx.cfg
        dy = _f32c(dy)
        dx = dw = db = None
        nws = lib.itcv_linear_workspace(B, K, N)
        need_p = _shared_ok(ctx, "param_grads")       # see SharedPass
        if ctx.needs_input_grad[0] and not (ctx.shared_first and not ctx.shared.input_grad):
            dx = torch.empty((B, K), dtype=F32, device=dy.device)
            ws = _ws(nws, dy.device) if nws else None
            call("itcv_linear_dgrad", ptr(dy), ptr(weight), ptr(dx), B, K, N, ptr(ws), nws, stream())
        if ctx.needs_input_grad[1] and need_p:
            tgt = _grad_target(weight)
            dw = None if tgt is not None else torch.empty((N, K), dtype=F32, device=dy.device)
            ws = _ws(nws, dy.device) if nws else None
            call("itcv_linear_wgrad", ptr(dy), ptr(x), ptr(tgt if tgt is not None else dw), B, K, N,
                 int(tgt is not None), ptr(ws), nws, stream())
        if has_bias and ctx.needs_input_grad[2] and need_p:
            db = bias_grad_raw(dy, B, N, 1, _grad_target(bias))
        return dx, dw, db


# ------------------------------------------------------------------ BatchNorm + LeakyReLU (+pool)
def _world(group):
    return dist.get_world_size(group) if (group is not None and dist.is_initialized()) else 1


class BnActFn(Function):
    """y = pool(lrelu(BN_train(x) (+skip), slope)).  slope=1 -> plain BatchNorm; pool in {0,1}.
    ``group``: process group for Sync-BN (moments all-reduced in fp64).
    ``bn_groups`` = G > 1: the batch holds G independent network passes of B/G images each (the solvers push passes
    that share their weights through the conv GEMMs as ONE batch); every pass is normalised with its own batch
    statistics and advances the running buffers on its own, in order -- exactly G separate BatchNorm calls
    (models.py:37-38), issued here as G launches on sub-batches of the same tensors."""

    @staticmethod
    def forward(ctx, x, gamma, beta, skip, running_mean, running_var, nbt, eps, momentum, slope, pool, training,
                group, out_planes=0, grad_planes=0, out_fp32=True, grad_fp32=True, bn_groups=1):
        x, gamma, beta = _f32c(x), _f32c(gamma), _f32c(beta)
        skip = None if skip is None else _f32c(skip)
        B, C, H, W = x.shape
        G = int(bn_groups) if training else 1
        if G < 1 or B % G:
            raise abi.HipExtensionError(f"BatchNorm groups: batch {B} is not {G} equal passes")
        Bg = B // G
        dev = x.device
        shared = _SHARED_PASS[0]
        uvar = None
        if shared is not None and (not training or _world(group) != 1 or skip is not None or G != int(bn_groups)
                                   or not lib.itcv_bn_act_planes_supported(C, H, W, 0)):
            _block_live(f"BatchNorm C={C} {H}x{W}: eval / Sync-BN / skip input / a shape the planes kernels do not take")
        if shared is not None and training:
            # mean and the unbiased variance blended into running_var go to the pass's persistent buffer (SharedPass.replay)
            mean, uvar = shared._stats(G, C, dev)
        else:
            mean = torch.empty((G, C), dtype=F32, device=dev)
        rstd = torch.empty((G, C), dtype=F32, device=dev)
        world = _world(group) if training else 1
        oshape = (B, C, H // 2, W // 2) if pool else (B, C, H, W)
        y = torch.empty(oshape, dtype=F32, device=dev)
        yp, pstride = None, 0
        if F16X2 in (out_planes, grad_planes) and not (training and world == 1):
            # fp16 planes carry one scale record per tensor, written by the single-call training forms (itcv_bn_train_fwd /
            # _bwd); the per-group eval / Sync-BN calls below hand the consumers fp32 tensors instead (split on demand)
            out_planes = 0 if out_planes == F16X2 else out_planes
            grad_planes = 0 if grad_planes == F16X2 else grad_planes
            out_fp32 = grad_fp32 = True
        if out_planes and lib.itcv_bn_act_planes_supported(C, H, W, int(pool)):
            yp = torch.empty(lib.itcv_planes_bytes(B, C, oshape[2] * oshape[3], out_planes) // 4, dtype=torch.int32,
                             device=dev)
            pstride = B * (C // 8) * oshape[2] * oshape[3]            # chunks between planes of the WHOLE tensor
        write_y = out_fp32 or yp is None or _POISON[0]
        nws = lib.itcv_bn_workspace(Bg, C, H * W) * G      # every group's partial sums (one launch for all groups)
        ts = _tile_stats_of(x, B, G, H * W) if (training and world == 1) else None
        if training and world == 1:
            # statistics + apply for all G groups in one call (small layers: one statistics launch walking the groups in
            # order + one apply launch; large layers: the groups one after the other inside the library)
            ws = _ws(nws, dev)
            head = (ptr(x), ptr(gamma), ptr(beta), ptr(skip), ptr(y) if write_y else None, ptr(yp), int(out_planes), Bg, C, H,
                    W, float(slope), int(pool), float(eps), float(momentum), ptr(running_mean), ptr(running_var), ptr(nbt),
                    ptr(mean), ptr(rstd))
            tail = (ptr(ws), nws, pstride, None if ts is None else ts[0].data_ptr(), ts[1] if ts else 0, ts[2] if ts else 0,
                    G, stream())
            if uvar is None:
                call("itcv_bn_train_fwd", *head, *tail)
            else:
                call("itcv_bn_train_fwd_uv", *head, ptr(uvar), *tail)
        for g in (range(G) if not (training and world == 1) else ()):
            r = slice(g * Bg, (g + 1) * Bg)
            xg, yg = x[r], (y[r] if write_y else None)
            sg = None if skip is None else skip[r]
            ypg = None if yp is None else yp[g * Bg * (C // 8) * oshape[2] * oshape[3] * 4:]    # int32 elements
            if training:
                ws = _ws(nws, dev)
                sums = torch.empty((2 * C,), dtype=torch.float64, device=dev)
                call("itcv_bn_moments", ptr(xg), ptr(sums), Bg, C, H * W, ptr(ws), nws, stream())
                dist.all_reduce(sums, group=group)
                call("itcv_bn_finalize_uv", ptr(sums), float(Bg * H * W * world), float(eps), float(momentum),
                     ptr(running_mean), ptr(running_var), ptr(nbt), ptr(mean[g]), ptr(rstd[g]),
                     None if uvar is None else ptr(uvar[g]), C, stream())
            else:
                call("itcv_bn_eval_stats", ptr(running_mean), ptr(running_var), float(eps), ptr(mean[g]), ptr(rstd[g]), C,
                     stream())
            call("itcv_bn_act_fwd", ptr(xg), ptr(mean[g]), ptr(rstd[g]), ptr(gamma), ptr(beta), ptr(sg), ptr(yg), Bg, C, H, W,
                 float(slope), int(pool), ptr(ypg), int(out_planes), pstride, stream())
        if yp is not None:
            if _POISON[0] and not out_fp32:
                y.fill_(float("nan"))
            _tag_planes(y, yp, out_planes, bool(out_fp32))
        if uvar is not None:
            shared.records.append((running_mean, running_var, nbt, mean, uvar, float(momentum)))
        ctx.shared = shared
        ctx.save_for_backward(x, gamma, beta, mean, rstd, skip)
        ctx.params = (gamma, beta)
        if not lib.itcv_bn_act_planes_supported(C, H, W, 0):
            grad_planes = 0
        ctx.cfg = (B, C, H, W, float(slope), int(pool), bool(training), group, world, int(grad_planes),
                   bool(grad_fp32) or not grad_planes, G)
        ctx.mark_non_differentiable(*[t for t in (running_mean, running_var, nbt) if t is not None])
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, gamma, beta, mean, rstd, skip = ctx.saved_tensors
        B, C, H, W, slope, pool, training, group, world, grad_planes, grad_fp32, G = ctx.cfg
        if not training:
            raise abi.HipExtensionError("BatchNorm backward in eval mode is not part of the training hot path")
        dy = _f32c(dy)
        dev = x.device
        Bg = B // G
        nws = lib.itcv_bn_workspace(Bg, C, H * W) * G
        # parameter gradients come out of the reduce launch: either added straight into .grad
        # (solver mode) or into fresh tensors handed to autograd
        need_g = ctx.needs_input_grad[1] and _shared_ok(ctx, "param_grads")       # see SharedPass
        need_b = ctx.needs_input_grad[2] and _shared_ok(ctx, "param_grads")
        tg = _grad_target(gamma) if need_g else None
        tb = _grad_target(beta) if need_b else None
        direct = tg is not None and tb is not None
        dgamma = dbeta = None
        if direct:
            pg, pb = tg, tb
        else:
            dgamma = torch.empty_like(gamma) if need_g else None
            dbeta = torch.empty_like(beta) if need_b else None
            pg, pb = dgamma, dbeta
        live = _live_images(ctx, B) if world == 1 else None
        if live is not None and (ctx.shared.live[1] != G or skip is not None):
            raise abi.HipExtensionError("BnActFn.backward: SharedPass.live does not match the BatchNorm groups of the pass")
        dx = _new_grad(x, live=live)
        dskip = torch.empty_like(x) if (skip is not None and ctx.needs_input_grad[3]) else None
        dxp, pstride = None, 0
        if grad_planes:
            dxp = torch.empty(lib.itcv_planes_bytes(B, C, H * W, grad_planes) // 4, dtype=torch.int32, device=dev)
            pstride = B * (C // 8) * H * W
        write_dx = grad_fp32 or dxp is None or _POISON[0]
        if world == 1:
            ws = _ws(nws, dev)
            local = torch.empty((G, 2 * C), dtype=torch.float64, device=dev)
            head = (ptr(x), ptr(dy), ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), ptr(skip), ptr(local),
                    ptr(dx) if write_dx else None, ptr(dskip), ptr(dxp), grad_planes, ptr(pg), ptr(pb), 1 if direct else 0, Bg,
                    C, H, W, slope, pool, 0, ptr(ws), nws, pstride, G)
            if live is None:
                call("itcv_bn_train_bwd", *head, stream())
            else:       # dy is zero outside the live group: no dy read, no apply, no stores there (fp16: the scale still sees x)
                call("itcv_bn_train_bwd_live", *head, ctx.shared.live[0], 1, stream())
        for g in (range(G) if world != 1 else ()):
            r = slice(g * Bg, (g + 1) * Bg)
            acc = 1 if (direct or g > 0) else 0       # the groups' parameter gradients add up
            xg, dyg = x[r], dy[r]
            sg = None if skip is None else skip[r]
            dxg = dx[r] if write_dx else None
            dsg = None if dskip is None else dskip[r]
            dxpg = None if dxp is None else dxp[g * Bg * (C // 8) * H * W * 4:]
            ws = _ws(nws, dev)
            local = torch.empty((2 * C,), dtype=torch.float64, device=dev)
            call("itcv_bn_act_bwd_reduce", ptr(xg), ptr(dyg), ptr(mean[g]), ptr(rstd[g]), ptr(gamma), ptr(beta), ptr(sg),
                 ptr(local), ptr(pg), ptr(pb), acc, Bg, C, H, W, slope, pool, 0, ptr(ws), nws, stream())
            total = local.clone()
            dist.all_reduce(total, group=group)
            call("itcv_bn_act_bwd_apply", ptr(xg), ptr(dyg), ptr(mean[g]), ptr(rstd[g]), ptr(gamma), ptr(beta), ptr(sg),
                 ptr(total), None, float(Bg * H * W * world), ptr(dxg), ptr(dsg), None, None, 0, Bg, C, H, W, slope,
                 pool, 0, ptr(dxpg), grad_planes, pstride, stream())
        if dxp is not None:
            if _POISON[0] and not grad_fp32:
                dx.fill_(float("nan"))
            _tag_planes(dx, dxp, grad_planes, bool(grad_fp32))
        return (dx, dgamma, dbeta, dskip) + (None,) * 14


# ------------------------------------------------------------------ pointwise / resampling
class LeakyReluFn(Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = _f32c(x)
        y = torch.empty_like(x)
        call("itcv_lrelu_fwd", ptr(x), ptr(y), x.numel(), float(slope), stream())
        ctx.save_for_backward(x)
        ctx.slope = float(slope)
        ctx.shared = _SHARED_PASS[0]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _f32c(dy)
        live = _live_images(ctx, x.shape[0]) if x.dim() else None
        if live is not None:
            # the live rows; the dead rows get the zeros a zero dy gives: what follows (LinearFn) runs its full form
            r = slice(live[0], live[0] + live[1])
            dx = torch.zeros_like(x)
            call("itcv_lrelu_bwd", ptr(x[r]), ptr(dy[r]), ptr(dx[r]), x[r].numel(), ctx.slope, stream())
            return dx, None
        dx = torch.empty_like(x)
        call("itcv_lrelu_bwd", ptr(x), ptr(dy), ptr(dx), x.numel(), ctx.slope, stream())
        return dx, None


class SigmoidFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        y = torch.empty_like(x)
        call("itcv_sigmoid_fwd", ptr(x), ptr(y), x.numel(), stream())
        ctx.save_for_backward(y)
        ctx.shared = _SHARED_PASS[0]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _f32c(dy)
        live = _live_images(ctx, y.shape[0]) if y.dim() else None
        dx = _new_grad(y, live=live)
        r = slice(None) if live is None else slice(live[0], live[0] + live[1])
        call("itcv_sigmoid_bwd", ptr(y[r]), ptr(dy[r]), ptr(dx[r]), y[r].numel(), stream())
        return dx


class AvgPool2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        B, C, H, W = x.shape
        y = torch.empty((B, C, H // 2, W // 2), dtype=F32, device=x.device)
        call("itcv_avgpool2_fwd", ptr(x), ptr(y), B * C, H, W, stream())
        _block_live("average pool")
        ctx.shape = (B, C, H, W)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _f32c(dy)
        dx = torch.empty((B, C, H, W), dtype=F32, device=dy.device)
        call("itcv_avgpool2_bwd", ptr(dy), ptr(dx), B * C, H, W, stream())
        return dx


class Upsample2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32c(x)
        B, C, H, W = x.shape
        y = torch.empty((B, C, 2 * H, 2 * W), dtype=F32, device=x.device)
        call("itcv_upsample2_fwd", ptr(x), ptr(y), B * C, H, W, stream())
        ctx.shape = (B, C, H, W)
        ctx.shared = _SHARED_PASS[0]
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, C, H, W = ctx.shape
        dy = _f32c(dy)
        live = _live_images(ctx, B)
        b0, nb = live if live is not None else (0, B)
        dx = _new_grad((B, C, H, W), dy.device, live)
        call("itcv_upsample2_bwd", ptr(dy[b0:b0 + nb]), ptr(dx[b0:b0 + nb]), nb * C, H, W, stream())
        return dx


class AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _f32c(a), _f32c(b)
        out = torch.empty_like(a)
        call("itcv_add", ptr(a), ptr(b), ptr(out), a.numel(), stream())
        _block_live("residual add")
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


# ------------------------------------------------------------------ latent math
class ReparamFn(Function):
    """ops.py:166-185 with the N(0,1) draw as an explicit input."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar, eps = _f32c(mu), _f32c(logvar), _f32c(eps)
        z = torch.empty_like(mu)
        call("itcv_reparam_fwd", ptr(mu), ptr(logvar), ptr(eps), ptr(z), mu.numel(), stream())
        ctx.save_for_backward(logvar, eps)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, dz):
        logvar, eps = ctx.saved_tensors
        dz = _f32c(dz)
        dmu, dlv = torch.empty_like(dz), torch.empty_like(dz)
        call("itcv_reparam_bwd", ptr(dz), ptr(logvar), ptr(eps), ptr(dmu), ptr(dlv), dz.numel(), stream())
        return dmu, dlv, None


class KlRowsFn(Function):
    """ops.py:161-163 -> [B]."""

    @staticmethod
    def forward(ctx, logvar, mu):
        logvar, mu = _f32c(logvar), _f32c(mu)
        B, D = logvar.shape
        kl = torch.empty((B,), dtype=F32, device=mu.device)
        call("itcv_kl_rows_fwd", ptr(logvar), ptr(mu), ptr(kl), B, D, stream())
        ctx.save_for_backward(logvar, mu)
        return kl

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logvar, mu = ctx.saved_tensors
        B, D = logvar.shape
        g = _f32c(g)
        dlv, dmu = torch.empty_like(logvar), torch.empty_like(mu)
        call("itcv_kl_rows_bwd", ptr(g), ptr(logvar), ptr(mu), ptr(dlv), ptr(dmu), B, D, stream())
        return dlv, dmu


_REDUCTION = {"none": 0, "sum": 1, "mean": 2}


class KlLossFn(Function):
    """scale * ops.kl_divergence(logvar, mu, reduce) (ops.py:136-163 + the hook's beta, solvers/vae.py:63-77): one launch."""

    @staticmethod
    def forward(ctx, logvar, mu, reduction, scale):
        logvar, mu = _f32c(logvar), _f32c(mu)
        B, D = logvar.shape
        out = torch.empty((B,) if reduction == 0 else (), dtype=F32, device=mu.device)
        call("itcv_kl_loss_fwd", ptr(logvar), ptr(mu), ptr(out), B, D, reduction, float(scale), stream())
        ctx.save_for_backward(logvar, mu)
        ctx.cfg = (B, D, reduction, float(scale))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logvar, mu = ctx.saved_tensors
        B, D, reduction, scale = ctx.cfg
        dlv, dmu = torch.empty_like(logvar), torch.empty_like(mu)
        call("itcv_kl_loss_bwd", ptr(_f32c(g)), ptr(logvar), ptr(mu), ptr(dlv), ptr(dmu), B, D, reduction, scale, stream())
        return dlv, dmu, None, None


class TcKlFn(Function):
    """coef_tc * total_correlation + coef_kl * kl_divergence with the hook's reduction (solvers/tc.py:69-89), fused into
    the estimator's launches (forward: partials, finish [, reduce]; backward: rows, columns)."""

    @staticmethod
    def forward(ctx, z, mu_all, logvar, dataset_size, row_offset, coef_tc, coef_kl, reduction):
        z, mu_all, logvar = _f32c(z), _f32c(mu_all), _f32c(logvar)
        Bl, D = z.shape
        Bt = mu_all.shape[0]
        dev = z.device
        out = torch.empty((Bl,) if reduction == 0 else (), dtype=F32, device=dev)
        rows = torch.empty((Bl,), dtype=F32, device=dev) if reduction else None
        prodm = torch.empty((Bl,), dtype=F32, device=dev)
        logqz = torch.empty((Bl,), dtype=F32, device=dev)
        lse = torch.empty((Bl, D), dtype=F32, device=dev)
        sjoint = torch.empty((Bl, Bt), dtype=F32, device=dev)
        nws = lib.itcv_tc_fwd_workspace(Bl, Bt, D)
        ws = _ws(nws, dev)
        call("itcv_tc_kl_fwd", ptr(z), ptr(mu_all), ptr(logvar), ptr(out), ptr(rows), ptr(prodm), ptr(logqz), ptr(lse),
             ptr(sjoint), Bl, Bt, int(row_offset), D, int(dataset_size), float(coef_tc), float(coef_kl), reduction, ptr(ws),
             nws, stream())
        ctx.save_for_backward(z, mu_all, logvar, logqz, lse, sjoint)
        ctx.cfg = (int(dataset_size), int(row_offset), float(coef_tc), float(coef_kl), reduction)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, mu_all, logvar, logqz, lse, sjoint = ctx.saved_tensors
        n, off, ctc, ckl, reduction = ctx.cfg
        Bl, D = z.shape
        Bt = mu_all.shape[0]
        dz, dlv, dmu = torch.empty_like(z), torch.empty_like(logvar), torch.empty_like(mu_all)
        nws = lib.itcv_tc_bwd_workspace(Bl, Bt)
        ws = _ws(nws, z.device)
        call("itcv_tc_kl_bwd", ptr(_f32c(g)), ptr(z), ptr(mu_all), ptr(logvar), ptr(logqz), ptr(lse), ptr(sjoint), ptr(dz),
             ptr(dmu), ptr(dlv), Bl, Bt, off, D, n, ctc, ckl, reduction, ptr(ws), nws, stream())
        return dz, dmu, dlv, None, None, None, None, None


def _packed_pair(a, b):
    """Row stride shared by two [Bt, D] column operands: D for two dense tensors, 2D for the two halves of one dense
    [Bt, 2D] tensor (a packed all-gather, read in place); None for any other layout."""
    Bt, D = a.shape
    if a.is_contiguous() and b.is_contiguous():
        return D
    if (a.stride() == b.stride() == (2 * D, 1) and b.data_ptr() == a.data_ptr() + D * a.element_size()
            and a.dtype == b.dtype == F32):
        return 2 * D
    return None


def _pair_in(mu_all, logvar_all):
    """(mu_all, logvar_all, ld) as the kernels read a [Bt, D] pair: the halves of one packed [Bt, 2D] tensor in place at
    ld = 2D, any other layout as two dense fp32 tensors at ld = D."""
    ld = _packed_pair(mu_all, logvar_all)
    if ld is None or ld == mu_all.shape[1]:
        mu_all, logvar_all = _f32c(mu_all), _f32c(logvar_all)
        ld = mu_all.shape[1]
    return mu_all, logvar_all, ld


def _pair_grads(Bt, D, ld, device):
    """(dmu, dlv) [Bt, D] in the layout ``_pair_in`` read the pair in."""
    if ld == D:
        return torch.empty((Bt, D), dtype=F32, device=device), torch.empty((Bt, D), dtype=F32, device=device)
    # one packed [Bt, 2D] gradient: the gather's adjoint reduce-scatters it in place
    dpk = torch.empty((Bt, 2 * D), dtype=F32, device=device)
    return dpk[:, :D], dpk[:, D:]


class TcFullFn(Function):
    """Per sample alpha*(logqcx - logqz) + beta*(logqz - prodm) + gamma*(prodm - logpz): the full decomposition loss of
    solvers/tc.py:91-144 (ops.py:24-29 density, variance of component i, stratified sampler) with the reduction,
    fused into the estimator's launches (forward: partials, finish [, reduce]; backward: rows, columns).  ``mu_all`` /
    ``logvar_all``: [Bt, D] column operands, two dense tensors or the halves of one packed [Bt, 2D] tensor (their
    gradients then come back as the halves of one packed tensor too).  Second output: the per-sample (mi, tc, dwkl)
    [3, Bl], no gradient."""

    @staticmethod
    def forward(ctx, z, mu_all, logvar_all, dataset_size, row_offset, alpha, beta, gamma, reduction):
        z = _f32c(z)
        abi.need_device(mu_all, logvar_all)
        mu_all, logvar_all, ld = _pair_in(mu_all, logvar_all)
        Bl, D = z.shape
        Bt = mu_all.shape[0]
        if tuple(mu_all.shape) != (Bt, D) or tuple(logvar_all.shape) != (Bt, D):
            raise ValueError(f"mu_all / logvar_all must be [Bt, {D}] (got {tuple(mu_all.shape)}, {tuple(logvar_all.shape)})")
        dev = z.device
        out = torch.empty((Bl,) if reduction == 0 else (), dtype=F32, device=dev)
        rows = torch.empty((Bl,), dtype=F32, device=dev) if reduction else None
        comps = torch.empty((3, Bl), dtype=F32, device=dev)
        prodm = torch.empty((Bl,), dtype=F32, device=dev)
        logqz = torch.empty((Bl,), dtype=F32, device=dev)
        lse = torch.empty((Bl, D), dtype=F32, device=dev)
        sjoint = torch.empty((Bl, Bt), dtype=F32, device=dev)
        ivar = torch.empty((Bt, D), dtype=F32, device=dev)
        nws = lib.itcv_tc_full_fwd_workspace(Bl, Bt, D)
        ws = _ws(nws, dev)
        call("itcv_tc_full_fwd", ptr(z), mu_all.data_ptr(), logvar_all.data_ptr(), ld, ptr(out), ptr(rows), ptr(comps),
             ptr(prodm), ptr(logqz), ptr(lse), ptr(sjoint), ptr(ivar), Bl, Bt, int(row_offset), D, int(dataset_size),
             float(alpha), float(beta), float(gamma), reduction, ptr(ws), nws, stream())
        ctx.save_for_backward(z, mu_all, logvar_all, logqz, lse, sjoint, ivar)
        ctx.cfg = (int(dataset_size), int(row_offset), float(alpha), float(beta), float(gamma), reduction, ld)
        ctx.mark_non_differentiable(comps)
        return out, comps

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_comps):
        z, mu_all, logvar_all, logqz, lse, sjoint, ivar = ctx.saved_tensors
        n, off, a, b, c, reduction, ld = ctx.cfg
        Bl, D = z.shape
        Bt = mu_all.shape[0]
        dz = torch.empty_like(z)
        dmu, dlv = _pair_grads(Bt, D, ld, z.device)
        nws = lib.itcv_tc_full_bwd_workspace(Bl, Bt)
        ws = _ws(nws, z.device)
        call("itcv_tc_full_bwd", ptr(_f32c(g)), ptr(z), mu_all.data_ptr(), logvar_all.data_ptr(), ld, ptr(logqz), ptr(lse),
             ptr(sjoint), ptr(ivar), ptr(dz), dmu.data_ptr(), dlv.data_ptr(), Bl, Bt, off, D, n, a, b, c, reduction,
             ptr(ws), nws, stream())
        return dz, dmu, dlv, None, None, None, None, None, None


def _loss_terms(n, device):
    """(out, terms): the fp32 scalar that an objective's finish kernel writes and its ``n`` logged terms."""
    return torch.empty((), dtype=F32, device=device), torch.empty((n,), dtype=F32, device=device)


def dip_kl_forward(mu_all, logvar_all, Bl, row_offset, kind, lambda_od, lambda_d, coef_kl):
    """itcv_dip_kl_fwd on a [Bt, D] pair in either layout (two dense tensors, or the halves of one packed [Bt, 2D] tensor,
    read in place; anything else is copied dense).  Returns (mu_all, logvar_all, ld) as read and (out, terms [3], W [D, D],
    mean [D] fp64).  No gradient: ``DipKlFn`` is the differentiable form."""
    abi.need_device(mu_all, logvar_all)
    if mu_all.dim() != 2 or mu_all.shape != logvar_all.shape:
        raise ValueError(f"mu_all / logvar_all must share one [Bt, D] shape (got {tuple(mu_all.shape)}, "
                         f"{tuple(logvar_all.shape)})")
    mu_all, logvar_all, ld = _pair_in(mu_all, logvar_all)
    Bt, D = mu_all.shape
    dev = mu_all.device
    out, terms = _loss_terms(3, dev)
    W = torch.empty((D, D), dtype=F32, device=dev)
    mean = torch.empty((D,), dtype=torch.float64, device=dev)
    nws = lib.itcv_dip_kl_workspace(Bt, D)
    ws = _ws(nws, dev)
    call("itcv_dip_kl_fwd", mu_all.data_ptr(), logvar_all.data_ptr(), ld, ptr(out), ptr(terms), ptr(W), ptr(mean),
         int(Bl), Bt, int(row_offset), D, int(kind), float(lambda_od), float(lambda_d), float(coef_kl), ptr(ws), nws,
         stream())
    return mu_all, logvar_all, ld, out, terms, W, mean


class DipKlFn(Function):
    """coef_kl * mean KL of this rank's rows + the DIP-VAE covariance regulariser of the whole global batch
    (include/itcv_hip.h: itcv_dip_kl_fwd; ``kind`` 1 = DIP-VAE-I, 2 = DIP-VAE-II): two launches forward, one backward.
    ``mu_all`` / ``logvar_all``: [Bt, D], two dense tensors or the halves of one packed [Bt, 2D] tensor (their gradients
    then come back as the halves of one packed tensor too); this rank's rows are ``row_offset .. row_offset + Bl - 1``.
    Second output: (mean KL, off-diagonal term, diagonal term) [3], no gradient.  Kept for the backward: the two inputs,
    W [D, D] and the fp64 column means the forward centred with."""

    @staticmethod
    def forward(ctx, mu_all, logvar_all, Bl, row_offset, kind, lambda_od, lambda_d, coef_kl):
        mu_all, logvar_all, ld, out, terms, W, mean = dip_kl_forward(mu_all, logvar_all, Bl, row_offset, kind, lambda_od,
                                                                     lambda_d, coef_kl)
        ctx.save_for_backward(mu_all, logvar_all, W, mean)
        ctx.cfg = (int(Bl), int(row_offset), int(kind), float(coef_kl), ld)
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms):
        mu_all, logvar_all, W, mean = ctx.saved_tensors
        Bl, off, kind, coef_kl, ld = ctx.cfg
        Bt, D = mu_all.shape
        dmu, dlv = _pair_grads(Bt, D, ld, W.device)
        call("itcv_dip_kl_bwd", ptr(_f32c(g)), mu_all.data_ptr(), logvar_all.data_ptr(), ld, ptr(W), ptr(mean),
             dmu.data_ptr(), dlv.data_ptr(), Bl, Bt, off, D, kind, coef_kl, stream())
        return dmu, dlv, None, None, None, None, None, None


MMD_KERNELS = {"rbf": 1, "imq": 2}


def mmd_kl_forward(z_all, prior, mu, logvar, kernel, h, lambda_mmd, coef_kl):
    """itcv_mmd_kl_fwd on z_all [Bt, D], prior [P, D] and this rank's mu / logvar [Bl, D] (made fp32-contiguous: a strided
    view is copied dense).  Returns (out, terms [5], Wt [Bt, Bt + P], rs [Bt] fp64).  No gradient: ``MmdKlFn`` is the
    differentiable form."""
    return _mmd_kl_forward(z_all, prior, mu, logvar, kernel, h, lambda_mmd, coef_kl)[4:]


def _mmd_kl_forward(z_all, prior, mu, logvar, kernel, h, lambda_mmd, coef_kl):
    abi.need_device(z_all, prior, mu, logvar)
    if z_all.dim() != 2 or prior.dim() != 2 or z_all.shape[1] != prior.shape[1]:
        raise ValueError(f"z_all [Bt, D] and prior [P, D] must share D (got {tuple(z_all.shape)}, {tuple(prior.shape)})")
    if mu.dim() != 2 or mu.shape != logvar.shape or mu.shape[1] != z_all.shape[1]:
        raise ValueError(f"mu / logvar must share one [Bl, D] shape with the D of z_all (got {tuple(mu.shape)}, "
                         f"{tuple(logvar.shape)}, D = {z_all.shape[1]})")
    z_all, prior, mu, logvar = _f32c(z_all), _f32c(prior), _f32c(mu), _f32c(logvar)
    (Bt, D), P, Bl = z_all.shape, prior.shape[0], mu.shape[0]
    dev = z_all.device
    out, terms = _loss_terms(5, dev)
    Wt = torch.empty((Bt, Bt + P), dtype=F32, device=dev)
    rs = torch.empty((Bt,), dtype=torch.float64, device=dev)
    nws = lib.itcv_mmd_kl_workspace(Bt, P)
    ws = _ws(nws, dev)
    call("itcv_mmd_kl_fwd", ptr(z_all), ptr(prior), ptr(mu), ptr(logvar), ptr(out), ptr(terms), ptr(Wt), ptr(rs), Bl, Bt, P,
         D, int(kernel), float(h), float(lambda_mmd), float(coef_kl), ptr(ws), nws, stream())
    return z_all, prior, mu, logvar, out, terms, Wt, rs


class MmdKlFn(Function):
    """coef_kl * mean KL of this rank's rows + lambda_mmd * the unbiased MMD^2 between the sampled latents of the whole
    global batch and draws from the prior (include/itcv_hip.h: itcv_mmd_kl_fwd; ``kernel`` 1 = rbf, 2 = imq with
    bandwidth ``h``): two launches forward, one backward.  Second output: (mean KL, MMD^2, S_zz, S_pp, S_zp) [5], no
    gradient.  ``prior`` is a constant.  Kept for the backward: the four inputs, Wt [Bt, Bt + P] and its fp64 row sums."""

    @staticmethod
    def forward(ctx, z_all, prior, mu, logvar, kernel, h, lambda_mmd, coef_kl):
        z_all, prior, mu, logvar, out, terms, Wt, rs = _mmd_kl_forward(z_all, prior, mu, logvar, kernel, h, lambda_mmd,
                                                                       coef_kl)
        ctx.save_for_backward(z_all, prior, mu, logvar, Wt, rs)
        ctx.cfg = (float(lambda_mmd), float(coef_kl))
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms):
        z_all, prior, mu, logvar, Wt, rs = ctx.saved_tensors
        lambda_mmd, coef_kl = ctx.cfg
        (Bt, D), P, Bl = z_all.shape, prior.shape[0], mu.shape[0]
        dz, dmu, dlv = torch.empty_like(z_all), torch.empty_like(mu), torch.empty_like(logvar)
        call("itcv_mmd_kl_bwd", ptr(_f32c(g)), ptr(z_all), ptr(prior), ptr(mu), ptr(logvar), ptr(Wt), ptr(rs), ptr(dz),
             ptr(dmu), ptr(dlv), Bl, Bt, P, D, lambda_mmd, coef_kl, stream())
        return dz, None, dmu, dlv, None, None, None, None


def _sw_forward(z_all, prior, t, mu, logvar, lambda_sw, coef_kl, keep):
    """itcv_sw_kl_fwd.  z_all / prior [Bt, D] are read in place when their columns have unit stride (the row stride goes to
    the kernel); t [L, D], mu / logvar [Bl, D] (None, None: no KL, ``coef_kl`` 0) are made dense.  ``keep``: also G
    [L, Bt].  Returns (mu, logvar, out, terms [3], per [L] fp64, Theta [L, D] fp64, G or None)."""
    abi.need_device(z_all, prior, t, mu, logvar)
    z_all, ldz = _rows_f32(z_all, "z_all")
    prior, ldp = _rows_f32(prior, "prior")
    if prior.shape != z_all.shape:
        raise ValueError(f"z_all and prior must share one [Bt, D] shape: the sliced distance pairs sorted samples of equal "
                         f"counts (got {tuple(z_all.shape)}, {tuple(prior.shape)})")
    Bt, D = z_all.shape
    if t.dim() != 2 or t.shape[1] != D:
        raise ValueError(f"the directions t must be [L, D] with the D of z_all (got {tuple(t.shape)}, D = {D})")
    t, L, Bl = _f32c(t), t.shape[0], 1
    if mu is not None:
        if mu.dim() != 2 or mu.shape != logvar.shape or mu.shape[1] != D:
            raise ValueError(f"mu / logvar must share one [Bl, D] shape with the D of z_all (got {tuple(mu.shape)}, "
                             f"{tuple(logvar.shape)}, D = {D})")
        mu, logvar, Bl = _f32c(mu), _f32c(logvar), mu.shape[0]
    dev = z_all.device
    out, terms = _loss_terms(3, dev)
    per = torch.empty((L,), dtype=torch.float64, device=dev)
    Theta = torch.empty((L, D), dtype=torch.float64, device=dev)
    G = torch.empty((L, Bt), dtype=torch.float64, device=dev) if keep else None
    nws = lib.itcv_sw_workspace(Bt, L, D)
    ws = _ws(nws, dev)
    call("itcv_sw_kl_fwd", z_all.data_ptr(), ldz, prior.data_ptr(), ldp, ptr(t), ptr(mu), ptr(logvar), ptr(out), ptr(terms),
         ptr(per), ptr(Theta), ptr(G), Bl, Bt, L, D, float(lambda_sw), float(coef_kl), ptr(ws), nws, stream())
    return mu, logvar, out, terms, per, Theta, G


def sw_kl_forward(z_all, prior, t, mu, logvar, lambda_sw, coef_kl):
    """itcv_sw_kl_fwd on z_all / prior [Bt, D], the directions t [L, D] and this rank's mu / logvar [Bl, D].  Returns (out,
    terms [3], per [L] fp64, Theta [L, D] fp64, G [L, Bt] fp64).  No gradient: ``SwKlFn`` is the differentiable form."""
    return _sw_forward(z_all, prior, t, mu, logvar, lambda_sw, coef_kl, True)[2:]


def sw_distance(a, b, t):
    """(SW^2 as an fp32 device scalar, per [L] fp64) of the sliced-Wasserstein distance between the rows of a and b [N, D]
    over the directions t [L, D]: the forward-only form of itcv_sw_kl_fwd (no KL, no G; nothing of size L x N is
    written).  No gradient."""
    with torch.no_grad():
        _, _, out, _, per, _, _ = _sw_forward(a, b, t, None, None, 1.0, 0.0, False)
    return out, per


class SwKlFn(Function):
    """coef_kl * mean KL of this rank's rows + lambda_sw * the sliced-Wasserstein distance SW^2 between the sampled latents
    of the whole global batch and as many draws from the prior over the directions ``t`` (include/itcv_hip.h:
    itcv_sw_kl_fwd): two launches forward, one backward.  Second output: (mean KL, SW^2, max_l SW_l^2) [3], no gradient.
    ``prior`` and ``t`` are constants.  Kept for the backward: mu, logvar, Theta [L, D] and the scattered differences G
    [L, Bt], both fp64."""

    @staticmethod
    def forward(ctx, z_all, prior, t, mu, logvar, lambda_sw, coef_kl):
        mu, logvar, out, terms, _, Theta, G = _sw_forward(z_all, prior, t, mu, logvar, lambda_sw, coef_kl, True)
        ctx.save_for_backward(mu, logvar, Theta, G)
        ctx.cfg = (float(lambda_sw), float(coef_kl))
        ctx.mark_non_differentiable(terms)
        return out, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms):
        mu, logvar, Theta, G = ctx.saved_tensors
        lambda_sw, coef_kl = ctx.cfg
        (L, Bt), D, Bl = G.shape, Theta.shape[1], mu.shape[0]
        dz = torch.empty((Bt, D), dtype=F32, device=G.device)
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        call("itcv_sw_kl_bwd", ptr(_f32c(g)), ptr(mu), ptr(logvar), ptr(G), ptr(Theta), ptr(dz), ptr(dmu), ptr(dlv), Bl, Bt, L,
             D, lambda_sw, coef_kl, stream())
        return dz, None, None, dmu, dlv, None, None


# ------------------------------------------------------------------ FactorVAE: permutation + discriminator
# None of this reads or claims _SHARED_PASS: the discriminator is no part of a recorded network pass, and the Soft-Intro
# bookkeeping (param_grads / input_grad / live) must not steer its two walks.  That is why LinearFn is not reused.
PERMUTE_MAX_B, PERMUTE_MAX_D = 4096, 512


def _unit_cols(t):
    """A 2-D tensor as the kernels take rows: a view with unit column stride and a row stride >= D as it is (its row
    stride goes to the kernel), anything else copied dense."""
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def _rows_f32(t, what):
    """A 2-D fp32 device tensor as (tensor, row stride in elements): a view with unit column stride is passed as it is."""
    abi.need_device(t)
    if t.dtype != F32:
        raise abi.HipExtensionError(f"HIP path is fp32 only (got {t.dtype})")
    if t.dim() != 2:
        raise ValueError(f"{what} must be a matrix (got {tuple(t.shape)})")
    B, D = t.shape
    if B == 1 and t.stride(1) == 1:
        return t, D
    t = _unit_cols(t)
    return t, t.stride(0)


def permute_dims(z, keys, out=None, zcopy=None):
    """FactorVAE's per-dimension batch permutation in one launch (include/itcv_hip.h: itcv_permute_dims):
    ``out[r, d] = z[i, d]`` with r the rank of ``keys[i, d]`` in column d (ties by row index), i.e.
    ``z[argsort(keys[:, d], stable), d]``.  z, keys [B, D] fp32 (row-strided views are read in place), B <= 4096,
    D <= 512.  ``out`` / ``zcopy``: dense [B, D] tensors to write the result / a copy of z into.  No gradient."""
    z, keys = z.detach(), keys.detach()
    if z.dim() != 2 or z.shape != keys.shape:
        raise ValueError(f"z and keys must share one [B, D] shape (got {tuple(z.shape)}, {tuple(keys.shape)})")
    (z, ldz), (keys, ldk) = _rows_f32(z, "z"), _rows_f32(keys, "keys")
    B, D = z.shape
    if not (1 <= B <= PERMUTE_MAX_B and 1 <= D <= PERMUTE_MAX_D):
        raise ValueError(f"permute_dims takes 1 <= B <= {PERMUTE_MAX_B} and 1 <= D <= {PERMUTE_MAX_D} (got {B}, {D})")
    if out is None:
        out = torch.empty((B, D), dtype=F32, device=z.device)
    for t in (out, zcopy):
        if t is not None and (tuple(t.shape) != (B, D) or t.dtype != F32 or t.device != z.device):
            raise ValueError("out / zcopy must be fp32 [B, D] tensors on z's device")
    call("itcv_permute_dims", z.data_ptr(), ldz, keys.data_ptr(), ldk, ptr(out), ptr(zcopy), B, D, stream())
    return out


# ------------------------------------------------------------------ Ada-GVAE / Ada-ML-VAE: the pair op
ADA_AVERAGINGS = {"gvae": 1, "mlvae": 2}
ADA_MAX_D = 512


class AdaGroupFn(Function):
    """The latent op of Ada-GVAE / Ada-ML-VAE on 2B stacked rows, rows b and B + b a pair (include/itcv_hip.h:
    itcv_ada_group_fwd; ``averaging`` 1 = gvae, 2 = mlvae): two launches forward, one backward.  ``mu`` / ``logvar`` /
    ``eps`` [2B, D]: fp32 views with unit column stride are read in place (the halves of one packed [2B, 2D] tensor too).
    ``own_in``: None (the adaptive threshold) or a [B, D] mask (non-zero: the dimension keeps its own posterior).  Outputs:
    z [2B, D] and the scalar beta * mean KL, both differentiable in ``mu`` and ``logvar``; the mask as used [B, D] uint8
    and (mean KL, mean shared dimensions per pair) [2], no gradient.  The mask is a constant of the backward pass.
    The arguments are those ``ops.ada_group`` has validated (shapes, the even row count, the range of D, the mask's shape):
    nothing of that is checked again here, only the layout is handled and the mask normalised."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, own_in, averaging, beta):
        (R, D), dev = mu.shape, mu.device
        B = R // 2
        (mu, ldm), (logvar, ldl), (eps, lde) = _rows_f32(mu, "mu"), _rows_f32(logvar, "logvar"), _rows_f32(eps, "eps")
        if own_in is not None:
            abi.need_device(own_in)
            own_in = (own_in != 0).to(torch.uint8).contiguous()
        z = torch.empty((R, D), dtype=F32, device=dev)
        own = torch.empty((B, D), dtype=torch.uint8, device=dev)
        part = torch.empty((3 * B,), dtype=torch.float64, device=dev)
        out, terms = _loss_terms(2, dev)
        call("itcv_ada_group_fwd", mu.data_ptr(), ldm, logvar.data_ptr(), ldl, eps.data_ptr(), lde, ptr(own_in), ptr(z),
             ptr(own), ptr(part), ptr(out), ptr(terms), B, D, int(averaging), float(beta), stream())
        ctx.save_for_backward(mu, logvar, eps, own)
        ctx.cfg = (int(averaging), float(beta), ldm, ldl, lde)
        ctx.mark_non_differentiable(own, terms)
        return z, out, own, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, g, _g_own, _g_terms):
        mu, logvar, eps, own = ctx.saved_tensors
        averaging, beta, ldm, ldl, lde = ctx.cfg
        R, D = mu.shape
        dz, ldz = _rows_f32(dz, "dz")
        dmu, dlv = torch.empty((R, D), dtype=F32, device=mu.device), torch.empty((R, D), dtype=F32, device=mu.device)
        call("itcv_ada_group_bwd", dz.data_ptr(), ldz, ptr(_f32c(g)), mu.data_ptr(), ldm, logvar.data_ptr(), ldl,
             eps.data_ptr(), lde, ptr(own), ptr(dmu), ptr(dlv), R // 2, D, averaging, beta, stream())
        return dmu, dlv, None, None, None, None


# ------------------------------------------------------------------ VampPrior: the mixture-prior KL op
VAMP_MAX_B, VAMP_MAX_K, VAMP_MAX_D, VAMP_MAX_PAIRS = 4096, 4096, 512, 1 << 22
VAMP_REDUCES = {"none": 0, "mean": 1, "sum": 2}


def vamp_check_shapes(B, K, D, what="vamp_latent"):
    """ValueError unless (B, K, D) is inside the limits of csrc/vamp.hip; host arithmetic only."""
    if not (1 <= B <= VAMP_MAX_B and 1 <= K <= VAMP_MAX_K):
        raise ValueError(f"{what} takes 1 <= B <= {VAMP_MAX_B} rows and 1 <= K <= {VAMP_MAX_K} components "
                         f"(got B = {B}, K = {K})")
    if not 1 <= D <= VAMP_MAX_D:
        raise ValueError(f"{what} takes 1 <= D <= {VAMP_MAX_D} (got {D})")
    if B * K > VAMP_MAX_PAIRS:
        raise ValueError(f"{what} takes B K <= 2^22 pairs (got B = {B}, K = {K})")


def vamp_latent_forward(mu, logvar, eps, p_mu, p_logvar, beta, reduce):
    """itcv_vamp_fwd on the posterior ``mu`` / ``logvar`` / ``eps`` [B, D] and the components ``p_mu`` / ``p_logvar``
    [K, D] (fp32 views with unit column stride are read in place).  Returns the five inputs as read with their row strides,
    then (z [B, D], out, rows [B], terms [3], logq [B] fp64, logp [B] fp64, r [B, K] fp64).  No gradient:
    ``VampLatentFn`` is the differentiable form."""
    (B, D), K, dev = mu.shape, p_mu.shape[0], mu.device
    ins = [_rows_f32(t, n) for t, n in ((mu, "mu"), (logvar, "logvar"), (eps, "eps"), (p_mu, "p_mu"),
                                        (p_logvar, "p_logvar"))]
    z = torch.empty((B, D), dtype=F32, device=dev)
    r = torch.empty((B, K), dtype=torch.float64, device=dev)
    logq, logp = torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.float64, device=dev)
    rows = torch.empty((B,), dtype=F32, device=dev)
    out, terms = _loss_terms(3, dev)
    nws = lib.itcv_vamp_workspace(B, K, D)
    ws = _ws(nws, dev)
    flat = [a for t, ld in ins for a in (t.data_ptr(), ld)]
    call("itcv_vamp_fwd", *flat, ptr(z), ptr(r), ptr(logq), ptr(logp), ptr(rows), ptr(out), ptr(terms), B, K, D,
         float(beta), int(reduce), ptr(ws), nws, stream())
    return ins, (z, out, rows, terms, logq, logp, r)


class VampLatentFn(Function):
    """The latent op of a VAE with a VampPrior (include/itcv_hip.h: itcv_vamp_fwd; ``reduce`` 0 = none, 1 = mean,
    2 = sum): two launches forward, one backward.  Outputs: z [B, D] and the loss (a scalar, or rows [B] under "none"),
    both differentiable in ``mu``, ``logvar``, ``p_mu`` and ``p_logvar``; (mean KL, mean logq, mean logp) [3], logq [B],
    logp [B] and r [B, K] (fp64), no gradient.  Kept for the backward: logvar, eps, the components, z and r.  The arguments
    are those ``ops.vamp_latent`` has validated (shapes and limits): only the layout is handled here."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, p_mu, p_logvar, beta, reduce):
        ins, (z, out, rows, terms, logq, logp, r) = vamp_latent_forward(mu, logvar, eps, p_mu, p_logvar, beta, reduce)
        (_, _), (lv, ldl), (ep, lde), (pm, ldpm), (pl, ldpl) = ins
        ctx.save_for_backward(lv, ep, pm, pl, z, r)
        ctx.cfg = (float(beta), int(reduce), ldl, lde, ldpm, ldpl)
        ctx.mark_non_differentiable(terms, logq, logp, r)
        return z, (rows if reduce == 0 else out), terms, logq, logp, r

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, g, *_unused):
        lv, ep, pm, pl, z, r = ctx.saved_tensors
        beta, reduce, ldl, lde, ldpm, ldpl = ctx.cfg
        (B, D), K, dev = z.shape, pm.shape[0], z.device
        gz, ldgz = _rows_f32(gz, "gz")
        dmu, dlv = torch.empty((B, D), dtype=F32, device=dev), torch.empty((B, D), dtype=F32, device=dev)
        dpm, dpl = torch.empty((K, D), dtype=F32, device=dev), torch.empty((K, D), dtype=F32, device=dev)
        call("itcv_vamp_bwd", gz.data_ptr(), ldgz, ptr(_f32c(g)), int(reduce == 0), 1.0 / B if reduce == 1 else 1.0,
             lv.data_ptr(), ldl, ep.data_ptr(), lde, ptr(z), pm.data_ptr(), ldpm, pl.data_ptr(), ldpl, ptr(r), ptr(dmu),
             ptr(dlv), ptr(dpm), ptr(dpl), B, K, D, beta, stream())
        return dmu, dlv, None, dpm, dpl, None, None


def vamp_log_prob(x, p_mu, p_logvar):
    """itcv_vamp_logprob: fp64 [N] log (1 / K) sum_k N(x_n; p_mu_k, diag exp(p_logvar_k)) of the fp32 rows ``x`` [N, D]
    (row-strided views are read in place).  Shapes and limits are the caller's (``ops.vamp_log_prob``).  No gradient."""
    (x, ldx), (pm, ldpm), (pl, ldpl) = _rows_f32(x, "x"), _rows_f32(p_mu, "p_mu"), _rows_f32(p_logvar, "p_logvar")
    (N, D), K = x.shape, pm.shape[0]
    logp = torch.empty((N,), dtype=torch.float64, device=x.device)
    nws = lib.itcv_vamp_workspace(N, K, D)
    ws = _ws(nws, x.device)
    call("itcv_vamp_logprob", x.data_ptr(), ldx, pm.data_ptr(), ldpm, pl.data_ptr(), ldpl, ptr(logp), N, K, D, ptr(ws),
         nws, stream())
    return logp


# ------------------------------------------------------------------ JointVAE / AnnealedVAE: the capacity-controlled latent op
JOINT_MAX_D = 512


def _row_ptr(t):
    """Device pointer of what ``_rows_f32`` returned (a row-strided view is passed as it is), or NULL for None."""
    return None if t is None else t.data_ptr()


class JointLatentFn(Function):
    """The latent op of JointVAE / AnnealedVAE (include/itcv_hip.h: itcv_joint_latent_fwd): two launches forward, one
    backward.  ``mu`` / ``logvar`` [B, n_cont + n_disc]: fp32 views with unit column stride are read in place (the halves of
    one packed [B, 2D] tensor too); ``eps`` [B, n_cont] and ``u`` [B, n_disc] (None where the block is empty); ``seg``
    [n_disc, 2] int32: the group of every discrete column; ``capacity`` [2] fp64 on the device, read when the kernel runs.
    Outputs: z [B, D] and the scalar beta (gamma_cont |KL_z - C_z| + gamma_disc |KL_c - C_c|), both differentiable in
    ``mu`` and ``logvar``, and (KL_z, KL_c, C_z, C_c) [4], no gradient.  The signs of the two differences are kept for the
    backward pass, so it does not read ``capacity`` again.  The arguments are those ``ops.joint_latent`` has validated
    (shapes, the latent spec against D, the device ``capacity``) with the table of ``ops.joint_segments``: nothing of that is
    checked again here, only the layout is handled."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, u, seg, capacity, n_cont, n_disc, tau, gamma_cont, gamma_disc, beta):
        B, D = mu.shape
        (mu, ldm), (logvar, ldl) = _rows_f32(mu, "mu"), _rows_f32(logvar, "logvar")
        (eps, lde) = _rows_f32(eps, "eps") if n_cont else (None, 0)
        (u, ldu) = _rows_f32(u, "u") if n_disc else (None, 0)
        seg = seg.contiguous() if n_disc else None
        dev = mu.device
        z = torch.empty((B, D), dtype=F32, device=dev)
        part = torch.empty((2 * B,), dtype=torch.float64, device=dev)
        sgn = torch.empty((2,), dtype=F32, device=dev)
        out, terms = _loss_terms(4, dev)
        call("itcv_joint_latent_fwd", mu.data_ptr(), ldm, logvar.data_ptr(), ldl, _row_ptr(eps), lde, _row_ptr(u), ldu,
             ptr(seg), ptr(capacity.contiguous()), ptr(z), ptr(part), ptr(out), ptr(sgn), ptr(terms), B, int(n_cont),
             int(n_disc), 0, float(tau), float(gamma_cont), float(gamma_disc), float(beta), stream())
        ctx.save_for_backward(mu, logvar, eps, u, seg, sgn)
        ctx.cfg = (int(n_cont), int(n_disc), float(tau), float(gamma_cont), float(gamma_disc), float(beta), ldm, ldl, lde,
                   ldu)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)         # no zero tensor is filled for ``terms`` (or an unused z / loss) per backward
        return z, out, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, g, _g_terms):
        mu, logvar, eps, u, seg, sgn = ctx.saved_tensors
        n_cont, n_disc, tau, gamma_cont, gamma_disc, beta, ldm, ldl, lde, ldu = ctx.cfg
        B, D = mu.shape
        if dz is None:                           # z unused: the loss alone is differentiated
            dz = torch.zeros((B, D), dtype=F32, device=mu.device)
        if g is None:
            g = torch.zeros((), dtype=F32, device=mu.device)
        dz, ldz = _rows_f32(dz, "dz")
        dmu, dlv = torch.empty((B, D), dtype=F32, device=mu.device), torch.empty((B, D), dtype=F32, device=mu.device)
        call("itcv_joint_latent_bwd", dz.data_ptr(), ldz, ptr(_f32c(g)), ptr(sgn), mu.data_ptr(), ldm, logvar.data_ptr(),
             ldl, _row_ptr(eps), lde, _row_ptr(u), ldu, ptr(seg), ptr(dmu), ptr(dlv), B, n_cont, n_disc, tau, gamma_cont,
             gamma_disc, beta, stream())
        return (dmu, dlv) + (None,) * 10


def joint_latent_hard(mu, seg, n_cont, n_disc):
    """The deterministic code of ``JointLatentFn``'s model, one launch, no gradient: the continuous columns of ``mu`` bit
    for bit, and per group the one-hot of the first maximum of the fp32 logits.  ``mu``, the spec and ``seg`` are those
    ``ops.joint_latent`` has validated; nothing of that is checked again here."""
    B, D = mu.shape
    mu, ldm = _rows_f32(mu.detach(), "mu")
    z = torch.empty((B, D), dtype=F32, device=mu.device)
    call("itcv_joint_latent_fwd", mu.data_ptr(), ldm, None, 0, None, 0, None, 0, ptr(seg.contiguous() if n_disc else None),
         None, ptr(z), None, None, None, None, B, int(n_cont), int(n_disc), 1, 1.0, 0.0, 0.0, 0.0, stream())
    return z


# ------------------------------------------------------------------ semi-supervised S2 objectives: the label regulariser
SUP_KINDS = {"xent": 1, "l2": 2, "cov": 3}
SUP_MAX_D = 512
SUP_MAX_F = 64
_SUP_SIZES = {}


def sup_sizes(factor_sizes, device):
    """The device table [F] int32 of the factor sizes.  Built once per (sizes, device) and kept."""
    key = (tuple(int(k) for k in factor_sizes), torch.device(device))
    t = _SUP_SIZES.get(key)
    if t is None:
        t = _SUP_SIZES[key] = torch.tensor(key[0], dtype=torch.int32).to(device)
    return t


class SupRegFn(Function):
    """gamma * the label regulariser of the S2 objectives (include/itcv_hip.h: itcv_sup_fwd; ``kind`` 1 = xent, 2 = l2,
    3 = cov): two launches forward, one backward.  ``mu`` [B_l, D] and ``y`` [B_l, F]: fp32 views with unit column stride
    are read in place.  ``factor_sizes``: a tuple of F ints (xent) or None.  ``gamma``: a float, or a [1] float64 device
    tensor read when the kernel runs.  Outputs: the scalar, differentiable in ``mu``, and (sup, gamma) [2], no gradient.
    Kept for the backward: the two inputs, the gamma that was used and, under cov, W and the fp64 column means of y."""

    @staticmethod
    def forward(ctx, mu, y, kind, factor_sizes, gamma, scale):
        (mu, ldm), (y, ldy) = _rows_f32(mu, "mu"), _rows_f32(y, "labels")
        (B, D), F = mu.shape, y.shape[1]
        dev = mu.device
        sizes = sup_sizes(factor_sizes, dev) if factor_sizes is not None else None
        min_size = min(int(k) for k in factor_sizes) if factor_sizes is not None else 0
        on_device = isinstance(gamma, torch.Tensor)
        if on_device:
            abi.need_device(gamma)
        out, terms = _loss_terms(2, dev)
        keep = torch.empty((1 + F,), dtype=torch.float64, device=dev)
        Wt = torch.empty((F, D), dtype=torch.float64, device=dev) if kind == SUP_KINDS["cov"] else None
        nws = lib.itcv_sup_workspace(B, D, F, int(kind))
        ws = _ws(nws, dev)
        call("itcv_sup_fwd", mu.data_ptr(), ldm, y.data_ptr(), ldy, ptr(sizes), min_size, ptr(gamma) if on_device else None,
             0.0 if on_device else float(gamma), float(scale), ptr(out), ptr(terms), ptr(Wt), ptr(keep), ptr(ws), nws, B, D,
             F, int(kind), stream())
        ctx.save_for_backward(mu, y, sizes, Wt, keep)
        ctx.cfg = (int(kind), min_size, float(scale), ldm, ldy)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return out, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms):
        mu, y, sizes, Wt, keep = ctx.saved_tensors
        kind, min_size, scale, ldm, ldy = ctx.cfg
        (B, D), F = mu.shape, y.shape[1]
        if g is None:
            return (None,) * 6
        dmu = torch.empty((B, D), dtype=F32, device=mu.device)
        call("itcv_sup_bwd", ptr(_f32c(g)), mu.data_ptr(), ldm, y.data_ptr(), ldy, ptr(sizes), min_size, scale, ptr(Wt),
             ptr(keep), ptr(dmu), B, D, F, kind, stream())
        return dmu, None, None, None, None, None


# ------------------------------------------------------------------ importance-weighted bound (csrc/iwae.hip)
IWAE_ESTIMATORS = {"iwae": 0, "stl": 1, "dreg": 2}
IWAE_MAX_D = 512
IWAE_MAX_K = 1024
IWAE_MAX_ROWS = 1 << 24


class IwaeSample:
    """What ``IwaeSampleFn`` returns and ``IwaeCombineFn`` completes: ``z`` [K B, D] fp32 and ``lat`` [K B] fp64 (both
    differentiable in ``mu`` and ``logvar``), the buffer ``weights`` [K B] fp64 that the combine fills with the normalised
    importance weights, and the code of the gradient estimator that the sample's backward applies (set by the combine;
    0 = "iwae" until then).  The backward reads the two when it runs."""
    __slots__ = ("z", "lat", "weights", "estimator", "B", "K")

    def __init__(self, B, K, device):
        self.B, self.K = B, K
        self.weights = torch.empty((K * B,), dtype=torch.float64, device=device)
        self.estimator = 0
        self.z = self.lat = None


class IwaeSampleFn(Function):
    """K reparameterised samples of each of B posteriors (include/itcv_hip.h: itcv_iwae_sample_fwd): one launch forward,
    one backward.  ``mu`` / ``logvar`` [B, D]: fp32 views with unit column stride are read in place; ``eps`` [K B, D]."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, sample):
        (mu, ldm), (logvar, ldl), (eps, lde) = _rows_f32(mu, "mu"), _rows_f32(logvar, "logvar"), _rows_f32(eps, "eps")
        (B, D), K = mu.shape, sample.K
        z = torch.empty((K * B, D), dtype=F32, device=mu.device)
        lat = torch.empty((K * B,), dtype=torch.float64, device=mu.device)
        call("itcv_iwae_sample_fwd", mu.data_ptr(), ldm, logvar.data_ptr(), ldl, eps.data_ptr(), lde, ptr(z), ptr(lat), B, K,
             D, stream())
        ctx.save_for_backward(mu, logvar, eps)
        ctx.cfg = (sample, ldm, ldl, lde)
        ctx.set_materialize_grads(False)
        return z, lat

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, h):
        mu, logvar, eps = ctx.saved_tensors
        sample, ldm, ldl, lde = ctx.cfg
        (B, D), K = mu.shape, sample.K
        if dz is None and h is None:
            return None, None, None, None
        if dz is None:
            dz = torch.zeros((K * B, D), dtype=F32, device=mu.device)
        if h is None:
            h = torch.zeros((K * B,), dtype=torch.float64, device=mu.device)
        dz, ldz = _rows_f32(dz, "dz")
        dmu, dlv = torch.empty((B, D), dtype=F32, device=mu.device), torch.empty((B, D), dtype=F32, device=mu.device)
        call("itcv_iwae_sample_bwd", dz.data_ptr(), ldz, ptr(h.contiguous()), ptr(sample.weights), mu.data_ptr(), ldm,
             logvar.data_ptr(), ldl, eps.data_ptr(), lde, ptr(dmu), ptr(dlv), B, K, D, int(sample.estimator), stream())
        return dmu, dlv, None, None


class IwaeRowsFn(Function):
    """rows[k B + b] = sum_p err(recon[k B + b][p], x[b][p]) (include/itcv_hip.h: itcv_iwae_rows_fwd): the bits of
    ``ReconRowsFn`` on ``x.repeat(K, 1)`` without the K copies; x is treated as a constant."""

    @staticmethod
    def forward(ctx, x, recon, loss_type):
        x, recon = _f32c(x), _f32c(recon)
        B, R = x.shape[0], recon.shape[0]
        P = x.numel() // B
        K = R // B
        rows = torch.empty((R,), dtype=F32, device=recon.device)
        nws = lib.itcv_iwae_rows_workspace(B, K, P)
        ws = _ws(nws, recon.device)
        call("itcv_iwae_rows_fwd", ptr(x), ptr(recon), ptr(rows), B, K, P, loss_type, ptr(ws), nws, stream())
        ctx.save_for_backward(x, recon)
        ctx.cfg = (B, K, P, loss_type)
        return rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, recon = ctx.saved_tensors
        B, K, P, lt = ctx.cfg
        d = torch.empty_like(recon)
        call("itcv_iwae_rows_bwd", ptr(x), ptr(recon), ptr(_f32c(g)), ptr(d), B, K, P, lt, stream())
        return None, d, None


class IwaeCombineFn(Function):
    """The K-sample bound from the per-row terms (include/itcv_hip.h: itcv_iwae_combine_fwd): two launches forward, one
    backward.  ``rows`` [K B] fp32, ``lat`` [K B] fp64.  Outputs: the scalar -mean_b bound_b, differentiable in both, and,
    without a gradient, terms [4] = (rec, kl, bound, ess) and img [4, B] fp64 = per image (bound, ess, sum_k w rows,
    sum_k w lat).  The normalised weights go into ``sample.weights`` and ``estimator`` into ``sample.estimator``."""

    @staticmethod
    def forward(ctx, rows, lat, sample, beta_rec, beta_kl, estimator):
        B, K = sample.B, sample.K
        rows, lat = _f32c(rows), lat.contiguous()
        if lat.dtype != torch.float64 or rows.numel() != K * B or lat.numel() != K * B:
            raise ValueError(f"rows (fp32) and lat (fp64) must hold K B = {K * B} values")
        dev = rows.device
        out, terms = _loss_terms(4, dev)
        img = torch.empty((4, B), dtype=torch.float64, device=dev)
        call("itcv_iwae_combine_fwd", ptr(rows), ptr(lat), float(beta_rec), float(beta_kl), ptr(sample.weights), ptr(img),
             ptr(out), ptr(terms), B, K, stream())
        sample.estimator = int(estimator)
        ctx.cfg = (sample, float(beta_rec), float(beta_kl))
        ctx.mark_non_differentiable(terms, img)
        ctx.set_materialize_grads(False)
        return out, terms, img

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms, _g_img):
        sample, beta_rec, beta_kl = ctx.cfg
        if g is None:
            return (None,) * 6
        B, K = sample.B, sample.K
        g_rows = torch.empty((K * B,), dtype=F32, device=g.device)
        g_lat = torch.empty((K * B,), dtype=torch.float64, device=g.device)
        call("itcv_iwae_combine_bwd", ptr(_f32c(g)), ptr(sample.weights), beta_rec, beta_kl, ptr(g_rows), ptr(g_lat), B, K,
             stream())
        return g_rows, g_lat, None, None, None, None


def iwae_accumulate(rows, lat, state, beta_rec, beta_kl):
    """Merge one chunk's ``rows`` [Kc B] fp32 and ``lat`` [Kc B] fp64 into ``state`` [5, B] fp64 (a zero-filled state is
    empty): include/itcv_hip.h, itcv_iwae_accumulate.  One launch, no gradient."""
    B = state.shape[1]
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[0] != 5 or lat.dtype != torch.float64 \
            or rows.numel() != lat.numel() or rows.numel() % B:
        raise ValueError("state must be [5, B] fp64, lat fp64, and rows and lat hold Kc B values each")
    call("itcv_iwae_accumulate", ptr(_f32c(rows)), ptr(lat.contiguous()), float(beta_rec), float(beta_kl), ptr(state), B,
         rows.numel() // B, stream())
    return state


def iwae_finalize(state):
    """(log_px, elbo, ess), each [B] fp64, of an accumulated ``state`` (itcv_iwae_finalize).  One launch."""
    B = state.shape[1]
    out = torch.empty((3, B), dtype=torch.float64, device=state.device)
    call("itcv_iwae_finalize", ptr(state), ptr(out[0]), ptr(out[1]), ptr(out[2]), B, stream())
    return out[0], out[1], out[2]


class DiscPass:
    """One forward of the discriminator MLP over R stacked rows, the first R0 labelled 0 ("from q(z)") and the rest 1
    ("from the product of the marginals"): the input ``x`` [R, zdim], the hidden activations, the logits [R, 2], the
    device vector ``stats`` = (tc, d_loss, d_acc) of itcv_disc_head_fwd and the weights it ran with.  ``DiscTcFn`` and
    ``DiscLossFn`` walk it backwards, each on its own."""
    __slots__ = ("x", "acts", "logits", "stats", "weights", "biases", "slope", "R", "R0")


def _linear_ws(shapes, device):
    nws = max(lib.itcv_linear_workspace(B, K, N) for B, K, N in shapes)
    return (_ws(nws, device) if nws else None), nws


def disc_forward(x, weights, biases, slope, R0):
    """x [R, zdim] (dense fp32) through Linear + LeakyReLU(slope) for all but the last (weight, bias) pair -- one fused
    launch per layer, two when its K is split -- the plain Linear for the last (2 logits) and the head.  No gradient."""
    x = _f32c(x.detach())
    abi.need_device(x)
    R = x.shape[0]
    dp = DiscPass()
    dp.weights = [_f32c(w.detach()) for w in weights]
    dp.biases = [None if b is None else _f32c(b.detach()) for b in biases]
    if x.dim() != 2 or dp.weights[0].shape[1] != x.shape[1] or dp.weights[-1].shape[0] != 2 or not 1 <= R0 <= R:
        raise ValueError(f"discriminator: x {tuple(x.shape)}, first weight {tuple(dp.weights[0].shape)}, last weight "
                         f"{tuple(dp.weights[-1].shape)}, R0 = {R0}")
    dp.x, dp.slope, dp.R, dp.R0 = x, float(slope), R, int(R0)
    dev = x.device
    ws, nws = _linear_ws([(R, w.shape[1], w.shape[0]) for w in dp.weights], dev)
    dp.acts, h = [], x
    for w, b in zip(dp.weights[:-1], dp.biases[:-1]):
        N, K = w.shape
        y = torch.empty((R, N), dtype=F32, device=dev)
        call("itcv_linear_lrelu_fwd", ptr(h), K, ptr(w), ptr(b), ptr(y), R, K, N, dp.slope, ptr(ws), nws, stream())
        dp.acts.append(y)
        h = y
    w, b = dp.weights[-1], dp.biases[-1]
    dp.logits = torch.empty((R, 2), dtype=F32, device=dev)
    call("itcv_linear_fwd", ptr(h), ptr(w), ptr(b), ptr(dp.logits), R, w.shape[1], 2, ptr(ws), nws, stream())
    dp.stats = torch.empty((3,), dtype=F32, device=dev)
    call("itcv_disc_head_fwd", ptr(dp.logits), R, dp.R0, ptr(dp.stats), stream())
    return dp


class DiscTcFn(Function):
    """tc = mean_{i < R0} (l_i0 - l_i1) of a ``DiscPass`` as a function of ``z``, its first R0 input rows.  The backward
    is the VAE walk: the data-gradient chain of those rows only (head, then one itcv_linear_dgrad_lrelu per hidden layer
    and the plain data gradient of the first).  The discriminator's parameters are constants here: no weight or bias
    gradient is computed and no ``.grad`` is touched."""

    @staticmethod
    def forward(ctx, z, dp):
        if tuple(z.shape) != (dp.R0, dp.x.shape[1]):
            raise ValueError(f"z {tuple(z.shape)} is not the first {dp.R0} rows of the pass {tuple(dp.x.shape)}")
        ctx.dp = dp
        return dp.stats[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dp = ctx.dp
        B, dev = dp.R0, dp.x.device
        dy = torch.empty((B, 2), dtype=F32, device=dev)
        call("itcv_disc_head_bwd", ptr(_f32c(g)), ptr(dp.logits), ptr(dy), dp.R, B, 0, stream())
        ws, nws = _linear_ws([(B, w.shape[1], w.shape[0]) for w in dp.weights], dev)
        for l in range(len(dp.weights) - 1, 0, -1):
            N, K = dp.weights[l].shape
            dx = torch.empty((B, K), dtype=F32, device=dev)
            call("itcv_linear_dgrad_lrelu", ptr(dy), N, ptr(dp.weights[l]), ptr(dp.acts[l - 1]), K, ptr(dx), B, K, N, dp.slope,
                 ptr(ws), nws, stream())
            dy = dx
        N, K = dp.weights[0].shape
        dz = torch.empty((B, K), dtype=F32, device=dev)
        call("itcv_linear_dgrad", ptr(dy), ptr(dp.weights[0]), ptr(dz), B, K, N, ptr(ws), nws, stream())
        return dz, None


class DiscLossFn(Function):
    """d_loss = 0.5 mean CE(l_i, 0) over the first R0 rows + 0.5 mean CE(l_i, 1) over the others of a ``DiscPass`` as a
    function of the discriminator's parameters (w_0, b_0, w_1, b_1, ...: those the pass ran with).  The backward is the
    discriminator's walk: weight and bias gradients from all R rows (added straight into the flat ``.grad`` buffers inside
    ``direct_grad_accumulation``), the data gradient from layer to layer but not of the first: the input rows are
    constants, nothing flows to the encoder."""

    @staticmethod
    def forward(ctx, dp, *params):
        if dp.R0 >= dp.R:
            raise ValueError("the discriminator's loss needs rows of both labels (R0 < R)")
        ctx.dp, ctx.params = dp, params
        return dp.stats[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dp, params = ctx.dp, ctx.params
        R, dev = dp.R, dp.x.device
        dy = torch.empty((R, 2), dtype=F32, device=dev)
        call("itcv_disc_head_bwd", ptr(_f32c(g)), ptr(dp.logits), ptr(dy), R, dp.R0, 1, stream())
        ws, nws = _linear_ws([(R, w.shape[1], w.shape[0]) for w in dp.weights], dev)
        grads = [None] * len(params)
        for l in range(len(dp.weights) - 1, -1, -1):
            N, K = dp.weights[l].shape
            x = dp.acts[l - 1] if l else dp.x
            if ctx.needs_input_grad[1 + 2 * l]:
                tgt = _grad_target(params[2 * l])
                dw = None if tgt is not None else torch.empty((N, K), dtype=F32, device=dev)
                call("itcv_linear_wgrad", ptr(dy), ptr(x), ptr(tgt if tgt is not None else dw), R, K, N,
                     int(tgt is not None), ptr(ws), nws, stream())
                grads[2 * l] = dw
            if params[2 * l + 1] is not None and ctx.needs_input_grad[2 + 2 * l]:
                grads[2 * l + 1] = bias_grad_raw(dy, R, N, 1, _grad_target(params[2 * l + 1]))
            if l:
                dx = torch.empty((R, K), dtype=F32, device=dev)
                call("itcv_linear_dgrad_lrelu", ptr(dy), N, ptr(dp.weights[l]), ptr(x), K, ptr(dx), R, K, N, dp.slope, ptr(ws),
                     nws, stream())
                dy = dx
        return (None, *grads)


class ReconLossFn(Function):
    """scale * ops.reconstruction_loss(x, recon, loss_type, reduction) (ops.py:188-236 + the hook's beta): two launches
    forward, one backward; x is a constant."""

    @staticmethod
    def forward(ctx, x, recon, loss_type, reduction, scale):
        x, recon = _f32c(x), _f32c(recon)
        B = recon.shape[0]
        P = recon.numel() // B
        out = torch.empty((B,) if reduction == 0 else (), dtype=F32, device=recon.device)
        nws = lib.itcv_recon_workspace(B, P)
        ws = _ws(nws, recon.device)
        call("itcv_recon_loss_fwd", ptr(x), ptr(recon), ptr(out), B, P, loss_type, reduction, float(scale), ptr(ws), nws,
             stream())
        ctx.save_for_backward(x, recon)
        ctx.cfg = (B, P, loss_type, reduction, float(scale))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, recon = ctx.saved_tensors
        B, P, lt, reduction, scale = ctx.cfg
        d = torch.empty_like(recon)
        call("itcv_recon_loss_bwd", ptr(x), ptr(recon), ptr(_f32c(g)), ptr(d), B, P, lt, reduction, scale, stream())
        return None, d, None, None, None


def ssim_window_host(K, sigma):
    """The K taps of the SSIM window as Python floats: exp(-(i - (K - 1) / 2)^2 / (2 sigma^2)), normalised to sum 1, in
    fp64 on the host -- the device never evaluates exp for it."""
    K, sigma = int(K), float(sigma)
    if K < 1 or not sigma > 0.0:
        raise ValueError(f"ssim window: K >= 1 taps and sigma > 0 are needed (got {K}, {sigma})")
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2.0
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return (g / g.sum()).tolist()


_SSIM_WINDOWS = {}


def ssim_window(K, sigma, device):
    """fp64 ``[K]`` on the device: ``ssim_window_host``, cached per (K, sigma, device)."""
    device = torch.device(device)
    key = (int(K), float(sigma), device.type, device.index if device.index is not None else torch.cuda.current_device())
    w = _SSIM_WINDOWS.get(key)
    if w is None:
        w = _SSIM_WINDOWS[key] = torch.tensor(ssim_window_host(K, sigma), dtype=torch.float64).to(device)
    return w


def _ssim_images(x, y):
    x, y = _f32c(x), _f32c(y)
    if x.dim() != 4 or x.shape != y.shape:
        raise abi.HipExtensionError(f"ssim: two [B, C, H, W] images of one shape are expected (got {tuple(x.shape)}, "
                                    f"{tuple(y.shape)})")
    abi.need_device(x, y)
    return x, y


class SsimLossFn(Function):
    """scale * reduction_b [P alpha (1 - SSIM_b) + (1 - alpha) sum |y - x|] (itcv_ssim_loss_fwd): two launches forward,
    one backward; x is a constant; nothing of image size is kept but the two operands themselves."""

    @staticmethod
    def forward(ctx, x, recon, reduction, scale, alpha, K, sigma):
        x, recon = _ssim_images(x, recon)
        B, C, H, W = recon.shape
        win = ssim_window(K, sigma, recon.device)
        out = torch.empty((B,) if reduction == 0 else (), dtype=F32, device=recon.device)
        nws = lib.itcv_ssim_workspace(B, C, H, W, int(K))                # 0 for what the call below refuses
        ws = _ws(nws, recon.device)
        call("itcv_ssim_loss_fwd", ptr(x), ptr(recon), ptr(win), ptr(out), B, C, H, W, int(K), float(alpha), reduction,
             float(scale), ptr(ws), nws, stream())
        ctx.save_for_backward(x, recon, win)
        ctx.cfg = (B, C, H, W, int(K), float(alpha), reduction, float(scale))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, recon, win = ctx.saved_tensors
        B, C, H, W, K, alpha, reduction, scale = ctx.cfg
        d = torch.empty_like(recon)
        call("itcv_ssim_loss_bwd", ptr(x), ptr(recon), ptr(win), ptr(_f32c(g)), ptr(d), B, C, H, W, K, alpha, reduction,
             scale, stream())
        return None, d, None, None, None, None, None


def ssim_stats(x, y, K=11, sigma=1.5):
    """fp64 ``[B, C, 2]`` on the device: the mean of S (SSIM) and the mean of cs (its contrast-structure factor) over the
    positions of every plane of y against x (itcv_ssim_stats): two launches, nothing is read back."""
    x, y = _ssim_images(x.detach(), y.detach())
    B, C, H, W = y.shape
    win = ssim_window(K, sigma, y.device)
    stats = torch.empty((B, C, 2), dtype=torch.float64, device=y.device)
    nws = lib.itcv_ssim_workspace(B, C, H, W, int(K))                    # 0 for what the call below refuses
    ws = _ws(nws, y.device)
    call("itcv_ssim_stats", ptr(x), ptr(y), ptr(win), ptr(stats), B, C, H, W, int(K), ptr(ws), nws, stream())
    return stats


class ExpElboFn(Function):
    """mean_j exp(c * (a_j + b_j)) (solvers/intro.py:102-103 with c = -2 * scale): one launch each way."""

    @staticmethod
    def forward(ctx, a, b, c):
        a, b = _f32c(a), _f32c(b)
        B = a.shape[0]
        out = torch.empty((), dtype=F32, device=a.device)
        w = torch.empty((B,), dtype=F32, device=a.device)
        call("itcv_exp_elbo_fwd", ptr(a), ptr(b), ptr(out), ptr(w), B, float(c), stream())
        ctx.save_for_backward(w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        da, db = torch.empty_like(w), torch.empty_like(w)
        call("itcv_exp_elbo_bwd", ptr(_f32c(g)), ptr(w), ptr(da), ptr(db), w.shape[0], stream())
        return da, db, None


class LinCombFn(Function):
    """sum_k weights[k] * terms[k] over up to 8 device scalars: the scalar arithmetic of a solver's loss in one launch."""

    @staticmethod
    def forward(ctx, weights, *terms):
        n = len(terms)
        terms = [_f32c(t) for t in terms]
        if any(t.numel() != 1 for t in terms):
            raise abi.HipExtensionError("LinCombFn: every term must be a scalar")
        out = torch.empty((), dtype=F32, device=terms[0].device)
        tp = (ctypes.c_void_p * n)(*[ptr(t) for t in terms])
        wp = (ctypes.c_float * n)(*[float(w) for w in weights])
        call("itcv_lincomb_fwd", tp, wp, n, ptr(out), stream())
        ctx.weights = [float(w) for w in weights]
        ctx.shapes = [t.shape for t in terms]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        n = len(ctx.weights)
        grads = torch.empty((n,), dtype=F32, device=g.device)
        wp = (ctypes.c_float * n)(*ctx.weights)
        call("itcv_lincomb_bwd", ptr(_f32c(g)), wp, n, ptr(grads), stream())
        return (None,) + tuple(grads[k].reshape(ctx.shapes[k]) for k in range(n))


def tc_components(z, mu_all, logvar, dataset_size, row_offset=0, flags=abi.TC_LIVE, with_joint=False):
    """(prodm[Bl], logqz[Bl], lse[Bl,D]) of the fused pairwise-density / sampling kernel (+ the joint terms
    S[Bl,Bt] the backward reads, with ``with_joint``)."""
    z, mu_all, logvar = _f32c(z), _f32c(mu_all), _f32c(logvar)
    Bl, D = z.shape
    Bt = mu_all.shape[0]
    dev = z.device
    prodm = torch.empty((Bl,), dtype=F32, device=dev)
    logqz = torch.empty((Bl,), dtype=F32, device=dev)
    lse = torch.empty((Bl, D), dtype=F32, device=dev)
    sjoint = torch.empty((Bl, Bt), dtype=F32, device=dev)
    nws = lib.itcv_tc_fwd_workspace(Bl, Bt, D)
    ws = _ws(nws, dev)
    call("itcv_tc_fwd", ptr(z), ptr(mu_all), ptr(logvar), ptr(prodm), ptr(logqz), ptr(lse), ptr(sjoint), Bl, Bt,
         int(row_offset), D, int(dataset_size), int(flags), ptr(ws), nws, stream())
    return (prodm, logqz, lse, sjoint) if with_joint else (prodm, logqz, lse)


class TcRowsFn(Function):
    """ops.py:52-89 (live estimator) per local sample: tc[j] = log q(z_j) - sum_l log q(z_jl).
    ``mu_all`` holds the means of the whole (global) batch; rows are the caller's samples."""

    @staticmethod
    def forward(ctx, z, mu_all, logvar, dataset_size, row_offset):
        prodm, logqz, lse, sjoint = tc_components(z, mu_all, logvar, dataset_size, row_offset, abi.TC_LIVE, True)
        ctx.save_for_backward(_f32c(z), _f32c(mu_all), _f32c(logvar), logqz, lse, sjoint)
        ctx.cfg = (int(dataset_size), int(row_offset))
        return logqz - prodm

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, mu_all, logvar, logqz, lse, sjoint = ctx.saved_tensors
        n, off = ctx.cfg
        Bl, D = z.shape
        Bt = mu_all.shape[0]
        g = _f32c(g)
        dz, dlv, dmu = torch.empty_like(z), torch.empty_like(logvar), torch.empty_like(mu_all)
        nws = lib.itcv_tc_bwd_workspace(Bl, Bt)
        ws = _ws(nws, z.device)
        call("itcv_tc_bwd", ptr(g), ptr(z), ptr(mu_all), ptr(logvar), ptr(logqz), ptr(lse), ptr(sjoint), ptr(dz), ptr(dmu),
             ptr(dlv), Bl, Bt, off, D, n, abi.TC_LIVE, ptr(ws), nws, stream())
        return dz, dmu, dlv, None, None


def _bc3(x, mu, logvar):
    """The three operands as (same-storage) views broadcast to one shape of at most three dimensions, with their element
    strides (0 on broadcast dimensions) as ctypes arrays."""
    x, mu, logvar = (t if t.dtype == F32 else t.float() for t in (x, mu, logvar))
    xb, mb, lb = torch.broadcast_tensors(x, mu, logvar)
    shape = tuple(xb.shape)
    if len(shape) > 3:    # collapse the leading dimensions (needs dense operands there)
        xb, mb, lb = (t.contiguous().reshape(-1, *shape[-2:]) for t in (xb, mb, lb))
    while xb.dim() < 3:
        xb, mb, lb = xb.unsqueeze(0), mb.unsqueeze(0), lb.unsqueeze(0)
    arr = lambda v: (ctypes.c_int64 * 3)(*v)
    return shape, (xb, mb, lb), arr(xb.shape), arr(xb.stride()), arr(mb.stride()), arr(lb.stride())


class GaussLogDensityFn(Function):
    """ops.py:15-21 (``eps_density``) / ops.py:24-29 on broadcastable operands, materialised."""

    @staticmethod
    def forward(ctx, x, mu, logvar, eps_density):
        shape, views, dims, sx, sm, sl = _bc3(x, mu, logvar)
        out = torch.empty(tuple(views[0].shape), dtype=F32, device=views[0].device)
        abi.need_device(*views)
        call("itcv_gauss_logdensity_fwd", views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), ptr(out), dims, sx,
             sm, sl, int(eps_density), stream())
        ctx.save_for_backward(x, mu, logvar)
        ctx.eps_density = int(eps_density)
        return out.reshape(shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, mu, logvar = ctx.saved_tensors
        shape, views, dims, sx, sm, sl = _bc3(x, mu, logvar)
        g = _f32c(g).reshape(tuple(views[0].shape))
        dx, dlv = torch.empty_like(g), torch.empty_like(g)
        call("itcv_gauss_logdensity_bwd", ptr(g), views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), ptr(dx),
             ptr(dlv), dims, sx, sm, sl, ctx.eps_density, stream())
        dx, dlv = dx.reshape(shape), dlv.reshape(shape)
        # un-broadcast (torch reduction: plumbing of this off-path helper, not step arithmetic)
        return (dx.sum_to_size(x.shape) if ctx.needs_input_grad[0] else None,
                (-dx).sum_to_size(mu.shape) if ctx.needs_input_grad[1] else None,
                dlv.sum_to_size(logvar.shape) if ctx.needs_input_grad[2] else None, None)


class SamplingFn(Function):
    """ops.py:104-115 / ops.py:92-101 on a materialised [B,B,D] log-density tensor -> (prodm[B], logqz[B])."""

    @staticmethod
    def forward(ctx, lp, dataset_size, weighted):
        lp = _f32c(lp)
        B, B2, D = lp.shape
        if B != B2:
            raise abi.HipExtensionError(f"sampling: log_qz_prob must be [B,B,D] (got {tuple(lp.shape)})")
        dev = lp.device
        prodm, logqz = torch.empty((B,), dtype=F32, device=dev), torch.empty((B,), dtype=F32, device=dev)
        lse, sj = torch.empty((B, D), dtype=F32, device=dev), torch.empty((B, B), dtype=F32, device=dev)
        call("itcv_sampling_fwd", ptr(lp), ptr(prodm), ptr(logqz), ptr(lse), ptr(sj), B, D, int(dataset_size), int(weighted),
             stream())
        ctx.save_for_backward(lp, lse, sj, logqz)
        ctx.cfg = (B, D, int(dataset_size), int(weighted))
        return prodm, logqz

    @staticmethod
    @once_differentiable
    def backward(ctx, gp, gq):
        lp, lse, sj, logqz = ctx.saved_tensors
        B, D, n, weighted = ctx.cfg
        dlp = torch.empty_like(lp)
        call("itcv_sampling_bwd", ptr(_f32c(gp)), ptr(_f32c(gq)), ptr(lp), ptr(lse), ptr(sj), ptr(logqz), ptr(dlp), B, D, n,
             weighted, stream())
        return dlp, None, None


def on_off_diag(x):
    x = _f32c(x)
    if x.dim() != 2 or not (x.shape[0] == x.shape[1] or x.shape[0] == 1):
        raise abi.HipExtensionError(f"on_off_diag: a [n,n] or [1,n] tensor is expected (got {tuple(x.shape)})")
    m, n = x.shape
    diag = torch.empty((min(m, n),), dtype=F32, device=x.device)
    off = torch.empty((m, n, n), dtype=F32, device=x.device)
    call("itcv_on_off_diag", ptr(x), ptr(diag), ptr(off), m, n, stream())
    return diag, off


def diag_logdensity_rows(z, mu, logvar):
    z, mu, logvar = _f32c(z), _f32c(mu), _f32c(logvar)
    B, D = z.shape
    a = torch.empty((B,), dtype=F32, device=z.device)
    b = torch.empty((B,), dtype=F32, device=z.device)
    call("itcv_diag_logdensity_rows", ptr(z), ptr(mu), ptr(logvar), ptr(a), ptr(b), B, D, stream())
    return a, b


def aggregate_logdensity(z, mu, logvar, logw=None, splits=0):
    """``(logqz [S], lse [S, D])`` of the samples ``z`` [S, D] under the mixture of the N diagonal Gaussians
    ``(mu, logvar)`` [N, D] with log weights ``logw`` [N] (None: -log N each), streamed over the components
    (itcv_aggregate_logdensity): logqz[j] = logsumexp_i(logw_i + sum_l lp[j, i, l]), lse[j, l] = logsumexp_i(logw_i +
    lp[j, i, l]) with the ops.py:24-29 density of component i, clamped at -50 per element.  ``splits``: slices of the
    component range (0: the library's choice); for a given value a row's results do not depend on the other rows."""
    z, mu, logvar = _f32c(z), _f32c(mu), _f32c(logvar)
    if z.dim() != 2 or mu.dim() != 2 or mu.shape != logvar.shape or mu.shape[1] != z.shape[1]:
        raise abi.HipExtensionError(f"aggregate_logdensity: z [S, D] and mu, logvar [N, D] are expected (got "
                                    f"{tuple(z.shape)}, {tuple(mu.shape)}, {tuple(logvar.shape)})")
    (S, D), N = z.shape, mu.shape[0]
    if logw is not None:
        logw = _f32c(logw)
        if tuple(logw.shape) != (N,):
            raise abi.HipExtensionError(f"aggregate_logdensity: logw must have shape ({N},)")
    dev = z.device
    logqz = torch.empty((S,), dtype=F32, device=dev)
    lse = torch.empty((S, D), dtype=F32, device=dev)
    nws = lib.itcv_aggregate_workspace(S, N, D, int(splits))
    ws = _ws(nws, dev)
    call("itcv_aggregate_logdensity", ptr(z), ptr(mu), ptr(logvar), ptr(logw), ptr(logqz), ptr(lse), S, N, D, int(splits),
         ptr(ws), nws, stream())
    return logqz, lse


class ReconRowsFn(Function):
    """ops.py:219-230: per-sample summed reconstruction error; x is treated as a constant."""

    @staticmethod
    def forward(ctx, x, recon, loss_type):
        x, recon = _f32c(x), _f32c(recon)
        B = recon.shape[0]
        P = recon.numel() // B
        rows = torch.empty((B,), dtype=F32, device=recon.device)
        nws = lib.itcv_recon_workspace(B, P)
        ws = _ws(nws, recon.device)
        call("itcv_recon_rows_fwd", ptr(x), ptr(recon), ptr(rows), B, P, loss_type, ptr(ws), nws, stream())
        ctx.save_for_backward(x, recon)
        ctx.cfg = (B, P, loss_type)
        return rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, recon = ctx.saved_tensors
        B, P, lt = ctx.cfg
        g = _f32c(g)
        d = torch.empty_like(recon)
        call("itcv_recon_rows_bwd", ptr(x), ptr(recon), ptr(g), ptr(d), B, P, lt, stream())
        return None, d, None


# ------------------------------------------------------------------ disentanglement scores (csrc/disent.hip)
def _disent_mu(mu):
    """mu as an fp32 [N, D] device tensor with unit column stride (a row stride is passed to the kernels as is)."""
    if mu.dim() != 2 or mu.shape[0] < 1 or mu.shape[1] < 1:
        raise abi.HipExtensionError(f"disent: representations must be a non-empty [N, D] tensor (got {tuple(mu.shape)})")
    if mu.dtype != F32:
        raise abi.HipExtensionError(f"HIP path is fp32 only (got {mu.dtype})")
    abi.need_device(mu)
    return _unit_cols(mu.detach())


def disent_flags(device):
    """The two sticky flags of the disent kernels ([0] non-finite representation, [1] factor value out of range)."""
    return torch.zeros(2, dtype=torch.int32, device=device)


def disent_minmax(mu, flags):
    """Per-column (min[D], max[D]) of mu[N, D]; sets flags[0] on a non-finite element."""
    mu = _disent_mu(mu)
    N, D = mu.shape
    mn, mx = torch.empty((D,), dtype=F32, device=mu.device), torch.empty((D,), dtype=F32, device=mu.device)
    nws = lib.itcv_disent_minmax_workspace(N, D)
    ws = _ws(nws, mu.device)
    call("itcv_disent_minmax", mu.data_ptr(), mu.stride(0), N, D, ptr(mn), ptr(mx), ptr(flags), ptr(ws), nws, stream())
    return mn, mx


def disent_bins(mu, mn, mx, bins):
    """int32 [N, D] bin numbers 1..bins of the fixed fp64 binning rule (include/itcv_hip.h)."""
    mu = _disent_mu(mu)
    N, D = mu.shape
    out = torch.empty((N, D), dtype=torch.int32, device=mu.device)
    call("itcv_disent_bins", mu.data_ptr(), mu.stride(0), N, D, ptr(mn), ptr(mx), int(bins), ptr(out), stream())
    return out


def _disent_factors(factors, factor_sizes, N, device):
    sizes = [int(s) for s in factor_sizes]
    v = factors if isinstance(factors, torch.Tensor) else torch.as_tensor(factors)
    if v.dim() != 2 or v.shape[0] != N or v.shape[1] != len(sizes):
        raise abi.HipExtensionError(
            f"disent: factors must be [N = {N}, K = {len(sizes)}] (got {tuple(v.shape)})")
    v = v.to(device=device, dtype=torch.int32).contiguous()
    return v, sizes, (ctypes.c_int * len(sizes))(*sizes)


def disent_hist(mu, factors, factor_sizes, mn, mx, bins, flags):
    """(counts, vcount) as flat uint32 tables viewed as int32 tensors: counts[d][bins * off[k] + b * size[k] + f] and
    vcount[off[k] + f]; sets flags[1] on a factor value outside its range.  The range checks of the library (bins, K, sizes)
    raise before any launch."""
    mu = _disent_mu(mu)
    N, D = mu.shape
    v, sizes, csizes = _disent_factors(factors, factor_sizes, N, mu.device)
    fsum = sum(sizes)
    n = lib.itcv_disent_counts_elems(D, fsum, int(bins))              # 0 for sizes the call below refuses
    counts = torch.empty((max(n, 1),), dtype=torch.int32, device=mu.device)
    vcount = torch.empty((max(fsum, 1),), dtype=torch.int32, device=mu.device)
    call("itcv_disent_hist", mu.data_ptr(), mu.stride(0), ptr(v), N, D, len(sizes), csizes, int(bins), ptr(mn), ptr(mx),
         ptr(counts), ptr(vcount), ptr(flags), stream())
    return counts, vcount


def disent_hist_tiling(D, factor_sizes, bins):
    """The launch plan ``disent_hist`` makes for these sizes, asked of the library's own planner without any GPU work: a
    dict of ``tc`` (columns per block), ``column_tiles``, ``groups`` (the first factor of every factor group) and
    ``lds_bytes``.  Raises what ``disent_hist`` raises for sizes outside the supported range."""
    sizes = [int(s) for s in factor_sizes]
    out = (ctypes.c_int * 21)()
    call("itcv_disent_hist_tiling", int(D), len(sizes), (ctypes.c_int * max(len(sizes), 1))(*sizes), int(bins), out)
    return dict(tc=out[0], column_tiles=out[1], groups=list(out[4:4 + out[2]]), lds_bytes=out[3])


def disent_mi(counts, vcount, N, D, factor_sizes, bins):
    """(MI[D, K], H[K]) in fp64 from the integer tables of ``disent_hist``."""
    sizes = [int(s) for s in factor_sizes]
    mi = torch.empty((D, len(sizes)), dtype=torch.float64, device=counts.device)
    h = torch.empty((len(sizes),), dtype=torch.float64, device=counts.device)
    call("itcv_disent_mi", ptr(counts), ptr(vcount), int(N), int(D), len(sizes), (ctypes.c_int * len(sizes))(*sizes),
         int(bins), ptr(mi), ptr(h), stream())
    return mi, h


# ------------------------------------------------------------------ classifier-based scores (csrc/logreg.hip)
F64 = torch.float64


def _lr_sizes(class_sizes):
    sizes = [int(s) for s in class_sizes]
    return sizes, (ctypes.c_int * max(len(sizes), 1))(*sizes)


def logreg_colstats(x, flags):
    """StandardScaler's (mean[D], scale[D]) of x[N, D] in fp64: population variance, scale 1 where it is 0."""
    x = _disent_mu(x)
    N, D = x.shape
    mean, scale = torch.empty((D,), dtype=F64, device=x.device), torch.empty((D,), dtype=F64, device=x.device)
    nws = lib.itcv_logreg_colstats_workspace(N, D)
    ws = _ws(nws, x.device)
    call("itcv_logreg_colstats", x.data_ptr(), x.stride(0), N, D, ptr(mean), ptr(scale), ptr(flags), ptr(ws), nws, stream())
    return mean, scale


class LogregProblem:
    """The fixed inputs of K softmax regressions that share x[N, D]: labels y[N, K], class counts, the class mask and the
    optional standardisation (mean, scale).  ``valgrad`` / ``proba`` evaluate at a theta[(D + 1), csum] fp64."""

    def __init__(self, x, y, class_sizes, cvalid, flags, stats=None, C=1.0):
        self.x = _disent_mu(x)
        self.N, self.D = self.x.shape
        self.y, self.sizes, self.csizes = _disent_factors(y, class_sizes, self.N, self.x.device)
        self.K, self.csum = len(self.sizes), sum(self.sizes)
        self.cvalid = cvalid.to(device=self.x.device, dtype=torch.int32).contiguous()
        if self.cvalid.numel() != self.csum:
            raise abi.HipExtensionError(f"logreg: the class mask needs {self.csum} entries (got {self.cvalid.numel()})")
        self.mean, self.scale = stats if stats is not None else (None, None)
        self.flags, self.C = flags, float(C)
        self.nws = lib.itcv_logreg_workspace(self.N, self.D, self.K, self.csum)      # 0 for what the calls refuse
        self.ws = torch.empty((max(self.nws, 8),), dtype=torch.uint8, device=self.x.device)

    def _theta(self, theta):
        if theta.dtype != F64 or tuple(theta.shape) != (self.D + 1, self.csum) or not theta.is_contiguous():
            raise abi.HipExtensionError(f"logreg: theta must be a dense fp64 [{self.D + 1}, {self.csum}] tensor")
        return theta

    def valgrad(self, theta):
        """(f[K], grad[(D + 1), csum]) at theta, as fp64 device tensors."""
        f = torch.empty((self.K,), dtype=F64, device=self.x.device)
        g = torch.empty((self.D + 1, self.csum), dtype=F64, device=self.x.device)
        call("itcv_logreg_valgrad", self.x.data_ptr(), self.x.stride(0), ptr(self.mean), ptr(self.scale), ptr(self.y), self.N,
             self.D, self.K, self.csizes, ptr(self.cvalid), ptr(self._theta(theta)), self.C, ptr(f), ptr(g), ptr(self.flags),
             ptr(self.ws), self.nws, stream())
        return f, g

    def proba(self, theta, x=None, y=None):
        """(P[N, csum] fp64, pred[N, K] int32) at theta, of this problem's rows or of another (x, y) of the same width."""
        x = self.x if x is None else _disent_mu(x)
        N = x.shape[0]
        if x.shape[1] != self.D:
            raise abi.HipExtensionError(f"logreg: x must have {self.D} columns (got {x.shape[1]})")
        y = self.y if y is None else _disent_factors(y, self.sizes, N, x.device)[0]
        P = torch.empty((N, self.csum), dtype=F64, device=x.device)
        pred = torch.empty((N, self.K), dtype=torch.int32, device=x.device)
        call("itcv_logreg_proba", x.data_ptr(), x.stride(0), ptr(self.mean), ptr(self.scale), ptr(y), N, self.D, self.K,
             self.csizes, ptr(self.cvalid), ptr(self._theta(theta)), ptr(P), ptr(pred), ptr(self.flags), stream())
        return P, pred


def logreg_auc(P, y, class_sizes, cvalid, flags):
    """(count2, pos, neg) as int64 [csum] tensors: the pair counts of every valid class over its problem's valid rows."""
    sizes, csizes = _lr_sizes(class_sizes)
    N = P.shape[0]
    y = _disent_factors(y, sizes, N, P.device)[0]
    if P.dtype != F64 or P.dim() != 2 or P.shape[1] != sum(sizes) or not P.is_contiguous():
        raise abi.HipExtensionError("logreg: P must be a dense fp64 [N, csum] tensor")
    cvalid = cvalid.to(device=P.device, dtype=torch.int32).contiguous()
    out = torch.empty((3, max(sum(sizes), 1)), dtype=torch.int64, device=P.device)
    call("itcv_logreg_auc", ptr(P), ptr(y), N, len(sizes), csizes, ptr(cvalid), ptr(out[0]), ptr(out[1]), ptr(out[2]),
         ptr(flags), stream())
    return out[0], out[1], out[2]


def zdiff_row(a, b, out):
    """out[d] = mean_b |a[b, d] - b[b, d]| (fp64 accumulation) into the fp32 row ``out`` of a preallocated buffer."""
    if a.shape != b.shape or a.dim() != 2 or a.dtype != F32 or b.dtype != F32 or a.stride(1) != 1 or b.stride(1) != 1 \
            or a.stride(0) != b.stride(0) or out.dtype != F32 or out.numel() != a.shape[1] or not out.is_contiguous():
        raise abi.HipExtensionError("zdiff_row: a, b must be fp32 [B, D] with one row stride, out a dense fp32 [D] row")
    call("itcv_zdiff_row", a.data_ptr(), b.data_ptr(), a.stride(0), a.shape[0], a.shape[1], out.data_ptr(), stream())
    return out


# ------------------------------------------------------------------ boosted trees for DCI (csrc/gbt.hip)
GBT_NODES = abi.DEFINES["ITCV_GBT_TREE_NODES"]          # heap slots of one tree
U8, I64 = torch.uint8, torch.int64


def _gbt_dense(t, dtype, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise abi.HipExtensionError(f"gbt: {what} must be a dense {dtype} device tensor; there is no CPU path")
    return t


def gbt_cuts(x_train, max_bin):
    """(cuts[D, max_bin - 1] fp32, nbins[D] int32) of the training rows: the columns are sorted on the device by
    ``torch.sort``, the cut selection is a kernel."""
    x = _disent_mu(x_train)
    N, D = x.shape
    srt = torch.sort(x.t().contiguous(), dim=1).values
    cuts = torch.zeros((D, max(int(max_bin) - 1, 1)), dtype=F32, device=x.device)
    nbins = torch.empty((D,), dtype=torch.int32, device=x.device)
    call("itcv_gbt_cuts", ptr(srt), N, D, int(max_bin), ptr(cuts), ptr(nbins), stream())
    return cuts, nbins


def gbt_bin(x, cuts, nbins, max_bin, flags):
    """uint8 bins[D, N] (feature-major) of x[N, D] under the given cuts; sets flags[0] on a non-finite element."""
    x = _disent_mu(x)
    N, D = x.shape
    if cuts.shape[0] != D:
        raise abi.HipExtensionError(f"gbt: x must have {cuts.shape[0]} columns (got {D})")
    out = torch.empty((D, N), dtype=U8, device=x.device)
    call("itcv_gbt_bin", x.data_ptr(), x.stride(0), N, D, int(max_bin), ptr(_gbt_dense(cuts, F32, "cuts")),
         ptr(_gbt_dense(nbins, torch.int32, "nbins")), ptr(out), ptr(flags), stream())
    return out


def gbt_grad(F, y, class_sizes, cvalid, flags, with_fp64=False):
    """(gq, hq) int64 [csum, N] from the margins F[csum, N] (``with_fp64``: also g, h before quantisation)."""
    sizes, csizes = _lr_sizes(class_sizes)
    F = _gbt_dense(F, F64, "the margins")
    csum, N = F.shape
    y = _disent_factors(y, sizes, N, F.device)[0]
    gq, hq = torch.empty((csum, N), dtype=I64, device=F.device), torch.empty((csum, N), dtype=I64, device=F.device)
    g = torch.empty((csum, N), dtype=F64, device=F.device) if with_fp64 else None
    h = torch.empty((csum, N), dtype=F64, device=F.device) if with_fp64 else None
    call("itcv_gbt_grad", ptr(F), ptr(y), N, len(sizes), csizes, ptr(_gbt_dense(cvalid, torch.int32, "cvalid")), ptr(gq),
         ptr(hq), ptr(g), ptr(h), ptr(flags), stream())
    return (gq, hq, g, h) if with_fp64 else (gq, hq)


def gbt_hist(bins, gq, hq, node, cvalid, level, max_bin, c0=0, nc=None):
    """int64 tab[nc, 2^level, D, max_bin, 2]: (G, H) sums of class slots c0..c0+nc-1 over the rows whose node id (heap
    index, uint8 [csum, N]) lies in ``level``."""
    bins, node = _gbt_dense(bins, U8, "bins"), _gbt_dense(node, U8, "node")
    D, N = bins.shape
    nc = gq.shape[0] - c0 if nc is None else nc
    tab = torch.empty((nc, 1 << int(level), D, int(max_bin), 2), dtype=I64, device=bins.device)
    call("itcv_gbt_hist", ptr(bins), N, D, int(max_bin), ptr(_gbt_dense(gq, I64, "gq")), ptr(_gbt_dense(hq, I64, "hq")),
         ptr(node), ptr(_gbt_dense(cvalid, torch.int32, "cvalid")), int(c0), int(nc), int(level), ptr(tab),
         tab.numel() * 8, stream())
    return tab


def gbt_tree_arrays(rounds, csum, device):
    """(tfeat, tbin, tvalue, tgain), each [rounds, csum, GBT_NODES]; tfeat filled with -1 (leaf or absent)."""
    shape = (int(rounds), int(csum), GBT_NODES)
    return (torch.full(shape, -1, dtype=torch.int32, device=device), torch.zeros(shape, dtype=torch.int32, device=device),
            torch.zeros(shape, dtype=F64, device=device), torch.zeros(shape, dtype=F64, device=device))


def gbt_split(tab, nbins, cvalid, level, trees, nsum, lam=1.0, eta=0.3, c0=0):
    """Choose the splits of the nodes of ``level`` from tab[nc, 2^level, D, max_bin, 2] and write them into ONE round's tree
    arrays ``trees`` = (tfeat, tbin, tvalue, tgain), each [csum, GBT_NODES], and the node sums nsum[csum, GBT_NODES, 2]."""
    tab = _gbt_dense(tab, I64, "the table")
    nc, nn, D, B, _ = tab.shape
    if nn != 1 << int(level):
        raise abi.HipExtensionError(f"gbt: a table of level {level} has {1 << int(level)} nodes (got {nn})")
    tfeat, tbin, tvalue, tgain = trees
    call("itcv_gbt_split", ptr(tab), ptr(_gbt_dense(nbins, torch.int32, "nbins")), D, B,
         ptr(_gbt_dense(cvalid, torch.int32, "cvalid")), int(c0), nc, int(level), float(lam), float(eta),
         ptr(_gbt_dense(nsum, I64, "nsum")), ptr(_gbt_dense(tfeat, torch.int32, "tfeat")),
         ptr(_gbt_dense(tbin, torch.int32, "tbin")), ptr(_gbt_dense(tvalue, F64, "tvalue")),
         ptr(_gbt_dense(tgain, F64, "tgain")), stream())


def gbt_advance(bins, cvalid, tfeat, tbin, level, node):
    """Move the rows that sit in a split node of ``level`` to its children, in place: node[csum, N] uint8 heap indices,
    tfeat / tbin [csum, GBT_NODES] of ONE round.  Rows in a leaf and rows of an invalid class stay."""
    bins, node = _gbt_dense(bins, U8, "bins"), _gbt_dense(node, U8, "node")
    csum, N = node.shape
    if bins.shape[1] != N or tuple(tfeat.shape) != (csum, GBT_NODES) or tuple(tbin.shape) != (csum, GBT_NODES):
        raise abi.HipExtensionError(f"gbt: node ids [{csum}, {N}] need bins [D, {N}] and trees [{csum}, {GBT_NODES}]")
    call("itcv_gbt_advance", ptr(bins), N, csum, ptr(_gbt_dense(cvalid, torch.int32, "cvalid")),
         ptr(_gbt_dense(tfeat, torch.int32, "tfeat")), ptr(_gbt_dense(tbin, torch.int32, "tbin")), int(level), ptr(node),
         stream())
    return node


def gbt_margins(bins, cvalid, node, trees, max_depth, F):
    """F[csum, N] += the value of every row's leaf in ONE round's ``trees`` = (tfeat, tbin, tvalue, tgain), each
    [csum, GBT_NODES], in place: the leaf is node[csum, N] where the node ids are given, else (``node`` None) the row
    walks the tree from the root for at most ``max_depth`` levels.  Invalid classes are left alone."""
    bins, F = _gbt_dense(bins, U8, "bins"), _gbt_dense(F, F64, "the margins")
    csum, N = F.shape
    tfeat, tbin, tvalue = trees[0], trees[1], trees[2]
    if bins.shape[1] != N or any(tuple(t.shape) != (csum, GBT_NODES) for t in (tfeat, tbin, tvalue)) \
            or (node is not None and tuple(node.shape) != (csum, N)):
        raise abi.HipExtensionError(f"gbt: margins [{csum}, {N}] need bins [D, {N}], node ids [{csum}, {N}] and trees "
                                    f"[{csum}, {GBT_NODES}]")
    call("itcv_gbt_margins", ptr(bins), N, csum, ptr(_gbt_dense(cvalid, torch.int32, "cvalid")),
         ptr(None if node is None else _gbt_dense(node, U8, "node")), ptr(_gbt_dense(tfeat, torch.int32, "tfeat")),
         ptr(_gbt_dense(tbin, torch.int32, "tbin")), ptr(_gbt_dense(tvalue, F64, "tvalue")), int(max_depth), ptr(F),
         stream())
    return F


def gbt_predict(F, y, class_sizes, cvalid, flags):
    """(pred[N, K] int32, correct[K] int64): first argmax of F[csum, N] over the valid classes and the number of rows whose
    label equals it; sets flags[1] on a label outside its range."""
    sizes, csizes = _lr_sizes(class_sizes)
    F = _gbt_dense(F, F64, "the margins")
    N = F.shape[1]
    y = _disent_factors(y, sizes, N, F.device)[0]
    pred = torch.empty((N, len(sizes)), dtype=torch.int32, device=F.device)
    correct = torch.empty((max(len(sizes), 1),), dtype=I64, device=F.device)
    call("itcv_gbt_predict", ptr(F), ptr(y), N, len(sizes), csizes, ptr(_gbt_dense(cvalid, torch.int32, "cvalid")),
         ptr(pred), ptr(correct), ptr(flags), stream())
    return pred, correct


def gbt_importance(tfeat, tgain, class_sizes, D):
    """fp64 imp[K, D]: xgboost's `gain` importance of every problem from the tree arrays [rounds, csum, GBT_NODES]."""
    sizes, csizes = _lr_sizes(class_sizes)
    imp = torch.empty((len(sizes), int(D)), dtype=F64, device=tfeat.device)
    call("itcv_gbt_importance", ptr(_gbt_dense(tfeat, torch.int32, "tfeat")), ptr(_gbt_dense(tgain, F64, "tgain")),
         tfeat.shape[0], len(sizes), csizes, int(D), ptr(imp), stream())
    return imp


# ------------------------------------------------------------------ FactorVAE and SAP scores (csrc/extra_scores.hip)
def extra_flags(device):
    """The three sticky flags of the FactorVAE / SAP kernels ([0] non-finite representation, [1] factor index or label out
    of range, [2] a SAP classifier that did not converge)."""
    return torch.zeros(3, dtype=torch.int32, device=device)


def _fvae_groups(mu, L):
    """mu[M * L, D] checked BEFORE anything touches the device: (mu, M, L)."""
    L = int(L)
    if L < 2:
        raise ValueError(f"factor_vae: a group needs L >= 2 rows for a ddof = 1 variance (got L = {L})")
    if mu.dim() != 2 or mu.shape[0] < L or mu.shape[0] % L:
        raise ValueError(f"factor_vae: the representations must be [M * L, D] with L = {L} (got {tuple(mu.shape)})")
    return _disent_mu(mu), mu.shape[0] // L, L


def fvae_gvar(mu, flags):
    """fp64 gvar[D]: the ddof = 1 variance of every column of mu[N, D], N >= 2; sets flags[0] on a non-finite element."""
    if mu.dim() == 2 and mu.shape[0] < 2:
        raise ValueError(f"factor_vae: the variance estimate needs at least 2 rows (got {mu.shape[0]})")
    mu = _disent_mu(mu)
    N, D = mu.shape
    gvar = torch.empty((D,), dtype=F64, device=mu.device)
    call("itcv_fvae_gvar", mu.data_ptr(), mu.stride(0), N, D, ptr(gvar), ptr(flags), stream())
    return gvar


def fvae_votes(mu, L, gvar, threshold, fidx, num_factors, flags):
    """int64 votes[D, K]: every group of L consecutive rows of mu[M * L, D] votes for (argmin over the active dimensions of
    its variance / gvar, fidx[group]).  Sets flags[0] / flags[1] on a non-finite element / an index outside [0, K)."""
    mu, M, L = _fvae_groups(mu, L)
    D, K = mu.shape[1], int(num_factors)
    fidx = torch.as_tensor(fidx).reshape(-1)
    if fidx.numel() != M:
        raise ValueError(f"factor_vae: {M} groups need {M} factor indices (got {fidx.numel()})")
    fidx = fidx.to(device=mu.device, dtype=torch.int32).contiguous()
    gvar = _gbt_dense(gvar, F64, "gvar")
    if gvar.numel() != D:
        raise abi.HipExtensionError(f"factor_vae: gvar needs {D} entries (got {gvar.numel()})")
    votes = torch.empty((D, max(K, 1)), dtype=I64, device=mu.device)
    call("itcv_fvae_votes", mu.data_ptr(), mu.stride(0), M, L, D, ptr(gvar), float(threshold), ptr(fidx), K, ptr(votes),
         ptr(flags), stream())
    return votes


def fvae_classify(votes_train, votes_eval, num_train, num_eval, gvar, threshold):
    """(classifier[D] int32, res[3] fp64 = train accuracy, eval accuracy, active dimensions) from the two vote tables."""
    vt, ve = _gbt_dense(votes_train, I64, "votes"), _gbt_dense(votes_eval, I64, "votes")
    D, K = vt.shape
    if ve.shape != vt.shape:
        raise abi.HipExtensionError("factor_vae: the two vote tables differ in shape")
    classifier = torch.empty((D,), dtype=torch.int32, device=vt.device)
    res = torch.empty((3,), dtype=F64, device=vt.device)
    call("itcv_fvae_classify", ptr(vt), ptr(ve), D, K, int(num_train), int(num_eval), ptr(_gbt_dense(gvar, F64, "gvar")),
         float(threshold), ptr(classifier), ptr(res), stream())
    return classifier, res


def sap_svc_lds_rows():
    """Train rows up to which itcv_sap_svc_fit keeps a block's column and labels in LDS (above: streamed)."""
    return lib.itcv_sap_svc_lds_rows()


def sap_svc_fit(x, y, class_sizes, flags, C=0.01, gtol=1e-10, max_iter=100):
    """Every (latent, factor, class) squared-hinge classifier of x[N, D] / y[N, K] in one solve launch.  Returns
    ``(theta [D, csum, 2], gnorm [D, csum], iters [D, csum] int32, cvalid [csum] int32)``; flags[2] is set when a problem
    did not converge."""
    x = _disent_mu(x)
    N, D = x.shape
    y, sizes, csizes = _disent_factors(y, class_sizes, N, x.device)
    K, csum = len(sizes), sum(sizes)
    nws = lib.itcv_sap_svc_workspace(N, D, K, csum)                     # 0 for what the call below refuses
    ws = torch.empty((max(nws, 8),), dtype=torch.uint8, device=x.device)
    theta = torch.empty((D, max(csum, 1), 2), dtype=F64, device=x.device)
    gnorm = torch.empty((D, max(csum, 1)), dtype=F64, device=x.device)
    iters = torch.empty((D, max(csum, 1)), dtype=torch.int32, device=x.device)
    cvalid = torch.empty((max(csum, 1),), dtype=torch.int32, device=x.device)
    call("itcv_sap_svc_fit", x.data_ptr(), x.stride(0), ptr(y), N, D, K, csizes, float(C), float(gtol), int(max_iter),
         ptr(theta), ptr(gnorm), ptr(iters), ptr(cvalid), ptr(flags), ptr(ws), nws, stream())
    return theta, gnorm, iters, cvalid


def sap_svc_score(x, y, class_sizes, cvalid, theta, flags, with_pred=False):
    """int64 correct[D, K]: the test rows of x[Nt, D] / y[Nt, K] whose prediction under ``theta`` equals the label
    (``with_pred``: also pred[D, K, Nt] int32)."""
    x = _disent_mu(x)
    Nt, D = x.shape
    y, sizes, csizes = _disent_factors(y, class_sizes, Nt, x.device)
    K, csum = len(sizes), sum(sizes)
    theta, cvalid = _gbt_dense(theta, F64, "theta"), _gbt_dense(cvalid, torch.int32, "cvalid")
    if tuple(theta.shape) != (D, csum, 2) or cvalid.numel() != csum:
        raise abi.HipExtensionError(f"sap: theta must be [{D}, {csum}, 2] and cvalid [{csum}]")
    correct = torch.empty((D, K), dtype=I64, device=x.device)
    pred = torch.empty((D, K, Nt), dtype=torch.int32, device=x.device) if with_pred else None
    call("itcv_sap_svc_score", x.data_ptr(), x.stride(0), ptr(y), Nt, D, K, csizes, ptr(cvalid), ptr(theta), ptr(correct),
         ptr(pred), ptr(flags), stream())
    return (correct, pred) if with_pred else correct


# ------------------------------------------------------------------ unsupervised scores and IRS (csrc/unsup_scores.hip)
def unsup_cov(x, flags):
    """fp64 ``(mean [D], cov [D, D])`` of x[N, D], N >= 2: the ddof = 1 covariance of the centred values, symmetric bit
    for bit; sets flags[0] on a non-finite element."""
    if x.dim() == 2 and x.shape[0] < 2:
        raise ValueError(f"covariance: at least 2 rows are needed (got {x.shape[0]})")
    x = _disent_mu(x)
    N, D = x.shape
    mean = torch.empty((D,), dtype=F64, device=x.device)
    cov = torch.empty((D, D), dtype=F64, device=x.device)
    nws = lib.itcv_unsup_cov_workspace(N, D)                            # 0 for what the call below refuses
    ws = _ws(nws, x.device)
    call("itcv_unsup_cov", x.data_ptr(), x.stride(0), N, D, ptr(mean), ptr(cov), ptr(flags), ptr(ws), nws, stream())
    return mean, cov


def unsup_gauss_lds_dim():
    """Largest D whose matrix itcv_unsup_gauss keeps in LDS (above: in its global workspace)."""
    return lib.itcv_unsup_gauss_lds_dim()


def unsup_gauss(cov):
    """``(res [5] fp64 = tc, w, w_norm, tr C, logdet C; eig [D] fp64; info [4] int32 = pivot failed, its dimension, Jacobi
    did not converge, sweeps)`` of a symmetric fp64 ``cov [D, D]``: one launch, nothing is read back."""
    cov = _gbt_dense(cov, F64, "cov")
    if cov.dim() != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] < 1:
        raise abi.HipExtensionError(f"unsup: the covariance must be a square [D, D] tensor (got {tuple(cov.shape)})")
    D = cov.shape[0]
    res = torch.empty((5,), dtype=F64, device=cov.device)
    eig = torch.empty((D,), dtype=F64, device=cov.device)
    info = torch.empty((4,), dtype=torch.int32, device=cov.device)
    nws = lib.itcv_unsup_gauss_workspace(D)
    ws = _ws(nws, cov.device)
    call("itcv_unsup_gauss", ptr(cov), D, ptr(res), ptr(eig), ptr(info), ptr(ws), nws, stream())
    return res, eig, info


def irs(x, factors, factor_sizes, mn, mx, flags, diff_quantile=0.99):
    """The IRS rule of include/itcv_hip.h on x[N, D] / factors[N, K]: a dict of device tensors ``maxdev [D]``, ``cum
    [D, K]``, ``M [D, K]``, ``score [D]`` (fp64), ``parent [D]``, ``active [D]`` (int32) and ``res [2]`` (IRS, number of
    active dimensions).  The rows of every factor value are made contiguous by one stable device sort of the factor
    columns; sets flags[1] on a factor value outside its range."""
    x = _disent_mu(x)
    N, D = x.shape
    v, sizes, csizes = _disent_factors(factors, factor_sizes, N, x.device)
    K, fsum = len(sizes), sum(sizes)
    order = torch.sort(v.t().contiguous(), dim=1, stable=True).indices.to(torch.int32).contiguous() if K else v
    dev = x.device
    out = dict(maxdev=torch.empty((D,), dtype=F64, device=dev), cum=torch.empty((D, max(K, 1)), dtype=F64, device=dev),
               M=torch.empty((D, max(K, 1)), dtype=F64, device=dev), score=torch.empty((D,), dtype=F64, device=dev),
               parent=torch.empty((D,), dtype=torch.int32, device=dev),
               active=torch.empty((D,), dtype=torch.int32, device=dev), res=torch.empty((2,), dtype=F64, device=dev))
    nws = lib.itcv_irs_workspace(N, D, K, fsum)                         # 0 for what the call below refuses
    ws = _ws(nws, dev)
    call("itcv_irs", x.data_ptr(), x.stride(0), ptr(v), ptr(order), N, D, K, csizes, float(diff_quantile), ptr(mn), ptr(mx),
         ptr(out["maxdev"]), ptr(out["cum"]), ptr(out["M"]), ptr(out["score"]), ptr(out["parent"]), ptr(out["active"]),
         ptr(out["res"]), ptr(flags), ptr(ws), nws, stream())
    return out


# ------------------------------------------------------------------ UDR: ranks and the Lasso matrix (csrc/udr.hip)
def udr_rank_lds_rows():
    """Largest N whose sorted keys itcv_udr_ranks keeps in LDS (above: in its global workspace)."""
    return lib.itcv_udr_rank_lds_rows()


def udr_ranks(x, flags):
    """fp32 ``r2 [N, D]``: twice the tie-averaged rank (``2 * scipy.stats.rankdata``) of every column of x[N >= 2, D], an
    exact integer; sets flags[0] on a non-finite element (the ranks are then unspecified)."""
    if x.dim() == 2 and x.shape[0] < 2:
        raise ValueError(f"udr ranks: at least 2 rows are needed (got {x.shape[0]})")
    x = _disent_mu(x)
    N, D = x.shape
    r2 = torch.empty((N, D), dtype=F32, device=x.device)
    nws = lib.itcv_udr_ranks_workspace(N, D)                            # 0 in LDS, and for what the call below refuses
    ws = _ws(nws, x.device)
    call("itcv_udr_ranks", x.data_ptr(), x.stride(0), N, D, ptr(r2), ptr(flags), ptr(ws), nws, stream())
    return r2


def udr_lasso(cov, Da, Db, alpha=0.1, gtol=1e-12, max_sweeps=1000):
    """``(W [Da, Db] fp64, info [3] int32)`` of the fp64 covariance ``cov [Da + Db, Da + Db]`` of the columns [a | b]:
    ``W[k, t] = |w_t[k]|``, the Lasso of include/itcv_hip.h that predicts the standardised column t of b from the
    standardised columns of a; ``info`` = (a target did not reach gtol, how many, the largest sweep count).  Nothing is read
    back."""
    cov = _gbt_dense(cov, F64, "cov")
    Da, Db = int(Da), int(Db)
    if cov.dim() != 2 or cov.shape[0] != cov.shape[1] or cov.shape[0] != Da + Db:
        raise abi.HipExtensionError(f"udr: the covariance must be a square [Da + Db, Da + Db] tensor (got "
                                    f"{tuple(cov.shape)} for Da = {Da}, Db = {Db})")
    W = torch.empty((max(Da, 0), max(Db, 0)), dtype=F64, device=cov.device)
    info = torch.empty((3,), dtype=torch.int32, device=cov.device)
    nws = lib.itcv_udr_lasso_workspace(Da, Db)                          # 0 for what the call below refuses
    ws = _ws(nws, cov.device)
    call("itcv_udr_lasso", ptr(cov), Da, Db, float(alpha), float(gtol), int(max_sweeps), ptr(W), ptr(info), ptr(ws), nws,
         stream())
    return W, info


# ------------------------------------------------------------------ sample quality (csrc/quality.hip)
def knn_radius(x, k, flags, splits=0):
    """fp64 ``r2 [N]``: the (k + 1)-th smallest squared distance from every row of x[N, D] to the rows of x, itself
    included (itcv_knn_radius).  ``splits``: slices of the candidate rows (0: the library's choice); the result does not
    depend on it.  Sets flags[0] on a non-finite element."""
    x = _disent_mu(x)
    N, D = x.shape
    r2 = torch.empty((N,), dtype=F64, device=x.device)
    nws = lib.itcv_knn_radius_workspace(N, D, int(k), int(splits))      # 0 for what the call below refuses
    ws = _ws(nws, x.device)
    call("itcv_knn_radius", x.data_ptr(), x.stride(0), N, D, int(k), int(splits), ptr(r2), ptr(flags), ptr(ws), nws,
         stream())
    return r2


def prdc_counts(real, fake, r2_real, r2_fake, flags, splits=0):
    """``(fake_hits [M] int32, real_covered [N] int32, real_min [N] fp64)`` of real[N, D] against fake[M, D] under the
    squared radii ``r2_real [N]``, ``r2_fake [M]`` (itcv_prdc_counts; every comparison strict)."""
    real, fake = _disent_mu(real), _disent_mu(fake)
    (N, D), M = real.shape, fake.shape[0]
    r2_real, r2_fake = _gbt_dense(r2_real, F64, "r2_real"), _gbt_dense(r2_fake, F64, "r2_fake")
    if fake.shape[1] != D or tuple(r2_real.shape) != (N,) or tuple(r2_fake.shape) != (M,):
        raise abi.HipExtensionError(f"prdc: real [N, D], fake [M, D], r2_real [N] and r2_fake [M] are expected (got "
                                    f"{tuple(real.shape)}, {tuple(fake.shape)}, {tuple(r2_real.shape)}, "
                                    f"{tuple(r2_fake.shape)})")
    dev = real.device
    hits = torch.empty((M,), dtype=torch.int32, device=dev)
    covered = torch.empty((N,), dtype=torch.int32, device=dev)
    rmin = torch.empty((N,), dtype=F64, device=dev)
    call("itcv_prdc_counts", real.data_ptr(), real.stride(0), fake.data_ptr(), fake.stride(0), N, M, D, ptr(r2_real),
         ptr(r2_fake), int(splits), ptr(hits), ptr(covered), ptr(rmin), ptr(flags), stream())
    return hits, covered, rmin


def poly_mmd(x, y, flags, degree=3, gamma=0.0, coef0=1.0):
    """fp64 ``res [4] = (Sxx, Syy, Sxy, mmd2)`` of the polynomial kernel (gamma a.b + coef0)^degree on x[N, D], y[M, D]
    (itcv_poly_mmd; gamma 0: 1 / D).  Nothing is read back."""
    x, y = _disent_mu(x), _disent_mu(y)
    (N, D), M = x.shape, y.shape[0]
    if y.shape[1] != D:
        raise abi.HipExtensionError(f"poly_mmd: x [N, D] and y [M, D] are expected (got {tuple(x.shape)}, {tuple(y.shape)})")
    res = torch.empty((4,), dtype=F64, device=x.device)
    nws = lib.itcv_poly_mmd_workspace(N, M, D)                          # 0 for what the call below refuses
    ws = _ws(nws, x.device)
    call("itcv_poly_mmd", x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), N, M, D, int(degree), float(gamma),
         float(coef0), ptr(res), ptr(flags), ptr(ws), nws, stream())
    return res


def frechet(mean1, cov1, mean2, cov2, eps=0.0):
    """``(res [5] fp64 = fd, |m1 - m2|^2, tr(C1 + eps I), tr(C2 + eps I), tr sqrt; eig [D] fp64; info [5] int32 = pivot of
    C1 + eps I failed, its dimension, Jacobi did not converge, sweeps, eigenvalues clipped at 0)`` of two fp64 means [D]
    and symmetric covariances [D, D] (itcv_frechet): one launch, nothing is read back."""
    mean1, mean2 = _gbt_dense(mean1, F64, "mean1"), _gbt_dense(mean2, F64, "mean2")
    cov1, cov2 = _gbt_dense(cov1, F64, "cov1"), _gbt_dense(cov2, F64, "cov2")
    D = mean1.numel()
    if cov1.dim() != 2 or D < 1 or tuple(cov1.shape) != (D, D) or tuple(cov2.shape) != (D, D) or mean2.numel() != D:
        raise abi.HipExtensionError(f"frechet: means [D] and covariances [D, D] are expected (got {tuple(mean1.shape)}, "
                                    f"{tuple(cov1.shape)}, {tuple(mean2.shape)}, {tuple(cov2.shape)})")
    dev = cov1.device
    res = torch.empty((5,), dtype=F64, device=dev)
    eig = torch.empty((D,), dtype=F64, device=dev)
    info = torch.empty((5,), dtype=torch.int32, device=dev)
    nws = lib.itcv_frechet_workspace(D)                                 # 0 for what the call below refuses
    ws = _ws(nws, dev)
    call("itcv_frechet", ptr(mean1), ptr(cov1), ptr(mean2), ptr(cov2), D, float(eps), ptr(res), ptr(eig), ptr(info),
         ptr(ws), nws, stream())
    return res, eig, info


# ------------------------------------------------------------------ Gaussian mixture (csrc/gmm.hip)
def _gmm_params(weights, means, third, what):
    """(K, D) of dense fp64 ``weights [K]``, ``means [K, D]`` and a third operand ``[K, D, D]`` named ``what``."""
    for t, n in ((weights, "weights"), (means, "means"), (third, what)):
        _gbt_dense(t, F64, n)
    if means.dim() != 2 or tuple(weights.shape) != means.shape[:1] or tuple(third.shape) != (*means.shape, means.shape[1]):
        raise abi.HipExtensionError(f"gmm: weights [K], means [K, D] and {what} [K, D, D] are expected (got "
                                    f"{tuple(weights.shape)}, {tuple(means.shape)}, {tuple(third.shape)})")
    return means.shape


def gmm_factor(cov):
    """``(chol, prec_chol, log_det [K], info [K] int32)`` of fp64 covariances ``cov [K, D, D]`` (itcv_gmm_factor; ``cov`` is
    not written): the lower Cholesky factors, their inverses, the log-determinants, and per component 0 or 1 + the dimension
    of the first failed pivot.  One launch, nothing is read back."""
    cov = _gbt_dense(cov, F64, "cov")
    if cov.dim() != 3 or cov.shape[1] != cov.shape[2] or cov.shape[0] < 1 or cov.shape[1] < 1:
        raise abi.HipExtensionError(f"gmm: the covariances must be a [K, D, D] tensor (got {tuple(cov.shape)})")
    K, D = cov.shape[:2]
    chol = cov.clone()
    linv = torch.empty_like(cov)
    logdet = torch.empty((K,), dtype=F64, device=cov.device)
    info = torch.empty((K,), dtype=torch.int32, device=cov.device)
    call("itcv_gmm_factor", ptr(chol), K, D, ptr(linv), ptr(logdet), ptr(info), stream())
    return chol, linv, logdet, info


def gmm_estep(x, weights, means, prec_chol, log_det, flags, hard=False):
    """``(lp [N, K], resp [N, K], loglik [N], sum_loglik [1])`` (fp64) of x[N, D] under the mixture (itcv_gmm_estep);
    ``hard``: one-hot responsibilities of the largest ``lp``.  Sets flags[0] on a non-finite element."""
    x = _disent_mu(x)
    N, D = x.shape
    K, Dm = _gmm_params(weights, means, prec_chol, "prec_chol")
    if Dm != D or tuple(_gbt_dense(log_det, F64, "log_det").shape) != (K,):
        raise abi.HipExtensionError(f"gmm: x [N, {Dm}] and log_det [{K}] are expected (got {tuple(x.shape)}, "
                                    f"{tuple(log_det.shape)})")
    dev = x.device
    lp, resp = torch.empty((N, K), dtype=F64, device=dev), torch.empty((N, K), dtype=F64, device=dev)
    loglik, total = torch.empty((N,), dtype=F64, device=dev), torch.empty((1,), dtype=F64, device=dev)
    nws = lib.itcv_gmm_estep_workspace(N, D, K)                         # 0 for what the call below refuses
    ws = _ws(nws, dev)
    call("itcv_gmm_estep", x.data_ptr(), x.stride(0), N, D, K, ptr(weights), ptr(means), ptr(prec_chol), ptr(log_det),
         int(bool(hard)), ptr(lp), ptr(resp), ptr(loglik), ptr(total), ptr(flags), ptr(ws), nws, stream())
    return lp, resp, loglik, total


def gmm_mstep(x, resp, flags, reg=0.0, with_cov=True):
    """``(nk [K], weights [K], means [K, D], covariances [K, D, D] or None)`` (fp64) of x[N, D] under the responsibilities
    ``resp [N, K]`` (itcv_gmm_mstep); ``with_cov`` false stops after the means."""
    x = _disent_mu(x)
    N, D = x.shape
    resp = _gbt_dense(resp, F64, "resp")
    if resp.dim() != 2 or resp.shape[0] != N or resp.shape[1] < 1:
        raise abi.HipExtensionError(f"gmm: resp [{N}, K] is expected (got {tuple(resp.shape)})")
    K, dev = resp.shape[1], x.device
    nk, w = torch.empty((K,), dtype=F64, device=dev), torch.empty((K,), dtype=F64, device=dev)
    mean = torch.empty((K, D), dtype=F64, device=dev)
    cov = torch.empty((K, D, D), dtype=F64, device=dev) if with_cov else None
    nws = lib.itcv_gmm_mstep_workspace(N, D, K, int(bool(with_cov)))    # 0 for what the call below refuses
    ws = _ws(nws, dev)
    call("itcv_gmm_mstep", x.data_ptr(), x.stride(0), ptr(resp), N, D, K, float(reg), int(bool(with_cov)), ptr(nk), ptr(w),
         ptr(mean), ptr(cov), ptr(flags), ptr(ws), nws, stream())
    return nk, w, mean, cov


def gmm_sample(means, chol, comp, eps, flags):
    """fp32 ``z [R, D]``, ``z[r] = (float)(means[c] + chol[c] eps[r])`` with ``c = comp[r]`` (int32 [R]) and fp32 ``eps
    [R, D]`` (itcv_gmm_sample); sets flags[1] on a component number outside [0, K)."""
    means, chol = _gbt_dense(means, F64, "means"), _gbt_dense(chol, F64, "chol")
    if means.dim() != 2 or tuple(chol.shape) != (*means.shape, means.shape[1]):
        raise abi.HipExtensionError(f"gmm: means [K, D] and chol [K, D, D] are expected (got {tuple(means.shape)}, "
                                    f"{tuple(chol.shape)})")
    K, D = means.shape
    eps = _gbt_dense(eps, F32, "eps")
    comp = _gbt_dense(comp, torch.int32, "comp")
    if eps.dim() != 2 or eps.shape[1] != D or tuple(comp.shape) != eps.shape[:1]:
        raise abi.HipExtensionError(f"gmm: eps [R, {D}] and comp [R] are expected (got {tuple(eps.shape)}, "
                                    f"{tuple(comp.shape)})")
    R = eps.shape[0]
    z = torch.empty((R, D), dtype=F32, device=eps.device)
    call("itcv_gmm_sample", ptr(means), ptr(chol), ptr(comp), ptr(eps), R, D, K, ptr(z), ptr(flags), stream())
    return z
