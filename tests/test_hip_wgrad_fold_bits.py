"""GPU: the fold of the weight-gradient split-K slabs (``wgrad_p_reduce_many`` behind ``itcv_wgrad_reduce_desc`` +
``itcv_wgrad_reduce_many``; ``wgrad_p_reduce`` behind ``itcv_conv2d_wgrad_bf16p``) adds what it is documented to add, in
the documented order.  The expected bytes are a numpy float32 emulation of the two orders, per (element, tap):

* wide tiles (every source has < 64 slices): per source, ``acc`` = the sequential sum over slices 0 .. S-1 from +0;
  ``tot += acc`` in source order; ``tot`` starts from ``dw`` (accumulate) or from +0;
* fine tiles (some source has >= 64 slices): per source q = ceil(S / 16), sixteen group sums over slices
  [g q, min((g + 1) q, S)), each sequential from +0; ``sum = (((0 + a0) + a1) ... + a15)``; ``tot += sum``.

Every comparison is an equality of bytes.  The slab values are normal deviates times 2^k, k in -8 .. 8, so that every
other order of the additions gives other bits.  Each slab buffer ends in NaN beyond its slices (read one slice too far
and the result is NaN) and ``dw`` lies inside a larger buffer of a sentinel that must survive.

Cases: wide with 1, 2, 3, 7 slices (pair loop, odd tail); fine with 64, 65, 81, 170 slices (q = 4, 5, 6, 11; at 65 and 81
the last groups are short or empty); 1, 2 and 4 sources with different slice counts, below and above 64 mixed;
accumulate 0 / 1; ``dw`` 16-byte aligned and one float past that; Co x Ci = 32 x 32 (one wide tile), 32 x 40 (a second, partly
empty one; 80 fine tile numbers, 20 blocks of four), 64 x 64, 128 x 64; one table of eleven descriptors, fine and wide alternating, with more work than the launch has
blocks (3584 tile numbers, 2432 of the kernel's work items, a grid of 2048): blocks take several items and cross
descriptors.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
FINE = 64                    # a descriptor is "fine" when one of its sources has at least this many slices


def dev():
    return torch.device("cuda:0")


def expected(srcs, dw0):
    """srcs: float32 arrays [S][9][coci]; dw0: [coci][9] or None -> [coci][9], the documented order in float32."""
    coci = srcs[0].shape[2]
    fine = any(s.shape[0] >= FINE for s in srcs)
    tot = np.zeros((9, coci), np.float32) if dw0 is None else np.ascontiguousarray(dw0.T)
    for s in srcs:
        S = s.shape[0]
        if fine:
            q = (S + 15) // 16
            acc = np.zeros((9, coci), np.float32)
            for g in range(16):
                a = np.zeros((9, coci), np.float32)
                for sl in range(g * q, min((g + 1) * q, S)):
                    a = a + s[sl]
                acc = acc + a
        else:
            acc = np.zeros((9, coci), np.float32)
            for sl in range(S):
                acc = acc + s[sl]
        tot = tot + acc
    assert tot.dtype == np.float32
    return np.ascontiguousarray(tot.T)


def make_slab(S, coci, gen):
    """Device buffer [S + 1][9][coci]: S slices of normal deviates times 2^k, then one slice of NaN."""
    n = S * 9 * coci
    v = torch.randn(n, generator=gen, device=dev()) * torch.exp2(torch.randint(-8, 9, (n,), generator=gen, device=dev()).float())
    buf = torch.full(((S + 1) * 9 * coci,), float("nan"), device=dev())
    buf[:n] = v
    return buf


def make_dw(coci, misalign, gen):
    """(buffer of sentinels, view of coci * 9 floats inside it, 16-byte aligned or one float past that)."""
    buf = torch.full((coci * 9 + 16,), SENTINEL, device=dev())
    start = 4 + (1 if misalign else 0)
    view = buf[start:start + coci * 9]
    assert view.data_ptr() % 16 == (4 if misalign else 0)
    view.copy_(torch.randn(coci * 9, generator=gen, device=dev()))
    return buf, view, start


def build_table(descs):
    """descs: (slab buffers, slice counts, dw view, Co, Ci, accumulate) -> (device table, n, tile numbers)."""
    from hipvae import abi
    nb = abi.lib.itcv_wgrad_reduce_desc_bytes()
    assert nb == 80
    host = (ctypes.c_uint8 * (nb * len(descs)))()
    blocks = 0
    for i, (slabs, splits, dw, Co, Ci, acc) in enumerate(descs):
        sl = (ctypes.c_void_p * len(slabs))(*[s.data_ptr() for s in slabs])
        sp = (ctypes.c_int * len(slabs))(*splits)
        got = abi.lib.itcv_wgrad_reduce_desc(ctypes.byref(host, i * nb), sl, sp, len(slabs), dw.data_ptr(), Co, Ci, acc, blocks)
        fine = any(s >= FINE for s in splits)
        assert got == (-(-Co * Ci // 16) if fine else -(-Co * Ci // 1024)), (i, got)     # the recorded tile counts stay
        blocks += got
    return torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev()), len(descs), blocks


def run_table(specs, seed):
    """specs: (Co, Ci, slice counts, accumulate, misalign) per descriptor; folds them in ONE launch and checks each."""
    from hipvae import abi
    gen = torch.Generator(device=dev()).manual_seed(seed)
    descs, keep = [], []
    for Co, Ci, splits, acc, mis in specs:
        coci = Co * Ci
        slabs = [make_slab(S, coci, gen) for S in splits]
        buf, view, start = make_dw(coci, mis, gen)
        dw0 = view.cpu().numpy().reshape(coci, 9).copy()
        descs.append((slabs, splits, view, Co, Ci, acc))
        keep.append((buf, start, dw0))
    table, n, blocks = build_table(descs)
    abi.call("itcv_wgrad_reduce_many", abi.ptr(table), n, blocks, abi.stream())
    torch.cuda.synchronize()
    for i, ((slabs, splits, view, Co, Ci, acc), (buf, start, dw0)) in enumerate(zip(descs, keep)):
        coci = Co * Ci
        srcs = [s.cpu().numpy()[:S * 9 * coci].reshape(S, 9, coci) for s, S in zip(slabs, splits)]
        want = expected(srcs, dw0 if acc else None)
        got = buf.cpu().numpy()
        tag = f"descriptor {i}: {Co} x {Ci}, slices {splits}, accumulate {acc}, misaligned {mis}"
        assert np.array_equal(got[start:start + coci * 9].view(np.uint8), want.reshape(-1).view(np.uint8)), tag
        assert (got[:start] == SENTINEL).all() and (got[start + coci * 9:] == SENTINEL).all(), tag + ": wrote outside dw"
    return blocks


def _variants(Co, Ci, splits, seed):
    for k, (acc, mis) in enumerate(((0, False), (1, False), (0, True), (1, True))):
        run_table([(Co, Ci, splits, acc, mis)], seed + k)


@pytest.mark.parametrize("S", [1, 2, 3, 7])
@pytest.mark.parametrize("Co, Ci", [(32, 32), (32, 40)])
def test_wide_tiles(Co, Ci, S):
    _variants(Co, Ci, [S], 10 * S + Ci)


@pytest.mark.parametrize("S", [64, 65, 81, 170])
@pytest.mark.parametrize("Co, Ci", [(32, 40), (64, 64), (128, 64)])
def test_fine_tiles(Co, Ci, S):
    _variants(Co, Ci, [S], 1000 + 10 * S + Co)


@pytest.mark.parametrize("Co, Ci, splits", [(32, 40, [2, 5]), (64, 64, [3, 7]), (32, 32, [3, 70]), (64, 64, [81, 2]),
                                            (32, 40, [1, 7, 3, 2]), (64, 64, [1, 7, 64, 3]), (128, 64, [65, 81, 170, 64])],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, list) else str(v))
def test_several_sources(Co, Ci, splits):
    _variants(Co, Ci, splits, 2000 + sum(splits))


def test_one_table_with_more_work_than_blocks():
    wide = [(512, 512, [1], k % 2, False) for k in range(8)]
    fine = [(128, 64, [64], 1, False), (128, 64, [65, 3], 0, True), (128, 64, [2, 81], 1, True)]
    specs = []
    for k in range(8):                                   # fine and wide alternating while there are fine ones
        specs.append(wide[k])
        if k < 3:
            specs.append(fine[k])
    assert len(specs) == 11
    blocks = run_table(specs, 77)
    assert blocks == 8 * 256 + 3 * 512 and 8 * 256 + 3 * 128 > 2048


# ---- the single-layer reduce behind itcv_conv2d_wgrad_bf16p: slabs from the real kernel, read back from its workspace
@pytest.mark.parametrize("B, Ci, H, W, Co, fine", [(8, 32, 8, 8, 32, False), (64, 64, 32, 32, 128, True)])
def test_single_layer_reduce(B, Ci, H, W, Co, fine):
    from hipvae import abi
    from hipvae import functional as HF
    S = abi.lib.itcv_conv2d_wgrad_bf16p_slabs(B, Ci, H, W, Co, 3)
    assert S >= 1 and (S >= FINE) == fine, S
    gen = torch.Generator(device=dev()).manual_seed(5)
    x = torch.randn(B, Ci, H, W, generator=gen, device=dev())
    dy = torch.randn(B, Co, H, W, generator=gen, device=dev()) * 1e-3
    xp, dyp = HF.split_planes(x, 4), HF.split_planes(dy, 4, gradient=True)
    nws = abi.lib.itcv_conv2d_wgrad_bf16p_workspace(B, Ci, H, W, Co, 3)
    coci = Co * Ci
    assert nws >= S * 9 * coci * 4
    for acc, mis in ((0, False), (1, True), (1, False)):
        ws = torch.zeros(nws // 4, device=dev())
        buf, view, start = make_dw(coci, mis, gen)
        dw0 = view.cpu().numpy().reshape(coci, 9).copy()
        abi.call("itcv_conv2d_wgrad_bf16p", abi.ptr(xp), abi.ptr(dyp), view.data_ptr(), B, Ci, H, W, Co, 3, 0, 4, acc,
                 abi.ptr(ws), nws, abi.stream())
        torch.cuda.synchronize()
        slabs = ws.cpu().numpy()[:S * 9 * coci].reshape(S, 9, coci)
        assert np.abs(slabs).max() > 0
        want = expected([slabs], dw0 if acc else None)
        got = buf.cpu().numpy()
        assert np.array_equal(got[start:start + coci * 9].view(np.uint8), want.reshape(-1).view(np.uint8)), (acc, mis)
        assert (got[:start] == SENTINEL).all() and (got[start + coci * 9:] == SENTINEL).all()
