"""GPU: the nn.Linear GEMMs (``gemm64_kernel`` / ``gemm64_vec_kernel`` / ``gemm64_reduce`` / ``gemm64_reduce_epi`` behind the
five ``itcv_linear_*`` entry points) give the bits they gave at the commit before operands were read in 16-byte pieces
(DESIGN section 6, round 7).  The MFMA's internal order cannot be emulated on a host, so tests/golden/linear_bits.npz was
recorded from a build of that commit; every comparison is an equality of bytes, with no tolerance.  Beside it every output
is held to an fp64 product with the normwise bar tests/test_hip_factor.py uses for these entry points (1e-4).

Cases (B, N, K) -- whole outputs are stored, so the weight gradient's N x K bounds the sizes:

* (8, 20, 96): 3 K-tiles, no split anywhere;            * (64, 64, 128): whole tiles, forward split in 2;
* (70, 20, 100): ragged M tile, ragged last K-tile;      * (8, 200, 128): ragged N tile; the data gradient (K' = 200:
* (8, 20, 1030): nothing 16-byte readable (the scalar      7 K-tiles) splits in 3 with a short last slice, under the
  kernel), forward split in 11 over 33 K-tiles;            fused mask epilogue too;
* (8, 20, 1024): forward split in 16;                    * (8, 20, 2048): the 32-slice cap (forward entry points only).
(The accumulating weight gradient of (8, 20, 1030) is left out: the fixture stays under 1 MB.)

Per case: forward with and without bias, data gradient, weight gradient without and with ``accumulate``, LeakyReLU forward
with and without bias and with x dense, inside rows 5 floats longer (no 16-byte alignment) and inside rows 8 floats longer
(aligned), masked data gradient with dy / y_prev laid out the same three ways.  The split counts are asserted through
``itcv_linear_workspace`` against the plan they are meant to come from.

    python tests/test_hip_linear_bits.py OUT.npz        # re-record (on a GPU, from a build of the PARENT commit)
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_bits.npz")
BAR = 1e-4
SLOPE = 0.2
# (B, N, K, forward splits, data-gradient splits, weight-gradient splits, what is left out to keep the fixture small:
#  "acc" the accumulating weight gradient, "back" every backward entry point)
CASES = [(8, 20, 96, 1, 1, 1, ""), (64, 64, 128, 2, 1, 1, ""), (70, 20, 100, 2, 1, 1, ""),
         (8, 20, 1030, 11, 1, 1, "acc"), (8, 20, 1024, 16, 1, 1, ""), (8, 200, 128, 2, 3, 1, ""),
         (8, 20, 2048, 32, 1, 1, "back")]


def _id(c):
    return f"b{c[0]}-n{c[1]}-k{c[2]}"


def dev():
    return torch.device("cuda:0")


def _hash(n, seed):
    """n floats in [-0.5, 0.5), multiples of 2^-24: integer arithmetic only."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 69069 + 12345)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    return ((h >> np.uint64(8)).astype(np.float64) * (1.0 / (1 << 24)) - 0.5).astype(np.float32)


def inputs(case):
    B, N, K = case[:3]
    s = 7 * B + 3 * N + K
    x = (_hash(B * K, s + 1) * 4.0).reshape(B, K)
    w = (_hash(N * K, s + 2) * 0.25).reshape(N, K)
    b = _hash(N, s + 3)
    dy = (_hash(B * N, s + 4) * 2.0).reshape(B, N)
    yprev = (_hash(B * K, s + 5) * 2.0).reshape(B, K).copy()
    yprev[_hash(B * K, s + 6).reshape(B, K) < -0.4] = 0.0        # exact zeros in the mask: they take the slope
    dw0 = _hash(N * K, s + 7).reshape(N, K)
    return x, w, b, dy, yprev, dw0


def plan(M, N, K):
    """Split count of one GEMM (csrc/conv_igemm.hip, plan_gemm64)."""
    cdiv = lambda a, b: -(-a // b)
    tiles, kt = cdiv(M, 64) * cdiv(N, 64), cdiv(K, 32)
    splits = 1
    if tiles < 128 and kt >= 4:
        splits = max(1, min(cdiv(256, tiles), 32, kt // 2))
    return cdiv(kt, cdiv(kt, splits))


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def place(a, pad):
    """Device view of ``a``: dense (pad 0), or inside rows ``pad`` floats longer whose other entries are NaN."""
    if pad == 0:
        return G(a)
    wide = np.full((a.shape[0], a.shape[1] + pad), np.nan, dtype=np.float32)
    lo = 4 if pad == 8 else 3
    wide[:, lo:lo + a.shape[1]] = a
    return G(wide)[:, lo:lo + a.shape[1]]


def run(case):
    """name -> device tensor, every output of the case; the strided layouts are checked against the dense ones here."""
    from hipvae import abi
    B, N, K, sf, sd, sw, left_out = case
    assert (plan(B, N, K), plan(B, K, N), plan(N, K, B)) == (sf, sd, sw), _id(case)
    nws = abi.lib.itcv_linear_workspace(B, K, N)
    assert nws == max(s * m * n * 4 if s > 1 else 0 for s, m, n in ((sf, B, N), (sd, B, K), (sw, N, K))), _id(case)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device=dev())
    x, w, b, dy, yprev, dw0 = inputs(case)
    tx, tw, tb, tdy = G(x), G(w), G(b), G(dy)
    st = abi.stream()
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev())
    out = {}
    for name, bias in (("fwd_bias", tb), ("fwd", None)):
        y = nan(B, N)
        abi.call("itcv_linear_fwd", abi.ptr(tx), abi.ptr(tw), abi.ptr(bias), abi.ptr(y), B, K, N, abi.ptr(ws), nws, st)
        out[name] = y
    for name, bias in (("lrelu_fwd_bias", tb), ("lrelu_fwd", None)):
        for pad in (0, 5, 8):
            xx = place(x, pad)
            y = nan(B, N)
            abi.call("itcv_linear_lrelu_fwd", xx.data_ptr(), xx.stride(0), abi.ptr(tw), abi.ptr(bias), abi.ptr(y), B, K, N,
                     SLOPE, abi.ptr(ws), nws, st)
            if pad:
                assert torch.equal(y, out[name]), (_id(case), name, pad)
            else:
                out[name] = y
    if left_out == "back":
        torch.cuda.synchronize()
        return out
    dx = nan(B, K)
    abi.call("itcv_linear_dgrad", abi.ptr(tdy), abi.ptr(tw), abi.ptr(dx), B, K, N, abi.ptr(ws), nws, st)
    out["dgrad"] = dx
    for pad in (0, 5, 8):
        dd, yy = place(dy, pad), place(yprev, pad)
        dx = nan(B, K)
        abi.call("itcv_linear_dgrad_lrelu", dd.data_ptr(), dd.stride(0), abi.ptr(tw), yy.data_ptr(), yy.stride(0),
                 abi.ptr(dx), B, K, N, SLOPE, abi.ptr(ws), nws, st)
        if pad:
            assert torch.equal(dx, out["dgrad_lrelu"]), (_id(case), pad)
        else:
            out["dgrad_lrelu"] = dx
    for name, acc in (("wgrad", 0), ("wgrad_acc", 1))[:1 if left_out == "acc" else 2]:
        dw = G(dw0) if acc else nan(N, K)
        abi.call("itcv_linear_wgrad", abi.ptr(tdy), abi.ptr(tx), abi.ptr(dw), B, K, N, acc, abi.ptr(ws), nws, st)
        out[name] = dw
    torch.cuda.synchronize()
    return out


def reference(case):
    x, w, b, dy, yprev, dw0 = (a.astype(np.float64) for a in inputs(case))
    lrelu = lambda v: np.where(v > 0, v, SLOPE * v)
    return {"fwd_bias": x @ w.T + b, "fwd": x @ w.T, "lrelu_fwd_bias": lrelu(x @ w.T + b), "lrelu_fwd": lrelu(x @ w.T),
            "dgrad": dy @ w, "dgrad_lrelu": (dy @ w) * np.where(yprev > 0, 1.0, SLOPE), "wgrad": dy.T @ x,
            "wgrad_acc": dw0 + dy.T @ x}


def _bytes(t):
    return t.contiguous().cpu().numpy().view(np.uint8).reshape(-1)


_golden = []


def golden():
    if not _golden:
        _golden.append(np.load(GOLDEN))
    return _golden[0]


def test_the_cases_reach_every_path():
    splits = {s for c in CASES for s in c[3:6]}
    assert {1, 2, 3, 11, 16, 32} <= splits
    assert any(c[2] % 32 and c[3] > 1 for c in CASES) and any(c[0] % 64 and c[0] > 64 for c in CASES)
    assert {c[0] for c in CASES} == {8, 64, 70} and {c[1] for c in CASES} == {20, 64, 200}
    assert {96, 100, 128, 1024, 1030} <= {c[2] for c in CASES}
    assert any(c[4] > 1 and -(-c[1] // 32) % c[4] for c in CASES)      # a split data gradient with a short last slice


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_linear_bits(case):
    got, ref = run(case), reference(case)
    for key, val in got.items():
        want = ref[key]
        err = float(np.abs(val.double().cpu().numpy() - want).max() / np.abs(want).max())
        print(_id(case), key, f"{err:.2e}")
        assert err <= BAR, (_id(case), key, err)
    for key, val in got.items():
        assert np.array_equal(_bytes(val), golden()[f"{_id(case)}/{key}"]), f"{_id(case)}: {key} differs from the recorded bytes"


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "intro-tc-vae_amd"))
    rec = {}
    for c in CASES:
        rec.update({f"{_id(c)}/{k}": _bytes(v) for k, v in run(c).items()})
    np.savez_compressed(sys.argv[1], **rec)
    print(f"recorded {len(CASES)} cases -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)")
