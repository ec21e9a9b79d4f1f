"""GPU: the backward of the live TC estimator (``tc_bwd_rows_kernel``, ``tc_bwd_cols_kernel``) gives the bits it gave at the
commit before its loads were batched.  tests/golden/tc_bwd_bits.npz was recorded from a build
of that commit; every comparison is an equality of bytes (uint8 views, so -0.0 and +0.0 differ), with no tolerance.

Per case ``itcv_tc_kl_fwd`` then ``itcv_tc_kl_bwd`` run through ``hipvae.abi`` and ``dz``, ``dlogvar``, ``dmu_all`` and
``wq`` (the backward's workspace: the row kernel writes it, the column kernel reads it) are compared whole.  The inputs are
exact integer hashes (the same floats on any host); z lies up to two units from its own mean at standard deviations of
0.05 .. 1, so about a third of the (row, column, dimension) terms falls under the -50 clamp and contributes nothing: the
terms are counted on the host in fp64 and the count is held to the one recorded with the bytes.

Shapes (Bl, Bt, D): (8, 8, 10) and (5, 7, 3) -- fewer columns / rows than one batch of a wave, Bt no multiple of 4, D < 64;
(64, 64, 128) -- the benchmarked size, one full batch per wave; (16, 64, 70) -- D no multiple of 64, Bl != Bt.  Each with
row_offset 0 and, where Bt > Bl, a nonzero one; a per-row and a broadcast (reduced output) upstream gradient; coef_kl 0
and nonzero.

    python tests/test_hip_tc_bwd_bits.py OUT.npz        # re-record (on a GPU, from a build of the PARENT commit)
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tc_bwd_bits.npz")
DATASET = 10000
SHAPES = [(8, 8, 10, 0), (5, 7, 3, 0), (5, 7, 3, 2), (64, 64, 128, 0), (16, 64, 70, 0), (16, 64, 70, 32)]
# (Bl, Bt, D, row_offset, reduction (0: per-row upstream gradient, 2: one scalar, mean), coef_kl)
CASES = [(*s, red, ckl) for s in SHAPES for red in (0, 2) for ckl in (0.0, 0.5)]
COEF_TC = 1.5


def _id(c):
    return f"r{c[0]}-c{c[1]}-d{c[2]}-off{c[3]}-{'rows' if c[4] == 0 else 'bcast'}-kl{c[5]}"


def _hash(n, seed):
    """n floats in [-0.5, 0.5), multiples of 2^-24: integer arithmetic only."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 69069 + 12345)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    return ((h >> np.uint64(8)).astype(np.float64) * (1.0 / (1 << 24)) - 0.5).astype(np.float32)


def inputs(case):
    Bl, Bt, D, off, red, _ = case
    seed = 100 * Bl + Bt + D + off
    mu = (_hash(Bt * D, seed + 1) * 4.0).reshape(Bt, D)
    lv = (_hash(Bl * D, seed + 2) * 6.0 - 3.0).reshape(Bl, D)          # standard deviations 0.05 .. 1
    z = mu[off:off + Bl] + (_hash(Bl * D, seed + 3) * 4.0).reshape(Bl, D)
    g = _hash(Bl if red == 0 else 1, seed + 4) * 2.0 + 1.5
    return z.astype(np.float32), mu, lv, g


def clamp_count(z, mu, lv):
    """Number of (j, i, l) terms under the -50 clamp, in fp64; none within 1e-3 of it."""
    z, mu, lv = (a.astype(np.float64) for a in (z, mu, lv))
    vh = np.maximum(np.exp(lv), 1e-4)[:, None, :]
    d = z[:, None, :] - mu[None, :, :]
    lp = -(0.5 * (np.log(vh) + d * d / vh) + 0.5 * np.log(2.0 * np.pi))
    assert np.abs(lp + 50.0).min() > 1e-9             # the count does not hang on the last bits of exp / log
    return int((lp < -50.0).sum()), lp.size


def run(case):
    from hipvae import abi
    Bl, Bt, D, off, red, ckl = case
    dev = torch.device("cuda:0")
    z, mu, lv, g = (torch.from_numpy(a).to(dev) for a in inputs(case))
    out = torch.empty((Bl,) if red == 0 else (), device=dev)
    rows = torch.empty(Bl, device=dev) if red else None
    prodm, logqz = torch.empty(Bl, device=dev), torch.empty(Bl, device=dev)
    lse, sjoint = torch.empty(Bl, D, device=dev), torch.empty(Bl, Bt, device=dev)
    nws = abi.lib.itcv_tc_fwd_workspace(Bl, Bt, D)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device=dev)
    abi.call("itcv_tc_kl_fwd", abi.ptr(z), abi.ptr(mu), abi.ptr(lv), abi.ptr(out), abi.ptr(rows), abi.ptr(prodm),
             abi.ptr(logqz), abi.ptr(lse), abi.ptr(sjoint), Bl, Bt, off, D, DATASET, COEF_TC, ckl, red, abi.ptr(ws), nws,
             abi.stream())
    dz = torch.full((Bl, D), float("nan"), device=dev)
    dlv = torch.full((Bl, D), float("nan"), device=dev)
    dmu = torch.full((Bt, D), float("nan"), device=dev)
    nwb = abi.lib.itcv_tc_bwd_workspace(Bl, Bt)
    assert nwb == Bl * Bt * 4
    wq = torch.full((Bl, Bt), float("nan"), device=dev)
    abi.call("itcv_tc_kl_bwd", abi.ptr(g), abi.ptr(z), abi.ptr(mu), abi.ptr(lv), abi.ptr(logqz), abi.ptr(lse),
             abi.ptr(sjoint), abi.ptr(dz), abi.ptr(dmu), abi.ptr(dlv), Bl, Bt, off, D, DATASET, COEF_TC, ckl, red,
             abi.ptr(wq), nwb, abi.stream())
    torch.cuda.synchronize()
    return {"dz": dz, "dlogvar": dlv, "dmu_all": dmu, "wq": wq}


def _bytes(t):
    return t.contiguous().cpu().numpy().view(np.uint8).reshape(-1)


_golden = []


def golden():
    if not _golden:
        _golden.append(np.load(GOLDEN))
    return _golden[0]


def test_the_clamp_fires_in_every_case():
    for case in CASES[::4]:
        z, mu, lv, _ = inputs(case)
        n, total = clamp_count(z, mu, lv)
        assert 0.005 * total < n < 0.9 * total, (_id(case), n, total)
        assert n == int(golden()[f"{_id(case)}/clamped"]), _id(case)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_backward_bits(case):
    got = run(case)
    for key, val in got.items():
        assert torch.isfinite(val).all(), f"{_id(case)}: {key} was not written everywhere"
        want = golden()[f"{_id(case)}/{key}"]
        assert np.array_equal(_bytes(val), want), f"{_id(case)}: {key} differs from the recorded bytes"


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "intro-tc-vae_amd"))
    rec = {}
    for c in CASES:
        rec.update({f"{_id(c)}/{k}": _bytes(v) for k, v in run(c).items()})
        rec[f"{_id(c)}/clamped"] = np.int64(clamp_count(*inputs(c)[:3])[0])
    np.savez_compressed(sys.argv[1], **rec)
    print(f"recorded {len(CASES)} cases -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)")
