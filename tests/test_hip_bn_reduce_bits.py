"""GPU: the BatchNorm reduce passes (``bn_moments_partial``, ``bn_bwd_partial_v4``) give the bits they gave at the commit
before the backward kernel got its live-range instantiation and its full / ragged trips.
tests/golden/bn_reduce_bits.npz was recorded from a build of that commit; every comparison is an equality of bytes
(``torch.equal`` on uint8 views, so -0.0 and +0.0 differ), with no tolerance.

Per case ``itcv_bn_train_fwd`` / ``itcv_bn_train_bwd`` / ``itcv_bn_train_bwd_live`` run through ``hipvae.abi`` on inputs
that are exact integer hashes (the same floats on any device), and these are compared: forward -- mean, rstd,
running_mean, running_var, num_batches_tracked, the fp16 scale record and the first 4096 bytes of each plane; backward --
dsums (fp64), dgamma / dbeta without and with ``accumulate``, the fp16 scale record and the first 4096 bytes of each
plane.  With a live range whose first group is dead, the window starts at the first live group (the plane's own first
4096 bytes must still hold the fill: nothing is stored there), a dead group's sums are +0.0, and the scale record is
also compared with that of the full call on a dy whose dead groups are zero.

Shapes: the smallest at which the trip loop can go wrong -- no, one and two trips of 4096 values per block, each with a
ragged last trip; the path of every shape is pinned with ``abi.bn_plan_query``:

* one block per channel: C = 256 with 2x64x64 (8192 values: 2 trips), 9x24x20 (4320: 2 trips, tail 224, width no power
  of two), and 3 x 40 x 6x12 (216: less than one trip);
* sliced, folded by the apply pass: 17 x 64 x 64x64 (chunk 4352: one full trip and a tail of 256) and 16 x 64 x 32x32
  (chunk 1024: under one trip); sliced with a combine launch: 6 x 24 x 12x20.

Modes plain / pool / up2, skip tensor on and off, plane formats 2 and 4, groups 1, 2 and 3, live ranges {all},
{first of 2}, {last of 2}, {middle of 3}: a rotation over the shapes in which every instantiation of the backward kernel
(mode x one-block / sliced x maxima x live range) runs, checked by ``test_every_kernel_form_has_a_case``.

    python tests/test_hip_bn_reduce_bits.py OUT.npz        # re-record (on a GPU, from a build of the PARENT commit)
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bn_reduce_bits.npz")
F16 = 4
SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1
WINDOW = 4096            # bytes compared per plane
FILL = 0x7fc07fc0        # planes are filled with this before the call

# (id, B per group, C, H, W, path)
SHAPES = [
    ("ob-2trips", 2, 256, 64, 64, "OneBlock"),
    ("ob-tail224", 9, 256, 24, 20, "OneBlock"),
    ("ob-short", 3, 40, 6, 12, "OneBlock"),
    ("fold-trip-tail", 17, 64, 64, 64, "SlicedFold"),
    ("fold-short", 16, 64, 32, 32, "SlicedFold"),
    ("combine", 6, 24, 12, 20, "SlicedCombine"),
]
MODES = ("plain", "pool", "up2")
# name -> (groups, live0, nlive)
CONFIGS = {"g1": (1, 0, 1), "g2": (2, 0, 2), "g3": (3, 0, 3), "g2-first": (2, 0, 1), "g2-last": (2, 1, 1),
           "g3-mid": (3, 1, 1)}
_FULL, _LIVE = ("g1", "g2"), ("g2-first", "g2-last", "g3-mid")


def _bwd_cases():
    cases = []
    for j, shape in enumerate(SHAPES):
        jc = j % 3                                   # position inside the one-block / sliced class
        for mode in range(3):
            for ni, ns in enumerate((2, F16)):
                r = (jc + mode + ni) % 3             # per (class, mode, format): one full call, two live ranges
                cfg = _FULL[(j + mode) % 2] if r == 0 else (_LIVE[(mode + ni) % 2] if r == 1 else "g3-mid")
                cases.append((shape, mode, ns, bool((jc + ni + (mode > 0)) % 2), cfg))
    # the production form (plain, fp16 planes) under every group configuration, at the two shapes with a full trip
    for shape in (SHAPES[0], SHAPES[3]):
        for cfg in CONFIGS:
            if not any(c[0] is shape and c[1] == 0 and c[2] == F16 and c[4] == cfg for c in cases):
                cases.append((shape, 0, F16, False, cfg))
    # one pool case with a live range at the shape the encoder's pool layers look like
    cases.append((SHAPES[3], 1, F16, False, "g2-last"))
    seen, out = set(), []
    for c in cases:
        if _bwd_id(c) not in seen:
            seen.add(_bwd_id(c))
            out.append(c)
    return out


def _bwd_id(c):
    return f"bwd-{c[0][0]}-{MODES[c[1]]}-ns{c[2]}-{'skip' if c[3] else 'noskip'}-{c[4]}"


def _fwd_cases():
    cases = []
    for j, shape in enumerate(SHAPES):
        jc = j % 3
        for pool in (0, 1):
            for ni, ns in enumerate((2, F16)):
                cases.append((shape, pool, ns, bool((j + pool + ni) % 2), 1 + (jc + pool + ni) % 3))
    return cases


def _fwd_id(c):
    return f"fwd-{c[0][0]}-{'pool' if c[1] else 'plain'}-ns{c[2]}-{'skip' if c[3] else 'noskip'}-g{c[4]}"


BWD_CASES, FWD_CASES = _bwd_cases(), _fwd_cases()


def dev():
    return torch.device("cuda:0")


def _hash(n, seed):
    """n floats in [-0.5, 0.5) on the device, multiples of 2^-24: integer arithmetic only, the same on every device."""
    h = (torch.arange(n, dtype=torch.int64, device=dev()) * 40503 + seed * 69069 + 12345) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x45D9F3B) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 0x45D9F3B) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    return (h >> 8).to(torch.float32) * (1.0 / (1 << 24)) - 0.5


def _bytes(t):
    return t.contiguous().view(torch.uint8).reshape(-1)


def _plane_windows(planes, ns, pstride, first_chunk):
    """The first WINDOW bytes of each plane from chunk `first_chunk` on, and the fp16 scale record (else empty)."""
    raw = _bytes(planes)
    nplanes = 3 if ns == 3 else 2
    wins = [raw[(p * pstride + first_chunk) * 16:(p * pstride + first_chunk) * 16 + WINDOW] for p in range(nplanes)]
    assert all(w.numel() == WINDOW for w in wins)
    return torch.cat(wins), raw[nplanes * pstride * 16:]


def run_fwd(case):
    from hipvae import abi
    (name, B, C, H, W, path), pool, ns, with_skip, G = case
    assert abi.bn_plan_query(False, B, C, H, W, pool=pool, groups=G, planes=True, ns=ns)[0] == path, name
    n, HWo = G * B * C * H * W, (H * W) // (4 if pool else 1)
    x = _hash(n, 1) * 3.0 + 0.5
    skip = _hash(n, 2) if with_skip else None
    gamma, beta = _hash(C, 3) + 1.0, _hash(C, 4) * 0.2
    rm, rv = _hash(C, 5), _hash(C, 6) * 0.5 + 1.0
    nbt = torch.zeros(1, dtype=torch.int64, device=dev())
    mean = torch.full((G, C), float("nan"), device=dev())
    rstd = torch.full((G, C), float("nan"), device=dev())
    nws = abi.lib.itcv_bn_workspace(B, C, H * W) * G
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device=dev())
    planes = torch.full((abi.lib.itcv_planes_bytes(G * B, C, HWo, ns) // 4,), FILL, dtype=torch.int32, device=dev())
    pstride = G * B * (C // 8) * HWo
    abi.call("itcv_bn_train_fwd", abi.ptr(x), abi.ptr(gamma), abi.ptr(beta), abi.ptr(skip), None, abi.ptr(planes), ns, B, C, H,
             W, SLOPE, pool, EPS, MOMENTUM, abi.ptr(rm), abi.ptr(rv), abi.ptr(nbt), abi.ptr(mean), abi.ptr(rstd), abi.ptr(ws),
             nws, pstride, None, 0, 0, G, abi.stream())
    torch.cuda.synchronize()
    win, rec = _plane_windows(planes, ns, pstride, 0)
    return {"mean": _bytes(mean), "rstd": _bytes(rstd), "running_mean": _bytes(rm), "running_var": _bytes(rv),
            "nbt": _bytes(nbt), "planes": win, "record": rec}


def _bwd_call(case, x, dy, skip, mean, rstd, gamma, beta, dgamma, dbeta, accumulate, live):
    """One backward call (`live` None: itcv_bn_train_bwd) -> (dsums, planes, plane stride)."""
    from hipvae import abi
    (name, B, C, H, W, path), mode, ns, _, cfg = case
    G = CONFIGS[cfg][0]
    dsums = torch.full((G, 2 * C), 7.0, dtype=torch.float64, device=dev())
    nws = abi.lib.itcv_bn_workspace(B, C, H * W) * G
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device=dev())
    planes = torch.full((abi.lib.itcv_planes_bytes(G * B, C, H * W, ns) // 4,), FILL, dtype=torch.int32, device=dev())
    pstride = G * B * (C // 8) * H * W
    head = (abi.ptr(x), abi.ptr(dy), abi.ptr(mean), abi.ptr(rstd), abi.ptr(gamma), abi.ptr(beta), abi.ptr(skip), abi.ptr(dsums),
            None, None, abi.ptr(planes), ns, abi.ptr(dgamma), abi.ptr(dbeta), accumulate, B, C, H, W, SLOPE, int(mode == 1),
            int(mode == 2), abi.ptr(ws), nws, pstride, G)
    if live is None:
        abi.call("itcv_bn_train_bwd", *head, abi.stream())
    else:
        abi.call("itcv_bn_train_bwd_live", *head, live[0], live[1], abi.stream())
    torch.cuda.synchronize()
    return dsums, planes, pstride


def run_bwd(case):
    from hipvae import abi
    (name, B, C, H, W, path), mode, ns, with_skip, cfg = case
    G, live0, nlive = CONFIGS[cfg]
    assert abi.bn_plan_query(True, B, C, H, W, pool=int(mode == 1), up2=int(mode == 2), groups=G, planes=True,
                             ns=ns)[0] == path, name
    n = G * B * C * H * W
    Hy, Wy = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[mode]
    x = (_hash(n, 11) * 3.0 + 0.5).view(G * B, C, H, W)
    dy = (_hash(G * B * C * Hy * Wy, 12) * 2.0).view(G * B, C, Hy, Wy)
    skip = _hash(n, 13) if with_skip else None
    mean, rstd = (_hash(G * C, 14) * 0.25 + 0.5).view(G, C), (_hash(G * C, 15) * 0.5 + 1.0).view(G, C)
    gamma, beta = _hash(C, 16) + 1.0, _hash(C, 17) * 0.2
    live = None if nlive == G else (live0, nlive)
    args = (x, dy, skip, mean, rstd, gamma, beta)
    dgamma = torch.full((C,), float("nan"), device=dev())
    dbeta = torch.full((C,), float("nan"), device=dev())
    dsums, planes, pstride = _bwd_call(case, *args, dgamma, dbeta, 0, live)
    dgamma_acc, dbeta_acc = _hash(C, 18), _hash(C, 19)
    dsums_acc, _, _ = _bwd_call(case, *args, dgamma_acc, dbeta_acc, 1, live)
    assert torch.equal(_bytes(dsums_acc), _bytes(dsums))
    group_chunks = B * (C // 8) * H * W
    win, rec = _plane_windows(planes, ns, pstride, live0 * group_chunks)
    if live is not None:
        dead = [g for g in range(G) if not live0 <= g < live0 + nlive]
        plus_zero = torch.zeros(2 * C, dtype=torch.float64, device=dev())
        for g in dead:
            assert torch.equal(_bytes(dsums[g]), _bytes(plus_zero)), "a dead group's sums are not +0.0"
        if live0 > 0:
            first, _ = _plane_windows(planes, ns, pstride, 0)
            assert bool((first.view(torch.int32) == FILL).all()), "a dead group's planes were written"
        zdy = dy.clone()
        for g in dead:
            zdy[g * B:(g + 1) * B] = 0.0
        full = _bwd_call(case, x, zdy, *args[2:], torch.zeros_like(dgamma), torch.zeros_like(dbeta), 0, None)
        assert torch.equal(_plane_windows(full[1], ns, pstride, 0)[1], rec), "scale record differs from the full call's"
    return {"dsums": _bytes(dsums), "dgamma": _bytes(dgamma), "dbeta": _bytes(dbeta), "dgamma_acc": _bytes(dgamma_acc),
            "dbeta_acc": _bytes(dbeta_acc), "planes": win, "record": rec}


_golden = []


def golden():
    if not _golden:
        _golden.append(np.load(GOLDEN))
    return _golden[0]


def _compare(cid, got):
    g = golden()
    for key, val in got.items():
        want = torch.from_numpy(g[f"{cid}/{key}"])
        assert torch.equal(val.cpu(), want), f"{cid}: {key} differs from the recorded bytes"


def test_every_kernel_form_has_a_case():
    """mode x (one block | sliced) x maxima x live range of bn_bwd_partial_v4, both skip settings per mode and class; groups
    1, 2, 3 and both plane formats of the forward per class and pool setting."""
    forms = {(c[1], c[0][5] == "OneBlock", c[2] == F16, CONFIGS[c[4]][2] != CONFIGS[c[4]][0]) for c in BWD_CASES}
    assert len(forms) == 3 * 2 * 2 * 2
    assert {(c[1], c[0][5] == "OneBlock", c[3]) for c in BWD_CASES} == {(m, o, s) for m in range(3) for o in (False, True)
                                                                         for s in (False, True)}
    assert {c[4] for c in BWD_CASES} == set(CONFIGS)
    assert {(c[0][5] == "OneBlock", c[1], c[2], c[4]) for c in FWD_CASES} == {(o, p, n, g) for o in (False, True) for p in (0, 1)
                                                                             for n in (2, F16) for g in (1, 2, 3)}
    assert {(c[0][5] == "OneBlock", c[3]) for c in FWD_CASES} == {(o, s) for o in (False, True) for s in (False, True)}


@pytest.mark.parametrize("case", FWD_CASES, ids=[_fwd_id(c) for c in FWD_CASES])
def test_forward_statistics_bits(case):
    _compare(_fwd_id(case), run_fwd(case))


@pytest.mark.parametrize("case", BWD_CASES, ids=[_bwd_id(c) for c in BWD_CASES])
def test_backward_sums_bits(case):
    _compare(_bwd_id(case), run_bwd(case))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "intro-tc-vae_amd"))
    out = {}
    for c in FWD_CASES:
        out.update({f"{_fwd_id(c)}/{k}": v.cpu().numpy() for k, v in run_fwd(c).items()})
    for c in BWD_CASES:
        out.update({f"{_bwd_id(c)}/{k}": v.cpu().numpy() for k, v in run_bwd(c).items()})
    np.savez_compressed(sys.argv[1], **out)
    print(f"recorded {len(FWD_CASES)} forward and {len(BWD_CASES)} backward cases -> {sys.argv[1]} "
          f"({os.path.getsize(sys.argv[1])} bytes)")
