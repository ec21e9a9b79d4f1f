#!/usr/bin/env python3
"""Time of the nn.Linear GEMMs (itcv_linear_fwd / _dgrad / _wgrad) at the c2 fc shapes: the encoder's 8192 -> 256 and the
decoder's 128 -> 8192, at batch 64 and 128.  Per entry point 20 calls are captured into a graph; the graph is replayed 50
times between device events and the median replay is reported per call (us), with the bytes of the weight over that time.
ITCV_LIB selects the library (parent against new: run the tool twice).  GPU box only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import torch  # noqa: E402

from hipvae import abi  # noqa: E402

dev = torch.device("cuda:0")
CALLS, REPS = 20, 50


def timed(once):
    """Median us per call of ``once`` over REPS replays of a graph holding CALLS calls."""
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CALLS):
            once()
    for _ in range(3):
        graph.replay()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


g = torch.Generator().manual_seed(0)
for K, N in ((8192, 256), (128, 8192)):
    for B in (64, 128):
        x = torch.randn(B, K, generator=g).to(dev)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
        b = torch.randn(N, generator=g).to(dev)
        dy = torch.randn(B, N, generator=g).to(dev)
        y, dx, dw = torch.empty(B, N, device=dev), torch.empty(B, K, device=dev), torch.zeros(N, K, device=dev)
        nws = abi.lib.itcv_linear_workspace(B, K, N)
        ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device=dev)
        runs = {
            "fwd": lambda: abi.call("itcv_linear_fwd", abi.ptr(x), abi.ptr(w), abi.ptr(b), abi.ptr(y), B, K, N, abi.ptr(ws), nws,
                                    abi.stream()),
            "dgrad": lambda: abi.call("itcv_linear_dgrad", abi.ptr(dy), abi.ptr(w), abi.ptr(dx), B, K, N, abi.ptr(ws), nws,
                                      abi.stream()),
            "wgrad": lambda: abi.call("itcv_linear_wgrad", abi.ptr(dy), abi.ptr(x), abi.ptr(dw), B, K, N, 1, abi.ptr(ws), nws,
                                      abi.stream()),
        }
        for name, once in runs.items():
            med, best = timed(once)
            print(f"linear {name:5s} K {K:5d} N {N:5d} B {B:4d}: {med:7.2f} us per call (median of {REPS}; min {best:7.2f}), "
                  f"weight {N * K * 4 / 1e6:5.2f} MB -> {N * K * 4 / 1e6 / med:5.2f} TB/s", flush=True)
