"""Micro-benchmark of the deferred weight-gradient slab fold (itcv_wgrad_reduce_many) on the c2 layer shapes: the slabs of one
backward pass are produced by the real weight-gradient kernels (random planes), the fold is timed alone with HIP events,
launched back to back.  Measured while the fold was rebuilt in round 3 (c2 shapes, 282 MB of slabs): 64 elements x 9 taps
per block with an LDS exchange 140-156 us whatever the tiling / persistence / plane padding; 4 elements x 9 taps per
thread without LDS 84 us (fine tiles for >= 64 slices; 157 us without them; 126 / 195 us with fine tiles from 16 / 8
slices).

Two conditions are timed.  WARM: the fold launched 20 times back to back, as above.  COLD, towards the step's condition: the
slabs are written by the real weight-gradient kernels, then 768 MB of unrelated traffic goes through the caches (a 384-MB
copy), then ONE fold is timed; median of 50.  In the c2 step the fold runs behind a whole backward and costs about twice
its warm time, so a change is judged by the cold figure before the warm one.  Round 7 (four fine tile numbers per block,
float4 loads, items dealt heaviest first): warm 85.4 -> 65.8 us, cold 99.2 -> 93.6 us, in the step 164 -> 145 us per launch
-- the cold condition does not reproduce all of what the step adds.  ITCV_LIB selects the library
(parent against new: run the tool twice).  GPU box only."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "intro-tc-vae_amd"))
from hipvae import functional as HF  # noqa: E402

dev = torch.device("cuda:0")
HF.set_conv_math("f16x3")
# (B, Ci, H, W, Co, up2) of the encoder's 3x3 convs at c2 (batched passes: B = 128) and the decoder's
LAYERS = [(128, 64, 32, 32, 128, 0), (128, 128, 16, 16, 256, 0), (128, 256, 8, 8, 512, 0), (128, 512, 4, 4, 512, 0),
          (128, 512, 8, 8, 512, 1), (128, 512, 16, 16, 256, 1), (128, 256, 32, 32, 128, 1), (128, 128, 64, 64, 64, 1),
          (128, 64, 64, 64, 64, 0), (128, 64, 64, 64, 64, 0)]
g = torch.Generator().manual_seed(0)
ops = []
for (B, Ci, H, W, Co, up2) in LAYERS:
    Hs, Ws = (H // 2, W // 2) if up2 else (H, W)
    x = torch.randn(B, Ci, Hs, Ws, generator=g).to(dev)
    dy = (torch.randn(B, Co, H, W, generator=g) * 1e-3).to(dev)
    xp, dyp = HF.split_planes(x, 4), HF.split_planes(dy, 4, gradient=True)
    dw = torch.zeros(Co, Ci, 3, 3, device=dev)
    ops.append((xp, dyp, B, Ci, H, W, Co, up2, dw))


def run():
    """Slabs of one backward, then the fold launched 20 times back to back between two events (the Python side of
    flush_wgrad_reduces takes longer than the kernel: timing one call would time the host)."""
    from hipvae.abi import call, ptr, stream
    with HF.deferred_wgrad_reduces():
        for (xp, dyp, B, Ci, H, W, Co, up2, dw) in ops:
            HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, out=dw, accumulate=True, ns=4)
        nbytes = sum(p[0].numel() for p in HF._DEFER["pending"])
        HF.flush_wgrad_reduces()
    (tab,) = HF._DEFER["tables"].values()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call("itcv_wgrad_reduce_many", ptr(tab[0]), tab[1], tab[2], stream())
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / 20, nbytes


def run_cold(reps=50):
    """Median us of one fold whose slabs were just written by the weight-gradient kernels and then pushed out of the caches."""
    from hipvae.abi import call, ptr, stream
    (tab,) = HF._DEFER["tables"].values()                 # run() left the table of this sequence of slab buffers
    junk = torch.empty(2, 96 << 20, device=dev)          # 2 x 384 MB
    ts = []
    for _ in range(reps):
        HF._DEFER["on"] = True
        try:
            for (xp, dyp, B, Ci, H, W, Co, up2, dw) in ops:
                HF.conv_wgrad_planes(xp, dyp, B, Ci, H, W, Co, 3, up2, out=dw, accumulate=True, ns=4)
        finally:
            HF._DEFER["on"] = False
        HF._DEFER["pending"].clear()                      # same pooled buffers as the table's: folded by hand below
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        junk[1].copy_(junk[0])                            # also keeps the device busy while the host enqueues what follows
        e0.record()
        call("itcv_wgrad_reduce_many", ptr(tab[0]), tab[1], tab[2], stream())
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


ts = []
for _ in range(4):
    HF._DEFER["tables"].clear()
    t, nbytes = run()
    ts.append(t)
print(f"warm fold {min(ts[1:]):7.1f} us (median {sorted(ts[1:])[1]:7.1f}), slabs {nbytes / 1e6:6.1f} MB -> {nbytes / 1e6 / min(ts[1:]):5.2f} TB/s of slab reads",
      flush=True)
cold, cold_min = run_cold()
print(f"cold fold {cold:7.1f} us median of 50 (min {cold_min:7.1f}) -> {nbytes / 1e6 / cold:5.2f} TB/s of slab reads", flush=True)
