#!/usr/bin/env python3
"""Time of the importance-weighted objective (solvers/iwae.py, csrc/iwae.hip).

1. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512)) as hipGraph
   replays in the f16x3 arithmetic: IWAESolver with B = 16 images and K = 8 samples (every estimator) next to VAESolver at
   batch 128 -- the same K B = 128 decoder rows, eight times the encoder rows.  After the capture, a host clock around
   ``--steps`` replayed steps, each of which ends in its one host read-back; the median and the range of ``--reps`` legs.
2. us of the bound alone, forward + backward from (mu, logvar, recon) to their gradients, at (B, K, D, P) = (16, 8, 128,
   12288) and (64, 64, 128, 12288), from HIP events around ``--calls`` calls after a warm-up: ``ops.iwae_sample`` +
   ``ops.iwae_bound`` against the same arithmetic in torch on the device, ``x.repeat`` included (what a user had to write
   before); the median of ``--reps`` legs.
3. The broadcast rows kernels alone at (B, K, P) = (64, 128, 12288) -- 403 MB of reconstructions, more than the 256 MiB
   last-level cache holds -- from HIP events around ``--calls`` calls: the bytes the algorithm needs (forward: K B P + B P
   floats read; backward: the same read and K B P written) over the time, against the 8 TB/s this project takes as HBM
   peak.  The time is that of the op's launches back to back (forward: two), not of one kernel in a trace.

Prints one line per figure and, last, all of them as one JSON line."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402
import ops  # noqa: E402
from hipvae import functional as HF  # noqa: E402
from solvers.iwae import IWAESolver  # noqa: E402
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
HBM_PEAK = 8.0e12


class DS:
    def __len__(self):
        return 10000


def make(cls, batch, **kw):
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
    return cls(DS(), model, batch, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), "mse", 0.5, 0.75, dev, True, None, clip=100.0, **kw)


def step_ms(solver, rows, steps, reps):
    """(median, min, max) ms per step over ``reps`` legs of ``steps`` replayed steps on ``rows`` images."""
    assert solver.conv_math == "f16x3"
    g = torch.Generator().manual_seed(1000)
    batches = [torch.rand(rows, 3, 64, 64, generator=g).to(dev) for _ in range(4)]
    solver.enable_graph()
    for i in range(6):                          # 3 eager warm-ups, capture + first replay, two more replays
        solver.train_step(batches[i % 4], i)
    assert solver._graph is not None and len(solver._graphs) == 1
    legs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            solver.train_step(batches[i % 4], i)
        torch.cuda.synchronize()
        legs.append((time.perf_counter() - t0) * 1e3 / steps)
    assert len(solver._graphs) == 1
    return float(np.median(legs)), min(legs), max(legs)


def event_us(once, calls, reps, warm=10):
    """Median us of ``once()`` from HIP events around ``calls`` calls."""
    for _ in range(warm):
        once()
    legs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            once()
        b.record()
        torch.cuda.synchronize()
        legs.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(legs))


def torch_bound(mu, logvar, eps, x, recon, K, beta_rec, beta_kl):
    """The bound as a user writes it with torch arithmetic on the device."""
    z = mu.repeat(K, 1) + torch.exp(0.5 * logvar).repeat(K, 1) * eps
    lat = 0.5 * (z * z - eps * eps - logvar.repeat(K, 1)).sum(1)
    rows = ((recon - x.repeat(K, 1)) ** 2).sum(1)
    logw = -(beta_rec * rows + beta_kl * lat).reshape(K, -1)
    return -(torch.logsumexp(logw, 0) - math.log(K)).mean(), z


def bound_us(B, K, D, P, calls, reps):
    g = torch.Generator().manual_seed(7)
    mu = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    logvar = (torch.randn(B, D, generator=g) * 0.5 - 1.0).to(dev).requires_grad_(True)
    eps = torch.randn(K * B, D, generator=g).to(dev)
    x = torch.rand(B, P, generator=g).to(dev)
    recon = torch.rand(K * B, P, generator=g).to(dev).requires_grad_(True)
    dz = torch.randn(K * B, D, generator=g).to(dev)

    def fused():
        sample = ops.iwae_sample(mu, logvar, K, eps=eps)
        loss = ops.iwae_bound(x, recon, sample, 0.75, 0.5, "mse", "dreg")
        torch.autograd.grad(loss + (sample.z * dz).sum(), (mu, logvar, recon))

    def plain():
        loss, z = torch_bound(mu, logvar, eps, x, recon, K, 0.75, 0.5)
        torch.autograd.grad(loss + (z * dz).sum(), (mu, logvar, recon))

    return event_us(fused, calls, reps), event_us(plain, calls, reps)


def rows_rates(B, K, P, calls, reps):
    g = torch.Generator().manual_seed(9)
    x = torch.rand(B, P, generator=g).to(dev)
    recon = torch.rand(K * B, P, device=dev)
    grow = torch.randn(K * B, device=dev)
    out = torch.empty_like(recon)
    rows = torch.empty(K * B, device=dev)
    nws = HF.lib.itcv_iwae_rows_workspace(B, K, P)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    st = HF.stream()
    fwd = event_us(lambda: HF.call("itcv_iwae_rows_fwd", x.data_ptr(), recon.data_ptr(), rows.data_ptr(), B, K, P, 0,
                                   ws.data_ptr(), nws, st), calls, reps)
    bwd = event_us(lambda: HF.call("itcv_iwae_rows_bwd", x.data_ptr(), recon.data_ptr(), grow.data_ptr(), out.data_ptr(), B,
                                   K, P, 0, st), calls, reps)
    fbytes, bbytes = 4.0 * (K * B * P + B * P), 4.0 * (2 * K * B * P + B * P)
    return dict(fwd_us=round(fwd, 2), fwd_bytes_per_s=fbytes / (fwd * 1e-6), fwd_share_of_peak=fbytes / (fwd * 1e-6) / HBM_PEAK,
                bwd_us=round(bwd, 2), bwd_bytes_per_s=bbytes / (bwd * 1e-6), bwd_share_of_peak=bbytes / (bwd * 1e-6) / HBM_PEAK)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "step", "bound", "rows"), default="all")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if args.only in ("all", "step"):
        legs = [("VAESolver b128", lambda: make(VAESolver, 128), 128)]
        legs += [(f"IWAESolver 16x8 {e}", lambda e=e: make(IWAESolver, 16, num_samples=8, estimator=e), 16)
                 for e in ops.IWAE_ESTIMATORS]
        for name, build, rows in legs:
            med, lo, hi = step_ms(build(), rows, args.steps, args.reps)
            out["step_ms " + name] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
            print(f"c2 step, graph, f16x3  {name:<21} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    if args.only in ("all", "bound"):
        for B, K, D, P in ((16, 8, 128, 12288), (64, 64, 128, 12288)):
            fused, plain = bound_us(B, K, D, P, args.calls, args.reps)
            out[f"bound_us ({B},{K},{D},{P})"] = dict(fused=round(fused, 2), torch=round(plain, 2))
            print(f"bound fwd+bwd ({B:>2}, {K:>2}, {D}, {P})  fused {fused:9.2f} us   torch arithmetic {plain:9.2f} us",
                  flush=True)
    if args.only in ("all", "rows"):
        r = rows_rates(64, 128, 12288, args.calls, args.reps)
        out["rows (64,128,12288)"] = r
        print(f"broadcast rows (64, 128, 12288)  fwd {r['fwd_us']:.1f} us = {r['fwd_bytes_per_s'] / 1e12:.2f} TB/s "
              f"({100 * r['fwd_share_of_peak']:.0f} % of 8 TB/s)   bwd {r['bwd_us']:.1f} us = "
              f"{r['bwd_bytes_per_s'] / 1e12:.2f} TB/s ({100 * r['bwd_share_of_peak']:.0f} % of 8 TB/s)", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
