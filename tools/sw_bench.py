#!/usr/bin/env python3
"""Time of the sliced-Wasserstein objective and score (solvers/swae.py, csrc/sw.hip, hipvae/quality.py).

1. us of the KL hook alone, forward + backward, at (Bt, D, L) = (64, 128, 50) and (512, 128, 50), from HIP events around
   ``--calls`` calls after a warm-up, for ``ops.sw_kl_loss``, for the same hook in torch arithmetic (what a user had to
   write before: ``matmul`` + ``torch.sort`` + autograd, fp32) and for ``ops.mmd_kl_loss`` ("imq") on the same batch; the
   median of ``--reps`` such legs.
2. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512), 64 images) as
   hipGraph replays in the f16x3 arithmetic, for VAESolver, SWAESolver and MMDSolver, all in this one run, the VAE step
   first and again last (the base of the comparison, and its drift over the run): after the capture, a host clock
   around ``--steps`` replayed steps, each of which ends in its one host read-back; the median and the range of
   ``--reps`` such legs.
3. ms of the score ``quality.sliced_wasserstein_distance`` at N = 10000, D = 128, L = 1024 (its one read-back included),
   against the same in torch arithmetic (fp32 ``matmul`` + ``torch.sort``), a host clock around ``--score-calls`` calls.

Prints one line per figure and, last, all of them as one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402
import ops  # noqa: E402
from hipvae import quality  # noqa: E402
from solvers.mmd import MMDSolver  # noqa: E402
from solvers.swae import SWAESolver  # noqa: E402
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
BATCH = 64


class DS:
    def __len__(self):
        return 10000


def make(cls, **kw):
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
    return cls(DS(), model, BATCH, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), "mse", 0.5, 0.75, dev, True, None, clip=100.0, **kw)


def step_ms(solver, steps, reps):
    """(median, min, max) ms per step over ``reps`` legs of ``steps`` replayed steps."""
    assert solver.conv_math == "f16x3"
    g = torch.Generator().manual_seed(1000)
    batches = [torch.rand(BATCH, 3, 64, 64, generator=g).to(dev) for _ in range(4)]
    solver.enable_graph()
    for i in range(6):                          # 3 eager warm-ups, capture + first replay, two more replays
        solver.train_step(batches[i % 4], i)
    assert solver._graph is not None
    legs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            solver.train_step(batches[i % 4], i)
        torch.cuda.synchronize()
        legs.append((time.perf_counter() - t0) * 1e3 / steps)
    return float(np.median(legs)), min(legs), max(legs)


def torch_sw2(a, b, t):
    """SW^2 as a user writes it with torch arithmetic."""
    theta = t / t.norm(dim=1, keepdim=True)
    u, _ = torch.sort(a @ theta.t(), dim=0)
    v, _ = torch.sort(b @ theta.t(), dim=0)
    return ((u - v) ** 2).mean()


def torch_hook(z, prior, t, mu, logvar, lam, beta):
    return beta * (-0.5 * (1.0 + logvar - mu * mu - logvar.exp()).sum(1)).mean() + lam * torch_sw2(z, prior, t)


def hook_us(fn, Bt, D, L, calls, reps):
    """Median us of one forward + backward of ``fn(z, prior, t, mu, logvar)`` from HIP events around ``calls`` calls."""
    g = torch.Generator().manual_seed(7)
    z = (1.2 * torch.randn(Bt, D, generator=g) + 0.3).to(dev).requires_grad_(True)
    mu = torch.randn(Bt, D, generator=g).to(dev).requires_grad_(True)
    lv = (0.5 * torch.randn(Bt, D, generator=g) - 1.5).to(dev).requires_grad_(True)
    prior, t = torch.randn(Bt, D, generator=g).to(dev), torch.randn(L, D, generator=g).to(dev)

    def once():
        z.grad = mu.grad = lv.grad = None
        fn(z, prior, t, mu, lv).backward()

    for _ in range(20):
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


def score_ms(fn, calls, reps):
    fn()
    legs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        legs.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(legs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--score-calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the hook and the score alone")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for Bt, D, L in ((64, 128, 50), (512, 128, 50)):
        fused = hook_us(lambda z, p, t, m, v: ops.sw_kl_loss(z, m, v, p, t, 0.5, 10.0), Bt, D, L, args.calls, args.reps)
        plain = hook_us(lambda z, p, t, m, v: torch_hook(z, p, t, m, v, 10.0, 0.5), Bt, D, L, args.calls, args.reps)
        mmd = hook_us(lambda z, p, t, m, v: ops.mmd_kl_loss(z, m, v, p, 0.5, 10.0, "imq"), Bt, D, L, args.calls, args.reps)
        out[f"hook_us ({Bt},{D},{L})"] = dict(fused=round(fused, 2), torch=round(plain, 2), mmd_imq=round(mmd, 2))
        print(f"hook fwd+bwd ({Bt:>3}, {D}, L={L})  fused {fused:8.2f} us   torch arithmetic {plain:8.2f} us   "
              f"MMD hook (imq) {mmd:8.2f} us", flush=True)
    if not args.no_steps:
        for name, build in (("VAESolver", lambda: make(VAESolver)), ("SWAESolver", lambda: make(SWAESolver)),
                            ("MMDSolver imq", lambda: make(MMDSolver, mmd_kernel="imq")),
                            ("VAESolver again", lambda: make(VAESolver))):
            med, lo, hi = step_ms(build(), args.steps, args.reps)
            out["step_ms " + name] = round(med, 4)
            print(f"c2 step, graph, f16x3  {name:<15} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    g = torch.Generator().manual_seed(3)
    N, D, L = 10000, 128, 1024
    real, fake = (1.2 * torch.randn(N, D, generator=g) + 0.3).to(dev), torch.randn(N, D, generator=g).to(dev)
    t = quality.sliced_wasserstein_directions(L, D, 0).to(dev)
    fused = score_ms(lambda: quality.sliced_wasserstein_distance(real, fake, L, 0)["sw2"], args.score_calls, args.reps)
    plain = score_ms(lambda: float(torch_sw2(real, fake, t)), args.score_calls, args.reps)
    a, b = quality.sliced_wasserstein_distance(real, fake, L, 0)["sw2"], float(torch_sw2(real, fake, t))
    out[f"score_ms ({N},{D},L={L})"] = dict(fused=round(fused, 3), torch=round(plain, 3), sw2=a, sw2_torch_fp32=b)
    print(f"score ({N}, {D}, L={L})  fused {fused:8.3f} ms   torch arithmetic {plain:8.3f} ms   (SW^2 {a:.6f} / {b:.6f})",
          flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
