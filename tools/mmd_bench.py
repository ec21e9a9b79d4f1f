#!/usr/bin/env python3
"""Time of the MMD objective (solvers/mmd.py, csrc/mmd.hip).

1. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512), 64 images) as
   hipGraph replays in the f16x3 arithmetic, for VAESolver, DIPSolver ("i"), TCSovler and MMDSolver ("imq" and "rbf"), all
   in this one run, the VAE step first and again last (the base of the comparison, and its drift over the run): after
   the capture, a host clock around ``--steps`` replayed steps, each of which ends in its one host read-back; the median
   and the range of ``--reps`` such legs.
2. us of the KL hook alone, forward + backward, at (Bt, P, D) = (64, 64, 128) and (512, 512, 128), from HIP events around
   ``--calls`` calls after a warm-up, for ``ops.mmd_kl_loss`` and for the same hook in torch arithmetic (what a user had
   to write before: about twenty at:: launches, the fp32 difference form through a [Bt, P, D] tensor), both kernels; the
   median of ``--reps`` such legs.

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
from solvers.dip import DIPSolver  # noqa: E402
from solvers.mmd import MMDSolver  # noqa: E402
from solvers.tc import TCSovler  # noqa: E402
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
BATCH = 64
SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


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


def torch_hook(z, prior, mu, logvar, kernel, lam, beta):
    """The hook as a user overrides it with torch arithmetic."""
    h = 2.0 * z.shape[1]

    def ker(a, b):
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
        if kernel == "rbf":
            return torch.exp(-d2 / h)
        return sum((s * h) / (s * h + d2) for s in SCALES)

    Bt, P = z.shape[0], prior.shape[0]
    kzz, kpp, kzp = ker(z, z), ker(prior, prior), ker(z, prior)
    mmd2 = (kzz.sum() - torch.diagonal(kzz).sum()) / (Bt * (Bt - 1)) + \
        (kpp.sum() - torch.diagonal(kpp).sum()) / (P * (P - 1)) - 2.0 * kzp.sum() / (Bt * P)
    return beta * (-0.5 * (1.0 + logvar - mu * mu - logvar.exp()).sum(1)).mean() + lam * mmd2


def hook_us(fn, Bt, P, D, calls, reps):
    """Median us of one forward + backward of ``fn(z, prior, mu, logvar)`` from HIP events around ``calls`` calls."""
    g = torch.Generator().manual_seed(7)
    z = (1.2 * torch.randn(Bt, D, generator=g) + 0.3).to(dev).requires_grad_(True)
    mu = torch.randn(Bt, D, generator=g).to(dev).requires_grad_(True)
    lv = (0.5 * torch.randn(Bt, D, generator=g) - 1.5).to(dev).requires_grad_(True)
    prior = torch.randn(P, D, generator=g).to(dev)

    def once():
        z.grad = mu.grad = lv.grad = None
        fn(z, prior, mu, lv).backward()

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the hook alone")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if not args.no_steps:
        for name, build in (("VAESolver", lambda: make(VAESolver)), ("DIPSolver i", lambda: make(DIPSolver, dip_type="i")),
                            ("TCSovler", lambda: make(TCSovler)),
                            ("MMDSolver imq", lambda: make(MMDSolver, mmd_kernel="imq")),
                            ("MMDSolver rbf", lambda: make(MMDSolver, mmd_kernel="rbf")),
                            ("VAESolver again", lambda: make(VAESolver))):
            med, lo, hi = step_ms(build(), args.steps, args.reps)
            out["step_ms " + name] = round(med, 4)
            print(f"c2 step, graph, f16x3  {name:<15} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    for Bt, P, D in ((64, 64, 128), (512, 512, 128)):
        for kernel in ("imq", "rbf"):
            fused = hook_us(lambda z, p, m, v: ops.mmd_kl_loss(z, m, v, p, 0.5, 10.0, kernel), Bt, P, D, args.calls,
                            args.reps)
            plain = hook_us(lambda z, p, m, v: torch_hook(z, p, m, v, kernel, 10.0, 0.5), Bt, P, D, args.calls, args.reps)
            out[f"hook_us ({Bt},{P},{D}) {kernel}"] = dict(fused=round(fused, 2), torch=round(plain, 2))
            print(f"hook fwd+bwd ({Bt:>3}, {P:>3}, {D}) {kernel}  fused {fused:8.2f} us   torch arithmetic {plain:8.2f} us",
                  flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
