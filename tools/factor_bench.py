#!/usr/bin/env python3
"""Time of the FactorVAE objective (solvers/factor.py, csrc/factor.hip, the fused discriminator layers).

1. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512), 64 images) as
   hipGraph replays in the f16x3 arithmetic, for VAESolver, TCSovler and FactorSolver (the default discriminator: 6 hidden
   layers of 1000, Adam 1e-4 (0.5, 0.9)), all in this one run, the VAE step first and again last (the base of the
   comparison, and its drift over the run): after the capture, a host clock around ``--steps`` replayed steps, each of
   which ends in its one host read-back; the median and the range of ``--reps`` such legs.
2. us of the discriminator part alone at (B, zdim) = (64, 128), hidden 1000 x 6 -- the permutation, ONE forward over the
   2B rows, the VAE walk (tc -> z), the discriminator's walk (d_loss -> parameters) and its Adam update -- on the fused
   kernels and for the same MLP in plain torch on the device (``nn.Sequential``, ``F.cross_entropy``, ``torch.optim.Adam``,
   argsort + gather for the permutation), each both as eager launches and as replays of one captured graph; HIP events
   around ``--calls`` calls after a warm-up, the median of ``--reps`` such legs.

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
import torch.nn.functional as F  # noqa: E402

import models  # noqa: E402
import ops  # noqa: E402
from hipvae.flat import FlatGroup, fused_update  # noqa: E402
from hipvae.functional import direct_grad_accumulation  # noqa: E402
from solvers.factor import FactorSolver  # noqa: E402
from solvers.tc import TCSovler  # noqa: E402
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
BATCH = 64


class DS:
    def __len__(self):
        return 10000


def disc_adam(disc, **kw):
    return torch.optim.Adam(disc.parameters(), lr=1e-4, betas=(0.5, 0.9), **kw)


def make(cls, **kw):
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
    if cls is FactorSolver:
        disc = models.Discriminator(C2["zdim"]).to(dev)
        kw.update(discriminator=disc, optimizer_disc=disc_adam(disc))
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


def fused_part(z):
    """One discriminator part of a step on the fused kernels: returns the callable."""
    torch.manual_seed(1)
    disc = models.Discriminator(z.shape[1]).to(dev)
    opt = disc_adam(disc)
    group = FlatGroup(list(disc.parameters()))
    spec = fused_update(opt)
    group.bind_optimizer(opt, spec)

    def once():
        z.grad = None
        dp = ops.factor_pass(z, disc)
        ops.factor_tc(z, disc, shared=dp).backward()
        group.zero_grad()
        with direct_grad_accumulation():
            ops.factor_disc_loss(z, disc, shared=dp).backward()
        group.fused_step(spec)

    return once


def torch_part(z, capturable):
    """The same part as a user writes it in torch."""
    torch.manual_seed(1)
    ref = models.Discriminator(z.shape[1])
    disc = torch.nn.Sequential(*[torch.nn.Linear(m.in_features, m.out_features) if isinstance(m, torch.nn.Linear)
                                 else torch.nn.LeakyReLU(m.negative_slope) for m in ref]).to(dev)
    opt = disc_adam(disc, capturable=capturable)
    B = z.shape[0]
    labels = torch.cat([torch.zeros(B, dtype=torch.long), torch.ones(B, dtype=torch.long)]).to(dev)
    params = list(disc.parameters())

    def once():
        z.grad = None
        zd = z.detach()
        z_perm = torch.gather(zd, 0, torch.argsort(torch.randn_like(zd), dim=0))
        l = disc(torch.cat([z, z_perm]))
        tc = (l[:B, 0] - l[:B, 1]).mean()
        z.grad, = torch.autograd.grad(tc, z, retain_graph=True)
        d_loss = 0.5 * F.cross_entropy(l[:B], labels[:B]) + 0.5 * F.cross_entropy(l[B:], labels[B:])
        grads = torch.autograd.grad(d_loss, params)
        for p, g in zip(params, grads):
            p.grad = g
        opt.step()

    return once


def part_us(once, calls, reps, graph):
    """Median us of ``once()`` from HIP events around ``calls`` calls (eager) or replays of its captured graph."""
    for _ in range(20):
        once()
    run = once
    if graph:
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            once()
        run = g.replay
        for _ in range(5):
            run()
    legs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            run()
        b.record()
        torch.cuda.synchronize()
        legs.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(legs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the discriminator part alone")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if not args.no_steps:
        for name, build in (("VAESolver", lambda: make(VAESolver)), ("TCSovler", lambda: make(TCSovler)),
                            ("FactorSolver", lambda: make(FactorSolver)), ("VAESolver again", lambda: make(VAESolver))):
            med, lo, hi = step_ms(build(), args.steps, args.reps)
            out["step_ms " + name] = round(med, 4)
            print(f"c2 step, graph, f16x3  {name:<15} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    g = torch.Generator().manual_seed(7)
    B, zdim = BATCH, C2["zdim"]
    for graph in (False, True):
        z = (1.2 * torch.randn(B, zdim, generator=g) + 0.3).to(dev).requires_grad_(True)
        fused = part_us(fused_part(z), args.calls, args.reps, graph)
        z = z.detach().clone().requires_grad_(True)
        mode = "graph" if graph else "eager"
        try:
            plain = part_us(torch_part(z, capturable=graph), args.calls, args.reps, graph)
        except RuntimeError as e:              # torch's own part may refuse a capture (the last leg: nothing runs after it)
            print(f"discriminator part, {mode}: torch's part was not measured ({str(e).splitlines()[0]})", flush=True)
            plain = float("nan")
        out[f"disc_part_us ({B},{zdim}) 1000x6 {mode}"] = dict(fused=round(fused, 2), torch=round(plain, 2))
        print(f"discriminator part ({B}, {zdim}) 1000 x 6, {mode}  fused {fused:9.2f} us   torch {plain:9.2f} us", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
