#!/usr/bin/env python3
"""Time of the JointVAE / AnnealedVAE objective (solvers/joint.py, csrc/joint.hip).

1. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512), batch 64) as
   hipGraph replays in the f16x3 arithmetic: JointVAESolver (cont = 118, disc = (10,)) and AnnealedVAESolver next to
   VAESolver, all in this one run, the VAE step first and again last (the base of the comparison, and its drift over the
   run): after the capture, HIP events around ``--steps`` replayed steps, each of which writes its capacity and ends in
   its one host read-back; the median and the range of ``--reps`` such legs.
2. us of the op alone, forward + backward, at B = 64, zdim = 128 (cont = 118, disc = (10,)), from HIP events around
   ``--calls`` calls after a warm-up, for ``ops.joint_latent`` and for the same arithmetic in plain torch (what a user had
   to write before: about forty at:: launches); the median and the range of ``--reps`` such legs.
3. the kernels the op launches, read from a profiler trace of one forward + backward (``--trace``).

Prints one line per figure and, last, all of them as one JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402
import ops  # noqa: E402
from solvers.joint import AnnealedVAESolver, JointVAESolver  # noqa: E402
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
ROWS, CONT, DISC = 64, 118, (10,)
TAU, GZ, GC = 0.67, 30.0, 30.0


class DS:
    def __len__(self):
        return 10000


def make(cls, **kw):
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
    return cls(DS(), model, ROWS, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), "mse", 0.5, 0.75, dev, True, None, clip=100.0, **kw)


def timed(fn, n, reps):
    """Median, min and max over ``reps`` legs of the HIP-event time of ``n`` calls of ``fn``, in ms per call."""
    legs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        legs.append(a.elapsed_time(b) / n)
    return float(np.median(legs)), min(legs), max(legs)


def step_ms(solver, steps, reps):
    assert solver.conv_math == "f16x3"
    g = torch.Generator().manual_seed(1000)
    batches = [torch.rand(ROWS, 3, 64, 64, generator=g).to(dev) for _ in range(4)]
    solver.enable_graph()
    for i in range(6):                          # 3 eager warm-ups, capture + first replay, two more replays
        solver.train_step(batches[i % 4], i)
    assert solver._graph is not None and len(solver._graphs) == 1
    out = timed(lambda i: solver.train_step(batches[i % 4], i), steps, reps)
    assert len(solver._graphs) == 1             # the rising capacity never re-captured
    return out


def torch_op(mu, logvar, eps, u, cap, beta):
    """The op as a user writes it with torch arithmetic (fp32), after Dupont's lines."""
    m, l = mu[:, :CONT], logvar[:, :CONT]
    cols = [m + eps * (0.5 * l).exp()]
    klz = (-0.5 * (1.0 + l - m * m - l.exp()).sum(1)).mean()
    klc, s = 0.0, CONT
    for k in DISC:
        a, uu = mu[:, s:s + k], u[:, s - CONT:s - CONT + k]
        gum = -torch.log(-torch.log(uu.clamp_min(2.0 ** -25)))
        cols.append(torch.softmax((a + gum) / TAU, dim=1))
        la = torch.log_softmax(a, dim=1)
        klc = klc + (math.log(k) + (la.exp() * la).sum(1)).mean()
        s += k
    loss = beta * (GZ * (klz - cap[0]).abs() + GC * (klc - cap[1]).abs())
    return torch.cat(cols, dim=1), loss.float()


def op_setup():
    g = torch.Generator().manual_seed(7)
    D = CONT + sum(DISC)
    mu = torch.randn(ROWS, D, generator=g).to(dev).requires_grad_(True)
    lv = (0.5 * torch.randn(ROWS, D, generator=g) - 1.5).to(dev).requires_grad_(True)
    eps = torch.randn(ROWS, CONT, generator=g).to(dev)
    u = torch.rand(ROWS, sum(DISC), generator=g).to(dev)
    dz = torch.randn(ROWS, D, generator=g).to(dev)
    cap = torch.tensor([5.0, 0.5], dtype=torch.float64, device=dev)
    return mu, lv, eps, u, dz, cap, torch.ones((), device=dev)


def op_once(fn, mu, lv, eps, u, dz, cap, one):
    mu.grad = lv.grad = None
    z, loss = fn(mu, lv, eps, u, cap)
    torch.autograd.backward((z, loss), (dz, one))


def op_us(fn, calls, reps):
    """Median, min and max us of one forward + backward of ``fn`` -> (z, loss), with a gradient into both outputs."""
    args = op_setup()
    for _ in range(20):
        op_once(fn, *args)
    return tuple(1e3 * v for v in timed(lambda i: op_once(fn, *args), calls, reps))


def fused(mu, lv, eps, u, cap):
    return ops.joint_latent(mu, lv, CONT, DISC, cap, GZ, GC, beta=0.5, temperature=TAU, eps=eps, u=u)


def plain(mu, lv, eps, u, cap):
    return torch_op(mu, lv, eps, u, cap, 0.5)


def kernel_names(fn):
    """The device kernels of one forward + backward of ``fn``, in launch order, from a profiler trace."""
    from torch.profiler import ProfilerActivity, profile
    args = op_setup()
    for _ in range(3):
        op_once(fn, *args)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        op_once(fn, *args)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
          and "memset" not in e.name.lower()]
    return [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the op alone")
    ap.add_argument("--trace", action="store_true", help="also list the kernels of the op from a profiler trace")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if not args.no_steps:
        joint = dict(latent_spec=dict(cont=CONT, disc=DISC), cont_capacity=(0.0, 5.0, 25000, GZ),
                     disc_capacity=(0.0, 5.0, 25000, GC), temperature=TAU)
        for name, build in (("VAESolver", lambda: make(VAESolver)),
                            ("JointVAESolver 118 + (10,)", lambda: make(JointVAESolver, **joint)),
                            ("AnnealedVAESolver", lambda: make(AnnealedVAESolver)),
                            ("VAESolver again", lambda: make(VAESolver))):
            med, lo, hi = step_ms(build(), args.steps, args.reps)
            out["step_ms " + name] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
            print(f"c2 step, batch 64, graph, f16x3  {name:<27} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    for name, fn in (("fused", fused), ("torch", plain)):
        med, lo, hi = op_us(fn, args.calls, args.reps)
        out[f"op_us ({ROWS},{CONT}+{DISC[0]}) {name}"] = dict(median=round(med, 2), min=round(lo, 2), max=round(hi, 2))
        print(f"op fwd+bwd (B = {ROWS}, cont = {CONT}, disc = {DISC}) {name:<6} {med:8.2f} us  (range {lo:.2f} .. {hi:.2f})",
              flush=True)
    if args.trace:
        for name, fn in (("fused", fused), ("torch", plain)):
            names = kernel_names(fn)
            out[f"kernels {name}"] = len(names)
            print(f"kernels of one forward + backward, {name}: {len(names)}", flush=True)
            if name == "fused":
                for n in names:
                    print("   ", n[:150], flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
