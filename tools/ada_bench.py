#!/usr/bin/env python3
"""Time of the Ada-GVAE / Ada-ML-VAE objective (solvers/ada.py, csrc/ada.hip).

1. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512)) as hipGraph
   replays in the f16x3 arithmetic: AdaGVAESolver ("gvae" and "mlvae") at 32 pairs next to VAESolver at batch 64 -- the
   same 64 rows -- all in this one run, the VAE step first and again last (the base of the comparison, and its drift over
   the run): after the capture, HIP events around ``--steps`` replayed steps, each of which ends in its one host
   read-back; the median and the range of ``--reps`` such legs.
2. us of the op alone, forward + backward, at (pairs, D) = (32, 128) and (256, 128), from HIP events around ``--calls``
   calls after a warm-up, for ``ops.ada_group`` and for the same arithmetic in plain torch (what a user had to write
   before: about thirty at:: launches); both averagings; the median of ``--reps`` such legs.

Prints one line per figure and, last, all of them as one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import models  # noqa: E402
import ops  # noqa: E402
from solvers.ada import AdaGVAESolver  # noqa: E402
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
ROWS = 64


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
    assert solver._graph is not None
    return timed(lambda i: solver.train_step(batches[i % 4], i), steps, reps)


def torch_op(mu, logvar, eps, beta, averaging):
    """The op as a user writes it with torch arithmetic (fp32), after the library's lines."""
    B = mu.shape[0] // 2
    m1, m2, l1, l2 = mu[:B], mu[B:], logvar[:B], logvar[B:]
    v1, v2 = l1.exp(), l2.exp()
    with torch.no_grad():
        kl = v1 / v2 + (m2 - m1) ** 2 / v2 - 1.0 + l2 - l1
        own = kl >= 0.5 * (kl.min(1, keepdim=True)[0] + kl.max(1, keepdim=True)[0])
    if averaging == "gvae":
        mb, lb = 0.5 * m1 + 0.5 * m2, (0.5 * v1 + 0.5 * v2).log()
    else:
        vb = 2.0 * v1 * v2 / (v1 + v2)
        mb, lb = (m1 / v1 + m2 / v2) * vb * 0.5, vb.log()
    mt = torch.cat([torch.where(own, m1, mb), torch.where(own, m2, mb)])
    lt = torch.cat([torch.where(own, l1, lb), torch.where(own, l2, lb)])
    z = mt + eps * (0.5 * lt).exp()
    return z, beta * (-0.5 * (1.0 + lt - mt * mt - lt.exp()).sum(1)).mean()


def op_us(fn, B, D, calls, reps):
    """Median us of one forward + backward of ``fn(mu, logvar, eps)`` -> (z, loss), with a gradient into both outputs."""
    g = torch.Generator().manual_seed(7)
    mu = torch.randn(2 * B, D, generator=g).to(dev).requires_grad_(True)
    lv = (0.5 * torch.randn(2 * B, D, generator=g) - 1.5).to(dev).requires_grad_(True)
    eps = torch.randn(2 * B, D, generator=g).to(dev)
    dz = torch.randn(2 * B, D, generator=g).to(dev)
    one = torch.ones((), device=dev)

    def once(_):
        mu.grad = lv.grad = None
        z, loss = fn(mu, lv, eps)
        torch.autograd.backward((z, loss), (dz, one))

    for i in range(20):
        once(i)
    return timed(once, calls, reps)[0] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the op alone")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if not args.no_steps:
        for name, build in (("VAESolver 64", lambda: make(VAESolver)),
                            ("AdaGVAESolver gvae 32 pairs", lambda: make(AdaGVAESolver, averaging="gvae")),
                            ("AdaGVAESolver mlvae 32 pairs", lambda: make(AdaGVAESolver, averaging="mlvae")),
                            ("VAESolver 64 again", lambda: make(VAESolver))):
            med, lo, hi = step_ms(build(), args.steps, args.reps)
            out["step_ms " + name] = round(med, 4)
            print(f"c2 step, graph, f16x3  {name:<29} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    for B, D in ((32, 128), (256, 128)):
        for averaging in ("gvae", "mlvae"):
            fused = op_us(lambda m, v, e: ops.ada_group(m, v, 0.5, averaging, eps=e), B, D, args.calls, args.reps)
            plain = op_us(lambda m, v, e: torch_op(m, v, e, 0.5, averaging), B, D, args.calls, args.reps)
            out[f"op_us ({B},{D}) {averaging}"] = dict(fused=round(fused, 2), torch=round(plain, 2))
            print(f"op fwd+bwd ({B:>3} pairs, {D}) {averaging:<5}  fused {fused:8.2f} us   torch arithmetic {plain:8.2f} us",
                  flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
