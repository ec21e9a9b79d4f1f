#!/usr/bin/env python3
"""Time of the semi-supervised S2 objectives (solvers/semi.py, csrc/sup.hip).

1. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512)) as hipGraph
   replays in the f16x3 arithmetic: S2VAESolver with B = B_l = 64, F = 5 (every form), and, as the upper reference,
   VAESolver at batch 128 -- the same encoder rows and twice the decoder rows -- and at batch 64.  After the capture, a
   host clock around ``--steps`` replayed steps, each of which ends in its one host read-back; the median and the range
   of ``--reps`` such legs.  ``--only vae`` runs the VAESolver legs alone (they need nothing of the S2 family, so the same
   file times the commit before it).
2. us of the term alone, forward + backward, at (B_l, D, F) = (64, 128, 5) and (512, 128, 64), from HIP events around
   ``--calls`` calls after a warm-up, for ``ops.supervised_regularizer`` and for the same arithmetic in torch on the
   device (what a user had to write before); the median of ``--reps`` such legs.

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
from solvers.vae import VAESolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
BATCH = 64
SIZES = (3, 6, 40, 32, 32)


class DS:
    def __len__(self):
        return 10000


def make(cls, batch, **kw):
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
    return cls(DS(), model, batch, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), "mse", 0.5, 0.75, dev, True, None, clip=100.0, **kw)


def step_ms(solver, rows, labelled, steps, reps):
    """(median, min, max) ms per step over ``reps`` legs of ``steps`` replayed steps on ``rows`` images, the last
    ``labelled`` of them with labels."""
    assert solver.conv_math == "f16x3"
    g = torch.Generator().manual_seed(1000)
    batches = [torch.rand(rows, 3, 64, 64, generator=g).to(dev) for _ in range(4)]
    if labelled:
        ys = [torch.stack([torch.randint(0, k, (labelled,), generator=g) for k in SIZES], 1).float().to(dev)
              for _ in range(4)]
        batches = list(zip(batches, ys))
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


def torch_term(mu, y, kind, sizes):
    """The term as a user writes it with torch arithmetic on the device."""
    F = y.shape[1]
    if kind == "xent":
        return torch.nn.functional.binary_cross_entropy_with_logits(mu[:, :F], y / sizes, reduction="sum")
    if kind == "l2":
        return ((mu[:, :F] - y) ** 2).sum()
    xc, yc = mu - mu.mean(0, keepdim=True), y - y.mean(0, keepdim=True)
    C = xc.t() @ yc / mu.shape[0]
    d = torch.diagonal(C)
    return (C * C).sum() - (d * d).sum()


def term_us(fn, B, D, F, calls, reps):
    """Median us of one forward + backward of ``fn(mu, y, sizes)`` from HIP events around ``calls`` calls."""
    g = torch.Generator().manual_seed(7)
    sizes = tuple(2 + f % 9 for f in range(F))
    mu = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    y = torch.stack([torch.randint(0, k, (B,), generator=g) for k in sizes], 1).float().to(dev)
    sizes_t = torch.tensor(sizes, dtype=torch.float32, device=dev)

    def once():
        mu.grad = None
        fn(mu, y, sizes, sizes_t).backward()

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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("all", "vae", "term"), default="all")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    legs = []
    if args.only in ("all", "vae"):
        legs += [("VAESolver b128", lambda: make(VAESolver, 2 * BATCH), 2 * BATCH, 0),
                 ("VAESolver b64", lambda: make(VAESolver, BATCH), BATCH, 0)]
    if args.only == "all":
        from solvers.semi import S2VAESolver
        legs += [(f"S2VAESolver {kind}", lambda kind=kind: make(S2VAESolver, BATCH, factor_sizes=SIZES, sup_kind=kind,
                                                                sup_schedule="anneal", sup_threshold=1000),
                  2 * BATCH, BATCH) for kind in ("xent", "l2", "cov")]
    for name, build, rows, labelled in legs:
        med, lo, hi = step_ms(build(), rows, labelled, args.steps, args.reps)
        out["step_ms " + name] = dict(median=round(med, 4), min=round(lo, 4), max=round(hi, 4))
        print(f"c2 step, graph, f16x3  {name:<17} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
    if args.only in ("all", "term"):
        for B, D, F in ((64, 128, 5), (512, 128, 64)):
            for kind in ("xent", "l2", "cov"):
                fused = term_us(lambda m, y, s, st: ops.supervised_regularizer(m, y, kind, s if kind == "xent" else None),
                                B, D, F, args.calls, args.reps)
                plain = term_us(lambda m, y, s, st: torch_term(m, y, kind, st), B, D, F, args.calls, args.reps)
                out[f"term_us ({B},{D},{F}) {kind}"] = dict(fused=round(fused, 2), torch=round(plain, 2))
                print(f"term fwd+bwd ({B:>3}, {D}, {F:>2}) {kind:<4}  fused {fused:8.2f} us   torch arithmetic {plain:8.2f} us",
                      flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
