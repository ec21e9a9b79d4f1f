#!/usr/bin/env python3
"""Time of the VampPrior objective (solvers/vamp.py, csrc/vamp.hip).

1. us of the latent op alone, forward + backward, at (B, K, D) = (64, 500, 128), from HIP events around ``--calls`` calls
   after a warm-up, for ``ops.vamp_latent`` and for the same statement in fp32 torch arithmetic (``torch.logsumexp`` over a
   [B, K, D] difference tensor, autograd), the median of ``--reps`` such legs.
2. ms per training step at the benchmark configuration c2 (64x64x3, z = 128, channels (64, 128, 256, 512), 64 images) as
   hipGraph replays in the f16x3 arithmetic, all in this one run: VAESolver (first and again last: the base of the
   comparison and its drift over the run), a VAESolver whose encoder sees 64 + 500 rows in one pass (the floor: the
   encoder pass over the K pseudo-inputs is inherent to the objective), and VampSolver with K = 500.  A host clock around
   ``--steps`` replayed steps, each of which ends in its one host read-back; the median and the range of ``--reps`` legs.
3. The op's share of the Vamp step: figure 1 over figure 2.

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
from solvers.vae import VAESolver  # noqa: E402
from solvers.vamp import VampSolver  # noqa: E402

dev = torch.device("cuda:0")
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
BATCH, K = 64, 500
LOG2PI = math.log(2.0 * math.pi)


class DS:
    def __len__(self):
        return 10000


class WideEncodeSolver(VAESolver):
    """The plain VAE step whose encoder sees BATCH + K rows in one pass (the KL over all of them), the decoder BATCH."""

    def _losses(self, real):
        mu, logvar = self.model.encode(torch.cat([real, self.extra]))
        loss_kl = self.compute_kl_loss(None, mu, logvar)
        z = ops.reparameterize(mu[:BATCH], logvar[:BATCH])
        loss_rec = self.compute_rec_loss(real, self.model.decode(z), reduction="mean")
        return z, loss_rec, loss_kl, None


def make(cls, **kw):
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
    return cls(DS(), model, BATCH, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), "mse", 0.5, 0.75, dev, True, None, clip=100.0, **kw)


def make_vamp():
    pseudo = models.PseudoInputs(K, C2["cdim"], C2["image_size"]).to(dev)
    return make(VampSolver, pseudo_inputs=pseudo, optimizer_prior=torch.optim.Adam(pseudo.parameters(), lr=2e-4))


def make_wide():
    solver = make(WideEncodeSolver)
    solver.extra = torch.rand(K, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)
    return solver


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


def torch_op(mu, logvar, eps, p_mu, p_logvar, beta):
    """The op as a user writes it in torch arithmetic (fp32)."""
    z = mu + eps * torch.exp(0.5 * logvar)
    logq = -0.5 * (LOG2PI + logvar + eps * eps).sum(1)
    diff = z[:, None, :] - p_mu[None, :, :]
    L = -0.5 * (LOG2PI + p_logvar[None] + diff * diff * torch.exp(-p_logvar)[None]).sum(2)
    return z, beta * (logq - (torch.logsumexp(L, dim=1) - math.log(p_mu.shape[0]))).mean()


def op_us(fn, B, Kc, D, calls, reps):
    """Median us of one forward + backward of ``fn`` (through the loss and through z) from HIP events around ``calls``."""
    g = torch.Generator().manual_seed(7)
    mu = (0.5 * torch.randn(B, D, generator=g)).to(dev).requires_grad_(True)
    lv = (torch.rand(B, D, generator=g) * 1.5 - 1.0).to(dev).requires_grad_(True)
    pm = (0.5 * torch.randn(Kc, D, generator=g)).to(dev).requires_grad_(True)
    pl = (torch.rand(Kc, D, generator=g) - 0.5).to(dev).requires_grad_(True)
    eps = torch.randn(B, D, generator=g).to(dev)
    gz = torch.randn(B, D, generator=g).to(dev)

    def once():
        mu.grad = lv.grad = pm.grad = pl.grad = None
        z, loss = fn(mu, lv, eps, pm, pl)
        torch.autograd.backward((z, loss), (gz, None))

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
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-steps", action="store_true", help="the op alone")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    D = C2["zdim"]
    fused = op_us(lambda m, v, e, pm, pl: ops.vamp_latent(m, v, pm, pl, beta=0.5, eps=e), BATCH, K, D, args.calls, args.reps)
    plain = op_us(lambda m, v, e, pm, pl: torch_op(m, v, e, pm, pl, 0.5), BATCH, K, D, args.calls, args.reps)
    out[f"op_us ({BATCH},{K},{D})"] = dict(fused=round(fused, 2), torch=round(plain, 2))
    print(f"op fwd+bwd ({BATCH}, {K}, {D})  fused {fused:8.2f} us   torch arithmetic {plain:8.2f} us", flush=True)
    if not args.no_steps:
        for name, build in (("VAESolver", lambda: make(VAESolver)), ("VAESolver 564-row encode", make_wide),
                            ("VampSolver K=500", make_vamp), ("VAESolver again", lambda: make(VAESolver))):
            med, lo, hi = step_ms(build(), args.steps, args.reps)
            out["step_ms " + name] = round(med, 4)
            print(f"c2 step, graph, f16x3  {name:<26} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f})", flush=True)
        share = fused * 1e-3 / out["step_ms VampSolver K=500"]
        out["op share of the Vamp step"] = round(share, 4)
        print(f"op share of the Vamp step (eager op time over replayed step time)  {100 * share:.1f} %", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
