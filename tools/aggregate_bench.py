#!/usr/bin/env python3
"""Time of the dataset-scale aggregate-posterior kernel (hipvae.functional.aggregate_logdensity, csrc/aggregate.hip) at
(S, N, D) = (1024, 65536, 10), (1024, 65536, 32), (1024, 65536, 128) and (256, 737280, 10), next to

  * the same two quantities from torch on the same device: the ops.py:24-29 density broadcast to [rows, N, D] and
    torch.logsumexp over the components, over chunks of rows (the tensor torch materialises is held to 2^27 elements);
  * the minibatch kernel it generalises, HF.tc_components(..., flags=WEIGHTED), at 512 x 512 x 128.

HIP events around the calls, after warm-up, once per shape; ns per (j, i, l) element for all three."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import torch  # noqa: E402

from hipvae import abi  # noqa: E402
from hipvae import functional as HF  # noqa: E402

dev = torch.device("cuda:0")
LOG_2PI = math.log(2.0 * math.pi)


def timed(once, warm, reps):
    """ms per call of ``once``."""
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_restatement(z, mu, lv, chunk):
    N = mu.shape[0]
    inv, lw = torch.exp(-lv).unsqueeze(0), -math.log(N)
    logqz, lse = [], []
    for a in range(0, z.shape[0], chunk):
        d = z[a:a + chunk].unsqueeze(1) - mu.unsqueeze(0)
        lp = torch.clamp(-0.5 * (d * d * inv + lv.unsqueeze(0) + LOG_2PI), min=-50)
        logqz.append(torch.logsumexp(lp.sum(2) + lw, 1))
        lse.append(torch.logsumexp(lp + lw, 1))
    return torch.cat(logqz), torch.cat(lse)


def inputs(S, N, D, seed=1):
    g = torch.Generator().manual_seed(seed)
    mu = ((0.7 / math.sqrt(D)) * torch.randn(N, D, generator=g)).to(dev)
    lv = (-0.3 + 0.2 * torch.randn(N, D, generator=g)).to(dev)
    rows = torch.randint(N, (S,), generator=g).to(dev)
    z = mu[rows] + torch.randn(S, D, generator=g).to(dev) * torch.exp(0.5 * lv[rows])
    return z.contiguous(), mu, lv


def main():
    for S, N, D in ((1024, 65536, 10), (1024, 65536, 32), (1024, 65536, 128), (256, 737280, 10)):
        z, mu, lv = inputs(S, N, D)
        elems = S * N * D
        t_new = timed(lambda: HF.aggregate_logdensity(z, mu, lv), 2, 5)
        chunk = max(1, (1 << 27) // (N * D))
        t_ref = timed(lambda: torch_restatement(z, mu, lv, chunk), 1, 2)
        a, b = HF.aggregate_logdensity(z, mu, lv), torch_restatement(z, mu, lv, chunk)
        err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
        print(f"aggregate_logdensity S {S:5d} x N {N:7d} x D {D:4d}: {t_new:9.3f} ms = {t_new * 1e6 / elems:7.4f} ns/element; "
              f"torch restatement (chunks of {chunk} rows) {t_ref:9.3f} ms = {t_ref * 1e6 / elems:7.4f} ns/element; "
              f"{t_ref / t_new:6.1f}x; largest relative difference {err:.1e}", flush=True)
    B, D = 512, 128
    z, mu, lv = inputs(B, B, D)
    t_old = timed(lambda: HF.tc_components(z, mu, lv, 10000, 0, flags=abi.TC_WEIGHTED), 5, 50)
    t_new = timed(lambda: HF.aggregate_logdensity(z, mu, lv), 5, 50)
    print(f"tc_components(WEIGHTED) {B} x {B} x {D}: {t_old * 1e3:8.1f} us = {t_old * 1e6 / (B * B * D):7.4f} ns/element; "
          f"aggregate_logdensity at the same size {t_new * 1e3:8.1f} us = {t_new * 1e6 / (B * B * D):7.4f} ns/element")


if __name__ == "__main__":
    main()
