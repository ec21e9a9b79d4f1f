#!/usr/bin/env python3
"""Time of the SSIM loss (ops.ssim_loss, csrc/ssim.hip), forward + backward, at (64, 3, 64, 64), (128, 3, 128, 128) and
(32, 3, 256, 256), next to
  (a) the mse loss of the same shape through itcv_recon_loss_fwd / _bwd: it moves the same bytes (two image reads each way,
      one image write) with next to no arithmetic, and is the floor;
  (b) an fp32 torch statement of the same loss on the same GPU: five grouped ``conv2d`` with the 2-D window, the map in
      torch arithmetic, autograd for the gradient;
and of a training step of the c2 model (64 x 64 x 3, z = 128, channels (64, 128, 256, 512), 64 images) of ``VAESolver``
with recon_loss_type "ssim" next to "mse", eager and as one captured graph.

HIP events around ``reps`` calls after ``warm`` warm-up calls of the same shape; the three sides are timed in alternating
rounds and the median round is reported with the range.  Agreement is printed first: what is timed computes the same
thing.  ``--json PATH`` also writes the records; ``--no-step`` leaves the training step out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import ops  # noqa: E402
from hipvae import functional as HF  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = ((64, 3, 64, 64), (128, 3, 128, 128), (32, 3, 256, 256))
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
K, SIGMA, C1c, C2c = 11, 1.5, 0.01 ** 2, 0.03 ** 2


def torch_ssim_loss(x, y, w):
    """sum_b P (1 - SSIM_b) in fp32: the statement (b)."""
    C = x.shape[1]
    f = lambda t: F.conv2d(t, w, groups=C)                                          # noqa: E731
    mx, my = f(x), f(y)
    sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    S = (2 * mx * my + C1c) * (2 * sxy + C2c) / ((mx * mx + my * my + C1c) * (sx + sy + C2c))
    return (x[0].numel() * (1 - S.flatten(1).mean(1))).sum()


def events(once, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(sides, warm, reps, nrounds):
    """name -> (median, min, max) ms per call over ``nrounds`` alternating rounds of ``reps`` calls each."""
    for once in sides.values():
        for _ in range(warm):
            once()
    torch.cuda.synchronize()
    ts = {k: [] for k in sides}
    for _ in range(nrounds):
        for k, once in sides.items():
            ts[k].append(events(once, reps))
    return {k: (float(np.median(t)), min(t), max(t)) for k, t in ts.items()}


def run_shape(shape, warm, reps, nrounds):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape, generator=g).to(dev)
    y = (0.8 * x.cpu() + 0.2 * torch.rand(shape, generator=g)).to(dev).requires_grad_(True)
    win = torch.tensor(HF.ssim_window_host(K, SIGMA), dtype=torch.float32, device=dev)
    w = (win[:, None] * win[None, :]).expand(C, 1, K, K).contiguous()

    def fb(loss):
        def once():
            y.grad = None
            loss().backward()
        return once

    sides = dict(ssim=fb(lambda: ops.ssim_loss(x, y)), mse=fb(lambda: ops.reconstruction_loss(x, y, "mse")),
                 torch_fp32=fb(lambda: torch_ssim_loss(x, y, w)))
    sides["ssim"]()
    ours, dours = float(ops.ssim_loss(x, y).detach()), y.grad.clone()
    sides["torch_fp32"]()
    theirs, dtheirs = float(torch_ssim_loss(x, y, w).detach()), y.grad.clone()
    agree = dict(loss_device=ours, loss_torch_fp32=theirs,
                 dy_rel=float((dours - dtheirs).abs().max() / dours.abs().max()))
    t = rounds(sides, warm, reps, nrounds)
    image_bytes = 4.0 * B * C * H * W
    rec = dict(shape=shape, warm=warm, reps=reps, rounds=nrounds, agreement=agree, ms=t,
               ssim_over_mse=t["ssim"][0] / t["mse"][0], torch_over_ssim=t["torch_fp32"][0] / t["ssim"][0],
               ssim_GBps_of_5_image_passes=5.0 * image_bytes / (t["ssim"][0] * 1e-3) / 1e9)
    print(f"{shape}: agreement {json.dumps(agree)}")
    for k, (med, lo, hi) in t.items():
        print(f"  {k:11s} fwd + bwd {med:9.4f} ms ({lo:.4f} .. {hi:.4f})")
    print(f"  ssim / mse {rec['ssim_over_mse']:.2f}x   torch fp32 / ssim {rec['torch_over_ssim']:.2f}x   "
          f"beats (b): {t['ssim'][0] < t['torch_fp32'][0]}")
    return rec


class _DS:
    def __len__(self):
        return 10000


def run_step(warm, reps, nrounds):
    import models
    from solvers import VAESolver
    x = torch.rand((64, 3, 64, 64), generator=torch.Generator().manual_seed(2)).to(dev)
    sides = {}
    for graph in (False, True):
        for lt in ("mse", "ssim"):
            torch.manual_seed(0)
            model = models.SoftIntroVAE(arch="conv", **C2).to(dev).train()
            solver = VAESolver(_DS(), model, 64, torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
                               torch.optim.Adam(model.decoder.parameters(), lr=2e-4), lt, 0.5, 0.75, dev, False, None, clip=100.0)
            if graph:
                solver.enable_graph()
            sides[f"{lt}_{'graph' if graph else 'eager'}"] = (lambda s=solver, n=[0]: (s.train_step(x, n[0]), n.__setitem__(0, n[0] + 1)))
    t = rounds(sides, max(warm, 5), reps, nrounds)              # five: past the three eager steps before a capture
    print("c2 VAESolver.train_step (64 images), ms per step, host read-back of the losses included:")
    for k, (med, lo, hi) in t.items():
        print(f"  {k:11s} {med:9.4f} ms ({lo:.4f} .. {hi:.4f})")
    return dict(ms=t, ssim_over_mse_eager=t["ssim_eager"][0] / t["mse_eager"][0],
                ssim_over_mse_graph=t["ssim_graph"][0] / t["mse_graph"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench: no GPU; nothing is measured without one")
    out = dict(shapes=[run_shape(s, 3, args.reps, args.rounds) for s in SHAPES])
    if not args.no_step:
        out["c2_step"] = run_step(5, args.reps, args.rounds)
    out["beats_torch_fp32_everywhere"] = all(r["ms"]["ssim"][0] < r["ms"]["torch_fp32"][0] for r in out["shapes"])
    print("beats the fp32 torch statement at all three shapes:", out["beats_torch_fp32_everywhere"])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
