#!/usr/bin/env python3
"""Fused optimiser updates on the MI355X: (a) each update kernel alone, (b) whole c2 intro-TC steps.

(a) times every update kernel with device events over flat buffers the size of the c2 encoder and decoder halves (the
    existing plain-Adam kernel included, for comparison) and reports algorithmic bytes / time as a fraction of 8 TB/s.
(b) times c2 intro-TC steps (f16x3, ``enable_graph()``) for plain Adam, and for SGD(momentum, nesterov) and AdamW each
    run fused and through a do-nothing subclass (which takes the ``opt.step()`` fallback).  The configurations alternate
    within one process; median and spread of the repeats are printed.

    python tools/optim_bench.py [--repeats 3] [--steps 20] [--only kernels|steps]

One JSON line per measurement on stdout.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "intro-tc-vae_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_HBM = 8.0e12
C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
O = torch.optim

# name -> (optimizer factory, bytes moved per element): p read+write, g read, each state buffer read+write
KERNELS = {
    "adam (plain, existing)": (lambda ps: O.Adam(ps, lr=2e-4), 4 * (2 + 1 + 2 * 2)),
    "adamx wd": (lambda ps: O.Adam(ps, lr=2e-4, weight_decay=1e-4), 4 * (2 + 1 + 2 * 2)),
    "adamx adamw": (lambda ps: O.AdamW(ps, lr=2e-4), 4 * (2 + 1 + 2 * 2)),
    "adamx adamw amsgrad": (lambda ps: O.AdamW(ps, lr=2e-4, amsgrad=True), 4 * (2 + 1 + 3 * 2)),
    "sgd": (lambda ps: O.SGD(ps, lr=1e-2), 4 * (2 + 1)),
    "sgd momentum nesterov wd": (lambda ps: O.SGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4),
                                 4 * (2 + 1 + 2)),
    "adagrad": (lambda ps: O.Adagrad(ps, lr=1e-2, weight_decay=1e-4), 4 * (2 + 1 + 2)),
    "rmsprop": (lambda ps: O.RMSprop(ps, lr=1e-2), 4 * (2 + 1 + 2)),
    "rmsprop momentum centered": (lambda ps: O.RMSprop(ps, lr=1e-2, momentum=0.9, centered=True), 4 * (2 + 1 + 3 * 2)),
}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def c2_model():
    import models
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return models.SoftIntroVAE(arch="conv", **C2)


def bench_kernels(reps):
    from hipvae.flat import FlatGroup, fused_update
    dev = torch.device("cuda:0")
    model = c2_model().to(dev)
    import models
    for part in ("encoder", "decoder"):
        mod = getattr(model, part)
        params = list(mod.parameters())
        grp = FlatGroup(params, grad_free=models.grad_free_parameters(mod))
        grp.flat_g.normal_()
        p0 = grp.flat_p.clone()
        for name, (make, bpe) in KERNELS.items():
            opt = make(params)
            spec = fused_update(opt)
            grp.bind_optimizer(opt, spec)
            for _ in range(3):
                grp.fused_step(spec)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            torch.cuda.synchronize()
            for a, b in ev:
                a.record()
                grp.fused_step(spec)          # the update kernel plus its one-thread step bump
                b.record()
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b) * 1e-3 for a, b in ev)
            t = statistics.median(ts)
            emit(part="a", half=part, kernel=name, spec=str(spec[:2]), elements=grp.numel, bytes_per_element=bpe,
                 median_us=round(t * 1e6, 2), min_us=round(ts[0] * 1e6, 2), max_us=round(ts[-1] * 1e6, 2),
                 tb_per_s=round(bpe * grp.numel / t * 1e-12, 3), frac_of_8tbs=round(bpe * grp.numel / t / PEAK_HBM, 4))
            grp.flat_p.copy_(p0)


class SGDSub(O.SGD):
    """Does nothing: being a subclass, it takes the opt.step() fallback."""


class AdamWSub(O.AdamW):
    pass


STEP_CONFIGS = {
    "adam (plain)": lambda ps: O.Adam(ps, lr=2e-4),
    "sgd fused": lambda ps: O.SGD(ps, lr=2e-4, momentum=0.9, nesterov=True),
    "sgd fallback": lambda ps: SGDSub(ps, lr=2e-4, momentum=0.9, nesterov=True),
    "adamw fused": lambda ps: O.AdamW(ps, lr=2e-4),
    "adamw fallback": lambda ps: AdamWSub(ps, lr=2e-4),
}


def bench_steps(repeats, steps, warmup):
    from hipvae.flat import fused_update
    from solvers.intro_tc import IntroTCSovler

    class DS:
        def __len__(self):
            return 10000

    dev = torch.device("cuda:0")
    B = 64
    g = torch.Generator().manual_seed(7)
    batches = [torch.rand(B, 3, 64, 64, generator=g).to(dev) for _ in range(4)]
    solvers = {}
    for name, make in STEP_CONFIGS.items():
        model = c2_model().to(dev).train()
        s = IntroTCSovler(DS(), model, B, make(model.encoder.parameters()), make(model.decoder.parameters()), "mse",
                          0.5, 0.75, 512.0, 1e-8, dev, True, None, clip=100.0)
        s.conv_math = "f16x3"
        s.enable_graph()
        for i in range(warmup):
            s.train_step(batches[i % 4], i)
        torch.cuda.synchronize()
        solvers[name] = s
    times = {name: [] for name in STEP_CONFIGS}
    for r in range(repeats):
        for name, s in solvers.items():           # alternate the configurations within each repeat
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                s.train_step(batches[i % 4], warmup + r * steps + i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps)
    for name, ts in times.items():
        s = solvers[name]
        emit(part="b", config=name, fused=fused_update(s.optimizer_e) is not None, graph=s._graph is not None,
             steps_per_repeat=steps, repeats=repeats, median_ms=round(statistics.median(ts) * 1e3, 3),
             min_ms=round(min(ts) * 1e3, 3), max_ms=round(max(ts) * 1e3, 3),
             images_per_s=round(B / statistics.median(ts), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--only", choices=["kernels", "steps"], default=None)
    args = ap.parse_args()
    if args.only in (None, "kernels"):
        bench_kernels(args.kernel_reps)
    if args.only in (None, "steps"):
        bench_steps(max(3, args.repeats), args.steps, args.warmup)


if __name__ == "__main__":
    main()
