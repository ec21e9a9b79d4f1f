"""GPU: one training step issues the same library calls, in the same order, with the same arguments as the step
recorded in tests/golden/step_calls.json.  The golden was recorded at the commit before the conv routing of
hipvae/functional.py was folded into one route record, so it pins every host decision of a step -- which kernel, which
plane format, which shapes, workspace sizes and flags -- as an equality, with no tolerance.

Recorded per call of ``hipvae.functional.call`` / ``hipvae.flat.call``: the entry point's name, every integer and float
argument (by the C signature of hipvae.abi.SIGNATURES), and a bit mask of the pointer arguments that were NULL; the
pointers themselves are dropped.  Steps: the intro-TC solver on the "conv" architecture (batched passes, the shared
decoder pass with its live range, deferred weight-gradient reduces, pack groups) at the smallest configuration
test_hip_model.py trains and at the 64..256-channel one that reaches the planes kernels, and the plain VAE solver on
the residual architecture (the shape-free producer hints); one warm-up step, then the recorded one.

    python tests/test_hip_call_trace.py OUT.json        # re-record (on a GPU)
"""
import contextlib
import ctypes
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_calls.json")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)          # test_hip_model.TINY
C1 = dict(cdim=3, zdim=10, channels=(64, 128, 256), image_size=32)         # test_hip_model.C1
# name -> (solver, architecture, network, conv math)
STEPS = {
    "intro_tc-conv-tiny-fp32": ("intro_tc", "conv", TINY, "fp32"),
    "intro_tc-conv-tiny-bf16x3": ("intro_tc", "conv", TINY, "bf16x3"),
    "intro_tc-conv-tiny-f16x3": ("intro_tc", "conv", TINY, "f16x3"),
    "intro_tc-conv-c1-bf16x3": ("intro_tc", "conv", C1, "bf16x3"),
    "intro_tc-conv-c1-f16x3": ("intro_tc", "conv", C1, "f16x3"),
    "vae-res-c1-bf16x3": ("vae", "res", C1, "bf16x3"),
}
_INT = (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t)
_FLOAT = (ctypes.c_float, ctypes.c_double)


@contextlib.contextmanager
def recorded_calls(log):
    """Wraps the ``call`` bound in hipvae.functional and in hipvae.flat: appends [name, ints and floats..., NULL mask]."""
    from hipvae import abi, flat, functional

    def wrap(inner):
        def call(name, *args):
            rec, null = [name], 0
            for k, (a, t) in enumerate(zip(args, abi.SIGNATURES[name][1])):
                if t in _INT:
                    rec.append(int(a))
                elif t in _FLOAT:
                    rec.append(float(a))
                elif a is None:
                    null |= 1 << k
            log.append(rec + [null])
            return inner(name, *args)
        return call

    saved = functional.call, flat.call
    functional.call, flat.call = wrap(saved[0]), wrap(saved[1])
    try:
        yield log
    finally:
        functional.call, flat.call = saved


def run_step(name):
    """Warm-up step + recorded step of STEPS[name] on fixed weights, inputs and draws -> the recorded calls."""
    import models
    import ops
    from test_hip_model import dev, make_solver
    solver_name, arch, net, math = STEPS[name]
    torch.manual_seed(3)
    model = models.SoftIntroVAE(arch=arch, **net).to(dev()).train()
    solver = make_solver(solver_name, model, [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4, 1000], math=math)
    g = torch.Generator().manual_seed(11)
    log = []
    for s in range(2):
        x = torch.rand(8, 3, 32, 32, generator=g)
        draws = [torch.randn(8, net["zdim"], generator=g) for _ in range(6 if solver_name.startswith("intro") else 1)]
        with ops.noise_queue(draws), (recorded_calls(log) if s else contextlib.nullcontext()):
            solver.train_step(x, s)
    torch.cuda.synchronize()
    return log


def encode(logs):
    """{step name: calls} -> {"calls": distinct calls, "steps": {name: indices into them}} (a step repeats most calls)."""
    uniq, index, steps = [], {}, {}
    for name, log in logs.items():
        seq = []
        for rec in log:
            k = json.dumps(rec)
            if k not in index:
                index[k] = len(uniq)
                uniq.append(rec)
            seq.append(index[k])
        steps[name] = seq
    return {"calls": uniq, "steps": steps}


@pytest.fixture(autouse=True)
def _time_limit():
    """Each test of this file runs under its own time limit (a step takes well under a second once it is warm)."""
    import signal

    def expired(signum, frame):
        raise TimeoutError("call-trace test exceeded its 120 s limit")

    prev = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, prev)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_every_step(golden):
    assert sorted(golden["steps"]) == sorted(STEPS)
    names = {golden["calls"][i][0] for seq in golden["steps"].values() for i in seq}
    # the step parts the trace is there for: planes convs with the live range, the deferred reduce, grouped packing,
    # the replayed BatchNorm update, the 5x5 matrix-core forms
    for want in ("itcv_conv2d_fwd_bf16p_sub", "itcv_wgrad_reduce_many", "itcv_conv2d_pack_weights_bf16s",
                 "itcv_bn_replay_many", "itcv_conv2d_wgrad5_bf16p", "itcv_conv2d_small_cout_fwd_bf16p",
                 "itcv_conv2d_small_cin_fwd_bf16x3", "itcv_conv2d_wgrad_bf16p", "itcv_conv2d_fwd", "itcv_conv2d_wgrad"):
        assert want in names, want


@pytest.mark.parametrize("name", sorted(STEPS))
def test_step_issues_the_recorded_calls(name, golden):
    want = [golden["calls"][i] for i in golden["steps"][name]]
    got = run_step(name)
    assert len(got) == len(want), (len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "intro-tc-vae_amd"), os.path.dirname(here), here):
        sys.path.insert(0, p)
    out = encode({name: run_step(name) for name in sorted(STEPS)})
    with open(sys.argv[1], "w") as f:
        f.write('{\n "calls": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in out["calls"]) + '\n ],\n "steps": {\n'
                + ",\n".join(f'  "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in out["steps"].items()) + "\n }\n}\n")
    print({k: len(v) for k, v in out["steps"].items()}, len(out["calls"]), "distinct calls")
