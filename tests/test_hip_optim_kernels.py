"""The optimiser kernels of csrc/optim.hip and the two plain-Adam kernels of csrc/loss_optim.hip on the MI355X, on the
tables of tests/optim_cases.py (held to their promises on the CPU by tests/test_optim_cases_host.py):

(a) every launchable instance (46 cases) through its raw entry point at 1, 2 and 5 blocks and at ``step_dev`` 0, 1 and
    999, against the real torch.optim class in fp64; n = 0; the unread momentum buffer of SGD's first step;
(b) one case per family and both plain kernels at exactly one grid trip, one thread past it and 77 past it, and the
    first 4100 elements of the largest launch bit for bit equal to a 4100-element launch;
(c) the ``live`` mask at the first, last, every other float4, across a block edge, across the trip edge and all dead:
    dead float4s (NaN in g and every state buffer) untouched bit for bit, live ones equal to the unmasked launch;
(d) the same four updates through FlatGroup with every padding length and two grad-free parameters, from a loaded
    state at step 7;
(e) one captured ``fused_step`` replayed five times equal to five eager calls, bit for bit.

Every array (``p``, the move ``dp = p_new - p_old`` and each state buffer) is judged by max |got - ref| / max |ref|
against ``max(4 * e32, 2^-22)``, e32 being the same figure of torch's fp32 CPU step on the same inputs; ``p`` is also
held elementwise to ``param_bound`` of tests/test_hip_optim.py against that fp32 step.  Measured figures: DESIGN.md §5.
"""
import functools

import numpy as np
import pytest
import torch

import optim_cases as oc
from test_hip_optim import param_bound, step_scale

pytestmark = pytest.mark.gpu

STEPS = (0, 1, 999)
# arrays held to the ceiling alone, by (case name, array): none
CEILING_ONLY = {}


def dev():
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def launch(case, arrays, step, live=None, nan_dead=False):
    """One call of the case's raw entry point on fresh device tensors holding ``arrays`` with ``step_dev`` preset to
    ``step``.  State the case keeps but ``arrays`` lacks (SGD's buffer before the first step) is filled with NaN, and
    so are g and every state buffer over the dead float4s of ``live`` when ``nan_dead``.  Returns ({name: cpu tensor}
    after the call, with the move ``dp`` in fp64; ``step_dev`` afterwards; the tensors before the call)."""
    from hipvae import abi
    n = arrays["p"].size
    t = {k: up(v) for k, v in arrays.items()}
    for k in case.states:
        if k not in t:
            t[k] = torch.full((n,), float("nan"), device=dev())
    lv = None
    if live is not None:
        lv = up(live)
        if nan_dead:
            dead = (lv == 0).repeat_interleave(4)
            for k in t:
                if k != "p":
                    t[k][dead] = float("nan")
    step_dev = torch.full((1,), step, dtype=torch.int32, device=dev())
    ptrs = {k: abi.ptr(v) for k, v in t.items()}
    start = {k: v.cpu() for k, v in t.items()}
    step_arg = step + 1 if case.kind == "adam" else abi.ptr(step_dev)
    abi.call(*oc.call_args(case, ptrs, abi.ptr(lv), n, step_arg, abi.stream()))
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in t.items() if k != "g"}
    assert torch.equal(bits(t["g"]), bits(start["g"])), "the gradient was written"
    out["dp"] = out["p"].double() - torch.from_numpy(arrays["p"]).double()
    return out, int(step_dev.item()), start


def judge(case, got, arrays, step, tag):
    """Each array of ``got`` against the fp64 torch.optim step, under max(4 e32, 2^-22); ``p`` under the ceiling."""
    ref = oc.reference(case, arrays, step).arrays
    r32 = oc.reference(case, arrays, step, torch.float32).arrays
    bad = []
    for k in ref:
        g = got[k].double().numpy()
        assert np.isfinite(g).all(), (case.name, tag, k)
        err, e32 = oc.figure(g, ref[k]), oc.figure(r32[k], ref[k])
        limit = oc.bar(e32)
        print(f"[optim] {case.name} {tag} {k}: err {err:.3e} e32 {e32:.3e} bar {limit:.3e}")
        if err > limit and (case.name, k) not in CEILING_ONLY:
            bad.append((k, err, e32, limit))
    assert not bad, (case.name, tag, bad)
    # the ceiling: param_bound's third argument is the largest update one step can make.  These gradients hold outliers
    # the moments have not seen (25 lr under Adam at beta2 = 0.999, lr |g| under SGD), so that is the reference's own
    # largest move where it exceeds step_scale: a weight that lands near 0 carries the rounding of its move.
    scale = max(step_scale(case.cls, case.kw), float(np.abs(ref["dp"]).max()))
    p32 = torch.from_numpy(r32["p"]).float()
    assert param_bound(got["p"], p32, scale, 1), (
        case.name, tag, float((got["p"] - p32).abs().max()))


# ---- (a) every instance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name)
def test_instance_vs_fp64(case):
    for n in oc.sizes(case)[oc.SMALL]:
        for step in STEPS:
            arrays = oc.inputs(case, n, step)
            got, step_after, _ = launch(case, arrays, step)
            if case.kind != "adam":
                assert step_after == step + 1, (n, step, step_after)
            judge(case, got, arrays, step, f"n={n} step={step}")
            if case.kind == "sgd" and case.states and step == 0:
                # the buffer held NaN before the call: the first step writes it without reading it
                ref = oc.reference(case, arrays, step).arrays["momentum_buffer"]
                assert torch.isfinite(got["momentum_buffer"]).all()
                assert oc.figure(got["momentum_buffer"].double().numpy(), ref) <= oc.FLOOR


@pytest.mark.parametrize("kind", list(oc.FAMILY))
def test_no_elements_only_advances_the_step(kind):
    from hipvae import abi
    case = oc.FAMILY[kind]
    arrays = oc.inputs(case, 4, 3)
    t = {k: up(v) for k, v in arrays.items()}
    start = {k: v.clone() for k, v in t.items()}
    step_dev = torch.full((1,), 3, dtype=torch.int32, device=dev())
    abi.call(*oc.call_args(case, {k: abi.ptr(v) for k, v in t.items()}, None, 0, abi.ptr(step_dev), abi.stream()))
    torch.cuda.synchronize()
    assert int(step_dev.item()) == 4
    for k in t:
        assert torch.equal(bits(t[k]), bits(start[k])), k


# ---- (b) grid trips ----------------------------------------------------------------------------------------------------
TRIP_CASES = dict(oc.FAMILY, **oc.PLAIN)
TRIP_STEP = 2


@pytest.mark.parametrize("kind", list(TRIP_CASES))
def test_grid_trips_vs_fp64(kind):
    case = TRIP_CASES[kind]
    last = None
    for n in oc.sizes(case)[oc.TRIPS]:
        arrays = oc.inputs(case, n, TRIP_STEP)
        got, step_after, _ = launch(case, arrays, TRIP_STEP)
        if case.kind != "adam":
            assert step_after == TRIP_STEP + 1
        judge(case, got, arrays, TRIP_STEP, f"n={n} step={TRIP_STEP}")
        last = (arrays, got)
    # an element's result does not depend on the launch it is part of
    arrays, got = last
    m = 4100
    small, _, _ = launch(case, {k: v[:m].copy() for k, v in arrays.items()}, TRIP_STEP)
    for k in small:
        assert torch.equal(bits(got[k][:m]), bits(small[k])), (kind, k)


# ---- (c) the live mask ---------------------------------------------------------------------------------------------------
MASK_N = oc.SIZES4[-1]
MASK_STEP = 2


@functools.lru_cache(maxsize=1)
def _unmasked(kind):
    case = oc.FAMILY[kind]
    arrays = oc.inputs(case, MASK_N, MASK_STEP)
    got, _, _ = launch(case, arrays, MASK_STEP)
    return arrays, got


@pytest.mark.parametrize("mask", list(oc.MASKS))
@pytest.mark.parametrize("kind", list(oc.FAMILY))
def test_live_mask(kind, mask):
    case = oc.FAMILY[kind]
    arrays, full = _unmasked(kind)
    live = oc.MASKS[mask](MASK_N // 4)
    got, step_after, start = launch(case, arrays, MASK_STEP, live=live, nan_dead=True)
    assert step_after == MASK_STEP + 1
    alive = torch.from_numpy(live).bool().repeat_interleave(4)
    assert int((~alive).sum()) >= 4
    for k in ("p",) + case.states:
        if k != "p":
            assert torch.isnan(start[k][~alive]).all(), k
        # dead float4s keep their bits (NaN payloads included), live ones are the unmasked launch's
        assert torch.equal(bits(got[k])[~alive], bits(start[k])[~alive]), (kind, mask, k, "dead")
        assert torch.equal(bits(got[k])[alive], bits(full[k])[alive]), (kind, mask, k, "live")


# ---- (d) through FlatGroup ---------------------------------------------------------------------------------------------
SHAPES = [(1,), (2,), (3,), (5,), (4, 4), (7, 3, 3, 3), (1030,)]
FREE = (2, 4)


def _numel(s):
    return int(np.prod(s))


def make_group(case, step):
    """Parameters of SHAPES on the device (FREE ones grad-free) under ``torch.optim.<case.cls>``, bound to a FlatGroup;
    ``step`` > 0: state of ``inputs()`` loaded through ``load_state_dict`` first.  Returns (group, optimiser, spec,
    parameters, the arrays of each parameter)."""
    from hipvae.flat import FlatGroup, fused_update
    arrays = [oc.inputs(case, _numel(s), step, seed=20 + i) for i, s in enumerate(SHAPES)]
    ps = [torch.nn.Parameter(up(a["p"]).view(s)) for a, s in zip(arrays, SHAPES)]
    opt = getattr(torch.optim, case.cls)(ps, **case.kw)
    if step:
        sd = opt.state_dict()
        sd["state"] = {}
        for i, (a, s) in enumerate(zip(arrays, SHAPES)):
            if i not in FREE:
                st = {k: torch.from_numpy(a[k]).view(s).clone() for k in case.states}
                if case.cls != "SGD":
                    st["step"] = torch.tensor(float(step))
                sd["state"][i] = st
        opt.load_state_dict(sd)
    spec = fused_update(opt)
    assert spec is not None
    grp = FlatGroup(ps, grad_free=[ps[i] for i in FREE])
    assert sorted({(-_numel(s)) % 4 for s in SHAPES}) == [0, 1, 2, 3]
    for i, (p, a, s) in enumerate(zip(ps, arrays, SHAPES)):
        if i not in FREE:
            p.grad.copy_(up(a["g"]).view(s))
    grp.bind_optimizer(opt, spec)
    return grp, opt, spec, ps, arrays


def padding_index(grp):
    pad = torch.ones(grp.numel, dtype=torch.bool)
    for p, o in zip(grp.params, grp.offsets):
        pad[o:o + p.numel()] = False
    return pad


@pytest.mark.parametrize("kind", list(oc.FAMILY))
def test_through_flat_group(kind):
    case = oc.FAMILY[kind]
    assert case.flags & oc.MAXIMIZE and case.hp[{"adamx": 4, "sgd": 3, "adagrad": 2, "rmsprop": 3}[kind]] > 0
    step = 7
    grp, opt, spec, ps, arrays = make_group(case, step)
    assert spec == (case.kind, case.flags, case.hp)
    assert grp.live is not None and int(grp.step_dev.item()) == (1 if kind == "sgd" else step)
    free0 = {i: ps[i].detach().clone() for i in FREE}
    grp.fused_step(spec)
    torch.cuda.synchronize()
    pad = padding_index(grp)
    assert int(pad.sum()) == 3 + 2 + 1 + 3 + 0 + 3 + 2
    assert bool((grp.flat_p.cpu()[pad] == 0).all())
    sd = opt.state_dict()["state"]
    for i, (p, a, s) in enumerate(zip(ps, arrays, SHAPES)):
        if i in FREE:
            assert torch.equal(bits(p), bits(free0[i])), (kind, s)
            for k in case.states:
                assert bool((opt.state[p][k] == 0).all()), (kind, s, k)
            continue
        got = {"p": p.detach().cpu().reshape(-1)}
        got["dp"] = got["p"].double() - torch.from_numpy(a["p"]).double()
        for k in case.states:
            assert opt.state[p][k].shape == p.shape
            got[k] = opt.state[p][k].detach().cpu().reshape(-1)
        judge(case, got, a, step, f"flat shape={s}")
        if kind != "sgd":
            assert float(sd[i]["step"]) == step + 1


# ---- (e) replay --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(oc.FAMILY) + ["adam_dev"])
def test_replay_equals_eager(kind):
    case = TRIP_CASES[kind]
    grp, opt, spec, ps, arrays = make_group(case, 0)
    assert spec[0] == ("adam" if kind == "adam_dev" else kind)
    bufs = [grp.flat_p] + [grp.slots[k] for k in case.states] + [grp.step_dev]
    start = [b.clone() for b in bufs]
    assert int(grp.step_dev.item()) == 0

    def restore():
        for b, s in zip(bufs, start):
            b.copy_(s)

    for _ in range(5):
        grp.fused_step(spec)
    torch.cuda.synchronize()
    eager = [b.clone() for b in bufs]
    assert int(eager[-1].item()) == 5 and not torch.equal(eager[0], start[0])
    restore()
    grp.fused_step(spec)                                            # warm up, then capture from the same start
    restore()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        grp.fused_step(spec)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    for name, b, e in zip(["p"] + list(case.states) + ["step_dev"], bufs, eager):
        assert torch.equal(bits(b) if b.dtype == torch.float32 else b.cpu(),
                           bits(e) if e.dtype == torch.float32 else e.cpu()), (kind, name)
    assert int(grp.step_dev.item()) == 5
