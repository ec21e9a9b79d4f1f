"""The fused SGD / Adam(W) / Adagrad / RMSprop updates on the MI355X: against torch.optim on the CPU in fp32, against
the reference's own solvers and optimisers (tests/golden/steps_optim.npz), under hipGraph capture and replay, with an
lr scheduler, through optimizer.state_dict() round trips and parameter ownership loss, and the fallback kept for
everything else."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
O = torch.optim


def dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.asarray(a))


def load_state(npz, prefix):
    return {k[len(prefix):].replace("/", "."): T(npz[k]).clone() for k in npz.files if k.startswith(prefix)}


def build(state):
    import models
    m = models.SoftIntroVAE(arch="conv", **TINY)
    m.load_state_dict(state, strict=True)
    return m.to(dev()).train()


class _DS:
    def __len__(self):
        return 1000


def make_solver(model, make_opt, hp=(0.5, 0.75, 512.0, 1e-8, 100.0)):
    from solvers.intro_tc import IntroTCSovler
    return IntroTCSovler(_DS(), model, 8, make_opt(model.encoder.parameters()), make_opt(model.decoder.parameters()),
                         "mse", hp[0], hp[1], hp[2], hp[3], dev(), False, None, clip=hp[4])


# ---- 1. every kernel x flag combination against torch.optim on the CPU ------------------------------------------
KERNEL_CASES = [
    ("Adam", dict(lr=1e-3, weight_decay=0.1)),
    ("Adam", dict(lr=1e-3, weight_decay=0.1, amsgrad=True)),
    ("Adam", dict(lr=1e-3, maximize=True)),
    ("Adam", dict(lr=1e-3, betas=(0.3, 0.9), weight_decay=0.1, decoupled_weight_decay=True)),
    ("AdamW", dict(lr=1e-3)),
    ("AdamW", dict(lr=1e-3, weight_decay=0.05, amsgrad=True, maximize=True)),
    ("SGD", dict(lr=1e-2)),
    ("SGD", dict(lr=1e-2, weight_decay=1e-2, maximize=True)),
    ("SGD", dict(lr=1e-2, momentum=0.9)),
    ("SGD", dict(lr=1e-2, momentum=0.9, dampening=0.3, weight_decay=1e-2)),
    ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=1e-4, maximize=True)),
    ("Adagrad", dict(lr=1e-2)),
    ("Adagrad", dict(lr=1e-2, lr_decay=1e-2, weight_decay=1e-4, initial_accumulator_value=0.1, eps=1e-8,
                     maximize=True)),
    ("RMSprop", dict(lr=1e-2)),
    ("RMSprop", dict(lr=1e-2, centered=True)),
    ("RMSprop", dict(lr=1e-2, momentum=0.9, weight_decay=1e-4)),
    ("RMSprop", dict(lr=1e-2, alpha=0.3, momentum=0.5, centered=True, weight_decay=1e-4, maximize=True)),
]
SHAPES = [(7, 3, 3, 3), (13,), (5, 11), (1,), (6, 2)]


def param_bound(p, p_ref, lr, k):
    """|p - p_ref| <= 2.4e-7 |p_ref| + 1e-6 lr k, elementwise (``lr``: the largest update one step can make)."""
    return bool(((p.detach().cpu() - p_ref.detach()).abs() <= 2.4e-7 * p_ref.detach().abs() + 1e-6 * lr * k).all())


def step_scale(cls, kw):
    """Largest per-element update of one step: lr, except for RMSprop, whose first steps move by up to
    lr / sqrt(1 - alpha) (10 lr at the default alpha), accumulated by momentum up to 1 / (1 - momentum) times."""
    lr = kw["lr"]
    if cls != "RMSprop":
        return lr
    return lr / (1.0 - kw.get("alpha", 0.99)) ** 0.5 / (1.0 - kw.get("momentum", 0.0))


def state_close(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) <= 1e-6 * float(b.abs().max()) + 1e-30


@pytest.mark.parametrize("case", range(len(KERNEL_CASES)))
def test_kernel_matches_torch(case):
    from hipvae.flat import FlatGroup, fused_update
    cls, kw = KERNEL_CASES[case]
    g = torch.Generator().manual_seed(40 + case)
    ps_ref = [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]
    ps = [torch.nn.Parameter(p.detach().clone().to(dev())) for p in ps_ref]
    free = ps[4]                                          # a parameter torch never sees a gradient for
    opt_ref, opt = getattr(O, cls)(ps_ref, **kw), getattr(O, cls)(ps, **kw)
    spec = fused_update(opt)
    assert spec is not None and spec[0] != "adam", spec
    grp = FlatGroup(ps, grad_free=[free])
    free0 = free.detach().clone()
    for k in range(1, 6):
        grads = [torch.randn(*s, generator=g) * (50.0 if k == 2 else 0.01) for s in SHAPES]
        for p, pr, gr in zip(ps, ps_ref, grads):
            if p is free:
                pr.grad = None
            else:
                pr.grad = gr.clone()
                p.grad.copy_(gr.to(dev()))
        opt_ref.step()
        grp.bind_optimizer(opt, spec)
        grp.fused_step(spec)
        torch.cuda.synchronize()
        for i, (p, pr) in enumerate(zip(ps[:4], ps_ref[:4])):
            assert param_bound(p, pr, step_scale(cls, kw), k), (cls, kw, k, i, float((p.detach() - pr.to(dev())).abs().max()))
        assert torch.equal(free.detach(), free0)
    sd = opt.state_dict()["state"]
    sd_ref = opt_ref.state_dict()["state"]
    for i in range(4):
        st, st_ref = sd.get(i, {}), sd_ref.get(i, {})           # SGD without momentum keeps no state
        assert set(st) == set(st_ref), (st.keys(), st_ref.keys())
        for name, t in st_ref.items():
            if name == "step":
                assert float(st[name]) == float(t)
            else:
                assert st[name].shape == t.shape and state_close(st[name], t), (cls, kw, i, name)


# ---- 2. the reference's solvers with the reference's optimisers --------------------------------------------------
FIXTURE = {
    "sgd": lambda ps, lr: O.SGD(ps, lr=lr, momentum=0.9, nesterov=True, weight_decay=1e-4),
    "adamw": lambda ps, lr: O.AdamW(ps, lr=lr, weight_decay=1e-2, amsgrad=True),
    "adagrad": lambda ps, lr: O.Adagrad(ps, lr=lr, lr_decay=1e-3, weight_decay=1e-4, initial_accumulator_value=0.1),
    "rmsprop": lambda ps, lr: O.RMSprop(ps, lr=lr, momentum=0.9, centered=True, weight_decay=1e-4),
}


def load_golden():
    """steps_optim.npz and steps_conv.npz, whose intro-TC run supplies the initial weights, inputs and noise draws
    (tests/golden/make_golden_optim.py checks they are the ones the reference optimiser runs started from)."""
    g = np.load(os.path.join(GOLDEN, "steps_optim.npz"))
    conv = np.load(os.path.join(GOLDEN, "steps_conv.npz"))
    draws = [[T(conv[f"intro_tc:s{s}:draw{i}"]) for i in range(len([k for k in conv.files
                                                                  if k.startswith(f"intro_tc:s{s}:draw")]))]
             for s in range(2)]
    return g, load_state(conv, "init:"), [T(conv["x0"]), T(conv["x1"])], draws


def sample(t):
    """Every 4th element of a weight tensor: the subset of the final weights the fixture holds."""
    return t.detach().cpu().reshape(-1)[::4]


def final_sample(g, init, name):
    """{weight key: sampled final weights of the reference run} (stored as the XOR of the fp32 bits with the initial
    weights, in 4 byte planes)."""
    bits = np.ascontiguousarray(g[f"{name}:final_xor"].T).view(np.uint32).reshape(-1)
    out, o = {}, 0
    for k in (str(k) for k in g["weight_keys"]):
        a = sample(init[k]).numpy()
        out[k] = T((a.view(np.uint32) ^ bits[o:o + a.size]).view(np.float32))
        o += a.size
    assert o == bits.size
    return out


@pytest.mark.parametrize("name", list(FIXTURE))
def test_reference_optimisers_golden(name):
    import ops
    from hipvae.flat import fused_update
    g, init, xs, draws = load_golden()
    hp = g["hp"]
    lr = float(g[f"{name}:lr"])
    model = build(init)
    solver = make_solver(model, lambda ps: FIXTURE[name](ps, lr), hp)
    assert fused_update(solver.optimizer_e) is not None
    for s in range(2):
        p = f"{name}:s{s}:"
        with ops.noise_queue([t.clone() for t in draws[s]]):
            d = solver.train_step(xs[s], s)
        got = np.array([d["loss_enc"], d["loss_dec"], d["loss_kl"], d["loss_rec"], d["L2"]])
        np.testing.assert_allclose(got, g[p + "dict"], rtol=1e-4 if s == 0 else 3e-4, err_msg=p)
    fin = final_sample(g, init, name)
    sd = model.state_dict()
    diffs = torch.cat([(sample(sd[k]) - v).abs() for k, v in fin.items()])
    # the family's own update size: the largest per-element move of the reference run over its 2 steps
    upd = torch.cat([(v - sample(init[k])).abs() for k, v in fin.items()])
    assert float(diffs.max()) <= 2.05 * float(upd.max()), (name, float(diffs.max()), float(upd.max()))
    assert float(diffs.median()) < 0.02 * float(upd.max()) / 2, (name, float(diffs.median()), float(upd.max()))
    free = [str(k) for k in g[f"{name}:no_grad"]]
    assert free and all("conv_expand" in k for k in free)
    for k in free:                       # the reference left them untouched (checked when the fixture was made)
        assert torch.equal(sd[k].detach().cpu(), init[k]), k


# ---- 3./4. graph capture and replay, and a scheduler ----------------------------------------------------------------
def _trajectory(make_opt, graph, nsteps=7, sched=None, sched_every=1):
    import models
    cfg = dict(cdim=3, zdim=16, channels=(16, 32, 64), image_size=32)
    xs = [torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(i)).to(dev()) for i in range(nsteps)]
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **cfg).to(dev()).train()
    solver = make_solver(model, make_opt, (0.5, 0.75, 512.0, 1e-8, 100.0))
    if graph:
        solver.enable_graph()
    scheds = [sched(solver.optimizer_e), sched(solver.optimizer_d)] if sched else []
    torch.cuda.manual_seed(1234)
    res, keys = [], set()
    for i, x in enumerate(xs):
        res.append(solver.train_step(x, i))
        if graph and solver._graph is not None:
            keys.add(solver._graph_key)
        if (i + 1) % sched_every == 0:
            for s in scheds:
                s.step()
    w = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()
    return solver, res, w, keys


def _same(a, b):
    for x, y in zip(a[1], b[1]):
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((a[2] - b[2]).abs().max()) < 1e-6


GRAPH_CASES = {
    "sgd": lambda ps: O.SGD(ps, lr=2e-4, momentum=0.9, nesterov=True, weight_decay=1e-4),
    "adamw": lambda ps: O.AdamW(ps, lr=2e-4, amsgrad=True),
    "adagrad": lambda ps: O.Adagrad(ps, lr=2e-4, lr_decay=1e-3, initial_accumulator_value=0.1),
    "rmsprop": lambda ps: O.RMSprop(ps, lr=2e-4, momentum=0.9, centered=True, weight_decay=1e-4),
}


@pytest.mark.parametrize("name", list(GRAPH_CASES))
def test_graph_replay_equals_eager(name):
    eager = _trajectory(GRAPH_CASES[name], False)
    graph = _trajectory(GRAPH_CASES[name], True)
    assert graph[0]._graph is not None, "graph was not captured"
    _same(eager, graph)


def test_scheduler_recaptures():
    make = GRAPH_CASES["sgd"]

    def sched(o):
        return O.lr_scheduler.StepLR(o, step_size=3, gamma=0.5)

    # an epoch of 2 batches: lr halves every 6 steps (the first graph is captured after 3 eager steps, a re-capture
    # after one)
    eager = _trajectory(make, False, nsteps=12, sched=sched, sched_every=2)
    graph = _trajectory(make, True, nsteps=12, sched=sched, sched_every=2)
    assert graph[0]._graph is not None
    assert len(graph[3]) >= 2, "the lr change did not re-capture"
    assert len({k[3] for k in graph[3]}) >= 2
    _same(eager, graph)


# ---- 5. optimizer state round trips ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURE))
def test_state_roundtrip_and_ownership(name):
    import ops
    from hipvae.flat import fused_update
    g, init, xs, draws = load_golden()
    hp = g["hp"]
    lr = float(g[f"{name}:lr"])

    def make(ps):
        return FIXTURE[name](ps, lr)

    def steps(solver, which):
        out = []
        for s in which:
            with ops.noise_queue([t.clone() for t in draws[s]]):
                out.append(solver.train_step(xs[s], s))
        return out

    m0 = build(init)
    s0 = make_solver(m0, make, hp)
    ref = steps(s0, (0, 1))
    # (a) state_dict after step 0 into a fresh model / optimisers
    m1 = build(init)
    s1 = make_solver(m1, make, hp)
    first = steps(s1, (0,))
    sd_e = {k: v for k, v in s1.optimizer_e.state_dict().items()}
    sd_e = {"state": {i: {k: v.clone() for k, v in st.items()} for i, st in sd_e["state"].items()},
            "param_groups": sd_e["param_groups"]}
    sd_d, sd_m = s1.optimizer_d.state_dict(), m1.state_dict()
    assert len(sd_e["state"]) == len(list(m1.encoder.parameters()))
    m2 = build({k: v.cpu() for k, v in sd_m.items()})
    s2 = make_solver(m2, make, hp)
    s2.optimizer_e.load_state_dict(sd_e)
    s2.optimizer_d.load_state_dict(sd_d)
    second = steps(s2, (1,))
    assert first[0] == ref[0]
    for k in ("loss_enc", "loss_dec", "loss_kl", "loss_rec"):
        assert abs(second[0][k] - ref[1][k]) <= 1e-6 * abs(ref[1][k]), (k, second[0][k], ref[1][k])
    # (b) the saved encoder state loads into torch's own optimiser on the CPU.  One more step there, from the weights
    # after step 0 and with the gradients s2's encoder update used (still in its flat buffer: the decoder phase's clip
    # coefficient is 1 at these norms), lands on s2's encoder weights after step 1.
    import models
    free = {id(p) for p in models.grad_free_parameters(m2.encoder)}
    names = [k for k, _ in m2.encoder.named_parameters()]
    enc_ps = [torch.nn.Parameter(sd_m["encoder." + k].detach().cpu().clone()) for k in names]
    for p, q in zip(enc_ps, m2.encoder.parameters()):
        p.grad = None if id(q) in free else q.grad.detach().cpu().clone()
    cpu_opt = make(enc_ps)
    cpu_opt.load_state_dict(sd_e)
    assert fused_update(cpu_opt) is not None
    cpu_opt.step()
    for k, p, q in zip(names, enc_ps, m2.encoder.parameters()):
        scale = step_scale("RMSprop", dict(lr=lr, momentum=0.9)) if name == "rmsprop" else lr
        assert param_bound(q, p, scale, 1), (k, float((q.detach().cpu() - p.detach()).abs().max()))
    # (c) ownership lost after step 0: parameters re-pointed out of the flat buffers keep their optimiser state
    m3 = build(init)
    s3 = make_solver(m3, make, hp)
    steps(s3, (0,))
    for p in m3.parameters():
        p.data = p.data.clone()
    third = steps(s3, (1,))
    for k in ref[1]:
        assert abs(third[0][k] - ref[1][k]) <= 1e-6 * abs(ref[1][k]), (k, third[0][k], ref[1][k])
    wa = torch.cat([p.detach().reshape(-1) for p in m0.parameters()])
    wb = torch.cat([p.detach().reshape(-1) for p in m3.parameters()])
    assert float((wa - wb).abs().max()) < 1e-7


# ---- 6. the fallback stays torch's own opt.step(), eager ----------------------------------------------------------------
def test_fallback_unchanged():
    from hipvae.flat import fused_update

    class MySGD(O.SGD):
        pass

    for make in (lambda ps: O.Adamax(ps, lr=2e-4), lambda ps: MySGD(ps, lr=2e-4, momentum=0.9)):
        solver, res, w, keys = _trajectory(make, True, nsteps=5)
        assert fused_update(solver.optimizer_e) is None
        assert solver._graph is None and not keys
        assert all(np.isfinite(list(r.values())).all() for r in res)
        # torch's own state, not a flat mirror
        st = solver.optimizer_e.state[next(solver.model.encoder.parameters())]
        assert not hasattr(solver.optimizer_e, "_itcv_group") and st
