"""The intro step's repeated decoder pass, recorded once (IntroSolver.share_decoder_pass), against the schedule that
issues it twice: the computation is the same, so every comparison here is ``torch.equal`` -- no tolerance.

* whole steps, IntroTCSovler on the conv architecture: returned values, ``model.state_dict()`` (every BatchNorm buffer,
  ``num_batches_tracked`` included) and both optimisers' state, for fp32 and f16x3, eager and through the captured graph
  (five calls there: three eager warm-up steps, the capture, two replays), at a small c2-shaped batch and at B = 64;
* a forward hook on a decoder submodule sends the solver back to the schedule with four batched decoder calls per step;
* the replay launch alone against the plain forward run twice on the same input, on every BatchNorm launch path
  (pinned with ``itcv_bn_plan_query`` as tests/test_hip_bn.py does), G = 1, 2, 3, momentum 0.1 and 1.0, with a null
  running buffer and through the Sync-BN finalisation entry.

Mutations that must fail (tried by hand when the schedule was written; the assertions they trip are named):
* replaying BEFORE ``dec(z_rec | z_fake)`` instead of after (move ``shared.replay()`` above that pass): the decoder's
  ``running_mean`` / ``running_var`` differ in the last bits -> the ``state_dict`` comparison of
  ``test_shared_pass_equals_repeated_pass``;
* letting phase E's backward add one decoder weight gradient (``SharedPass.param_grads`` left True during it): the
  stale-gradient norm changes -> ``norm_E`` (``L2``) and from there the encoder's weights in the same test.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)
HP = dict(beta_kl=0.5, beta_rec=0.75, beta_neg=512.0, gamma_r=1e-8, clip=100.0, lr=2e-4)
F16 = 4


def dev():
    return torch.device("cuda:0")


class _DS:
    def __len__(self):
        return 10000


def make(math, B, share, graph):
    import models
    from solvers.intro_tc import IntroTCSovler
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **C2).to(dev()).train()
    solver = IntroTCSovler(_DS(), model, B, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                           torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", HP["beta_kl"], HP["beta_rec"],
                           HP["beta_neg"], HP["gamma_r"], dev(), math == "f16x3", None, clip=HP["clip"])
    solver.conv_math = math
    solver.share_decoder_pass = share
    if graph:
        solver.enable_graph()
    return model, solver


def run(math, B, share, graph, steps):
    model, solver = make(math, B, share, graph)
    xs = [torch.rand(B, 3, 64, 64, generator=torch.Generator().manual_seed(10 + s)).to(dev()) for s in range(steps)]
    torch.manual_seed(1234)                      # the device-side N(0,1) draws of the steps
    res = [solver.train_step(xs[s], s) for s in range(steps)]
    torch.cuda.synchronize()
    if graph:
        assert solver._graph is not None, "the captured graph was not used"
    state = {k: v.clone() for k, v in model.state_dict().items()}
    opt = {}
    for name, o in (("e", solver.optimizer_e), ("d", solver.optimizer_d)):
        for i, (p, st) in enumerate(o.state_dict()["state"].items()):
            for k, v in st.items():
                opt[f"{name}.{i}.{k}"] = v.clone() if isinstance(v, torch.Tensor) else torch.tensor(v)
    return res, state, opt


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("B", [8, 64])
@pytest.mark.parametrize("math", ["fp32", "f16x3"])
def test_shared_pass_equals_repeated_pass(math, B, graph):
    steps = 5 if graph else 3
    new = run(math, B, True, graph, steps)
    old = run(math, B, False, graph, steps)
    for s, (a, b) in enumerate(zip(new[0], old[0])):
        assert a.keys() == b.keys()
        for k in a:
            print(f"step {s} {k}: shared {a[k]!r} repeated {b[k]!r}")
            assert a[k] == b[k], (s, k, a[k], b[k])
    for which, x, y in (("state_dict", new[1], old[1]), ("optimiser", new[2], old[2])):
        assert x.keys() == y.keys() and len(x) > 0
        bad = [k for k in x if not torch.equal(x[k], y[k])]
        assert not bad, (which, bad[:8])
    nbt = [v for k, v in new[1].items() if k.startswith("decoder") and k.endswith("num_batches_tracked")]
    assert nbt and all(int(v) == 8 * steps for v in nbt)          # eight decoder passes per step, counted as before


def test_hooked_decoder_takes_the_repeated_schedule():
    model, solver = make("fp32", 8, True, False)
    calls, inner = [], []
    model.decoder.register_forward_hook(lambda m, i, o: calls.append(tuple(o.shape)))
    model.decoder.main.sigmoid.register_forward_hook(lambda m, i, o: inner.append(1))
    assert not solver._shares_pass()
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev())
    for s in range(2):
        del calls[:], inner[:]
        solver.train_step(x, s)
        assert calls == [(16, 3, 64, 64)] * 4 and len(inner) == 4, calls    # four batched decoder calls per step
    # without hooks the same solver records the pass once: three decoder calls per step
    model2, solver2 = make("fp32", 8, True, False)
    assert solver2._shares_pass()
    n = []
    fwd = model2.decoder.forward
    model2.decoder.forward = lambda z: (n.append(1), fwd(z))[1]
    solver2.train_step(x, 0)
    assert len(n) == 3


# (id, (B per group, C, H, W), pool, planes format or 0, forward path, workspace: "full" | "one")
REPLAY_CASES = [
    ("sliced-fold", (64, 64, 64, 64), 0, F16, "SlicedFold", "full"),
    ("one-block", (64, 256, 16, 16), 0, F16, "OneBlock", "full"),
    ("one-block-pool", (64, 512, 8, 8), 1, 2, "OneBlock", "full"),
    ("sliced-combine", (64, 128, 8, 8), 0, F16, "SlicedCombine", "full"),
    ("fallback-sliced", (16, 32, 16, 16), 0, 0, "Fallback", "full"),
    ("fallback-fused", (4, 6, 8, 8), 0, 0, "Fallback", "full"),
]


def _bn_forward(HF, x, par, bufs, G, pool, ns, momentum, shared=None):
    """One BnActFn forward over G groups; ``bufs`` = [running_mean, running_var, nbt] (entries may be None)."""
    import contextlib
    ctxm = shared.record() if shared is not None else contextlib.nullcontext()
    with ctxm:
        return HF.BnActFn.apply(x, par[0], par[1], None, bufs[0], bufs[1], bufs[2], 1e-5, momentum, 0.2, bool(pool), True,
                                None, ns, 0, True, True, G)


@pytest.mark.parametrize("momentum", [0.1, 1.0])
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("c", REPLAY_CASES, ids=[c[0] for c in REPLAY_CASES])
def test_replay_equals_second_forward(c, G, momentum):
    from hipvae import abi, functional as HF
    _, (B, C, H, W), pool, ns, path, _ws = c
    want = path if G == 1 or ns else "PerGroup"           # grouped calls without planes go out group by group
    assert abi.bn_plan_query(False, B, C, H, W, pool=pool, groups=G, planes=bool(ns), ns=ns)[0] == want
    g = torch.Generator().manual_seed(C + G)
    x = (torch.randn(G * B, C, H, W, generator=g) * 1.7 + 0.3).to(dev())
    par = [(torch.rand(C, generator=g) + 0.5).to(dev()), torch.randn(C, generator=g).to(dev())]
    start = [torch.randn(C, generator=g).to(dev()), (torch.rand(C, generator=g) + 0.5).to(dev()),
             torch.tensor(7, dtype=torch.int64, device=dev())]
    for null in (None, 0, 1):                               # all buffers | no running_mean | no running_var
        twice = [None if i == null else t.clone() for i, t in enumerate(start)]
        y1 = _bn_forward(HF, x, par, twice, G, pool, ns, momentum)
        _bn_forward(HF, x, par, twice, G, pool, ns, momentum)
        once = [None if i == null else t.clone() for i, t in enumerate(start)]
        sp = HF.SharedPass()
        y2 = _bn_forward(HF, x, par, once, G, pool, ns, momentum, shared=sp)
        assert torch.equal(y1, y2) and len(sp.records) == 1
        sp.replay()
        torch.cuda.synchronize()
        for a, b, name in zip(once, twice, ("running_mean", "running_var", "num_batches_tracked")):
            if a is not None:
                assert torch.equal(a, b), (c[0], G, momentum, null, name, float((a - b).abs().max()))
        assert int(once[2]) == 7 + 2 * G
        sp.replay()                                         # a second replay == a third forward; one table, reused
        _bn_forward(HF, x, par, twice, G, pool, ns, momentum)
        torch.cuda.synchronize()
        assert all(a is None or torch.equal(a, b) for a, b in zip(once, twice)) and len(sp._tables) == 1


def test_replay_per_group_and_tile_stats_paths():
    """The two paths BnActFn does not reach on its own: a grouped call with one group's workspace (PerGroup with planes)
    and the statistics from a conv epilogue's tile sums (TileStats), straight through the C ABI."""
    from hipvae import abi, functional as HF
    from hipvae.abi import call, lib, ptr, stream
    B, C, H, W, G = 16, 64, 32, 32, 2
    ws1 = lib.itcv_bn_workspace(B, C, H * W)
    assert abi.bn_plan_query(False, B, C, H, W, groups=G, planes=True, ns=2, ws_bytes=ws1)[0] == "PerGroup"
    assert abi.bn_plan_query(False, B, C, H, W, planes=True, ns=2, tile_stats=True)[0] == "TileStats"
    g = torch.Generator().manual_seed(5)
    x = torch.randn(G * B, C, H, W, generator=g).to(dev())
    gamma, beta = torch.ones(C, device=dev()), torch.zeros(C, device=dev())
    pstride = G * B * (C // 8) * H * W

    def fwd(bufs, uvar, mean, groups, tiles=None, xx=x):
        rstd = torch.empty_like(mean)
        y = torch.empty_like(xx)
        yp = torch.empty(lib.itcv_planes_bytes(xx.shape[0], C, H * W, 2) // 4, dtype=torch.int32, device=dev())
        ws = torch.empty(ws1, dtype=torch.uint8, device=dev())
        call("itcv_bn_train_fwd_uv", ptr(xx), ptr(gamma), ptr(beta), None, ptr(y), ptr(yp), 2, B, C, H, W,
             0.2, 0, 1e-5, 0.1, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(mean), ptr(rstd), ptr(uvar), ptr(ws), ws1,
             pstride if groups > 1 else 0, ptr(tiles), 0 if tiles is None else tiles.shape[2],
             0 if tiles is None else tiles.shape[2], groups, stream())

    def fresh():
        return [torch.zeros(C, device=dev()), torch.ones(C, device=dev()), torch.zeros((), dtype=torch.int64, device=dev())]

    # PerGroup
    twice, once = fresh(), fresh()
    mean, uvar = torch.empty(G, C, device=dev()), torch.empty(G, C, device=dev())
    fwd(twice, None, torch.empty(G, C, device=dev()), G)
    fwd(twice, None, torch.empty(G, C, device=dev()), G)
    fwd(once, uvar, mean, G)
    HF.replay_bn_running([(once[0], once[1], once[2], mean, uvar, 0.1)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(once, twice))
    # TileStats: per-tile sums of one group's x, 256 consecutive (image, pixel) positions per tile
    x1 = x[:B].contiguous()
    t = x1.permute(1, 0, 2, 3).reshape(C, -1, 256)
    tiles = torch.stack([t.sum(-1), (t * t).sum(-1)]).contiguous()
    twice, once = fresh(), fresh()
    mean, uvar = torch.empty(1, C, device=dev()), torch.empty(1, C, device=dev())
    fwd(twice, None, torch.empty(1, C, device=dev()), 1, tiles, x1)
    fwd(twice, None, torch.empty(1, C, device=dev()), 1, tiles, x1)
    fwd(once, uvar, mean, 1, tiles, x1)
    HF.replay_bn_running([(once[0], once[1], once[2], mean, uvar, 0.1)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(once, twice))


def test_replay_after_sync_bn_finalize():
    """itcv_bn_finalize_uv (the Sync-BN finalisation) exports the same float: replay == a second finalisation."""
    from hipvae import functional as HF
    from hipvae.abi import call, ptr, stream
    C = 300
    g = torch.Generator().manual_seed(9)
    v = torch.randn(4096, C, generator=g, dtype=torch.float64) * 3 + 1
    sums = torch.cat([v.sum(0), (v * v).sum(0)]).to(dev())

    def fin(bufs, mean, uvar):
        rstd = torch.empty(C, device=dev())
        call("itcv_bn_finalize_uv", ptr(sums), 4096.0, 1e-5, 0.1, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(mean),
             ptr(rstd), ptr(uvar), C, stream())

    def fresh():
        return [torch.full((C,), 0.25, device=dev()), torch.full((C,), 0.9, device=dev()),
                torch.ones((), dtype=torch.int64, device=dev())]

    twice, once = fresh(), fresh()
    mean, uvar = torch.empty(1, C, device=dev()), torch.empty(1, C, device=dev())
    fin(twice, torch.empty(C, device=dev()), None)
    fin(twice, torch.empty(C, device=dev()), None)
    fin(once, mean, uvar)
    HF.replay_bn_running([(once[0], once[1], once[2], mean, uvar, 0.1)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(once, twice)) and int(once[2]) == 3
