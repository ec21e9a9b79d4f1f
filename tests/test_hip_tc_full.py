"""The full beta-TC decomposition loss (solvers/tc.py:91-144) on the MI355X: ``ops.tc_full_loss`` forward and backward
against the unmodified reference (tests/golden/tc_full.npz, made by make_golden_tc_full.py), the 512 x 128 batch as 8
data-parallel shards, general (alpha, beta, gamma) against fp64 autograd, bitwise reproducibility and graph replay, and
the solvers trained with ``kl_loss="full"`` against the reference's own override of ``compute_kl_loss``
(tests/golden/steps_tc_full.npz), the CPU oracle and a 2-process data-parallel step."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)


def dev():
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.asarray(a))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def latent(tag):
    src = "ops_c4.npz" if tag == "d" else "ops.npz"
    g = np.load(os.path.join(GOLDEN, src))
    B, D, N = (int(v) for v in g[f"{tag}_BDN"])
    return [T(g[f"{tag}_{k}"]).to(dev()) for k in ("z", "mu", "logvar")], N


# ---- 1. the op against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_op_against_reference_golden(tag):
    import ops
    G = np.load(os.path.join(GOLDEN, "tc_full.npz"))
    (z, mu, lv), N = latent(tag)
    st = int(G[f"{tag}_stride"])
    for beta, bt in ((512.0, "512p0"), (0.5, "0p5"), (1.0, "1p0")):
        zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, lv))
        loss = ops.tc_full_loss(zz, mm, ll, N, beta=beta)
        loss.backward()
        p = f"{tag}_b{bt}"
        assert loss.shape == () and rel_err(loss, T(G[p])) < 1e-4, p
        for k, t in (("dz", zz), ("dmu", mm), ("dlogvar", ll)):
            assert rel_err(t.grad.reshape(-1)[::st], T(G[f"{p}_{k}"])) < 1e-4, (p, k)
    zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, lv))
    rows = ops.tc_full_loss(zz, mm, ll, N, beta=512.0, reduce="none")
    assert rows.shape == (z.shape[0],) and rel_err(rows, T(G[f"{tag}_w_rows"])) < 1e-4
    (T(G[f"{tag}_w"]).to(dev()) * rows).sum().backward()
    for k, t in (("dz", zz), ("dmu", mm), ("dlogvar", ll)):
        assert rel_err(t.grad.reshape(-1)[::st], T(G[f"{tag}_w_{k}"])) < 1e-4, (tag, k)
    # the reference's quirk: only "mean" reduces
    assert ops.tc_full_loss(z, mu, lv, N, reduce="sum").shape == (z.shape[0],)


def test_c4_eight_shards_against_golden():
    """The 512 x 128 batch (N = 10000) as 8 shards of 64 rows, each with the whole batch's (mu, logvar) and its global
    row offset -- what each rank of an 8-GPU run computes.  The shards' gradients with respect to the shared column
    operands add up (the reduce-scatter)."""
    import ops
    G = np.load(os.path.join(GOLDEN, "tc_full.npz"))
    (z, mu, lv), N = latent("d")
    assert (z.shape, N) == ((512, 128), 10000)
    R, Bl, st = 8, 64, int(G["d_stride"])

    def sharded(zz, mm, ll, beta, reduce):
        parts = [ops.tc_full_loss(zz[r * Bl:(r + 1) * Bl], None, None, N, beta=beta, reduce="none", mu_all=mm,
                                  logvar_all=ll, row_offset=r * Bl) for r in range(R)]
        rows = torch.cat(parts)
        return rows.mean() if reduce == "mean" else rows

    for beta, bt in ((512.0, "512p0"), (0.5, "0p5"), (1.0, "1p0")):
        zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, lv))
        loss = sharded(zz, mm, ll, beta, "mean")
        loss.backward()
        p = f"d_b{bt}"
        assert rel_err(loss, T(G[p])) < 1e-4, p
        for k, t in (("dz", zz), ("dmu", mm), ("dlogvar", ll)):
            assert rel_err(t.grad.reshape(-1)[::st], T(G[f"{p}_{k}"])) < 1e-4, (p, k)
    zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, lv))
    rows = sharded(zz, mm, ll, 512.0, "none")
    assert rel_err(rows, T(G["d_w_rows"])) < 1e-4
    (T(G["d_w"]).to(dev()) * rows).sum().backward()
    for k, t in (("dz", zz), ("dmu", mm), ("dlogvar", ll)):
        assert rel_err(t.grad.reshape(-1)[::st], T(G[f"d_w_{k}"])) < 1e-4, k


# ---- 2. general weights against fp64 autograd, bitwise reproducibility, graph replay --------------------------------
def oracle_rows(z, mu_all, lv_all, N, off, a, b, c):
    """Rows [off, off + len(z)) of a*mi + b*tc + c*dwkl of the global batch, from the oracle's building blocks."""
    from oracle import latent_math as lm
    Bl = z.shape[0]
    lcx = lm.log_density_plain(z, mu_all[off:off + Bl], lv_all[off:off + Bl]).sum(1)
    lpz = lm.log_density_plain(z, torch.zeros_like(z), torch.zeros_like(z)).sum(1)
    lp = lm.log_density_plain(z.unsqueeze(1), mu_all.unsqueeze(0), lv_all.unsqueeze(0))
    lw = lm.log_importance_weights(mu_all.shape[0], N, z.dtype)[off:off + Bl]
    prodm = torch.logsumexp(lw.unsqueeze(2) + lp, 1).sum(1)
    logqz = torch.logsumexp(lw + lp.sum(2), 1)
    return a * (lcx - logqz) + b * (logqz - prodm) + c * (prodm - lpz)


def clamped_inputs(B=48, D=70, seed=5):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(B, D, generator=g)
    lv = -2.0 + 2.0 * torch.randn(B, D, generator=g)
    z = mu + torch.randn(B, D, generator=g) * (0.5 * lv).exp()
    z[:4, :5] += 30.0                                     # elements far outside every component: the -50 clamp fires
    return z, mu, lv


@pytest.mark.parametrize("abc, reduce, packed", [((1.0, 4.0, 1.0), "mean", False), ((0.3, -2.0, 1.7), "none", True),
                                                 ((2.0, 0.5, 0.0), "mean", True)])
def test_general_weights_against_fp64_autograd(abc, reduce, packed):
    import ops
    from oracle import latent_math as lm
    a, b, c = abc
    z, mu, lv = clamped_inputs()
    B, D, N = z.shape[0], z.shape[1], 3000
    lp = lm.log_density_plain(z.double().unsqueeze(1), mu.double().unsqueeze(0), lv.double().unsqueeze(0))
    assert float((lp <= -50).double().mean()) > 1e-3                 # the clamp is active somewhere
    w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    zr, mr, lr = (t.double().requires_grad_(True) for t in (z, mu, lv))
    ref = oracle_rows(zr, mr, lr, N, 0, a, b, c)
    ref = ref.mean() if reduce == "mean" else ref
    (ref if reduce == "mean" else (w * ref).sum()).backward()
    zg = z.to(dev()).requires_grad_(True)
    if packed:             # the halves of one [B, 2D] tensor, as the data-parallel gather hands them over
        pk = torch.cat([mu, lv], 1).to(dev()).requires_grad_(True)
        mg, lg = pk[:, :D], pk[:, D:]
    else:
        mg, lg = mu.to(dev()).requires_grad_(True), lv.to(dev()).requires_grad_(True)
    got = ops.tc_full_loss(zg, mg, lg, N, a, b, c, reduce)
    assert rel_err(got, ref) < 1e-4
    (got if reduce == "mean" else (w.float().to(dev()) * got).sum()).backward()
    dmu, dlv = (pk.grad[:, :D], pk.grad[:, D:]) if packed else (mg.grad, lg.grad)
    assert rel_err(zg.grad, zr.grad) < 1e-4
    assert rel_err(dmu, mr.grad) < 1e-4
    assert rel_err(dlv, lr.grad) < 1e-4


def test_rows_of_a_shard_with_row_stride():
    """A shard's rows with the packed global (mu, logvar) equal the same rows of the full batch, bit for bit."""
    import ops
    z, mu, lv = (t.to(dev()) for t in clamped_inputs(B=40, D=33))
    full = ops.tc_full_loss(z, mu, lv, 700, 1.0, 3.0, 1.0, "none")
    pk = torch.cat([mu, lv], 1)
    part = ops.tc_full_loss(z[8:24], None, None, 700, 1.0, 3.0, 1.0, "none", mu_all=pk[:, :33], logvar_all=pk[:, 33:],
                            row_offset=8)
    assert torch.equal(part, full[8:24])


def _fwd_bwd(z, mu, lv, N):
    import ops
    zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, lv))
    loss = ops.tc_full_loss(zz, mm, ll, N, beta=6.0)
    loss.backward()
    return [loss.detach(), zz.grad, mm.grad, ll.grad]


def test_two_calls_bitwise_equal():
    (z, mu, lv), N = latent("c")
    a, b = _fwd_bwd(z, mu, lv, N), _fwd_bwd(z, mu, lv, N)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_replay_equals_eager():
    import ops
    (z, mu, lv), N = latent("b")
    eager = _fwd_bwd(z, mu, lv, N)
    zs, ms, ls = (t.clone().requires_grad_(True) for t in (z, mu, lv))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                # warm-up off the capture
        for _ in range(2):
            loss = ops.tc_full_loss(zs, ms, ls, N, beta=6.0)
            torch.autograd.grad(loss, (zs, ms, ls))
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = ops.tc_full_loss(zs, ms, ls, N, beta=6.0)
        grads = torch.autograd.grad(loss, (zs, ms, ls))
    with torch.no_grad():
        for t in (zs, ms, ls):
            t.mul_(0.5)
    graph.replay()
    with torch.no_grad():
        for t, v in zip((zs, ms, ls), (z, mu, lv)):
            t.copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager[0]) and all(torch.equal(g, e) for g, e in zip(grads, eager[1:]))


# ---- 3. the solvers -------------------------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


def load_steps():
    g = np.load(os.path.join(GOLDEN, "steps_tc_full.npz"))
    conv = np.load(os.path.join(GOLDEN, "steps_conv.npz"))
    init = {k[5:].replace("/", "."): T(conv[k]).clone() for k in conv.files if k.startswith("init:")}
    return g, conv, init


def draws_of(conv, name, s):
    n = len([k for k in conv.files if k.startswith(f"{name}:s{s}:draw")])
    return [T(conv[f"{name}:s{s}:draw{i}"]) for i in range(n)]


def build(init):
    import models
    m = models.SoftIntroVAE(arch="conv", **TINY)
    m.load_state_dict(init, strict=True)
    return m.to(dev()).train()


def make(name, model, hp, cls=None, **kw):
    from solvers.intro_tc import IntroTCSovler
    from solvers.tc import TCSovler
    cls = cls or (IntroTCSovler if name == "intro_tc" else TCSovler)
    args = [_DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
            torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1]]
    if name == "intro_tc":
        args += [hp[2], hp[3]]
    return cls(*args, dev(), False, None, clip=hp[4], **kw)


def run_steps(solver, conv, name, nsteps=2):
    import ops
    res = []
    for s in range(nsteps):
        with ops.noise_queue(draws_of(conv, name, s)):
            d = solver.train_step(T(conv[f"x{s}"]), s)
        res.append([d["loss_enc"], d["loss_dec"], d["loss_kl"], d["loss_rec"], d["L2"]])
    return res


def final_sample(g, init, name):
    bits = np.ascontiguousarray(g[f"{name}:final_xor"].T).view(np.uint32).reshape(-1)
    out, o = {}, 0
    for k in (str(k) for k in g["weight_keys"]):
        a = init[k].reshape(-1)[::4].numpy()
        out[k] = T((a.view(np.uint32) ^ bits[o:o + a.size]).view(np.float32))
        o += a.size
    assert o == bits.size
    return out


def check_final(g, init, name, sd):
    fin = final_sample(g, init, name)
    diffs = torch.cat([(sd[k].detach().cpu().reshape(-1)[::4] - v).abs() for k, v in fin.items()])
    upd = torch.cat([(v - init[k].reshape(-1)[::4]).abs() for k, v in fin.items()])
    assert float(diffs.max()) <= 2.05 * float(upd.max()), (name, float(diffs.max()), float(upd.max()))
    assert float(diffs.median()) < 0.01 * float(upd.max()), (name, float(diffs.median()), float(upd.max()))


@pytest.mark.parametrize("name", ["tc", "intro_tc"])
def test_solver_full_hook_against_reference_steps(name):
    g, conv, init = load_steps()
    hp = g["hp"]
    model = build(init)
    solver = make(name, model, hp, kl_loss="full")
    res = run_steps(solver, conv, name)
    for s in range(2):
        np.testing.assert_allclose(res[s], g[f"{name}:s{s}:dict"], rtol=1e-4 if s == 0 else 1e-3, err_msg=f"{name} s{s}")
    check_final(g, init, name, model.state_dict())
    # the simple hook gives other losses on the same data: the option is live
    model2 = build(init)
    res2 = run_steps(make(name, model2, hp), conv, name, 1)
    assert abs(res2[0][2] - res[0][2]) > 1e-3 * abs(res[0][2])


@pytest.mark.parametrize("name", ["tc", "intro_tc"])
def test_override_path_bitwise_equals_keyword(name):
    """A user subclass that overrides compute_kl_loss to call _compute_kl_loss_full (the reference's extension point)
    trains exactly as kl_loss="full"."""
    from solvers.intro_tc import IntroTCSovler
    from solvers.tc import TCSovler
    base = IntroTCSovler if name == "intro_tc" else TCSovler

    class Override(base):
        def compute_kl_loss(self, z, mu, logvar, reduce="mean", beta=None, write=False):
            return TCSovler._compute_kl_loss_full(self, z, mu, logvar, reduce, beta, write)

    g, conv, init = load_steps()
    hp = g["hp"]
    m1, m2 = build(init), build(init)
    r1 = run_steps(make(name, m1, hp, kl_loss="full"), conv, name)
    r2 = run_steps(make(name, m2, hp, cls=Override), conv, name)
    assert r1 == r2
    s1, s2 = m1.state_dict(), m2.state_dict()
    assert all(torch.equal(s1[k], s2[k]) for k in s1)


def test_graph_key_holds_the_mode():
    """A captured step replays the hook it was captured with: switching kl_loss re-captures, and the captured
    trajectory follows the eager one through both switches."""
    g, conv, init = load_steps()
    hp = g["hp"]
    xs = [T(conv["x0"]).to(dev()), T(conv["x1"]).to(dev())]
    modes = ["simple"] * 4 + ["full"] * 3 + ["simple"] * 2

    def trajectory(graph):
        model = build(init)
        solver = make("intro_tc", model, hp)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], set()
        for k, mode in enumerate(modes):
            solver.kl_loss = mode
            res.append(solver.train_step(xs[k % 2], k))
            if graph and solver._graph is not None:
                keys.add(solver._graph_key)
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), keys

    (e, we, _), (gr, wg, keys) = trajectory(False), trajectory(True)
    assert {k[-1] for k in keys} == {"simple", "full"}, keys
    for x, y in zip(e, gr):
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((we - wg).abs().max()) < 1e-6


C2 = dict(cdim=3, zdim=128, channels=(64, 128, 256, 512), image_size=64)


def test_f16x3_step_vs_oracle_full_hook():
    """One intro-TC step with kl_loss="full" at the benchmark shape (64x64x3, z=128, B=8) in the f16x3 arithmetic
    against an oracle Trainer whose kl_loss is the full formula, on identical weights and draws, at STEP_TOL."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import models
    from oracle import latent_math as lm
    from oracle.network import Net
    from oracle.steps import Trainer
    from step_trace import STEP_TOL, compare_traces, traced_hip_step, traced_oracle_step

    class FullTrainer(Trainer):
        def kl_loss(self, z, mu, logvar, reduce="mean", beta=None):
            beta = self.beta_kl if beta is None else beta
            mi, tc, dw = lm.decomposition(z, mu, logvar, self.n)
            if reduce == "mean":
                mi, tc, dw = mi.mean(), tc.mean(), dw.mean()
            out = mi + beta * tc + dw
            self.trace.setdefault("kl", []).append(out.detach().reshape(-1).clone())
            return out

    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **C2).state_dict().items()}
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    draws = [torch.randn(8, 128, generator=g) for _ in range(6)]
    ref = {}
    for name, dt in (("o32", torch.float32), ("o64", torch.float64)):
        st = {k: (v.clone().to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
        tr = FullTrainer("intro_tc", Net("conv", state=st, **C2), dataset_size=10000, beta_kl=0.5, beta_rec=0.75,
                         beta_neg=512.0, gamma_r=1e-8, clip=100.0, lr=2e-4)
        ref[name] = traced_oracle_step(tr, x.to(dt), [t.to(dt) for t in draws])
    model = models.SoftIntroVAE(arch="conv", **C2)
    model.load_state_dict(sd)
    model = model.to(dev()).train()
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]

    class DS:
        def __len__(self):
            return 10000

    from solvers.intro_tc import IntroTCSovler
    solver = IntroTCSovler(DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
                           torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1], hp[2], hp[3],
                           dev(), False, None, clip=hp[4], kl_loss="full")
    solver.conv_math = "f16x3"
    got = traced_hip_step(solver, model, x, [t.clone() for t in draws])
    d, r = got["dict"], ref["o32"]["dict"]
    for k in ("loss_enc", "loss_dec", "loss_kl", "loss_rec", "L2"):
        assert abs(d[k] - r[k]) <= 1e-4 * abs(r[k]), (k, d[k], r[k])
    compare_traces(got, ref["o32"], ref["o64"], STEP_TOL["f16x3"], "f16x3")


# ---- 4. a data-parallel step ----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out):
    import torch.distributed as dist
    for p in (os.path.join(ROOT, "intro-tc-vae_amd"), ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ops
    from hipvae import ddp
    ddp.init(sync_bn=True)
    g, conv, init = load_steps()
    hp = g["hp"]
    model = build(init)
    Bl = 8 // world
    sl = slice(rank * Bl, (rank + 1) * Bl)
    solver = make("intro_tc", model, hp, kl_loss="full")
    solver.batch_size = Bl
    res = []
    for s in range(2):
        draws = [t[sl] for t in draws_of(conv, "intro_tc", s)]
        with ops.noise_queue(draws):
            d = solver.train_step(T(conv[f"x{s}"])[sl], s)
        res.append([d["loss_enc"], d["loss_dec"], d["loss_kl"], d["loss_rec"], d["L2"]])
    fin = final_sample(g, init, "intro_tc")
    sd = model.state_dict()
    diffs = torch.cat([(sd[k].detach().cpu().reshape(-1)[::4] - v).abs() for k, v in fin.items()])
    upd = torch.cat([(v - init[k].reshape(-1)[::4]).abs() for k, v in fin.items()])
    out[rank] = dict(res=res, max=float(diffs.max()), upd=float(upd.max()), med=float(diffs.median()))
    ddp.shutdown()
    dist.destroy_process_group()


def test_ddp_two_process_step_against_reference():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    g = np.load(os.path.join(GOLDEN, "steps_tc_full.npz"))
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_dp_worker, args=(world, port, out), nprocs=world, join=True)
        res = dict(out)
    assert set(res) == {0, 1}
    for r in (0, 1):
        for s in range(2):
            np.testing.assert_allclose(res[r]["res"][s], g[f"intro_tc:s{s}:dict"], rtol=1e-4 if s == 0 else 1e-3)
        assert res[r]["max"] <= 2.05 * res[r]["upd"] and res[r]["med"] < 0.01 * res[r]["upd"]
    assert res[0]["res"] == res[1]["res"]
