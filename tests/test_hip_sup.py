"""GPU tests of the semi-supervised S2 family (csrc/sup.hip, ops.supervised_regularizer, solvers/semi.py,
hipvae.dataset.DeviceLabelledLoader) against the fp64 restatement tests/sup_ref.py.

Bounds, all normwise: the loss and the unweighted term relative to the fp64 value, the gradient as max |err| / max |value|.
The ceiling is the project's fp32 bar, 1e-4; whatever is exactly zero in fp64 (the gradient columns >= F under xent / l2,
cov at D = F = 1, everything under gamma = 0) must come out exactly zero.  With fp64 arithmetic inside, the kernels' only
error is the fp32 rounding of their outputs.  Worst values measured on an MI355X over every case of
test_kernel_against_restatement (printed by it):

    loss 5.47e-08   sup 5.52e-08   dmu 5.01e-08

test_step_equals_its_expression_tree: the flat gradients of the twelve steps within 1.6e-07 normwise, the returned dicts
in the seventh digit.  test_gamma_zero_step_equals_the_wrapped_step prints whether its match is bitwise: in that run it
was, for all four solvers (the test itself asserts the bar, not the bits).
"""
import os

import numpy as np
import pytest
import torch

import sup_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
# B_l around the four-rows-a-block edge, D and F at the lane / tile edges, F = D included; the cov tile is 32 x 32 over rows
# staged 64 at a time (forward), the gradient 16 rows x 64 columns over chunks of 32 factors (backward): -1 / 0 / +1 of each
SHAPES = [(1, 1, 1), (2, 3, 3), (5, 10, 7), (64, 128, 5), (33, 65, 64),
          (3, 63, 5), (4, 64, 64), (5, 65, 33), (65, 512, 64), (65, 64, 31), (4, 33, 32), (5, 32, 32), (3, 31, 31),
          (17, 33, 33), (16, 65, 1), (15, 63, 32), (64, 32, 31), (63, 512, 5)]
BIG = [(5, 10, 7), (65, 64, 64)]
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())             # a copy: the stored cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "sup.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def case(golden, B, D, F, kind, big=False):
    """The stored inputs of a shape and the restatement's values, computed once per (shape, kind) and never modified."""
    key = (B, D, F, kind, big)
    if key not in _CASES:
        p = f"{'big:' if big else ''}{B}x{D}x{F}:{kind}:"
        gamma, scale = (float(v) for v in golden["hp"])
        mu, y, sizes = (R.make_big_inputs if big else R.make_inputs)(B, D, F, int(golden[p + "seed"]))
        assert np.array_equal(golden[p + "checksum"], [mu.astype(np.float64).sum(), y.astype(np.float64).sum()])
        ref = R.sup(mu, y, kind, sizes, gamma, scale)
        assert abs(ref["loss"] - float(golden[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        for a in (mu, y, ref["dmu"]):
            a.setflags(write=False)
        _CASES[key] = dict(mu=mu, y=y, sizes=sizes, ref=ref, hp=(gamma, scale))
    return _CASES[key]


def layouts(mu, y, layout):
    """(mu, labels) device tensors holding the given values as leaves of the given layout."""
    (B, D), F = mu.shape, y.shape[1]
    if layout == "dense":
        return G(mu), G(y)
    if layout == "strided":       # the row slice [B0:, :D] of a wider nan-filled [B0 + B, 2D] tensor; y likewise
        wide = np.full((3 + B, 2 * D), np.nan, dtype=np.float32)
        wide[3:, :D] = mu
        ywide = np.full((2 + B, F + 3), np.nan, dtype=np.float32)
        ywide[2:, :F] = y
        a, b = G(wide)[3:, :D], G(ywide)[2:, :F]
        assert B == 1 or (a.stride() == (2 * D, 1) and b.stride() == (F + 3, 1))
        assert a.storage_offset() == 3 * 2 * D
        return a, b
    raise ValueError(layout)


def run(mu, y, kind, sizes, gamma, scale, layout="dense", g=1.0):
    import ops
    a, b = layouts(mu, y, layout)
    a = a.detach().requires_grad_(True)
    loss, terms = ops.supervised_regularizer(a, b, kind, sizes if kind == "xent" else None, gamma=gamma, scale=scale,
                                             with_terms=True)
    assert not terms.requires_grad and loss.shape == () and terms.shape == (2,) and loss.dtype == torch.float32
    (dmu,) = torch.autograd.grad(loss * g if g != 1.0 else loss, (a,))
    assert dmu.shape == a.shape and dmu.dtype == torch.float32
    return dict(loss=loss.detach(), terms=terms, dmu=dmu)


def errors(got, ref, gamma):
    """Normwise errors of a run against the restatement; a quantity that is exactly zero there must be exactly zero."""
    def rel(x, want):
        x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
        scale = np.abs(want).max()
        if scale == 0.0:
            assert not x.any()
            return 0.0
        assert np.isfinite(x).all()
        return float(np.abs(x - want).max() / scale)

    t = N(got["terms"])
    assert t[1] == np.float32(gamma)
    zero = ref["dmu"] == 0.0
    assert not N(got["dmu"])[zero].any()
    return dict(loss=rel(N(got["loss"]), ref["loss"]), sup=rel(t[0], ref["sup"]), dmu=rel(N(got["dmu"]), ref["dmu"]))


def check(got, ref, gamma, tag):
    e = errors(got, ref, gamma)
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= BAR, (tag, k, v)
    return e


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B, D, F", SHAPES)
def test_kernel_against_restatement(golden, B, D, F, kind):
    c = case(golden, B, D, F, kind)
    gamma, scale = c["hp"]
    dense = run(c["mu"], c["y"], kind, c["sizes"], gamma, scale)
    check(dense, c["ref"], gamma, f"[{B}x{D}x{F} {kind} dense]")
    if kind != "cov" and F < D:
        assert not dense["dmu"][:, F:].any()
    # the same bits from a strided, offset slice read in place: the nan around it is not read
    other = run(c["mu"], c["y"], kind, c["sizes"], gamma, scale, layout="strided")
    for k in dense:
        assert torch.equal(dense[k], other[k]), k
    p = f"{B}x{D}x{F}:{kind}:"
    if p + "dmu" in golden:               # the stored expected values themselves
        assert np.abs(N(dense["dmu"]) - golden[p + "dmu"]).max() <= BAR * max(np.abs(golden[p + "dmu"]).max(), 1e-300)
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B, D, F", BIG)
def test_large_means_do_not_overflow(golden, B, D, F, kind):
    """|mu| up to 80: exp(80) is outside fp32, the softplus must not be evaluated that way."""
    c = case(golden, B, D, F, kind, big=True)
    assert np.abs(c["mu"]).max() == 80.0
    gamma, scale = c["hp"]
    got = run(c["mu"], c["y"], kind, c["sizes"], gamma, scale, layout="strided", g=-0.375)
    ref = dict(c["ref"], dmu=-0.375 * c["ref"]["dmu"])
    check(got, ref, gamma, f"[big {B}x{D}x{F} {kind} g=-0.375]")


# ---- 2. exact zeros ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_exact_zeros(golden, kind):
    c = case(golden, 5, 10, 7, kind)
    got = run(c["mu"], c["y"], kind, c["sizes"], 2.0, 1.25)
    if kind != "cov":
        assert not got["dmu"][:, 7:].any() and got["dmu"][:, :7].abs().min() > 0
    else:
        assert got["dmu"][:, 7:].any()                   # cov penalises the columns behind F too
    # gamma = 0: a zero loss and zero gradients, the logged term still the term
    zero = run(c["mu"], c["y"], kind, c["sizes"], 0.0, 1.25)
    assert float(zero["loss"]) == 0.0 and not zero["dmu"].any()
    assert torch.equal(zero["terms"][0], got["terms"][0]) and float(zero["terms"][1]) == 0.0
    gz = torch.zeros(1, dtype=torch.float64, device=dev())
    zero = run(c["mu"], c["y"], kind, c["sizes"], gz, 1.25)
    assert float(zero["loss"]) == 0.0 and not zero["dmu"].any()
    # cov at D = F = 1: the one entry of C is on the zeroed diagonal
    one = case(golden, 1, 1, 1, "cov")
    got = run(one["mu"], one["y"], "cov", None, 3.0, 1.0)
    assert float(got["loss"]) == 0.0 and float(got["terms"][0]) == 0.0 and not got["dmu"].any()
    mu, y, _ = R.make_inputs(9, 1, 1, seed=5)
    got = run(mu, y, "cov", None, 3.0, 1.0)
    assert float(got["loss"]) == 0.0 and not got["dmu"].any()


# ---- 3. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B, D, F", [(65, 512, 64), (33, 65, 64), (5, 10, 7)])
def test_bitwise_reproducible(golden, B, D, F, kind):
    c = case(golden, B, D, F, kind)
    gamma, scale = c["hp"]
    a = run(c["mu"], c["y"], kind, c["sizes"], gamma, scale)
    b = run(c["mu"], c["y"], kind, c["sizes"], gamma, scale)
    # other work queued in between: a large product on the same stream and one on a side stream
    side = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device=dev())
    with torch.cuda.stream(side):
        _ = big @ big
    _ = big @ big
    d = run(c["mu"], c["y"], kind, c["sizes"], gamma, scale)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], d[k]), k


# ---- 4. gamma on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_gamma_as_a_device_tensor(golden, kind):
    """The kernel reads the weight when it runs: new content, no other argument changed, another result -- and the same
    bits as the float of that value."""
    import ops
    c = case(golden, 5, 10, 7, kind)
    gt = torch.tensor([0.75], dtype=torch.float64, device=dev())
    ptr = gt.data_ptr()
    first = run(c["mu"], c["y"], kind, c["sizes"], gt, 1.25)
    as_float = run(c["mu"], c["y"], kind, c["sizes"], 0.75, 1.25)
    for k in first:
        assert torch.equal(first[k], as_float[k]), k
    gt.fill_(3.0)
    assert gt.data_ptr() == ptr
    second = run(c["mu"], c["y"], kind, c["sizes"], gt, 1.25)
    check(second, R.sup(c["mu"], c["y"], kind, c["sizes"], 3.0, 1.25), 3.0, f"[gamma on the device {kind}]")
    assert float(second["loss"]) != float(first["loss"]) and torch.equal(second["terms"][0], first["terms"][0])
    # the backward uses the weight the forward read, not what the tensor holds later
    a = G(c["mu"]).requires_grad_(True)
    loss = ops.supervised_regularizer(a, G(c["y"]), kind, c["sizes"] if kind == "xent" else None, gamma=gt, scale=1.25)
    gt.fill_(100.0)
    (dmu,) = torch.autograd.grad(loss, (a,))
    assert torch.equal(dmu, second["dmu"])
    with pytest.raises(ValueError, match="labels must be"):
        ops.supervised_regularizer(a, torch.from_numpy(c["y"]), "l2")
    with pytest.raises(ValueError, match="float64"):
        ops.supervised_regularizer(a, G(c["y"]), "l2", gamma=torch.ones(1, device=dev()))


# ---- 5. the step against its expression tree ---------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


HP = dict(beta_kl=0.5, beta_rec=0.75, lr=2e-4)
SIZES = (3, 6, 40, 10)
B_U = B_L = 8
SOLVERS = ("S2VAESolver", "S2TCSolver", "S2DIPSolver", "S2FactorSolver")


def _init_state():
    import models
    torch.manual_seed(0)
    vae = {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}
    disc = {k: v.clone() for k, v in models.Discriminator(TINY["zdim"], hidden=32, layers=3).state_dict().items()}
    return vae, disc


def _model(state):
    import models
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state[0])
    return model.to(dev()).train()


def _disc(state):
    import models
    disc = models.Discriminator(TINY["zdim"], hidden=32, layers=3)
    disc.load_state_dict(state[1])
    return disc.to(dev()).train()


def _solver(name, state, **kw):
    import solvers
    model = _model(state)
    if name.endswith("FactorSolver"):
        disc = _disc(state)
        kw.update(discriminator=disc, optimizer_disc=torch.optim.Adam(disc.parameters(), lr=1e-4, betas=(0.5, 0.9)))
    if name.endswith("DIPSolver"):
        kw.update(dip_type="ii", lambda_od=2.0, lambda_d=5.0)
    if name.startswith("S2"):
        kw.setdefault("factor_sizes", SIZES)
    solver = getattr(solvers, name)(_DS(), model, B_U, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                                    torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", HP["beta_kl"],
                                    HP["beta_rec"], dev(), False, None, clip=None, **kw)
    assert solver.conv_math == "fp32"
    return solver, model


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B_U + B_L, 3, 32, 32, generator=g)
    y = torch.stack([torch.randint(0, k, (B_L,), generator=g) for k in SIZES], dim=1).float()
    draws = [torch.randn(B_U, TINY["zdim"], generator=g) for _ in range(2)]       # the reparameterisation, FactorVAE's keys
    return x, y, draws


def _grads(model):
    out = []
    for p in model.parameters():
        out.append(torch.zeros(p.numel(), device=dev()) if p.grad is None else p.grad.detach().reshape(-1).clone())
    return torch.cat(out)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", SOLVERS)
def test_step_equals_its_expression_tree(name, kind):
    """One eager ``train_step`` against the same loss assembled from the public ops on the first B rows plus the term in
    plain torch fp64 on ``model.encode(x_l)[0]``: the returned dict and the flat gradients within the bar."""
    import ops
    from hipvae.functional import conv_math_scope
    state = _init_state()
    x, y, draws = _batch()
    ndraws = 2 if name == "S2FactorSolver" else 1
    gamma = 0.05
    solver, model = _solver(name, state, sup_kind=kind, gamma_sup=gamma, sup_scale=1.25)
    with ops.noise_queue([d.clone() for d in draws[:ndraws]]):
        got = solver.train_step((x, y), 0)
    grads = _grads(model)
    # the expression tree on a twin
    twin = _model(state)
    xd, yd = x.to(dev()), y.to(dev())
    with conv_math_scope("fp32"), ops.noise_queue([d.clone() for d in draws[:ndraws]]):
        mu, logvar, z, rec = twin(xd[:B_U])
        loss_rec = ops.reconstruction_loss(xd[:B_U], rec, "mse", "mean", scale=HP["beta_rec"])
        if name == "S2VAESolver":
            hook = ops.kl_divergence(logvar, mu, reduce="mean", scale=HP["beta_kl"])
        elif name == "S2TCSolver":
            hook = ops.tc_kl_loss(z, mu, logvar, 1000, HP["beta_kl"], "mean")
        elif name == "S2DIPSolver":
            hook = ops.dip_kl_loss(mu, logvar, HP["beta_kl"], 2.0, 5.0, "ii")
        else:
            disc = _disc(state)
            hook = ops.kl_divergence(logvar, mu, reduce="mean", scale=HP["beta_kl"]) + 10.0 * ops.factor_tc(
                z, disc, shared=ops.factor_pass(z, disc))
        mu_l = twin.encode(xd[B_U:])[0]
        sup = R.torch_sup(mu_l.double(), yd.double(), kind, SIZES, scale=1.25)
        loss_kl = hook + (gamma * sup).float()
        loss = solver.scale * (loss_rec + loss_kl)
        loss.backward()
    loss, loss_kl, loss_rec, sup = loss.detach(), loss_kl.detach(), loss_rec.detach(), sup.detach()
    want = dict(loss_enc=float(loss), loss_dec=float(loss), loss_kl=float(loss_kl), loss_rec=float(loss_rec),
                loss_sup=float(sup), gamma_sup=gamma)
    print(name, kind, {k: (got[k], want[k]) for k in want})
    assert got["L2"] is None and set(want) <= set(got)
    if name == "S2FactorSolver":
        assert {"loss_tc", "loss_disc", "disc_acc"} <= set(got)
    for k in want:
        assert abs(got[k] - want[k]) <= BAR * abs(want[k]), (k, got[k], want[k])
    assert want["loss_sup"] > 0
    ref = _grads(twin)
    err = float((grads - ref).abs().max() / ref.abs().max())
    print(name, kind, "flat gradients", err)
    assert err <= BAR, err
    assert solver.steps_taken == 1


@pytest.mark.parametrize("name", SOLVERS)
def test_gamma_zero_step_equals_the_wrapped_step(name):
    """With gamma_sup = 0 the returned loss_kl and loss_rec are those of the wrapped solver on the first B rows."""
    import ops
    state = _init_state()
    x, y, draws = _batch(2)
    ndraws = 2 if name == "S2FactorSolver" else 1
    s2, _ = _solver(name, state, gamma_sup=0.0)
    plain, _ = _solver(name[2:].replace("TCSolver", "TCSovler"), state)
    with ops.noise_queue([d.clone() for d in draws[:ndraws]]):
        got = s2.train_step((x, y), 0)
    with ops.noise_queue([d.clone() for d in draws[:ndraws]]):
        want = plain.train_step(x[:B_U], 0)
    print(name, "gamma_sup = 0:", {k: (got[k], want[k]) for k in ("loss_kl", "loss_rec")},
          "bitwise" if all(got[k] == want[k] for k in ("loss_kl", "loss_rec")) else "within the bar, not bitwise")
    for k in ("loss_kl", "loss_rec"):
        assert abs(got[k] - want[k]) <= BAR * abs(want[k]), (k, got[k], want[k])
    assert got["gamma_sup"] == 0.0 and got["loss_sup"] > 0.0


class _Recorder:
    def __init__(self):
        self.log = {}

    def add_scalar(self, tag, value, global_step=None):
        self.log[tag] = (float(value), global_step)

    def add_scalars(self, tag, values, global_step=None):
        self.log[tag] = ({k: float(v) for k, v in values.items()}, global_step)

    def add_images(self, tag, images, global_step=None):
        self.log[tag] = (tuple(images.shape), global_step)

    def flush(self):
        pass


@pytest.mark.parametrize("name", ["S2VAESolver", "S2FactorSolver"])
def test_writer_gets_the_record_sup_next_to_the_wrapped_records(name):
    import ops
    from utils import SingletonWriter
    x, y, draws = _batch(3)
    solver, _ = _solver(name, _init_state(), sup_kind="l2", gamma_sup=0.25)
    rec, sw = _Recorder(), SingletonWriter()
    saved = sw.writer, sw.cur_iter
    solver.writer = sw.writer = rec
    sw.cur_iter = 1
    try:
        with ops.noise_queue([d.clone() for d in draws[:2 if name == "S2FactorSolver" else 1]]):
            got = solver.train_step((x, y), 1)
    finally:
        sw.writer, sw.cur_iter = saved
    assert rec.log["sup"] == (dict(loss=got["loss_sup"], gamma=got["gamma_sup"]), 1) and got["gamma_sup"] == 0.25
    assert rec.log["losses"] == (dict(r_loss=got["loss_rec"], kl_loss=got["loss_kl"]), 1)
    assert "kl_loss_unscaled" in rec.log and "r_loss_unscaled" in rec.log
    if name == "S2FactorSolver":
        assert rec.log["factor"][0] == dict(tc=got["loss_tc"], d_loss=got["loss_disc"], d_acc=got["disc_acc"])


def test_batch_refusal_names_the_shapes():
    solver, _ = _solver("S2VAESolver", _init_state())
    x, y, _ = _batch()
    with pytest.raises(ValueError, match=r"y \[B_l, 4\]"):
        solver.train_step((x, y[:, :3]), 0)
    with pytest.raises(ValueError, match=r"x \[B \+ B_l, C, H, W\]"):
        solver.train_step(x, 0)


# ---- 6. graph capture --------------------------------------------------------------------------------------------------
def test_captured_steps_follow_the_schedule_in_one_graph():
    """``enable_graph()``, the "anneal" schedule with T = 4: three eager warm-up steps, then six steps that replay ONE
    captured graph while gamma_sup(t) moves; the eager twin is fed the same draws through ``ops.noise_queue`` (taken from
    the device generator under the same seed, which is what the captured step consumes).  Then a change of ``sup_kind``
    re-captures."""
    import ops
    state = _init_state()
    batches = [_batch(5)[:2], _batch(6)[:2]]
    batches = [(x.to(dev()), y.to(dev())) for x, y in batches]
    kw = dict(sup_kind="xent", gamma_sup=0.05, sup_schedule="anneal", sup_threshold=4)
    steps = 9

    captured, _ = _solver("S2VAESolver", state, **kw)
    captured.enable_graph()
    torch.cuda.manual_seed(1234)
    got = [captured.train_step(batches[k % 2], k) for k in range(steps)]
    assert len(captured._graphs) == 1 and captured._graph is not None
    key = captured._graph_key

    eager, _ = _solver("S2VAESolver", state, **kw)
    torch.cuda.manual_seed(1234)
    want = []
    for k in range(steps):
        draw = torch.randn((B_U, TINY["zdim"]), device=dev())
        with ops.noise_queue([draw]):
            want.append(eager.train_step(batches[k % 2], k))
    assert not hasattr(eager, "_graphs") or not eager._graphs
    for k, (a, b) in enumerate(zip(got, want)):
        sched = 0.05 * min(1.0, k / 4)
        print(k, a["gamma_sup"], sched, a["loss_kl"], b["loss_kl"], a["loss_sup"], b["loss_sup"])
        assert abs(a["gamma_sup"] - sched) <= 1e-6 * 0.05 and a["gamma_sup"] == b["gamma_sup"]
        for name in ("loss_enc", "loss_kl", "loss_rec", "loss_sup"):
            assert abs(a[name] - b[name]) <= BAR * abs(b[name]), (k, name, a[name], b[name])
    assert got[3]["gamma_sup"] < got[4]["gamma_sup"] == got[8]["gamma_sup"]        # it moved inside the one graph
    # another kind selects other kernels: one eager warm-up step under the new key, then a second graph
    captured.sup_kind = "l2"
    for k in range(steps, steps + 2):
        captured.train_step(batches[k % 2], k)
    assert len(captured._graphs) == 2 and captured._graph_key != key


# ---- 7. the loader -------------------------------------------------------------------------------------------------------
def _table():
    from hipvae.dataset import DeviceImageTable
    imgs = np.random.default_rng(3).integers(0, 256, size=(60, 8, 8), dtype=np.uint8)
    table = DeviceImageTable.from_arrays(imgs, None, dev())
    table.factor_sizes, table.latent_indices = [3, 1, 4, 5], [0, 2, 3]          # the second factor does not vary
    return table


def test_labelled_loader():
    from hipvae.dataset import DeviceLabelledLoader, factor_bases
    table = _table()
    B, Bl, NL = 8, 5, 7
    loader = DeviceLabelledLoader(table, B, labelled_batch_size=Bl, num_labelled=NL, seed=9)
    assert len(loader) == 7 and loader.factor_sizes == (3, 4, 5)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    bases = torch.tensor([factor_bases(table.factor_sizes)[c] for c in (0, 2, 3)], device=dev())
    epochs, seen = [], set()
    for _ in range(3):
        batches, unl = [], []
        for x, y in loader:
            assert x.shape == (B + Bl, 1, 8, 8) and x.dtype == torch.float32 and x.device == dev()
            assert y.shape == (Bl, 3) and y.dtype == torch.float32 and torch.equal(y, y.round())
            assert (y >= 0).all() and (y < torch.tensor([3.0, 4.0, 5.0], device=dev())).all()
            idx = (y.long() * bases).sum(1)
            # the labelled rows are exactly the table's images at the indices rebuilt from the labels
            assert torch.equal(x[B:], table.gather(idx))
            seen.update(idx.tolist())
            batches.append((x.clone(), y.clone()))
            unl.append(x[:B])
        assert len(batches) == 7
        # the unlabelled rows of an epoch are distinct images of the table (a permutation, drop_last)
        flat = torch.cat(unl).flatten(1)
        assert len({tuple(r) for r in (flat * 255).round().long().tolist()}) == 56
        epochs.append(batches)
    assert 1 <= len(seen) <= NL and seen <= set(loader.labelled_indices.tolist())
    assert len(set(loader.labelled_indices.tolist())) == NL
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(epochs[0], epochs[1]))
    again = DeviceLabelledLoader(table, B, labelled_batch_size=Bl, num_labelled=NL, seed=9)
    for ep in epochs:
        for (x, y), (x2, y2) in zip(ep, again):
            assert torch.equal(x, x2) and torch.equal(y, y2)
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state(dev()))
    other = next(iter(DeviceLabelledLoader(table, B, labelled_batch_size=Bl, num_labelled=NL, seed=10)))
    assert not torch.equal(other[0], epochs[0][0][0])
    sub = DeviceLabelledLoader(table, B, num_labelled=NL, factors=(3, 0), seed=9, pre_process=lambda x, y: (x * 2, y))
    x, y = next(iter(sub))
    assert sub.factor_sizes == (5, 3) and y.shape == (B, 2) and x.shape == (2 * B, 1, 8, 8)
    assert torch.equal(sub.labelled_indices, loader.labelled_indices) and float(x.max()) > 1.0


def test_labelled_loader_feeds_the_solver():
    from hipvae.dataset import DeviceImageTable, DeviceLabelledLoader
    imgs = np.random.default_rng(4).integers(0, 256, size=(60, 32, 32, 3), dtype=np.uint8)
    table = DeviceImageTable.from_arrays(imgs, None, dev())
    table.factor_sizes, table.latent_indices = [3, 1, 4, 5], [0, 2, 3]
    loader = DeviceLabelledLoader(table, 8, num_labelled=20, seed=1)
    solver, _ = _solver("S2VAESolver", _init_state(), factor_sizes=loader.factor_sizes, sup_kind="cov", gamma_sup=0.1)
    for k, batch in zip(range(2), loader):
        out = solver.train_step(batch, k)
        assert np.isfinite(out["loss_enc"]) and out["loss_sup"] >= 0.0 and out["gamma_sup"] == np.float32(0.1)
