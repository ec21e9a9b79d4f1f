"""GPU tests of the DIP-VAE KL hook (csrc/dip.hip, ops.dip_kl_loss, solvers/dip.py) against the fp64 restatement
tests/dip_ref.py.

Bounds, all normwise: the loss and each of the three terms relative to the fp64 value, each gradient tensor (and W) as
max |err| / max |value|.  The ceiling is the project's fp32 bar, 1e-4; a quantity whose fp64 value is exactly zero (the
off-diagonal term at D = 1, dlogvar of kind I without KL) must come out exactly zero.  With fp64 accumulation the kernels
stay orders of magnitude below the ceiling.  Worst values measured on an MI355X over every case of
test_kernel_against_restatement (printed by it):

    no figure recorded yet
"""
import os

import numpy as np
import pytest
import torch

import dip_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
KIND_NO = {"i": 1, "ii": 2}
# the issue's shapes, then the edges of the kernels' tiles -1 / 0 / +1 in both dimensions: C is tiled 32 x 32 over rows
# staged 64 at a time (forward), the gradient 16 rows x 64 columns over chunks of 32 (backward)
SHAPES = [(2, 1), (2, 3), (3, 64), (35, 10), (64, 128), (33, 130), (65, 65), (512, 128), (16, 300), (7, 512),
          (63, 31), (64, 32), (65, 33), (15, 63), (16, 64), (17, 65)]
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "dip.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def case(golden, Bt, D, kind):
    """The stored inputs of a shape and the restatement's values, computed once per (shape, kind) and never modified."""
    key = (Bt, D, kind)
    if key not in _CASES:
        p = f"{Bt}x{D}:{kind}:"
        lam_od, lam_d, beta = (float(v) for v in golden["hp"])
        mu, lv = R.make_inputs(Bt, D, int(golden[p + "seed"]))
        assert np.array_equal(golden[p + "checksum"], [mu.astype(np.float64).sum(), lv.astype(np.float64).sum()])
        ref = R.dip(mu, lv, kind, lam_od, lam_d, beta)
        assert abs(ref["loss"] - float(golden[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        for a in (mu, lv, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _CASES[key] = dict(mu=mu, lv=lv, ref=ref, hp=(lam_od, lam_d, beta))
    return _CASES[key]


def layouts(mu, lv, layout):
    """(mu_all, logvar_all) device tensors holding the values of ``mu`` / ``lv`` as leaves of the given layout."""
    Bt, D = mu.shape
    if layout == "dense":
        return G(mu), G(lv)
    if layout == "packed":            # the halves of one [Bt, 2D] tensor, inside nan rows that must not be read
        buf = np.full((Bt + 2, 2 * D), np.nan, dtype=np.float32)
        buf[1:-1, :D], buf[1:-1, D:] = mu, lv
        t = G(buf)[1:-1]
        a, b = t[:, :D], t[:, D:]
        assert Bt == 1 or a.stride() == (2 * D, 1)
        return a, b
    if layout == "strided":           # the right parts of wider nan tensors, as tests/test_hip_udr.py's strided()
        out = []
        for x in (mu, lv):
            wide = np.full((Bt, D + 3), np.nan, dtype=np.float32)
            wide[:, 3:] = x
            out.append(G(wide)[:, 3:])
        assert out[0].stride() == (D + 3, 1)
        return tuple(out)
    raise ValueError(layout)


def run(mu, lv, kind, lam_od, lam_d, beta, off=0, Bl=None, layout="dense", g=1.0):
    """loss, terms, W and both gradients of ops.dip_kl_loss on the device (W from the same forward entry)."""
    import ops
    from hipvae import functional as HF
    Bt, D = mu.shape
    Bl = Bt - off if Bl is None else Bl
    a, b = layouts(mu, lv, layout)
    a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    local = a[off:off + Bl]
    loss, terms = ops.dip_kl_loss(local, b[off:off + Bl], beta, lam_od, lam_d, kind, mu_all=a, logvar_all=b,
                                  row_offset=off, with_terms=True)
    assert not terms.requires_grad and loss.shape == () and terms.shape == (3,)
    dmu, dlv = torch.autograd.grad(loss * g if g != 1.0 else loss, (a, b))
    W = HF.dip_kl_forward(a.detach(), b.detach(), Bl, off, KIND_NO[kind], lam_od, lam_d, beta)[5]
    if layout == "packed" and Bt > 1:     # the gradients come back as the halves of one packed tensor
        assert dmu.stride() == dlv.stride() == (2 * D, 1) and dlv.data_ptr() == dmu.data_ptr() + 4 * D
    return dict(loss=loss.detach(), terms=terms, W=W, dmu=dmu, dlv=dlv)


def errors(got, ref):
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
    return dict(loss=rel(N(got["loss"]), ref["loss"]), kl=rel(t[0], ref["terms"][0]), offdiag=rel(t[1], ref["terms"][1]),
                diag=rel(t[2], ref["terms"][2]), W=rel(N(got["W"]), ref["W"]), dmu=rel(N(got["dmu"]), ref["dmu"]),
                dlogvar=rel(N(got["dlv"]), ref["dlogvar"]))


def check(got, ref, tag):
    e = errors(got, ref)
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= BAR, (tag, k, v)
    return e


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("Bt, D", SHAPES)
def test_kernel_against_restatement(golden, Bt, D, kind):
    c = case(golden, Bt, D, kind)
    lam_od, lam_d, beta = c["hp"]
    dense = run(c["mu"], c["lv"], kind, lam_od, lam_d, beta)
    check(dense, c["ref"], f"[{Bt}x{D} {kind} dense]")
    # the same bits from the packed pair read in place and from strided views (copied dense by the binding): the nan
    # around them is not read
    for layout in ("packed", "strided"):
        other = run(c["mu"], c["lv"], kind, lam_od, lam_d, beta, layout=layout)
        for k in dense:
            assert torch.equal(dense[k], other[k]), (layout, k)
    p = f"{Bt}x{D}:{kind}:"
    if p + "dmu" in golden:               # the stored expected values themselves
        assert np.abs(N(dense["dmu"]) - golden[p + "dmu"]).max() <= BAR * np.abs(golden[p + "dmu"]).max()
        assert np.abs(N(dense["W"]) - golden[p + "W"]).max() <= BAR * np.abs(golden[p + "W"]).max()
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("Bt, D, off, Bl", [(35, 10, 7, 5), (65, 65, 64, 1), (33, 130, 0, 16), (64, 128, 48, 16)])
def test_local_rows_and_upstream_gradient(golden, Bt, D, off, Bl, kind):
    """The KL of a rank's rows only, its gradient on those rows only, and an upstream gradient other than 1."""
    c = case(golden, Bt, D, kind)
    ref = R.dip(c["mu"], c["lv"], kind, 2.0, 5.0, 1.5, off, Bl)
    check(run(c["mu"], c["lv"], kind, 2.0, 5.0, 1.5, off, Bl), ref, f"[{Bt}x{D} {kind} rows {off}+{Bl}]")
    got = run(c["mu"], c["lv"], kind, 2.0, 5.0, 1.5, off, Bl, layout="packed", g=-0.375)
    ref = dict(ref, dmu=-0.375 * ref["dmu"], dlogvar=-0.375 * ref["dlogvar"])
    check(got, ref, f"[{Bt}x{D} {kind} rows {off}+{Bl} g=-0.375 packed]")


# ---- 2. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("Bt, D", [(64, 128), (33, 130), (7, 512), (512, 128)])
def test_bitwise_reproducible_and_independent_of_the_split(golden, Bt, D, kind):
    c = case(golden, Bt, D, kind)
    lam_od, lam_d, beta = c["hp"]
    a = run(c["mu"], c["lv"], kind, lam_od, lam_d, beta)
    b = run(c["mu"], c["lv"], kind, lam_od, lam_d, beta)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # another row_offset / Bl split of the KL part: W and the regulariser's terms keep their bits, and so does the
    # gradient of every row that is local in neither split; without the KL (coef_kl = 0) nothing changes at all
    off, Bl = Bt // 4, max(Bt // 4, 1)
    s = run(c["mu"], c["lv"], kind, lam_od, lam_d, beta, off, Bl)
    assert torch.equal(a["W"], s["W"]) and torch.equal(a["terms"][1:], s["terms"][1:])
    full = run(c["mu"], c["lv"], kind, lam_od, lam_d, beta, 0, off)           # rows [0, off) local
    outside = slice(off + Bl, Bt)
    assert torch.equal(full["dmu"][outside], s["dmu"][outside]) and torch.equal(full["dlv"][outside], s["dlv"][outside])
    r0 = run(c["mu"], c["lv"], kind, lam_od, lam_d, 0.0)
    r1 = run(c["mu"], c["lv"], kind, lam_od, lam_d, 0.0, off, Bl)
    for k in ("loss", "W", "dmu", "dlv"):
        assert torch.equal(r0[k], r1[k]), k
    assert torch.equal(r0["terms"][1:], r1["terms"][1:])
    assert torch.equal(r0["W"], r0["W"].t())


# ---- 3. shard algebra on one GPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_shard_algebra(kind):
    """8 shards of 8 rows of one global batch (Bt = 64, D = 16), the same gathered pair on every "rank": the mean over
    the shards of the loss and of the gradients is the single-rank loss and gradient -- what the reduce-scatter adjoint
    and the gradient average of a data-parallel step compute."""
    mu, lv = R.make_inputs(64, 16, seed=77)
    lam_od, lam_d, beta = 3.0, 7.0, 0.5
    ref = R.dip(mu, lv, kind, lam_od, lam_d, beta)
    one = run(mu, lv, kind, lam_od, lam_d, beta)
    shards = [run(mu, lv, kind, lam_od, lam_d, beta, 8 * r, 8, layout="packed") for r in range(8)]
    mean = dict(loss=torch.stack([s["loss"].double() for s in shards]).mean(),
                terms=torch.stack([s["terms"].double() for s in shards]).mean(0), W=shards[0]["W"],
                dmu=torch.stack([s["dmu"].double() for s in shards]).mean(0),
                dlv=torch.stack([s["dlv"].double() for s in shards]).mean(0))
    check(one, ref, f"[shards {kind} single rank]")
    check(mean, ref, f"[shards {kind} mean of 8]")
    for s in shards:                       # every rank sees the same regulariser
        assert torch.equal(s["W"], one["W"]) and torch.equal(s["terms"][1:], one["terms"][1:])
    e = errors(mean, dict(loss=float(one["loss"]), terms=N(one["terms"]), W=N(one["W"]), dmu=N(one["dmu"]),
                          dlogvar=N(one["dlv"])))
    assert max(e.values()) <= BAR, e


# ---- 4. the parts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_kl_and_regulariser_parts(golden, kind):
    import ops
    c = case(golden, 35, 10, kind)
    beta, lam_od, lam_d = 0.75, 3.0, 7.0

    def grads(fn):
        a, b = G(c["mu"]).requires_grad_(True), G(c["lv"]).requires_grad_(True)
        out = fn(a, b)
        return (out.detach(),) + torch.autograd.grad(out, (a, b), allow_unused=True)

    def close(x, y, tag):
        x, y = N(x), N(y)
        err = np.abs(x - y).max() / np.abs(y).max()
        print(tag, f"{err:.2e}")
        assert err <= BAR, (tag, err)

    whole = grads(lambda a, b: ops.dip_kl_loss(a, b, beta, lam_od, lam_d, kind))
    reg = grads(lambda a, b: ops.dip_regularizer(a, b, lam_od, lam_d, kind))
    kl = grads(lambda a, b: ops.kl_divergence(b, a, reduce="mean", scale=beta))
    close(whole[0], reg[0] + kl[0], "loss = regulariser + beta KL")
    close(whole[1], reg[1] + kl[1], "dmu")
    if kind == "i":
        assert not reg[2].any()            # kind I: the regulariser does not depend on logvar
    close(whole[2], reg[2] + kl[2], "dlogvar")
    plain = grads(lambda a, b: ops.dip_kl_loss(a, b, beta, 0.0, 0.0, kind))
    for x, y, tag in zip(plain, kl, ("beta KL", "its dmu", "its dlogvar")):
        close(x, y, "lambda = 0: " + tag)
    if kind == "i":
        # without a KL coefficient the KL's value does not reach the result: kind I never reads logvar
        lv_inf = c["lv"].copy()
        lv_inf[0, 0] = 100.0              # exp overflows fp32: the KL is infinite
        lone = grads(lambda a, b: ops.dip_regularizer(a, G(lv_inf).requires_grad_(True), lam_od, lam_d, kind))
        assert torch.equal(lone[0], reg[0]) and torch.equal(lone[1], reg[1])


# ---- 5. training steps against the oracle ----------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


def _oracle_trainer(name, state, kind, lam_od, lam_d, hp):
    from oracle import latent_math as lm
    from oracle.network import Net
    from oracle.steps import Trainer

    class DipTrainer(Trainer):
        """The oracle's step with the torch restatement of the DIP hook on every ``reduce="mean"`` call."""

        def kl_loss(self, z, mu, logvar, reduce="mean", beta=None):
            beta = self.beta_kl if beta is None else beta
            if reduce == "mean":
                out = R.torch_hook(mu, logvar, kind, lam_od, lam_d, beta)
            else:
                out = beta * lm.kl(logvar, mu, reduce)
            self.trace.setdefault("kl", []).append(out.detach().reshape(-1).clone())
            return out

    return DipTrainer(name, Net("conv", state={k: v.clone() for k, v in state.items()}, **TINY), dataset_size=1000,
                      beta_kl=hp[0], beta_rec=hp[1], beta_neg=hp[2], gamma_r=hp[3], clip=hp[4], lr=hp[5])


def _hip_solver(name, state, kind, lam_od, lam_d, hp):
    import models
    from solvers.dip import DIPSolver, IntroDIPSolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    args = [_DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
            torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1]]
    if name == "intro":
        args += [hp[2], hp[3]]
    cls = IntroDIPSolver if name == "intro" else DIPSolver
    solver = cls(*args, dev(), False, None, clip=hp[4], dip_type=kind, lambda_od=lam_od, lambda_d=lam_d)
    assert solver.conv_math == "fp32"
    return solver, model


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


@pytest.mark.parametrize("name, kind", [("vae", "i"), ("vae", "ii"), ("intro", "i"), ("intro", "ii")])
def test_two_steps_against_the_oracle(name, kind):
    """Two training steps of the tiny model (B = 8, fp32 arithmetic, recorded draws) against the CPU oracle whose KL hook
    is the torch restatement.  Tolerances: those of test_hip_model.py's run_golden_steps for this model -- the returned
    dict to 1e-4 at step 0 and 3e-4 at step 1, every hook output to 3e-4 / 3e-3 of its scale."""
    import ops
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    lam_od, lam_d = (2.0, 20.0) if kind == "i" else (50.0, 50.0)
    state = _init_state()
    tr = _oracle_trainer(name, state, kind, lam_od, lam_d, hp)
    solver, _ = _hip_solver(name, state, kind, lam_od, None, hp)           # lambda_d by the sweep convention
    assert solver.lambda_d == lam_d
    kl_log, kl0 = [], solver.compute_kl_loss
    solver.compute_kl_loss = lambda *a, _f=kl0, **k: (kl_log.append(_f(*a, **k)), kl_log[-1])[1]
    g = torch.Generator().manual_seed(1)
    nd = 6 if name == "intro" else 1
    keys = ("loss_enc", "loss_dec", "loss_kl", "loss_rec", "L2")
    for s in range(2):
        x = torch.rand(8, 3, 32, 32, generator=g)
        draws = [torch.randn(8, 10, generator=g) for _ in range(nd)]
        kl_log.clear()
        with ops.noise_queue([t.clone() for t in draws]):
            got = solver.train_step(x, s)
        ref = tr.step(x, draws)
        first = got if s == 0 else first
        print(name, kind, s, {k: (got[k], ref[k]) for k in keys})
        np.testing.assert_allclose([got[k] for k in keys], [ref[k] for k in keys], rtol=1e-4 if s == 0 else 3e-4)
        tol = 3e-4 if s == 0 else 3e-3
        assert len(kl_log) == len(tr.trace["kl"]) == (5 if name == "intro" else 1)
        for i, (t, want) in enumerate(zip(kl_log, tr.trace["kl"])):
            err = float((t.detach().reshape(-1).cpu() - want).abs().max())
            assert err < tol * float(want.abs().max()), (name, kind, s, i, err)
    # the regulariser is live: the same first step without it reports another KL term
    plain, _ = _hip_solver(name, state, kind, 0.0, 0.0, hp)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 3, 32, 32, generator=g)
    with ops.noise_queue([torch.randn(8, 10, generator=g) for _ in range(nd)]):
        d0 = plain.train_step(x, 0)
    assert abs(d0["loss_kl"] - first["loss_kl"]) > 1e-2 * abs(first["loss_kl"]), (d0["loss_kl"], first["loss_kl"])


# ---- 6. graph capture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "intro"])
def test_captured_steps_equal_eager_steps_and_lambda_recaptures(name):
    """With enable_graph() the trajectory follows the eager one from the same state through the capture; after
    ``lambda_od *= 2`` (and with it lambda_d, by the convention) it still does, which it could not if the step replayed
    the graph captured with the old values: the key re-captures."""
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    state = _init_state()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(8, 3, 32, 32, generator=gen).to(dev()) for _ in range(2)]

    def trajectory(graph):
        solver, model = _hip_solver(name, state, "i", 2.0, None, hp)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], []
        for k in range(9):
            if k == 6:
                solver.lambda_od *= 2
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8) else None)
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), keys

    (e, we, _), (gr, wg, keys) = trajectory(False), trajectory(True)
    def holds(key, triple):
        return key is not None and any(key[i:i + 3] == triple for i in range(len(key) - 2))

    assert holds(keys[3], ("i", 2.0, 20.0)) and keys[3] == keys[4] == keys[5]
    assert holds(keys[7], ("i", 4.0, 40.0)) and keys[7] == keys[8] != keys[5]
    for x, y in zip(e, gr):
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((we - wg).abs().max()) < 1e-6
    # the doubled regulariser is visible in the eager trajectory itself (the check above is not vacuous)
    assert abs(e[6]["loss_kl"] - e[5]["loss_kl"]) > 1e-2 * abs(e[5]["loss_kl"])
