"""GPU tests of the MMD KL hook (csrc/mmd.hip, ops.mmd_kl_loss, solvers/mmd.py) against the fp64 restatement
tests/mmd_ref.py.

Bounds, all normwise: the loss and each of the five terms relative to the fp64 value, Wt, rs and each gradient tensor as
max |err| / max |value|.  The ceiling is the project's fp32 bar, 1e-4; a quantity whose fp64 value is exactly zero (the
KL gradients without a KL coefficient, dz without the statistic) must come out exactly zero.  The stored inputs keep
|MMD^2| >= 1e-2 of the largest of its three sums, so the relative bound on MMD^2 is a bound on the sums to 1e-6.  With
fp64 arithmetic throughout the kernels stay orders of magnitude below the ceiling.  Worst values measured on an MI355X
over every case of test_kernel_against_restatement (printed by it):

    loss 6.4e-08, mean KL 5.4e-08, MMD^2 5.0e-08, S_zz 5.4e-08, S_pp 3.8e-08, S_zp 5.4e-08, Wt 5.2e-08, rs 5.0e-15,
    dz 2.3e-07, dmu 5.6e-08, dlogvar 7.4e-08
"""
import os

import numpy as np
import pytest
import torch

import mmd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
# (Bt, P, D): the issue's shapes, then the edges -1 / 0 / +1 of the kernels' tiles.  Forward: strips of 32 points in Bt
# (row tile) and in P (column tile), D staged in chunks of 64 -> Bt, P in {31, 32, 33}, D in {63, 64, 65}.  Backward: 16
# rows x 64 columns of [Bt, D] over chunks of 32 of the Bt + P points -> Bt in {15, 16, 17}, D in {63, 64, 65}, Bt + P in
# {31, 32, 33}.  The finish folds rs 1024 rows a block -> Bt in {1024, 1025} (512 is below).
SHAPES = [(2, 2, 1), (2, 3, 3), (3, 2, 64), (35, 20, 10), (64, 64, 128), (33, 65, 130), (65, 64, 65), (512, 512, 128),
          (16, 16, 300), (7, 9, 512),
          (31, 33, 63), (32, 32, 64), (33, 31, 65), (15, 17, 64), (17, 15, 65), (16, 15, 9), (16, 17, 9), (1024, 3, 2),
          (1025, 2, 3)]
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())       # a copy: the stored cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "mmd.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def case(golden, Bt, P, D, kernel, h=None):
    """The stored inputs of a shape and the restatement's values, computed once per (shape, kernel, h) and never
    modified."""
    key = (Bt, P, D, kernel, h)
    if key not in _CASES:
        p = f"{Bt}x{P}x{D}:{kernel}:"
        lam, beta = (float(v) for v in golden["hp"])
        z, prior, mu, lv = R.make_inputs(Bt, P, D, int(golden[p + "seed"]))
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in (z, prior, mu, lv)])
        ref = R.mmd(z, prior, mu, lv, kernel, 2.0 * D if h is None else h, lam, beta)
        if h is None:
            assert abs(ref["loss"] - float(golden[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        assert abs(ref["terms"][1]) >= 1e-2 * ref["terms"][2:].max()
        for a in (z, prior, mu, lv, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _CASES[key] = dict(z=z, prior=prior, mu=mu, lv=lv, ref=ref, hp=(lam, beta))
    return _CASES[key]


def place(x, layout):
    """A device tensor holding the values of ``x``: dense, or the right part of a wider nan tensor that must not be read."""
    if layout == "dense":
        return G(x)
    wide = np.full((x.shape[0], x.shape[1] + 3), np.nan, dtype=np.float32)
    wide[:, 3:] = x
    t = G(wide)[:, 3:]
    assert t.stride() == (x.shape[1] + 3, 1)
    return t


def run(z, prior, mu, lv, kernel, lam, beta, h=None, layout="dense", g=1.0):
    """loss, terms, Wt, rs and the three gradients of ops.mmd_kl_loss on the device (Wt, rs from the same forward entry)."""
    import ops
    from hipvae import functional as HF
    D = z.shape[1]
    tz, tm, tl = (place(a, layout).detach().requires_grad_(True) for a in (z, mu, lv))
    tp = place(prior, layout).detach().requires_grad_(True)
    loss, terms = ops.mmd_kl_loss(tz, tm, tl, tp, beta, lam, kernel, h, with_terms=True)
    assert not terms.requires_grad and loss.shape == () and terms.shape == (5,)
    dz, dmu, dlv, dp = torch.autograd.grad(loss * g if g != 1.0 else loss, (tz, tm, tl, tp), allow_unused=True)
    assert dp is None                                   # the prior is a constant
    _, _, Wt, rs = HF.mmd_kl_forward(tz.detach(), tp.detach(), tm.detach(), tl.detach(), HF.MMD_KERNELS[kernel],
                                     2.0 * D if h is None else h, lam, beta)
    assert Wt.shape == (z.shape[0], z.shape[0] + prior.shape[0]) and rs.dtype == torch.float64
    return dict(loss=loss.detach(), terms=terms, Wt=Wt, rs=rs, dz=dz, dmu=dmu, dlv=dlv)


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
    e = dict(loss=rel(N(got["loss"]), ref["loss"]))
    for i, name in enumerate(("kl", "mmd2", "s_zz", "s_pp", "s_zp")):
        e[name] = rel(t[i], ref["terms"][i])
    for k, r in (("Wt", "Wt"), ("rs", "rs"), ("dz", "dz"), ("dmu", "dmu"), ("dlv", "dlogvar")):
        e[r] = rel(N(got[k]), ref[r])
    return e


def check(got, ref, tag):
    e = errors(got, ref)
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= BAR, (tag, k, v)
    return e


def same_bits(a, b, keys=None):
    for k in (a if keys is None else keys):
        assert torch.equal(a[k], b[k]), k


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("Bt, P, D", SHAPES)
def test_kernel_against_restatement(golden, Bt, P, D, kernel):
    c = case(golden, Bt, P, D, kernel)
    lam, beta = c["hp"]
    dense = run(c["z"], c["prior"], c["mu"], c["lv"], kernel, lam, beta)
    check(dense, c["ref"], f"[{Bt}x{P}x{D} {kernel} dense]")
    # the same bits from strided views (copied dense by the binding): the nan around them is not read
    same_bits(dense, run(c["z"], c["prior"], c["mu"], c["lv"], kernel, lam, beta, layout="strided"))
    A = dense["Wt"][:, :Bt]
    assert torch.equal(A, A.t()) and not torch.diagonal(A).any()
    p = f"{Bt}x{P}x{D}:{kernel}:"
    if p + "dz" in golden:                # the stored expected values themselves
        assert np.abs(N(dense["dz"]) - golden[p + "dz"]).max() <= BAR * np.abs(golden[p + "dz"]).max()
        assert np.abs(N(dense["Wt"]) - golden[p + "Wt"]).max() <= BAR * np.abs(golden[p + "Wt"]).max()
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("Bt, P, D", [(35, 20, 10), (33, 65, 130)])
def test_another_bandwidth(golden, Bt, P, D, kernel):
    c = case(golden, Bt, P, D, kernel, h=0.5 * D)
    lam, beta = c["hp"]
    check(run(c["z"], c["prior"], c["mu"], c["lv"], kernel, lam, beta, h=0.5 * D), c["ref"],
          f"[{Bt}x{P}x{D} {kernel} h = D / 2]")


# ---- 2. the parts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("Bt, P, D, Bl", [(35, 20, 10, 5), (65, 64, 65, 1), (33, 65, 130, 33)])
def test_local_rows_and_upstream_gradient(golden, Bt, P, D, Bl, kernel):
    """The KL of a rank's rows only (Bl need not be Bt) and an upstream gradient other than 1."""
    c = case(golden, Bt, P, D, kernel)
    mu, lv = c["mu"][:Bl], c["lv"][:Bl]
    ref = R.mmd(c["z"], c["prior"], mu, lv, kernel, 2.0 * D, 2.0, 1.5)
    check(run(c["z"], c["prior"], mu, lv, kernel, 2.0, 1.5), ref, f"[{Bt}x{P}x{D} {kernel} Bl {Bl}]")
    got = run(c["z"], c["prior"], mu, lv, kernel, 2.0, 1.5, layout="strided", g=-0.375)
    ref = dict(ref, dz=-0.375 * ref["dz"], dmu=-0.375 * ref["dmu"], dlogvar=-0.375 * ref["dlogvar"])
    check(got, ref, f"[{Bt}x{P}x{D} {kernel} Bl {Bl} g=-0.375 strided]")


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_kl_and_statistic_parts(golden, kernel):
    import ops
    c = case(golden, 35, 20, 10, kernel)
    beta, lam = 0.75, 3.0
    prior = G(c["prior"])

    def grads(fn, lv=None):
        z, mu = G(c["z"]).requires_grad_(True), G(c["mu"]).requires_grad_(True)
        lv = G(c["lv"] if lv is None else lv).requires_grad_(True)
        out = fn(z, mu, lv)
        return (out.detach(),) + torch.autograd.grad(out, (z, mu, lv), allow_unused=True)

    def close(x, y, tag):
        x, y = N(x), N(y)
        err = np.abs(x - y).max() / np.abs(y).max()
        print(tag, f"{err:.2e}")
        assert err <= BAR, (tag, err)

    whole = grads(lambda z, mu, lv: ops.mmd_kl_loss(z, mu, lv, prior, beta, lam, kernel))
    reg = grads(lambda z, mu, lv: ops.mmd_regularizer(z, prior, lam, kernel))
    kl = grads(lambda z, mu, lv: ops.kl_divergence(lv, mu, reduce="mean", scale=beta))
    assert reg[2] is None and reg[3] is None and kl[1] is None    # the regulariser reads z only, the KL never
    close(whole[0], reg[0] + kl[0], "loss = regulariser + beta KL")
    assert torch.equal(whole[1], reg[1])                         # dz does not depend on the KL at all
    close(whole[2], kl[2], "dmu")
    close(whole[3], kl[3], "dlogvar")
    plain = grads(lambda z, mu, lv: ops.mmd_kl_loss(z, mu, lv, prior, beta, 0.0, kernel))
    close(plain[0], kl[0], "lambda = 0: beta KL")
    assert not plain[1].any()                                    # ... and no gradient reaches z
    close(plain[2], kl[2], "lambda = 0: its dmu")
    close(plain[3], kl[3], "lambda = 0: its dlogvar")
    # without a KL coefficient the KL's value does not reach the result, whatever it is
    lv_inf = c["lv"].copy()
    lv_inf[0, 0] = 100.0                  # exp overflows fp32: the KL is infinite
    r0 = grads(lambda z, mu, lv: ops.mmd_kl_loss(z, mu, lv, prior, 0.0, lam, kernel))
    r1 = grads(lambda z, mu, lv: ops.mmd_kl_loss(z, mu, lv, prior, 0.0, lam, kernel), lv=lv_inf)
    assert torch.isfinite(r1[0]) and torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    assert not r1[2].any() and not r1[3].any()
    assert torch.equal(r0[0], reg[0]) and torch.equal(r0[1], reg[1])


# ---- 3. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("Bt, P, D", [(64, 64, 128), (33, 65, 130), (7, 9, 512), (512, 512, 128)])
def test_bitwise_reproducible_and_independent_of_the_split(golden, Bt, P, D, kernel):
    c = case(golden, Bt, P, D, kernel)
    lam, beta = c["hp"]
    a = run(c["z"], c["prior"], c["mu"], c["lv"], kernel, lam, beta)
    same_bits(a, run(c["z"], c["prior"], c["mu"], c["lv"], kernel, lam, beta))
    # another split of the local rows (another Bl, mu / logvar taken from other rows): the statistic keeps its bits
    Bl = max(Bt // 4, 1)
    s = run(c["z"], c["prior"], c["mu"][Bt - Bl:], c["lv"][Bt - Bl:], kernel, lam, beta)
    for k in ("Wt", "rs", "dz"):
        assert torch.equal(a[k], s[k]), k
    assert torch.equal(a["terms"][1:], s["terms"][1:])
    A = a["Wt"][:, :Bt]
    assert torch.equal(A, A.t())


# ---- 4. shard algebra on one GPU -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_shard_algebra(kernel):
    """8 shards of 8 rows of one global batch (Bt = 64, D = 16), the same gathered samples and prior on every "rank" and
    its own mu / logvar rows: the mean over the shards of the loss and of the gradients is the single-rank loss and
    gradient -- what the reduce-scatter adjoint and the gradient average of a data-parallel step compute."""
    z, prior, mu, lv = R.make_inputs(64, 64, 16, seed=77)
    lam, beta = 3.0, 0.5
    ref = R.mmd(z, prior, mu, lv, kernel, 32.0, lam, beta)
    one = run(z, prior, mu, lv, kernel, lam, beta)
    shards = [run(z, prior, mu[8 * r:8 * r + 8], lv[8 * r:8 * r + 8], kernel, lam, beta) for r in range(8)]
    mean = dict(loss=torch.stack([s["loss"].double() for s in shards]).mean(),
                terms=torch.stack([s["terms"].double() for s in shards]).mean(0), Wt=shards[0]["Wt"], rs=shards[0]["rs"],
                dz=torch.stack([s["dz"].double() for s in shards]).mean(0),
                dmu=torch.cat([s["dmu"].double() for s in shards]) / 8,
                dlv=torch.cat([s["dlv"].double() for s in shards]) / 8)
    check(one, ref, f"[shards {kernel} single rank]")
    check(mean, ref, f"[shards {kernel} mean of 8]")
    for s in shards:                       # every rank sees the same statistic
        for k in ("Wt", "rs", "dz"):
            assert torch.equal(s[k], one[k]), k
        assert torch.equal(s["terms"][1:], one["terms"][1:])
    e = errors(mean, dict(loss=float(one["loss"]), terms=N(one["terms"]), Wt=N(one["Wt"]), rs=N(one["rs"]), dz=N(one["dz"]),
                          dmu=N(one["dmu"]), dlogvar=N(one["dlv"])))
    assert max(e.values()) <= BAR, e


# ---- 5. training steps against the oracle ----------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


def _oracle_trainer(name, state, kernel, lam, hp, priors):
    from oracle import latent_math as lm
    from oracle.network import Net
    from oracle.steps import Trainer

    class MmdTrainer(Trainer):
        """The oracle's step with the torch restatement of the MMD hook on every ``reduce="mean"`` call; the prior draws
        of those calls come from ``priors``, in call order.  The oracle is evaluated in fp64 (its network, the batch and
        the draws are widened; the hook is written for any dtype), see test_two_steps_against_the_oracle."""

        def kl_loss(self, z, mu, logvar, reduce="mean", beta=None):
            beta = self.beta_kl if beta is None else beta
            if reduce == "mean":
                out = R.torch_hook(z, priors.pop(0), mu, logvar, kernel, None, lam, beta)
            else:
                out = beta * lm.kl(logvar, mu, reduce)
            self.trace.setdefault("kl", []).append(out.detach().reshape(-1).clone())
            return out

    state = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    return MmdTrainer(name, Net("conv", state=state, **TINY), dataset_size=1000,
                      beta_kl=hp[0], beta_rec=hp[1], beta_neg=hp[2], gamma_r=hp[3], clip=hp[4], lr=hp[5])


def _hip_solver(name, state, kernel, lam, hp):
    import models
    from solvers.mmd import IntroMMDSolver, MMDSolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    args = [_DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
            torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1]]
    if name == "intro":
        args += [hp[2], hp[3]]
    cls = IntroMMDSolver if name == "intro" else MMDSolver
    solver = cls(*args, dev(), False, None, clip=hp[4], lambda_mmd=lam, mmd_kernel=kernel)
    assert solver.conv_math == "fp32"
    return solver, model


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


def _queue(name, draws, priors):
    """The recorded draws in the HIP solver's call order: the prior of a ``reduce="mean"`` call is drawn inside that call.
    VAE: eps, prior.  Intro: noise, eps_real, prior (real), eps_rec, eps_fake, eps_rec_D, eps_fake_D, prior (rec), prior
    (fake)."""
    if name == "vae":
        return [draws[0], priors[0]]
    return [draws[0], draws[1], priors[0], draws[2], draws[3], draws[4], draws[5], priors[1], priors[2]]


@pytest.mark.parametrize("name, kernel", [("vae", "imq"), ("vae", "rbf"), ("intro", "imq")])
def test_two_steps_against_the_oracle(name, kernel):
    """Two training steps of the tiny model (B = 8, fp32 arithmetic on the device, recorded draws) against the CPU oracle
    whose KL hook is the torch restatement.  Tolerances: those of test_hip_dip.py's step test, which are
    test_hip_model.py's run_golden_steps for this model -- the returned dict to 1e-4 at step 0 and 3e-4 at step 1, every
    hook output to 3e-4 / 3e-3 of its scale.

    The oracle runs in fp64.  Its fp32 evaluation is not a yardstick at these tolerances on every host: Adam's first
    update is lr * g / (|g| + eps), which turns a gradient error of 1e-5 at step 0 into one of 1e-3 at step 1, and torch's
    multi-threaded fp32 CPU convolutions reach that.  Measured on the 16-thread host of an MI355X machine, the fp32
    oracle against its own fp64 value (VAE step, imq, lambda_mmd = 2): L2 2.4e-5 at step 0, then loss_kl 8.7e-4 and L2
    1.5e-3 at step 1 (plain KL, lambda_mmd = 0: 4.5e-4 and 2.7e-3); with one thread 1e-7.  The device step agrees with
    the fp64 oracle to 2e-7 in the same run."""
    import ops
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    lam = 2.0                             # the statistic is a fifth of the KL term here: neither hides the other
    state = _init_state()
    priors = []
    tr = _oracle_trainer(name, state, kernel, lam, hp, priors)
    solver, _ = _hip_solver(name, state, kernel, lam, hp)
    kl_log, kl0 = [], solver.compute_kl_loss
    solver.compute_kl_loss = lambda *a, _f=kl0, **k: (kl_log.append(_f(*a, **k)), kl_log[-1])[1]
    g = torch.Generator().manual_seed(1)
    nd, npr = (6, 3) if name == "intro" else (1, 1)
    keys = ("loss_enc", "loss_dec", "loss_kl", "loss_rec", "L2")
    for s in range(2):
        x = torch.rand(8, 3, 32, 32, generator=g)
        draws = [torch.randn(8, 10, generator=g) for _ in range(nd)]
        pri = [torch.randn(8, 10, generator=g) for _ in range(npr)]
        kl_log.clear()
        with ops.noise_queue([t.clone() for t in _queue(name, draws, pri)]):
            got = solver.train_step(x, s)
            assert not ops._noise["queue"]                       # every recorded draw was taken
        priors[:] = [t.clone() for t in pri]
        ref = tr.step(x.double(), [t.double() for t in draws])
        assert not priors
        first = got if s == 0 else first
        print(name, kernel, s, {k: (got[k], ref[k]) for k in keys})
        np.testing.assert_allclose([got[k] for k in keys], [ref[k] for k in keys], rtol=1e-4 if s == 0 else 3e-4)
        tol = 3e-4 if s == 0 else 3e-3
        assert len(kl_log) == len(tr.trace["kl"]) == (5 if name == "intro" else 1)
        for i, (t, want) in enumerate(zip(kl_log, tr.trace["kl"])):
            err = float((t.detach().reshape(-1).cpu() - want).abs().max())
            assert err < tol * float(want.abs().max()), (name, kernel, s, i, err)
    # the statistic is live: the same first step without it reports another KL term
    plain, _ = _hip_solver(name, state, kernel, 0.0, hp)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 3, 32, 32, generator=g)
    draws = [torch.randn(8, 10, generator=g) for _ in range(nd)]
    pri = [torch.randn(8, 10, generator=g) for _ in range(npr)]
    with ops.noise_queue(_queue(name, draws, pri)):
        d0 = plain.train_step(x, 0)
    assert abs(d0["loss_kl"] - first["loss_kl"]) > 1e-2 * abs(first["loss_kl"]), (d0["loss_kl"], first["loss_kl"])


# ---- 6. graph capture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "intro"])
def test_captured_steps_equal_eager_steps_and_changes_recapture(name):
    """With enable_graph() the trajectory follows the eager one from the same state through the capture; after
    ``lambda_mmd *= 2`` it still does, which it could not if the step replayed the graph captured with the old value:
    the key re-captures.  A change of ``mmd_kernel`` re-captures too."""
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    state = _init_state()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(8, 3, 32, 32, generator=gen).to(dev()) for _ in range(2)]

    def trajectory(graph):
        solver, model = _hip_solver(name, state, "imq", 2.0, hp)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], []
        for k in range(12):
            if k == 6:
                solver.lambda_mmd *= 2
            if k == 9:
                solver.mmd_kernel = "rbf"
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8, 10, 11) else None)
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), keys

    (e, we, _), (gr, wg, keys) = trajectory(False), trajectory(True)

    def holds(key, triple):
        return key is not None and any(key[i:i + 3] == triple for i in range(len(key) - 2))

    assert holds(keys[3], (2.0, "imq", None)) and keys[3] == keys[4] == keys[5]
    assert holds(keys[7], (4.0, "imq", None)) and keys[7] == keys[8] != keys[5]
    assert holds(keys[10], (4.0, "rbf", None)) and keys[10] == keys[11] != keys[8]
    for x, y in zip(e, gr):
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((we - wg).abs().max()) < 1e-6
    # the doubled statistic is visible in the eager trajectory itself (the check above is not vacuous)
    assert abs(e[6]["loss_kl"] - e[5]["loss_kl"]) > 1e-2 * abs(e[5]["loss_kl"])
