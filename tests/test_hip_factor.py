"""GPU tests of the FactorVAE objective (csrc/factor.hip, the fused discriminator layers of csrc/conv_igemm.hip,
ops.permute_dims / factor_tc / factor_disc_loss, models.Discriminator, solvers/factor.py) against the fp64 restatement
tests/factor_ref.py.

Bounds: the permutation is compared bit for bit.  Everything else is normwise, max |err| / max |value| per tensor (scalars
relative to the fp64 value), against the project's fp32 bar of 1e-4; a quantity whose fp64 value is exactly zero must come
out exactly zero.  The stored head inputs keep |tc| >= 1e-2 mean |l0 - l1| and 0 < d_acc < 1, so that the relative bounds
on both mean something.  Worst values measured on an MI355X over every case (printed by the tests):

    layers: lrelu_fwd 1.2e-06, dgrad_lrelu 1.6e-06
    head:   tc 4.8e-08, d_loss 4.7e-08, d_acc 1.5e-08, dlogits of tc 5.8e-08, dlogits of d_loss 4.7e-08
    ops:    logits 5.3e-07, tc 1.2e-07, d_loss 2.5e-08, dz 3.6e-07, dW0 1.4e-06, db0 4.2e-07, dW1 2.1e-06, db1 1.6e-07,
            dW2 3.4e-06, db2 1.4e-07
    steps:  D's gradients per tensor 7.6e-07
"""
import os

import numpy as np
import pytest
import torch

import factor_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
SLOPE = 0.2
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())       # a copy: the stored cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "factor.npz"))
    return {k: g[k] for k in g.files}


def place(x, layout):
    """A device tensor holding the values of ``x``: dense, or the middle of a wider nan tensor that must not be read."""
    if layout == "dense":
        return G(x)
    wide = np.full((x.shape[0], x.shape[1] + 5), np.nan, dtype=np.float32)
    wide[:, 3:3 + x.shape[1]] = x
    t = G(wide)[:, 3:3 + x.shape[1]]
    assert t.stride(1) == 1 and (x.shape[0] == 1 or t.stride(0) == x.shape[1] + 5)
    return t


def rel(x, want, tag=None):
    """Normwise error; a quantity that is exactly zero in fp64 must be exactly zero."""
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    assert x.shape == want.shape, (tag, x.shape, want.shape)
    scale = np.abs(want).max()
    if scale == 0.0:
        assert not x.any(), tag
        return 0.0
    assert np.isfinite(x).all(), tag
    return float(np.abs(x - want).max() / scale)


def note(kind, err, tag):
    print(tag, kind, f"{err:.2e}")
    WORST[kind] = max(WORST.get(kind, 0.0), err)
    assert err <= BAR, (tag, kind, err)


def print_worst():
    print("worst so far:", ", ".join(f"{k} {v:.1e}" for k, v in WORST.items()))


# ---- 1. the permutation, bit for bit ----------------------------------------------------------------------------------------
def _key_sets(B, D, rng):
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], np.float32)
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)
    return dict(normal=rng.normal(size=(B, D)).astype(np.float32),
                ties=rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), size=(B, D)),
                equal=np.full((B, D), 0.5, np.float32),
                special=rng.choice(np.concatenate([special, neg_nan]), size=(B, D)))


PERM_SHAPES = [(B, D) for B in (1, 2, 63, 64, 65) for D in (1, 10, 129, 512)] + \
    [(B, D) for B in (1024, 1025, 4096) for D in (1, 10)]


@pytest.mark.parametrize("B, D", PERM_SHAPES)
def test_permutation_bitwise(B, D):
    from hipvae import functional as HF
    rng = np.random.default_rng(100 * B + D)
    z = rng.normal(size=(B, D)).astype(np.float32)
    for name, keys in _key_sets(B, D, rng).items():
        want = R.permute_dims(z, keys)
        for layout in ("dense", "strided"):
            tz, tk = place(z, layout), place(keys, layout)
            zc = torch.full((B, D), float("nan"), device=dev())
            got = HF.permute_dims(tz, tk, zcopy=zc)
            assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), (name, layout)
            assert np.array_equal(zc.cpu().numpy(), z), (name, layout)
        got = got.cpu().numpy()
        for d in range(D):                                 # every output column is a permutation of its input column
            assert np.array_equal(np.sort(got[:, d]), np.sort(z[:, d])), (name, d)


def test_permutation_op_draws_its_keys_from_the_noise_source():
    import ops
    z, keys = R.make_inputs(65, 10, seed=7)
    tz = G(z).requires_grad_(True)
    with ops.noise_queue([torch.from_numpy(keys)]):
        out = ops.permute_dims(tz)
        assert not ops._noise["queue"]
    assert not out.requires_grad and np.array_equal(out.cpu().numpy(), R.permute_dims(z, keys))
    torch.cuda.manual_seed(3)
    out = ops.permute_dims(tz).cpu().numpy()               # device keys: a permutation of every column, not the identity
    assert np.array_equal(np.sort(out, 0), np.sort(z, 0)) and not np.array_equal(out, z)
    with pytest.raises(ValueError):
        ops.permute_dims(torch.zeros(4097, 2, device=dev()))
    with pytest.raises(ValueError):
        ops.permute_dims(torch.zeros(2, 513, device=dev()))


# ---- 2. the layer kernels against fp64 ------------------------------------------------------------------------------------
def _lrelu_fwd(x, w, b, slope=SLOPE):
    """itcv_linear_lrelu_fwd on a (possibly row-strided) x."""
    from hipvae import abi
    from hipvae.functional import _ws
    B, K = x.shape
    Nn = w.shape[0]
    y = torch.full((B, Nn), float("nan"), device=dev())
    nws = abi.lib.itcv_linear_workspace(B, K, Nn)
    ws = _ws(nws, dev())
    abi.call("itcv_linear_lrelu_fwd", x.data_ptr(), max(x.stride(0), K), abi.ptr(w), abi.ptr(b), abi.ptr(y), B, K, Nn, slope,
             abi.ptr(ws), nws, abi.stream())
    return y


def _dgrad_lrelu(dy, w, yprev, slope=SLOPE):
    """itcv_linear_dgrad_lrelu on (possibly row-strided) dy [B, N] and y_prev [B, K]; w [N, K]."""
    from hipvae import abi
    from hipvae.functional import _ws
    B, Nn = dy.shape
    K = w.shape[1]
    dx = torch.full((B, K), float("nan"), device=dev())
    nws = abi.lib.itcv_linear_workspace(B, K, Nn)
    ws = _ws(nws, dev())
    abi.call("itcv_linear_dgrad_lrelu", dy.data_ptr(), max(dy.stride(0), Nn), abi.ptr(w), yprev.data_ptr(),
             max(yprev.stride(0), K), abi.ptr(dx), B, K, Nn, slope, abi.ptr(ws), nws, abi.stream())
    return dx


def _layer_case(B, K, Nn, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, K)).astype(np.float32)
    w = rng.uniform(-1, 1, size=(Nn, K)).astype(np.float32) / np.float32(np.sqrt(K))
    b = rng.uniform(-1, 1, size=Nn).astype(np.float32) / np.float32(np.sqrt(K))
    dy = rng.normal(size=(B, Nn)).astype(np.float32)
    yprev = rng.normal(size=(B, K)).astype(np.float32)
    yprev[rng.random(size=(B, K)) < 0.1] = 0.0             # exact zeros in the mask: they take the slope
    return x, w, b, dy, yprev


def _check_layer(B, K, Nn, seed, tag):
    x, w, b, dy, yprev = _layer_case(B, K, Nn, seed)
    tw, tb = G(w), G(b)
    y = _lrelu_fwd(G(x), tw, tb)
    note("lrelu_fwd", rel(N(y), R.linear_lrelu(x, w, b, SLOPE), tag), tag)
    assert torch.equal(y, _lrelu_fwd(place(x, "strided"), tw, tb)), tag          # the nan around x is not read
    y0 = _lrelu_fwd(G(x), tw, None)                                              # no bias
    note("lrelu_fwd", rel(N(y0), R.linear_lrelu(x, w, None, SLOPE), tag), tag)
    dx = _dgrad_lrelu(G(dy), tw, G(yprev))
    note("dgrad_lrelu", rel(N(dx), R.dgrad_lrelu(dy, w, yprev, SLOPE), tag), tag)
    assert torch.equal(dx, _dgrad_lrelu(place(dy, "strided"), tw, place(yprev, "strided"))), tag
    assert torch.equal(dx, _dgrad_lrelu(G(dy), tw, G(yprev))), tag               # the same bits run to run


# K = 10 (zdim) and the other short K run un-split, K = 1000 splits K over the grid at these batch sizes
@pytest.mark.parametrize("K", [10, 31, 32, 33, 1000])
@pytest.mark.parametrize("Nn", [2, 63, 64, 65, 1000])
def test_layer_kernels_against_fp64(K, Nn):
    for B in (1, 63, 64, 65, 128):
        _check_layer(B, K, Nn, 1000 * K + 10 * Nn + B, f"[B {B} K {K} N {Nn}]")
    print_worst()


def test_layer_kernels_long_k_unsplit():
    """128 tiles of 64 x 64: a long K runs in one pass, with the epilogue in the GEMM itself -- the forward at N = 4096
    (2 x 64 tiles), the data gradient at K = 4096 outputs."""
    from hipvae import abi
    assert abi.lib.itcv_linear_workspace(128, 1000, 1000) > 0        # ... while 2 x 16 tiles split
    _check_layer(128, 1000, 4096, 5, "[B 128 K 1000 N 4096]")
    _check_layer(128, 4096, 1000, 6, "[B 128 K 4096 N 1000]")
    _check_layer(65, 1000, 1000, 7, "[B 65 K 1000 N 1000]")
    print_worst()


@pytest.mark.parametrize("K, Nn", [(10, 64), (1000, 65)])
def test_mask_convention_at_exactly_zero(K, Nn):
    """A zero input row with a zero bias: the pre-activation is exactly 0, so is the output, and the derivative read from
    that output is the slope, as torch's leaky_relu has it."""
    x, w, b, dy, _ = _layer_case(5, K, Nn, 9)
    x[2] = 0.0
    b[:] = 0.0
    y = _lrelu_fwd(G(x), G(w), G(b))
    assert not y[2].any() and y[[0, 1, 3, 4]].abs().min() > 0
    rng = np.random.default_rng(10)
    w2 = rng.uniform(-1, 1, size=(7, Nn)).astype(np.float32)
    dy2 = rng.normal(size=(5, 7)).astype(np.float32)
    dx = _dgrad_lrelu(G(dy2), G(w2), y)
    want = R.dgrad_lrelu(dy2, w2, N(y), SLOPE)
    assert np.allclose(want[2], SLOPE * (dy2[2].astype(np.float64) @ w2.astype(np.float64)), rtol=1e-13, atol=0)
    note("dgrad_lrelu", rel(N(dx), want), f"[zero row K {K} N {Nn}]")
    # torch's own convention, for the record: the gradient at the pre-activation of the zero row
    F = torch.nn.functional
    pre = F.linear(torch.from_numpy(x).double(), torch.from_numpy(w).double()).requires_grad_(True)
    out = F.linear(F.leaky_relu(pre, SLOPE), torch.from_numpy(w2).double())
    (g,) = torch.autograd.grad(out, pre, torch.from_numpy(dy2).double())
    assert not pre[2].any() and rel(N(dx)[2], g.numpy()[2]) <= BAR


# ---- 3. the head against fp64 -----------------------------------------------------------------------------------------------
def _head(logits, R0, g=1.0):
    from hipvae import abi
    l = G(logits)
    Rr = l.shape[0]
    out = torch.full((3,), float("nan"), device=dev())
    abi.call("itcv_disc_head_fwd", abi.ptr(l), Rr, R0, abi.ptr(out), abi.stream())
    tg = torch.tensor([g], dtype=torch.float32, device=dev())
    d0 = torch.full((R0, 2), float("nan"), device=dev())
    abi.call("itcv_disc_head_bwd", abi.ptr(tg), abi.ptr(l), abi.ptr(d0), Rr, R0, 0, abi.stream())
    d1 = None
    if R0 < Rr:
        d1 = torch.full((Rr, 2), float("nan"), device=dev())
        abi.call("itcv_disc_head_bwd", abi.ptr(tg), abi.ptr(l), abi.ptr(d1), Rr, R0, 1, abi.stream())
    return out, d0, d1


def _check_head(logits, R0, tag, g=1.0):
    ref = R.head(logits, R0)
    out, d0, d1 = _head(logits, R0, g)
    o = N(out)
    assert np.isfinite(o).all()
    for i, k in enumerate(("tc", "d_loss", "d_acc")):
        note("head " + k, rel(o[i], ref[k], tag), tag)
    note("head dl_tc", rel(N(d0), g * ref["dl_tc"], tag), tag)
    note("head dl_d", rel(N(d1), g * ref["dl_d"], tag), tag)
    again = _head(logits, R0, g)
    assert all(torch.equal(a, b) for a, b in zip((out, d0, d1), again)), tag
    return ref, o


@pytest.mark.parametrize("R0", [1, 2, 63, 64, 65, 4096])
def test_head_against_fp64(golden, R0):
    p = f"head:{R0}:"
    l = R.make_logits(R0, int(golden[p + "seed"]))
    assert l.astype(np.float64).sum() == float(golden[p + "checksum"])
    ref, o = _check_head(l, R0, f"[head R0 {R0}]")
    d = np.abs(l[:, 0].astype(np.float64) - l[:, 1]).mean()
    assert abs(ref["tc"]) >= 1e-2 * d and 0.0 < ref["d_acc"] < 1.0
    for i, k in enumerate(("tc", "d_loss", "d_acc")):          # the stored expected values themselves
        assert abs(o[i] - float(golden[p + k])) <= BAR * abs(float(golden[p + k])), k
    # scaled so that |l0 - l1| reaches 80: finite, and still at the bar
    big = (l * np.float32(80.0 / np.abs(l[:, 0] - l[:, 1]).max())).astype(np.float32)
    assert np.abs(big[:, 0].astype(np.float64) - big[:, 1]).max() >= 79.99
    _check_head(big, R0, f"[head R0 {R0} |d| -> 80]", g=-0.375)
    # equal logits on the label-0 rows: tc is exactly zero in fp64 and here
    flat = l.copy()
    flat[:R0, 1] = flat[:R0, 0]
    ref, o = _check_head(flat, R0, f"[head R0 {R0} tc = 0]")
    assert ref["tc"] == 0.0 and o[0] == 0.0
    print_worst()


def test_head_extremes_are_finite():
    l = np.array([[80.0, 0.0], [-90.0, 30.0], [0.0, 80.0], [60.0, -60.0]], np.float32)
    ref, o = _check_head(l, 2, "[head +-80 / 120]")
    assert o[2] == 0.5
    out, d0, _ = _head(l[:2], 2)                                # a pass over rows of label 0 alone (ops.factor_tc)
    assert np.isfinite(N(out)).all() and rel(N(out)[0], R.head(l[:2], 2)["tc"]) <= BAR


# ---- 4. the ops against the restatement ---------------------------------------------------------------------------------------
_OPS = {}


def op_case(golden, B, zdim, hidden):
    key = (B, zdim, hidden)
    if key not in _OPS:
        p = f"op:{B}x{zdim}x{hidden}:"
        seed = int(golden[p + "seed"])
        z, keys = R.make_inputs(B, zdim, seed)
        Ws, bs = R.make_mlp(zdim, hidden, 2, seed + 1)
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in (z, keys, *Ws, *bs)])
        ref = R.factor(z, R.permute_dims(z, keys), Ws, bs, SLOPE)
        assert abs(ref["tc"] - float(golden[p + "tc"])) <= 1e-12 * abs(ref["tc"])
        _OPS[key] = dict(z=z, keys=keys, Ws=Ws, bs=bs, ref=ref)
    return _OPS[key]


def make_disc(c, zdim, hidden):
    import models
    d = models.Discriminator(zdim, hidden=hidden, layers=2, slope=SLOPE)
    with torch.no_grad():
        for m, W, b in zip(d.linears(), c["Ws"], c["bs"]):
            m.weight.copy_(torch.from_numpy(W))
            m.bias.copy_(torch.from_numpy(b))
    return d.to(dev())


def run_ops(c, zdim, hidden):
    import ops
    disc = make_disc(c, zdim, hidden)
    z = G(c["z"]).requires_grad_(True)
    with ops.noise_queue([torch.from_numpy(c["keys"])]):
        dp = ops.factor_pass(z, disc)
    tc, terms = ops.factor_tc(z, disc, with_terms=True, shared=dp)
    d_loss = ops.factor_disc_loss(z, disc, shared=dp)
    assert tc.shape == () and d_loss.shape == () and terms.shape == (3,) and not terms.requires_grad
    d_loss.backward()                                      # the discriminator's walk: nothing reaches z
    assert z.grad is None
    grads = [p.grad.clone() for p in disc.parameters()]
    tc.backward()                                          # the VAE walk: the parameters' gradients keep their bits
    assert all(torch.equal(p.grad, g) for p, g in zip(disc.parameters(), grads))
    return dict(tc=tc.detach(), d_loss=d_loss.detach(), terms=terms, dz=z.grad, grads=grads, logits=dp.logits, x=dp.x)


@pytest.mark.parametrize("hidden", [64, 1000])
@pytest.mark.parametrize("B, zdim", [(8, 10), (64, 128), (65, 33)])
def test_ops_against_restatement(golden, B, zdim, hidden):
    import ops
    c = op_case(golden, B, zdim, hidden)
    ref, tag = c["ref"], f"[op {B}x{zdim}x{hidden}]"
    got = run_ops(c, zdim, hidden)
    assert np.array_equal(got["x"].cpu().numpy(), np.concatenate([c["z"], R.permute_dims(c["z"], c["keys"])]))
    note("logits", rel(N(got["logits"]), ref["logits"], tag), tag)
    t = N(got["terms"])
    assert t[0] == float(got["tc"]) and t[1] == float(got["d_loss"])
    note("tc", rel(t[0], ref["tc"], tag), tag)
    note("d_loss", rel(t[1], ref["d_loss"], tag), tag)
    assert abs(t[2] - ref["d_acc"]) <= 1.0 / (2 * B) + 1e-7          # one row at a tie of fp32 logits at the most
    note("dz", rel(N(got["dz"]), ref["dz"], tag), tag)
    for l in range(3):
        note(f"dW{l}", rel(N(got["grads"][2 * l]), ref["dW"][l], tag), tag)
        note(f"db{l}", rel(N(got["grads"][2 * l + 1]), ref["db"][l], tag), tag)
    p = f"op:{B}x{zdim}x{hidden}:"
    if p + "dz" in golden:                                 # the stored expected values themselves
        assert np.abs(N(got["dz"]) - golden[p + "dz"]).max() <= BAR * np.abs(golden[p + "dz"]).max()
        assert np.abs(N(got["grads"][0]) - golden[p + "dW0"]).max() <= BAR * np.abs(golden[p + "dW0"]).max()
    # two runs: the same bits
    again = run_ops(c, zdim, hidden)
    for k in ("tc", "d_loss", "terms", "dz", "logits"):
        assert torch.equal(got[k], again[k]), k
    assert all(torch.equal(a, b) for a, b in zip(got["grads"], again["grads"]))
    # the ops on their own (no shared pass): tc from a forward over z alone, d_loss from a given z_perm
    disc = make_disc(c, zdim, hidden)
    z = G(c["z"]).requires_grad_(True)
    tc = ops.factor_tc(z, disc)
    (dz,) = torch.autograd.grad(tc, z)
    note("tc", rel(float(tc.detach()), ref["tc"], tag), tag + " alone")
    note("dz", rel(N(dz), ref["dz"], tag), tag + " alone")
    d_loss = ops.factor_disc_loss(z, disc, z_perm=G(R.permute_dims(c["z"], c["keys"])))
    d_loss.backward()
    assert z.grad is None
    note("d_loss", rel(float(d_loss.detach()), ref["d_loss"], tag), tag + " alone")
    note("dW0", rel(N(disc[0].weight.grad), ref["dW"][0], tag), tag + " alone")
    logits = disc(G(c["z"]))
    assert not logits.requires_grad
    note("logits", rel(N(logits), ref["logits"][:B], tag), tag + " module")
    print_worst()


# ---- 5. training steps against the oracle ----------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


DISC = dict(hidden=64, layers=2)
# fp32 storage rounds a parameter of magnitude < 0.5 by up to 2^-26 = 1.5e-8: the bound 1e-4 lr on the parameter change
# is above that for lr >= 1.5e-4 only, so the step tests train D at 1e-3 (bound 1e-7), not at the recommended 1e-4
LR_DISC, BETAS_DISC = 1e-3, (0.5, 0.9)


def _init_state():
    import models
    torch.manual_seed(0)
    model = {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}
    disc = {k: v.clone() for k, v in models.Discriminator(TINY["zdim"], **DISC).state_dict().items()}
    return model, disc


def _hip_solver(state, dstate, gamma, hp, lr_disc=LR_DISC, plain=False):
    import models
    from solvers import FactorSolver, VAESolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    args = [_DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
            torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1], dev(), False, None]
    if plain:
        return VAESolver(*args, clip=hp[4]), model, None
    disc = models.Discriminator(TINY["zdim"], **DISC)
    disc.load_state_dict(dstate)
    disc = disc.to(dev())
    solver = FactorSolver(*args, clip=hp[4], discriminator=disc, gamma=gamma,
                          optimizer_disc=torch.optim.Adam(disc.parameters(), lr=lr_disc, betas=BETAS_DISC))
    assert solver.conv_math == "fp32"
    return solver, model, disc


def _oracle_trainer(state, dparams, gamma, hp, keys_q, side):
    from oracle import latent_math as lm
    from oracle.network import Net
    from oracle.steps import Trainer

    class FactorTrainer(Trainer):
        """The oracle's VAE step with the torch restatement of the FactorVAE hook and an fp64 copy of D; the keys of the
        permutation come from ``keys_q``.  d_loss of the same z is left in ``side`` for the test, which walks and updates
        D itself."""

        def kl_loss(self, z, mu, logvar, reduce="mean", beta=None):
            beta = self.beta_kl if beta is None else beta
            if reduce == "mean":
                out, side["d_loss"], side["tc"] = R.torch_hook(z, keys_q.pop(0), mu, logvar, dparams, SLOPE, gamma, beta)
            else:
                out = beta * lm.kl(logvar, mu, reduce)
            self.trace.setdefault("kl", []).append(out.detach().reshape(-1).clone())
            return out

    state = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    return FactorTrainer("vae", Net("conv", state=state, **TINY), dataset_size=1000, beta_kl=hp[0], beta_rec=hp[1],
                         beta_neg=hp[2], gamma_r=hp[3], clip=hp[4], lr=hp[5])


class _Adam64:
    """torch.optim.Adam's default update in fp64, one state per tensor."""

    def __init__(self, n, lr, betas, eps=1e-8):
        self.lr, self.betas, self.eps, self.t = lr, betas, eps, 0
        self.m, self.v = [0.0] * n, [0.0] * n

    def step(self, params, grads):
        """The updated values of ``params`` (fp64 arrays) for ``grads``."""
        b1, b2 = self.betas
        self.t += 1
        out = []
        for i, (p, g) in enumerate(zip(params, grads)):
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            denom = np.sqrt(self.v[i]) / np.sqrt(1 - b2 ** self.t) + self.eps
            out.append(p - self.lr / (1 - b1 ** self.t) * self.m[i] / denom)
        return out


def test_two_steps_against_the_oracle():
    """Two training steps of the tiny model (B = 8, fp32 arithmetic on the device, recorded draws: eps, then the keys)
    against the fp64 CPU oracle whose KL hook is the torch restatement with an fp64 copy of D; D's fp64 walk and Adam
    update are done here after each oracle step.  Tolerances: those of test_hip_mmd.py's step test -- the returned dict to
    1e-4 at step 0 and 3e-4 at step 1, the hook's output to 3e-4 / 3e-3 of its scale.  D's gradients per tensor at the
    bar; D's parameter change against fp64 Adam applied to the device's OWN gradient to 1e-4 lr (Adam's first step maps
    g to g / (|g| + eps), which would amplify a gradient difference)."""
    import ops
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    gamma = 2.0
    state, dstate = _init_state()
    names = [k for k in dstate]
    dparams = [(dstate[f"{2 * i}.weight"].double().requires_grad_(True), dstate[f"{2 * i}.bias"].double().requires_grad_(True))
               for i in range(DISC["layers"] + 1)]
    flat = [t for pair in dparams for t in pair]
    keys_q, side = [], {}
    tr = _oracle_trainer(state, dparams, gamma, hp, keys_q, side)
    solver, _, disc = _hip_solver(state, dstate, gamma, hp)
    assert [k for k, _ in disc.named_parameters()] == names
    kl_log, kl0 = [], solver.compute_kl_loss
    solver.compute_kl_loss = lambda *a, _f=kl0, **k: (kl_log.append(_f(*a, **k)), kl_log[-1])[1]
    oracle_adam = _Adam64(len(flat), LR_DISC, BETAS_DISC)
    device_adam = _Adam64(len(flat), LR_DISC, BETAS_DISC)
    g = torch.Generator().manual_seed(1)
    keys_ = ("loss_enc", "loss_dec", "loss_kl", "loss_rec", "L2")
    for s in range(2):
        x = torch.rand(8, 3, 32, 32, generator=g)
        eps = torch.randn(8, 10, generator=g)
        pk = torch.randn(8, 10, generator=g)
        before = [N(p) for p in disc.parameters()]
        kl_log.clear()
        with ops.noise_queue([eps.clone(), pk.clone()]):
            got = solver.train_step(x, s)
            assert not ops._noise["queue"]                       # every recorded draw was taken
        keys_q[:] = [pk.clone()]
        ref = tr.step(x.double(), [eps.double()])
        assert not keys_q
        first = got if s == 0 else first
        tc64, dl64 = float(side["tc"].detach()), float(side["d_loss"].detach())
        print(s, {k: (got[k], ref[k]) for k in keys_}, got["loss_tc"], tc64, got["loss_disc"], dl64, got["disc_acc"])
        np.testing.assert_allclose([got[k] for k in keys_], [ref[k] for k in keys_], rtol=1e-4 if s == 0 else 3e-4)
        tol = 3e-4 if s == 0 else 3e-3
        assert len(kl_log) == len(tr.trace["kl"]) == 1
        want = tr.trace["kl"][0]
        err = float((kl_log[0].detach().reshape(-1).cpu() - want).abs().max())
        assert err < tol * float(want.abs().max()), (s, err)
        assert abs(got["loss_disc"] - dl64) <= tol * dl64
        assert abs(got["loss_tc"] - tc64) <= tol * max(abs(tc64), abs(float(want)) / gamma)
        assert 0.0 <= got["disc_acc"] <= 1.0
        # D's walk in fp64, per tensor at the bar
        want_g = [t.numpy() for t in torch.autograd.grad(side["d_loss"], flat)]
        dev_g = [N(p.grad) for p in disc.parameters()]
        for name, a, b in zip(names, dev_g, want_g):
            note("step dD", rel(a, b, name), f"[step {s} {name}]")
        # D's update: fp64 Adam on the device's own gradient
        after = [N(p) for p in disc.parameters()]
        for name, a, b, p0 in zip(names, after, device_adam.step(before, dev_g), before):
            assert np.abs(a - b).max() <= 1e-4 * LR_DISC, (s, name, np.abs(a - b).max())
            assert np.abs(a - p0).max() > 0.1 * LR_DISC, name          # ... and it did move
        new = oracle_adam.step([t.detach().numpy() for t in flat], want_g)
        with torch.no_grad():
            for t, v in zip(flat, new):
                t.copy_(torch.from_numpy(v))
    # gamma > 0 is live: the same first step without the term reports another KL term
    plain, _, _ = _hip_solver(state, dstate, 0.0, hp)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(8, 3, 32, 32, generator=g)
    eps, pk = torch.randn(8, 10, generator=g), torch.randn(8, 10, generator=g)
    with ops.noise_queue([eps, pk]):
        d0 = plain.train_step(x, 0)
    assert abs(d0["loss_kl"] - first["loss_kl"]) > 1e-2 * abs(first["loss_kl"]), (d0["loss_kl"], first["loss_kl"])
    print_worst()


def test_gamma_zero_leaves_the_vae_step_bitwise_alone():
    """gamma = 0: encoder and decoder after three steps are bit for bit those of a VAESolver from the same state and
    draws, while D has trained."""
    import ops
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    state, dstate = _init_state()
    fs, fm, disc = _hip_solver(state, dstate, 0.0, hp)
    vs, vm, _ = _hip_solver(state, dstate, 0.0, hp, plain=True)
    g = torch.Generator().manual_seed(2)
    for s in range(3):
        x = torch.rand(8, 3, 32, 32, generator=g)
        eps, pk = torch.randn(8, 10, generator=g), torch.randn(8, 10, generator=g)
        with ops.noise_queue([eps.clone(), pk]):
            a = fs.train_step(x, s)
        with ops.noise_queue([eps.clone()]):
            b = vs.train_step(x, s)
        assert all(a[k] == b[k] for k in b), (a, b)
        assert a["loss_disc"] > 0 and a["loss_tc"] == a["loss_tc"]
    for (k, p), (_, q) in zip(fm.state_dict().items(), vm.state_dict().items()):
        assert torch.equal(p, q), k
    moved = [float((p.detach().cpu() - dstate[k]).abs().max()) for k, p in disc.named_parameters()]
    assert min(moved) > 0.1 * LR_DISC, moved


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------
def test_captured_steps_equal_eager_steps_and_changes_recapture():
    """With enable_graph() the trajectory follows the eager one from the same state through the capture; after ``gamma *=
    2`` and after halving D's learning rate it still does, which it could not if the step replayed a graph captured with
    the old values: both are part of the key and re-capture."""
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    state, dstate = _init_state()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(8, 3, 32, 32, generator=gen).to(dev()) for _ in range(2)]

    def trajectory(graph):
        solver, model, disc = _hip_solver(state, dstate, 2.0, hp, lr_disc=1e-4)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], []
        for k in range(12):
            if k == 6:
                solver.gamma *= 2
            if k == 9:
                solver.optimizer_disc.param_groups[0]["lr"] /= 2
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8, 10, 11) else None)
        flat = torch.cat([p.detach().reshape(-1) for p in list(model.parameters()) + list(disc.parameters())]).cpu()
        return res, flat, keys, solver.optimizer_disc.state_dict(), sum(p.numel() for p in disc.parameters())

    (e, we, _, sd_e, nd), (gr, wg, keys, sd_g, _) = trajectory(False), trajectory(True)

    def spec(lr):
        return ("adam", 0, (lr, BETAS_DISC, 1e-8))

    def holds(key, pair):
        return key is not None and any(key[i:i + 2] == pair for i in range(len(key) - 1))

    assert holds(keys[3], (2.0, spec(1e-4))) and keys[3] == keys[4] == keys[5]
    assert holds(keys[7], (4.0, spec(1e-4))) and keys[7] == keys[8] != keys[5]
    assert holds(keys[10], (4.0, spec(5e-5))) and keys[10] == keys[11] != keys[8]
    for x, y in zip(e, gr):
        assert set(x) == set(y) >= {"loss_tc", "loss_disc", "disc_acc"}
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((we - wg).abs().max()) < 1e-6
    assert float((we[-nd:] - torch.cat([v.reshape(-1) for v in dstate.values()])).abs().max()) > 1e-4   # D has trained
    # the optimiser's own view of its state: the bound moments and the step count, replays included
    for sd in (sd_e, sd_g):
        assert len(sd["state"]) == 2 * (DISC["layers"] + 1)
        for st in sd["state"].values():
            assert float(st["step"]) == 12.0 and st["exp_avg"].abs().max() > 0 and st["exp_avg_sq"].abs().max() > 0
    # the doubled term is visible in the eager trajectory itself (the check above is not vacuous)
    assert abs(e[6]["loss_kl"] - e[5]["loss_kl"]) > 1e-2 * abs(e[5]["loss_kl"])
