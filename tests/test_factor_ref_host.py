"""CPU-only tests of the FactorVAE objective: the fp64 restatement (tests/factor_ref.py) against torch's own fp64
``nn.Linear`` / ``leaky_relu`` / ``F.cross_entropy`` autograd and against central differences, the permutation against
``np.argsort(kind="stable")``, the softplus form at logit differences of +-80, the stored vectors (golden/factor.npz),
the surface of ``FactorSolver`` / ``Discriminator``, and what the new entry points refuse before any launch."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import factor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
NEW = ("itcv_permute_dims", "itcv_disc_head_fwd", "itcv_disc_head_bwd", "itcv_linear_lrelu_fwd", "itcv_linear_dgrad_lrelu")
SLOPE = 0.2


def rel(x, want):
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    return float(np.abs(x - want).max() / np.abs(want).max())


# ---- the restatement against torch's fp64 autograd -------------------------------------------------------------------------
def _torch_case(B, zdim, hidden, layers, seed):
    z, keys = R.make_inputs(B, zdim, seed)
    Ws, bs = R.make_mlp(zdim, hidden, layers, seed + 1)
    zp = R.permute_dims(z, keys)
    ref = R.factor(z, zp, Ws, bs, SLOPE)
    tz = torch.from_numpy(z).double().requires_grad_(True)
    params = [(torch.from_numpy(W).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True))
              for W, b in zip(Ws, bs)]
    return z, keys, zp, Ws, bs, ref, tz, params


@pytest.mark.parametrize("B, zdim, hidden, layers", [(8, 10, 16, 2), (5, 3, 7, 1), (9, 4, 12, 6)])
def test_restatement_equals_torch_fp64_autograd(B, zdim, hidden, layers):
    z, keys, zp, Ws, bs, ref, tz, params = _torch_case(B, zdim, hidden, layers, seed=11)
    x = torch.cat([tz, torch.from_numpy(zp).double()])
    h = x
    for W, b in params[:-1]:
        h = F.leaky_relu(F.linear(h, W, b), SLOPE)
    l = F.linear(h, *params[-1])
    tc = (l[:B, 0] - l[:B, 1]).mean()
    lab = torch.cat([torch.zeros(B, dtype=torch.long), torch.ones(B, dtype=torch.long)])
    d_loss = 0.5 * F.cross_entropy(l[:B], lab[:B]) + 0.5 * F.cross_entropy(l[B:], lab[B:])
    acc = (l.argmax(1) == lab).double().mean()
    flat = [t for pair in params for t in pair]
    (dz,) = torch.autograd.grad(tc, tz, retain_graph=True)
    grads = torch.autograd.grad(d_loss, flat)
    errs = dict(logits=rel(ref["logits"], l.detach().numpy()), tc=rel(ref["tc"], tc.item()),
                d_loss=rel(ref["d_loss"], d_loss.item()), dz=rel(ref["dz"], dz.numpy()))
    for i in range(len(Ws)):
        errs[f"dW{i}"] = rel(ref["dW"][i], grads[2 * i].numpy())
        errs[f"db{i}"] = rel(ref["db"][i], grads[2 * i + 1].numpy())
    print(errs)
    assert ref["d_acc"] == acc.item()
    assert max(errs.values()) <= 1e-12, errs
    # the torch form of the hook (what the step tests hand to the oracle) is the same thing
    mu = torch.zeros(B, zdim, dtype=torch.float64)
    hook, d2, tc2 = R.torch_hook(tz, torch.from_numpy(keys), mu, mu.clone(), params, SLOPE, 3.0, 0.5)
    assert abs(hook.item() - 3.0 * ref["tc"]) <= 1e-12 * abs(3.0 * ref["tc"])      # KL(N(0, 1) || N(0, 1)) = 0
    assert abs(d2.item() - ref["d_loss"]) <= 1e-12 * ref["d_loss"] and abs(tc2.item() - ref["tc"]) <= 1e-12 * abs(ref["tc"])
    (dz2,) = torch.autograd.grad(hook, tz)
    assert rel(dz2.numpy(), 3.0 * ref["dz"]) <= 1e-12
    assert all(p.grad is None for p in flat)


def test_gradients_agree_with_central_differences():
    z, keys = R.make_inputs(6, 4, seed=21)
    Ws, bs = R.make_mlp(4, 9, 2, seed=22)
    z, zp = z.astype(np.float64), R.permute_dims(z, keys).astype(np.float64)
    Ws, bs = [W.astype(np.float64) for W in Ws], [b.astype(np.float64) for b in bs]
    ref = R.factor(z, zp, Ws, bs, SLOPE)
    step = 1e-6

    def diff(arr, which):
        g = np.zeros_like(arr)
        for idx in np.ndindex(*arr.shape):
            keep = arr[idx]
            arr[idx] = keep + step
            up = R.values_only(z, zp, Ws, bs, SLOPE)[which]
            arr[idx] = keep - step
            dn = R.values_only(z, zp, Ws, bs, SLOPE)[which]
            arr[idx] = keep
            g[idx] = (up - dn) / (2 * step)
        return g

    errs = [np.abs(diff(z, 0) - ref["dz"]).max()]
    for l in range(3):
        errs += [np.abs(diff(Ws[l], 1) - ref["dW"][l]).max(), np.abs(diff(bs[l], 1) - ref["db"][l]).max()]
    print(errs)
    assert max(errs) <= 1e-8


def test_mask_convention_at_exactly_zero():
    """A zero input row with a zero bias: every pre-activation is exactly 0 and the derivative is the slope, as torch's."""
    a = F.linear(torch.zeros(1, 3, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64)).requires_grad_(True)
    y = F.leaky_relu(a, SLOPE)                           # the hidden layer: pre-activation a, output y, both all zero
    W2 = torch.full((2, 4), 1.5, dtype=torch.float64)
    (g,) = torch.autograd.grad(F.linear(y, W2).sum(), a)
    assert not a.any() and not y.any()
    want = R.dgrad_lrelu(np.ones((1, 2)), W2.numpy(), y.detach().numpy(), SLOPE)
    assert np.array_equal(want, g.numpy()) and np.array_equal(want, np.full((1, 4), 3.0 * SLOPE))


# ---- the permutation ---------------------------------------------------------------------------------------------------------
def _key_sets(B, D, rng):
    normal = rng.normal(size=(B, D)).astype(np.float32)
    ties = rng.choice(np.array([-1.5, 0.25, 2.0], np.float32), size=(B, D))
    equal = np.full((B, D), 0.5, np.float32)
    special = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], np.float32), size=(B, D))
    return dict(normal=normal, ties=ties, equal=equal, special=special)


@pytest.mark.parametrize("B, D", [(1, 1), (2, 3), (65, 10), (300, 7)])
def test_permute_dims_is_a_stable_argsort_per_column(B, D):
    rng = np.random.default_rng(5)
    z = rng.normal(size=(B, D)).astype(np.float32)
    for name, keys in _key_sets(B, D, rng).items():
        out = R.permute_dims(z, keys)
        for d in range(D):
            # np.nan is the positive-sign NaN: numpy sorts it last, and so does the image; +0 and -0 compare equal in both
            assert np.array_equal(out[:, d], z[np.argsort(keys[:, d], kind="stable"), d]), (name, d)
            assert np.array_equal(np.sort(out[:, d]), np.sort(z[:, d]))
    assert np.array_equal(R.permute_dims(z, np.full((B, D), 0.5, np.float32)), z)


def test_key_image_is_monotone_and_total():
    vals = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf, np.nan], np.float32)
    img = R.key_image(vals).astype(np.int64)
    assert img[4] == img[5] and (np.diff(np.delete(img, 4)) > 0).all()
    neg_nan = np.array([0xFFC00000], np.uint32).view(np.float32)
    assert R.key_image(neg_nan)[0] < R.key_image(np.array([-np.inf], np.float32))[0]


# ---- the head ------------------------------------------------------------------------------------------------------------------
def test_softplus_form_at_large_logit_differences():
    l = np.array([[80.0, 0.0], [0.0, 80.0], [-40.0, 40.0], [40.0, -40.0]], np.float32)
    h = R.head(l, 2)
    assert np.isfinite([h["tc"], h["d_loss"], h["d_acc"]]).all() and np.isfinite(h["dl_d"]).all()
    assert R.softplus(80.0) == 80.0 and 0.0 < R.softplus(-80.0) < 1e-34
    assert abs(R.softplus(-80.0) - np.exp(-80.0)) <= 1e-15 * np.exp(-80.0)
    assert R.sigmoid(-80.0) > 0.0 and R.sigmoid(80.0) == 1.0
    t = torch.from_numpy(l).double()
    want = 0.5 * F.cross_entropy(t[:2], torch.tensor([0, 0])) + 0.5 * F.cross_entropy(t[2:], torch.tensor([1, 1]))
    assert abs(h["d_loss"] - want.item()) <= 1e-12 * want.item()
    assert h["tc"] == 0.0 and h["d_acc"] == 0.5
    # the naive form overflows in fp32 where this one does not
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.log(1 + np.exp(np.float32(100.0))))
    assert R.softplus(100.0) == 100.0


def test_head_of_a_single_label():
    l = R.make_logits(5, 1)[:5]
    h = R.head(l, 5)
    assert h["dl_d"] is None and h["dl_tc"].shape == (5, 2) and np.allclose(h["dl_tc"].sum(1), 0.0)


# ---- the stored vectors ------------------------------------------------------------------------------------------------------
def test_golden_vectors_reproduce():
    g = np.load(os.path.join(GOLDEN, "factor.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "factor.npz")) < 1 << 20
    for R0 in g["head_r0"]:
        p = f"head:{int(R0)}:"
        l = R.make_logits(int(R0), int(g[p + "seed"]))
        assert l.astype(np.float64).sum() == float(g[p + "checksum"])
        h = R.head(l, int(R0))
        d = np.abs(l[:, 0].astype(np.float64) - l[:, 1]).mean()
        assert abs(h["tc"]) >= 1e-2 * d and 0.0 < h["d_acc"] < 1.0
        for k in ("tc", "d_loss", "d_acc"):
            assert abs(h[k] - float(g[p + k])) <= 1e-12 * abs(float(g[p + k])), (p, k)
    slope = float(g["slope"])
    for B, zdim, hidden in g["ops"][:3]:
        p = f"op:{B}x{zdim}x{hidden}:"
        z, keys = R.make_inputs(int(B), int(zdim), int(g[p + "seed"]))
        Ws, bs = R.make_mlp(int(zdim), int(hidden), 2, int(g[p + "seed"]) + 1)
        assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in (z, keys, *Ws, *bs)])
        ref = R.factor(z, R.permute_dims(z, keys), Ws, bs, slope)
        for k in ("tc", "d_loss", "d_acc"):
            assert abs(ref[k] - float(g[p + k])) <= 1e-12 * abs(float(g[p + k])), (p, k)
        if p + "dz" in g.files:
            assert rel(ref["dz"], g[p + "dz"]) <= 1e-12 and rel(ref["dW"][0], g[p + "dW0"]) <= 1e-12


# ---- the surface -----------------------------------------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


def _solver(**kw):
    import models
    from solvers import FactorSolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    disc = models.Discriminator(10, hidden=16, layers=2)
    opt = lambda m: torch.optim.Adam(m.parameters(), lr=1e-4, betas=(0.5, 0.9))   # noqa: E731
    return FactorSolver(_DS(), model, 8, opt(model.encoder), opt(model.decoder), "mse", 1.0, 1.0, torch.device("cpu"),
                        False, None, discriminator=disc, optimizer_disc=opt(disc), **kw), disc


def test_solver_surface_and_validation():
    from solvers import VAESolver
    from solvers.factor import FactorSolver
    s, disc = _solver()
    assert isinstance(s, VAESolver) and s.gamma == 10.0 and s.discriminator is disc
    assert list(inspect.signature(FactorSolver.compute_kl_loss).parameters) == \
        list(inspect.signature(VAESolver.compute_kl_loss).parameters)
    for bad in (-1.0, float("nan"), float("inf"), "3", None, True):
        with pytest.raises(ValueError):
            s.gamma = bad
    s.gamma = 4
    assert s.gamma == 4.0 and isinstance(s.gamma, float)
    k0 = s._graph_key_extra()
    assert 4.0 in k0
    s.gamma = 8.0
    s.optimizer_disc.param_groups[0]["lr"] = 5e-5
    k1 = s._graph_key_extra()
    assert 8.0 in k1 and k1 != k0 and any(isinstance(e, tuple) and e[0] == "adam" and e[2][0] == 5e-5 for e in k1)
    with pytest.raises(ValueError):
        s.compute_kl_loss(None, torch.zeros(2, 10), torch.zeros(2, 10))
    with pytest.raises(ValueError):
        _solver(gamma=-2.0)
    # an optimiser without a fused update: no graph, whatever else holds
    s.enable_graph()
    s.optimizer_disc = torch.optim.Adadelta(disc.parameters())
    assert s._graph_ok() is False


def test_discriminator_module():
    import models
    from hipvae import abi
    torch.manual_seed(3)
    d = models.Discriminator(10)
    keys = list(d.state_dict())
    assert keys == [f"{2 * i}.{n}" for i in range(7) for n in ("weight", "bias")]
    assert d[0].weight.shape == (1000, 10) and d[12].weight.shape == (2, 1000) and d[1].negative_slope == 0.2
    torch.manual_seed(3)
    plain = torch.nn.Sequential(*[m for i in range(6) for m in (torch.nn.Linear(10 if i == 0 else 1000, 1000),
                                                                 torch.nn.LeakyReLU(0.2))], torch.nn.Linear(1000, 2))
    for (k, a), (_, b) in zip(d.state_dict().items(), plain.state_dict().items()):
        assert torch.equal(a, b), k                       # torch's default initialisation, in torch's order
    plain.load_state_dict(d.state_dict())
    assert [tuple(p.shape) for p in d.flat_parameters()] == [tuple(p.shape) for p in d.parameters()]
    with pytest.raises(abi.HipExtensionError):
        d(torch.zeros(4, 10))
    for bad in (0.0, -0.2, float("inf")):
        with pytest.raises(ValueError):
            models.Discriminator(10, slope=bad)


def test_no_cpu_path():
    import models
    import ops
    from hipvae import abi
    d = models.Discriminator(3, hidden=4, layers=1)
    z = torch.zeros(2, 3, requires_grad=True)
    for fn in (lambda: ops.permute_dims(z), lambda: ops.permute_dims(z, torch.zeros(2, 3)),
               lambda: ops.factor_tc(z, d), lambda: ops.factor_disc_loss(z, d), lambda: ops.factor_pass(z, d)):
        with pytest.raises(abi.HipExtensionError):
            fn()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_refuse_bad_arguments_before_any_launch():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    for n in NEW:
        assert n in abi.SIGNATURES and n + "(" in header and hasattr(ctypes.CDLL(abi.LIB_PATH), n)
    lib, X = abi.lib, ctypes.c_void_p(4096)            # a non-NULL pointer that is never followed: every call is refused
    # permute_dims: NULL pointers, B > 4096, D > 512, zero sizes, a row stride below D
    assert lib.itcv_permute_dims(None, 10, X, 10, X, None, 8, 10, None) != 0 and "itcv_permute_dims" in abi.last_error()
    assert lib.itcv_permute_dims(X, 10, None, 10, X, None, 8, 10, None) != 0
    assert lib.itcv_permute_dims(X, 10, X, 10, None, None, 8, 10, None) != 0
    assert lib.itcv_permute_dims(X, 10, X, 10, X, None, 4097, 10, None) != 0
    assert lib.itcv_permute_dims(X, 513, X, 513, X, None, 8, 513, None) != 0
    assert lib.itcv_permute_dims(X, 10, X, 10, X, None, 0, 10, None) != 0
    assert lib.itcv_permute_dims(X, 10, X, 10, X, None, 8, 0, None) != 0
    assert lib.itcv_permute_dims(X, 9, X, 10, X, None, 8, 10, None) != 0
    assert lib.itcv_permute_dims(X, 10, X, 9, X, None, 8, 10, None) != 0
    # the layers: NULL pointers, sizes, strides, slope <= 0 or not finite
    ok = (X, 10, X, X, X, 8, 10, 16, 0.2, None, 0, None)
    for k, v in ((0, None), (2, None), (4, None), (5, 0), (6, 0), (7, 0), (1, 9), (8, 0.0), (8, -0.2), (8, float("inf")),
                 (8, float("nan"))):
        a = list(ok)
        a[k] = v
        assert lib.itcv_linear_lrelu_fwd(*a) != 0, (k, v)
        assert "itcv_linear_lrelu_fwd" in abi.last_error()
    ok = (X, 16, X, X, 10, X, 8, 10, 16, 0.2, None, 0, None)
    for k, v in ((0, None), (2, None), (3, None), (5, None), (6, 0), (7, 0), (8, 0), (1, 15), (4, 9), (9, 0.0), (9, -1.0),
                 (9, float("nan"))):
        a = list(ok)
        a[k] = v
        assert lib.itcv_linear_dgrad_lrelu(*a) != 0, (k, v)
        assert "itcv_linear_dgrad_lrelu" in abi.last_error()
    # a split-K shape without its workspace is refused as well (K = 1000 at B = 64 splits)
    assert abi.lib.itcv_linear_workspace(64, 1000, 1000) > 0
    assert lib.itcv_linear_lrelu_fwd(X, 1000, X, X, X, 64, 1000, 1000, 0.2, None, 0, None) != 0
    assert "workspace" in abi.last_error()
    # the head: NULL pointers, R0 outside 1..R, the D walk without rows of label 1, another mode
    assert lib.itcv_disc_head_fwd(None, 4, 2, X, None) != 0 and lib.itcv_disc_head_fwd(X, 4, 2, None, None) != 0
    assert lib.itcv_disc_head_fwd(X, 4, 0, X, None) != 0 and lib.itcv_disc_head_fwd(X, 4, 5, X, None) != 0
    assert lib.itcv_disc_head_fwd(X, (1 << 24) + 1, 2, X, None) != 0
    for a in ((None, X, X, 4, 2, 1), (X, None, X, 4, 2, 1), (X, X, None, 4, 2, 1), (X, X, X, 4, 0, 0), (X, X, X, 4, 5, 0),
              (X, X, X, 4, 4, 1), (X, X, X, 4, 2, 2), (X, X, X, 4, 2, -1)):
        assert lib.itcv_disc_head_bwd(*a, None) != 0, a
        assert "itcv_disc_head_bwd" in abi.last_error()
