"""GPU tests of the Ada-GVAE / Ada-ML-VAE latent op (csrc/ada.hip, ops.ada_group), its solver (solvers/ada.py) and the
pair loader (hipvae.dataset.DevicePairLoader) against the fp64 restatement tests/ada_ref.py.

Bounds: the own mask equals the restatement's exactly (the inputs hold the margin condition of ada_ref.make_inputs, so the
mask does not hang on the last bit of an exp); the loss and the two terms relative to the fp64 value; z, dmu and dlogvar
normwise, max |err| / max |value|.  The ceiling is the project's fp32 bar, 1e-4; a quantity that is exactly zero in fp64
must come out exactly zero.  The kernels compute in fp64 and round once to fp32, so they stay near 2^-24 = 6e-8.  Worst
values measured on an MI355X over every case of test_kernel_against_restatement (printed by it):

    loss 5.60e-08  kl 5.79e-08  shared 4.15e-08  z 5.07e-08  dmu 5.21e-08  dlogvar 4.82e-08
"""
import os

import numpy as np
import pytest
import torch

import ada_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
# the wave's 64-column edges at -1 / 0 / +1, the four-pairs-per-block tail, the register maximum (D = 512: 8 per lane) and
# a grid larger than one trip (256 blocks of 4 pairs)
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 64), (4, 63), (5, 65), (33, 10), (7, 128), (32, 128), (9, 129), (2, 511), (3, 512),
          (1025, 10)]
G_LOSS = -1.25
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a, order="C")).to(dev())      # a copy: the cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "ada.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def case(golden, B, D, averaging, mask):
    """The stored inputs of a shape and the restatement's values, computed once per case and never modified."""
    key = (B, D, averaging, mask)
    if key not in _CASES:
        p = f"{B}x{D}:"
        beta = float(golden["hp"][0])
        mu, lv, eps, seed = R.make_inputs(B, D, int(golden[p + "seed"]))
        assert seed == int(golden[p + "seed"])
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in (mu, lv, eps)])
        own = R.make_mask(B, D, seed) if mask == "external" else None
        dz = R.make_dz(B, D, seed)
        ref = R.ada(mu, lv, eps, beta, averaging, own, dz, G_LOSS)
        want = float(golden[p + f"{averaging}:{mask}:loss"])
        assert abs(ref["loss"] - want) <= 1e-12 * abs(want)
        for a in (mu, lv, eps, dz, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _CASES[key] = dict(mu=mu, lv=lv, eps=eps, own=own, dz=dz, ref=ref, beta=beta)
    return _CASES[key]


def strided(x):
    """The right part of a wider nan tensor."""
    wide = np.full((x.shape[0], x.shape[1] + 3), np.nan, dtype=np.float32)
    wide[:, 3:] = x
    return G(wide)[:, 3:]


def layouts(mu, lv, eps, layout):
    """(mu, logvar, eps) device tensors holding the given values in the given layout."""
    R2, D = mu.shape
    if layout == "dense":
        return G(mu), G(lv), G(eps)
    if layout == "packed":            # the halves of one [2B, 2D] tensor, inside nan rows that must not be read
        buf = np.full((R2 + 2, 2 * D), np.nan, dtype=np.float32)
        buf[1:-1, :D], buf[1:-1, D:] = mu, lv
        t = G(buf)[1:-1]
        a, b = t[:, :D], t[:, D:]
        assert a.stride() == (2 * D, 1) and b.data_ptr() == a.data_ptr() + 4 * D
        return a, b, G(eps)
    if layout == "strided":
        out = tuple(strided(x) for x in (mu, lv, eps))
        assert out[0].stride() == (D + 3, 1)
        return out
    raise ValueError(layout)


def run(c, averaging, layout="dense", dz=None, g=G_LOSS, beta=None):
    """z, loss, mask, terms and both gradients of ops.ada_group on the device; ``dz`` a device tensor or None (the
    case's, dense)."""
    import ops
    a, b, e = layouts(c["mu"], c["lv"], c["eps"], layout)
    a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    own = None if c["own"] is None else G(c["own"])
    z, loss, mask, terms = ops.ada_group(a, b, c["beta"] if beta is None else beta, averaging, own=own, eps=e,
                                         with_terms=True)
    R2, D = c["mu"].shape
    assert z.shape == (R2, D) and loss.shape == () and mask.shape == (R2 // 2, D) and terms.shape == (2,)
    assert mask.dtype == torch.uint8 and not mask.requires_grad and not terms.requires_grad
    assert z.requires_grad and loss.requires_grad
    dz = G(c["dz"]) if dz is None else dz
    dmu, dlv = torch.autograd.grad((z, loss), (a, b), grad_outputs=(dz, torch.tensor(g, device=dev())))
    return dict(z=z.detach(), loss=loss.detach(), own=mask, terms=terms, dmu=dmu, dlv=dlv)


def errors(got, ref):
    """Errors of a run against the restatement; a quantity that is exactly zero there must be exactly zero."""
    def rel(x, want):
        x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
        scale = np.abs(want).max()
        if scale == 0.0:
            assert not x.any()
            return 0.0
        assert np.isfinite(x).all()
        return float(np.abs(x - want).max() / scale)

    assert np.array_equal(got["own"].cpu().numpy() != 0, ref["own"]), "the own mask differs from the restatement's"
    t = N(got["terms"])
    return dict(loss=rel(N(got["loss"]), ref["loss"]), kl=rel(t[0], ref["terms"][0]), shared=rel(t[1], ref["terms"][1]),
                z=rel(N(got["z"]), ref["z"]), dmu=rel(N(got["dmu"]), ref["dmu"]), dlogvar=rel(N(got["dlv"]), ref["dlogvar"]))


def check(got, ref, tag):
    e = errors(got, ref)
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= BAR, (tag, k, v)
    return e


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("averaging", R.AVERAGINGS)
@pytest.mark.parametrize("B, D", SHAPES)
def test_kernel_against_restatement(golden, B, D, averaging, mask):
    c = case(golden, B, D, averaging, mask)
    dense = run(c, averaging)
    check(dense, c["ref"], f"[{B}x{D} {averaging} {mask} dense]")
    # the same bits from the packed pair and from strided views, both read in place: the nan around them is not read
    for layout in ("packed", "strided"):
        other = run(c, averaging, layout=layout)
        for k in dense:
            assert torch.equal(dense[k], other[k]), (layout, k)
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


@pytest.mark.parametrize("averaging", R.AVERAGINGS)
def test_exact_zeros(golden, averaging):
    """What is exactly zero in fp64 is exactly zero: without an incoming gradient of z and with beta = 0 both gradients and
    the loss; with an all-own mask the shared count; with beta = 0 alone the KL's share of the gradients."""
    c = case(golden, 33, 10, averaging, "external")
    zero = torch.zeros(66, 10, device=dev())
    got = run(c, averaging, dz=zero, beta=0.0)
    assert not got["dmu"].any() and not got["dlv"].any() and float(got["loss"]) == 0.0
    ref = R.ada(c["mu"], c["lv"], c["eps"], 0.0, averaging, c["own"], c["dz"], G_LOSS)
    check(run(c, averaging, beta=0.0), ref, f"[33x10 {averaging} beta = 0]")
    ref = R.ada(c["mu"], c["lv"], c["eps"], c["beta"], averaging, c["own"], None, G_LOSS)
    check(run(c, averaging, dz=zero), ref, f"[33x10 {averaging} dz = 0]")
    allown = dict(c, own=np.ones((33, 10), np.uint8))
    ref = R.ada(c["mu"], c["lv"], c["eps"], c["beta"], averaging, allown["own"], c["dz"], G_LOSS)
    got = run(allown, averaging)
    check(got, ref, f"[33x10 {averaging} all own]")
    assert float(got["terms"][1]) == 0.0 and got["own"].all()


# ---- 2. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("averaging", R.AVERAGINGS)
@pytest.mark.parametrize("B, D", [(33, 10), (32, 128), (9, 129), (3, 512), (1025, 10)])
def test_bitwise_repeatable(golden, B, D, averaging, mask):
    c = case(golden, B, D, averaging, mask)
    a, b = run(c, averaging), run(c, averaging)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    if mask == "threshold":
        # the mask the op returned, handed back as an external one, gives the same bits again
        again = run(dict(c, own=a["own"].cpu().numpy()), averaging)
        for k in a:
            assert torch.equal(a[k], again[k]), k


@pytest.mark.parametrize("averaging", R.AVERAGINGS)
@pytest.mark.parametrize("B, D", [(5, 65), (33, 10)])
def test_non_contiguous_output_gradient(golden, B, D, averaging):
    """An incoming dz with a row stride (read in place), with a column stride (copied dense) and a broadcast one (what
    ``z.sum().backward()`` sends) give the bits of the dense dz."""
    import ops
    c = case(golden, B, D, averaging, "threshold")
    dense = run(c, averaging)
    wide = strided(c["dz"])
    assert not wide.is_contiguous()
    tr = G(np.ascontiguousarray(c["dz"].T)).t()
    assert tr.shape == (2 * B, D) and tr.stride() == (1, 2 * B)
    for dz in (wide, tr):
        got = run(c, averaging, dz=dz)
        for k in dense:
            assert torch.equal(dense[k], got[k]), k
    a, b = G(c["mu"]).requires_grad_(True), G(c["lv"]).requires_grad_(True)
    z, loss = ops.ada_group(a, b, c["beta"], averaging, eps=G(c["eps"]))
    (z.sum() + G_LOSS * loss).backward()
    ones = run(c, averaging, dz=torch.ones(2 * B, D, device=dev()))
    assert torch.equal(a.grad, ones["dmu"]) and torch.equal(b.grad, ones["dlv"])


def test_noise_source_and_refusals():
    """``eps=None`` takes ONE draw from the project's noise source; what the op cannot take is refused."""
    import ops
    from hipvae import abi
    mu, lv, eps, _ = R.make_inputs(4, 10, 5)
    with ops.noise_queue([torch.from_numpy(eps), torch.zeros(1)]) as _:
        z, loss = ops.ada_group(G(mu), G(lv), 0.5)
        assert len(ops._noise["queue"]) == 1
    want, _ = ops.ada_group(G(mu), G(lv), 0.5, eps=G(eps))
    assert torch.equal(z, want)
    with pytest.raises(ValueError):
        ops.ada_group(G(mu)[:7], G(lv)[:7], 0.5)
    with pytest.raises(ValueError):
        ops.ada_group(G(mu), G(lv), 0.5, averaging="argmax")
    with pytest.raises(abi.HipExtensionError):
        ops.ada_group(G(mu), G(lv), 0.5, eps=torch.from_numpy(eps))
    with pytest.raises(abi.HipExtensionError):
        ops.ada_group(G(mu).double(), G(lv).double(), 0.5)


# ---- 3. the solver -----------------------------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


HP = dict(beta_kl=0.5, beta_rec=0.75, clip=100.0, lr=2e-4)
PAIRS = 4


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


def _model(state):
    import models
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    return model.to(dev()).train()


def _solver(state, cls=None, **kw):
    from solvers import AdaGVAESolver
    cls = AdaGVAESolver if cls is None else cls
    model = _model(state)
    solver = cls(_DS(), model, 2 * PAIRS, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                 torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", HP["beta_kl"], HP["beta_rec"], dev(),
                 False, None, clip=HP["clip"], **kw)
    assert solver.conv_math == "fp32"
    return solver, model


def _batch(seed=1):
    """[2B, 3, 32, 32]: the second image of a pair is the first with one quadrant redrawn, so the pairs share structure."""
    g = torch.Generator().manual_seed(seed)
    first = torch.rand(PAIRS, 3, 32, 32, generator=g)
    second = first.clone()
    second[:, :, :16, :16] = torch.rand(PAIRS, 3, 16, 16, generator=g)
    return torch.cat([first, second]), torch.randn(2 * PAIRS, TINY["zdim"], generator=g)


def _params_close(model, other, lr, steps=1):
    """The bar of tests/test_hip_model.py's run_golden_steps: Adam's first updates are +-lr sign(g), so where |g| is at
    rounding level 2 lr of a weight can differ; the bulk is bounded tightly and every element by the Adam limit."""
    a, b = model.state_dict(), other.state_dict()
    diffs = torch.cat([(a[k] - b[k]).abs().reshape(-1) for k in a if a[k].dtype.is_floating_point and "running" not in k])
    assert float(diffs.max()) <= 2.05 * lr * steps, float(diffs.max())
    assert float((diffs > 0.25 * lr * steps).float().mean()) < 2e-3
    assert float(diffs.median()) < 0.02 * lr
    for k in a:
        if "running" in k:
            err = float((a[k] - b[k]).abs().max() / b[k].abs().max())
            assert err < 1e-3, (k, err)


@pytest.mark.parametrize("averaging", R.AVERAGINGS)
def test_train_step_equals_the_assembled_step(averaging):
    """One ``train_step`` with a queued draw against the same step assembled from ``model.encode``, the torch-fp64
    transcription of the op, ``model.decode``, the existing loss ops, torch's clip and torch's Adam: the returned dict to
    1e-4 (the bar of the existing solver tests at step 0), the parameters within their Adam bar."""
    import ops
    from hipvae.functional import conv_math_scope
    state = _init_state()
    x, eps = _batch()
    solver, model = _solver(state, averaging=averaging)
    with ops.noise_queue([eps.clone()]):
        got = solver.train_step(x, 0)
    # the assembled step
    ref_model = _model(state)
    opts = [torch.optim.Adam(m.parameters(), lr=HP["lr"]) for m in (ref_model.encoder, ref_model.decoder)]
    xd = x.to(dev())
    with conv_math_scope("fp32"):
        mu, logvar = ref_model.encode(xd)
        z64, kl64, own, terms = R.torch_op(mu.double(), logvar.double(), eps.to(dev()).double(), HP["beta_kl"], averaging)
        loss_kl = kl64.float()
        rec = ref_model.decode(z64.float())
        loss_rec = ops.reconstruction_loss(xd, rec, "mse", "mean", scale=HP["beta_rec"])
        loss = solver.scale * (loss_rec + loss_kl)
        loss.backward()
    params = [p for p in ref_model.parameters() if p.grad is not None]
    norm = torch.nn.utils.clip_grad_norm_(params, HP["clip"])
    for o in opts:
        o.step()
    loss, loss_kl, loss_rec = loss.detach(), loss_kl.detach(), loss_rec.detach()
    want = dict(loss_enc=float(loss), loss_dec=float(loss), loss_kl=float(loss_kl), loss_rec=float(loss_rec),
                L2=float(norm), shared_dims=float(terms[1]))
    print(averaging, {k: (got[k], want[k]) for k in want})
    assert set(got) == set(want)
    assert want["shared_dims"] == got["shared_dims"] and 0.0 < want["shared_dims"] < TINY["zdim"]
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]), (k, got[k], want[k])
    _params_close(model, ref_model, HP["lr"])


def test_all_own_step_equals_the_vae_step():
    """With every dimension own the op is reparameterize + kl_divergence, and the step that of ``VAESolver`` on the same
    2B rows with the same draw -- WITHIN THE BAR, not bit for bit: the op evaluates z and the KL sums in fp64 and rounds
    once, ``itcv_reparam_fwd`` / ``itcv_kl_loss_fwd`` work in fp32, so z differs in its last bit here and there."""
    import ops
    from solvers import VAESolver
    state = _init_state()
    x, eps = _batch(2)
    ada, m_ada = _solver(state)
    ada.own_mask = torch.ones(PAIRS, TINY["zdim"], dtype=torch.uint8, device=dev())
    vae, m_vae = _solver(state, cls=VAESolver)
    with ops.noise_queue([eps.clone()]):
        got = ada.train_step(x, 0)
    with ops.noise_queue([eps.clone()]):
        want = vae.train_step(x, 0)
    print({k: (got[k], want[k]) for k in want})
    assert got.pop("shared_dims") == 0.0 and set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]), (k, got[k], want[k])
    _params_close(m_ada, m_vae, HP["lr"])


def test_captured_steps_equal_eager_steps_and_averaging_recaptures():
    """With enable_graph() the trajectory follows the eager one from the same state through the capture (steps 3-5 are
    replays); after ``averaging = "mlvae"`` it still does, under another graph key: the switch re-captures."""
    state = _init_state()
    xs = [_batch(5)[0].to(dev()), _batch(6)[0].to(dev())]

    def trajectory(graph, switch=True):
        solver, model = _solver(state)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], []
        for k in range(9):
            if k == 6 and switch:
                solver.averaging = "mlvae"
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8) else None)
        ngraphs = len(solver._graphs) if graph else 0
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), keys, ngraphs

    (e, we, _, _), (gr, wg, keys, ngraphs) = trajectory(False), trajectory(True)
    assert keys[3] is not None and "gvae" in keys[3] and keys[3] == keys[4] == keys[5]
    assert keys[7] is not None and "mlvae" in keys[7] and keys[7] == keys[8] != keys[5]
    assert ngraphs == 2
    for x, y in zip(e, gr):
        assert set(x) == set(y) and "shared_dims" in x
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((we - wg).abs().max()) < 1e-6
    # the switch is visible in the eager trajectory itself: without it the last step reports other numbers
    never = trajectory(False, switch=False)[0]
    print("switched / not:", e[8], never[8])
    assert any(abs(e[8][k] - never[8][k]) > 1e-5 * abs(e[8][k]) + 1e-9 for k in ("loss_kl", "loss_rec", "shared_dims"))


# ---- 4. the pair loader --------------------------------------------------------------------------------------------------
def _table():
    from hipvae.dataset import DeviceImageTable
    imgs = np.random.default_rng(3).integers(0, 256, size=(60, 4, 4, 3), dtype=np.uint8)
    table = DeviceImageTable.from_arrays(imgs, np.arange(60), dev())
    table.factor_sizes, table.latent_indices = [4, 3, 5], [0, 2]          # the middle factor does not vary
    return table


@pytest.mark.parametrize("k", [1, 2, -1])
def test_pair_loader(k):
    from hipvae.dataset import DevicePairLoader, factor_bases
    table = _table()
    B = 16
    if k == 2:                                    # two latent factors: both change
        loader = DevicePairLoader(table, B, k=2, seed=9, steps_per_epoch=3)
    elif k == -1:                                 # 1 .. num_latents - 1 = 1
        loader = DevicePairLoader(table, B, k=-1, seed=9, steps_per_epoch=3)
    else:
        loader = DevicePairLoader(table, B, seed=9, steps_per_epoch=3, device=dev())
    assert len(loader) == 3 and len(DevicePairLoader(table, 5)) == 6
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    bases = np.array(factor_bases(table.factor_sizes))
    assert bases.tolist() == [15, 5, 1]
    epochs = []
    for _ in range(2):
        batches = []
        for x, changed in loader:
            first, second = (f.cpu().numpy() for f in loader.factors)
            assert x.shape == (2 * B, 3, 4, 4) and x.dtype == torch.float32 and x.device == dev()
            assert changed.shape == (B, 2) and changed.dtype == torch.bool
            # the gathered pairs are the table's images at the indices recomputed on the host from the factors
            assert torch.equal(x[:B], table.gather(first @ bases)) and torch.equal(x[B:], table.gather(second @ bases))
            ch = changed.cpu().numpy()
            assert (ch.sum(1) == (2 if k == 2 else 1)).all()
            full = np.zeros((B, 3), bool)
            full[:, [0, 2]] = ch
            assert not ((first != second) & ~full).any()          # only flagged factors may differ; factor 1 never does
            for f in (first, second):
                assert (f >= 0).all() and (f < np.array([4, 3, 5])).all()
            batches.append((x.clone(), changed.clone()))
        epochs.append(batches)
        assert len(batches) == 3
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(*epochs))      # the generator moves on between epochs
    differs = torch.cat([(x[:B] != x[B:]).flatten(1).any(1) for ep in epochs for x, _ in ep])
    assert differs.any() and not differs.all() or k == 2                  # a redrawn value may equal the old one
    # the same seed gives the same epochs; torch's global streams are untouched
    again = DevicePairLoader(table, B, k=k, seed=9, steps_per_epoch=3)
    for ep in epochs:
        for (x, ch), (x2, ch2) in zip(ep, again):
            assert torch.equal(x, x2) and torch.equal(ch, ch2)
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state(dev()))
    other = next(iter(DevicePairLoader(table, B, k=k, seed=10, steps_per_epoch=1)))
    assert not torch.equal(other[0], epochs[0][0][0])
    # pre_process sees (x, changed)
    pre = next(iter(DevicePairLoader(table, B, k=k, seed=9, steps_per_epoch=1, pre_process=lambda x, c: (x * 2, c))))
    assert torch.equal(pre[0], epochs[0][0][0] * 2)


def test_pair_loader_feeds_the_solver():
    """Two steps of the solver on the loader's batches (3-channel 32 x 32 table of 4 * 3 * 5 images)."""
    from hipvae.dataset import DeviceImageTable, DevicePairLoader
    imgs = np.random.default_rng(4).integers(0, 256, size=(60, 32, 32, 3), dtype=np.uint8)
    table = DeviceImageTable.from_arrays(imgs, None, dev())
    table.factor_sizes, table.latent_indices = [4, 3, 5], [0, 1, 2]
    solver, _ = _solver(_init_state())
    torch.cuda.manual_seed(7)
    for i, (x, changed) in enumerate(DevicePairLoader(table, PAIRS, k=1, seed=1, steps_per_epoch=2)):
        out = solver.train_step(x, i)
        assert np.isfinite([v for v in out.values()]).all() and 0.0 <= out["shared_dims"] <= TINY["zdim"]
