"""GPU tests of the importance-weighted bound (csrc/iwae.hip, ops.iwae_sample / iwae_bound, solvers/iwae.py,
hipvae.likelihood) against the fp64 restatement tests/iwae_ref.py.

Bounds, all normwise: scalars relative to the fp64 value, gradients and vectors as max |err| / max |value|.  The ceiling for
everything that leaves a kernel as fp32 (z, the loss and its terms, dmu, dlogvar, g_rows) is the project's fp32 bar, 1e-4;
with fp64 arithmetic inside, the expected error is the fp32 rounding of the outputs.  What stays fp64 end to end (lat, the
normalised weights, the per-image bound and ess, g_lat, the streaming state and its finalise) is held to 1e-11: at most 4096
terms of 2^-53 each, with room for the few ulp of exp and log.  The kernels and the restatement are fed the same fp32 rows;
otherwise a test would measure the conditioning of the softmax in rows (values of tens to hundreds, weights exponential in
them) and not the kernels.  The broadcast rows are compared bit for bit with itcv_recon_rows_fwd / _bwd on x.repeat.

Worst values measured on an MI355X over every case of test_sample_and_combine_against_restatement (printed by it):

    z 4.7e-08   loss 4.5e-08   rec 4.5e-08   kl 4.2e-08   bound 4.5e-08   ess 5.3e-08   g_rows 7.6e-08
    dmu  iwae 5.1e-08  stl 1.9e-07  dreg 1.9e-07        dlogvar  iwae 4.1e-08  stl 1.5e-07  dreg 1.5e-07
    lat 2.8e-16   w 3.1e-15   bound_b 1.6e-16   ess_b 3.0e-15                               (fp64 end to end)

(the upstream g = 1.7 reaches the kernels as an fp32 scalar, 2.8e-8 off, which the one-element shape amplifies by a mild
cancellation under stl / dreg).  Broadcast rows against the restatement: rows 9.1e-08, drecon 7.4e-08, and bit for bit equal
to the materialised form in all 36 cases.  Streaming form: 1.3e-15.  test_step_equals_its_expression_tree: the flat
gradients within 3.7e-07 (K = 1) and 1.9e-06 (K = 3) normwise, the returned dicts in the seventh digit.
"""
import math
import os

import numpy as np
import pytest
import torch

import iwae_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4            # what leaves a kernel as fp32
BAR64 = 1e-11         # what stays fp64 end to end
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())             # a copy: the stored cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    scale = np.abs(want).max()
    if scale == 0.0:
        assert not got.any()
        return 0.0
    return float(np.abs(got - want).max() / scale)


def hold(tag, name, got, want, bar):
    e = rel(got, want)
    WORST[name] = max(WORST.get(name, 0.0), e)
    assert e <= bar, (tag, name, e)
    return e


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "iwae.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def case(golden, B, K, D):
    """The inputs of a stored shape and the restatement's values, computed once per shape and never modified."""
    key = (B, K, D)
    if key not in _CASES:
        p = f"{B}x{K}x{D}:"
        seed = int(golden[p + "seed"])
        beta_rec, beta_kl = (float(v) for v in golden["hp"])
        mu, logvar, eps = R.make_inputs(B, K, D, seed)
        rows = np.random.default_rng(seed + 1).uniform(20.0, 60.0, size=K * B).astype(np.float32)
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in (mu, logvar, eps, rows)])
        z, lat = R.sample(mu, logvar, eps)
        ref = R.combine(rows, lat, B, beta_rec, beta_kl)
        assert abs(ref["loss"] - float(golden[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        dz = np.random.default_rng(seed + 2).normal(size=(K * B, D)).astype(np.float32)
        g = 1.7
        g_rows, g_lat = R.combine_grads(ref["w"], B, beta_rec, beta_kl, g)
        grads = {e: R.encoder_grads(mu, logvar, eps, dz, g_lat, ref["w"], e) for e in R.ESTIMATORS}
        for a in (mu, logvar, eps, rows, dz, z, lat):
            a.setflags(write=False)
        _CASES[key] = dict(mu=mu, logvar=logvar, eps=eps, rows=rows, dz=dz, z=z, lat=lat, ref=ref, g=g, g_rows=g_rows,
                           g_lat=g_lat, grads=grads, hp=(beta_rec, beta_kl))
    return _CASES[key]


def posterior(mu, logvar, layout):
    """(mu, logvar) device leaves: dense, or the two halves of the row slice [3:] of a wider nan-filled [3 + B, 2 D + 5]."""
    B, D = mu.shape
    if layout == "dense":
        return G(mu).requires_grad_(True), G(logvar).requires_grad_(True)
    wide = np.full((3 + B, 2 * D + 5), np.nan, dtype=np.float32)
    wide[3:, :D], wide[3:, D:2 * D] = mu, logvar
    w = G(wide).requires_grad_(True)
    a, b = w[3:, :D], w[3:, D:2 * D]
    assert B == 1 or a.stride() == (2 * D + 5, 1)
    return (a, b), w


# ---- 1. sample, combine and the three estimators against the restatement ---------------------------------------------------
SHAPES = [(1, 1, 1), (3, 2, 31), (4, 3, 32), (5, 63, 33), (65, 64, 64), (3, 65, 65), (4, 1024, 10), (1, 3, 512), (5, 1, 10),
          (65, 2, 1)]


@pytest.mark.parametrize("layout", ["dense", "strided"])
@pytest.mark.parametrize("B, K, D", SHAPES)
def test_sample_and_combine_against_restatement(golden, B, K, D, layout):
    import ops
    from hipvae import functional as HF
    assert golden["shapes"].tolist() == [list(s) for s in SHAPES]
    c = case(golden, B, K, D)
    beta_rec, beta_kl = c["hp"]
    ref, tag = c["ref"], f"[{B}x{K}x{D} {layout}]"
    for est in R.ESTIMATORS:
        if layout == "dense":
            m, l = posterior(c["mu"], c["logvar"], layout)
            leaves = (m, l)
        else:
            (m, l), wide = posterior(c["mu"], c["logvar"], layout)
            leaves = (wide,)
        sample = ops.iwae_sample(m, l, K, eps=G(c["eps"]))
        assert sample.z.shape == (K * B, D) and sample.z.dtype == torch.float32 and sample.z.is_contiguous()
        assert sample.lat.shape == (K * B,) and sample.lat.dtype == torch.float64
        rows = G(c["rows"]).requires_grad_(True)
        loss, terms, img = HF.IwaeCombineFn.apply(rows, sample.lat, sample, beta_rec, beta_kl, HF.IWAE_ESTIMATORS[est])
        assert loss.shape == () and loss.dtype == torch.float32 and not terms.requires_grad and not img.requires_grad
        total = c["g"] * loss + (sample.z * G(c["dz"])).sum()
        grads = torch.autograd.grad(total, (rows,) + leaves)
        if layout == "dense":
            dmu, dlv = N(grads[1]), N(grads[2])
        else:
            gw = N(grads[1])
            dmu, dlv = gw[3:, :D], gw[3:, D:2 * D]
            rest = gw.copy()
            rest[3:, :2 * D] = 0.0
            assert not rest.any()                                     # nothing outside the two views was touched
        want_dmu, want_dlv = c["grads"][est]
        e = dict(
            z=hold(tag, "z", N(sample.z), c["z"], BAR), lat=hold(tag, "lat", N(sample.lat), c["lat"], BAR64),
            w=hold(tag, "w", N(sample.weights), ref["w"], BAR64),
            bound_b=hold(tag, "bound_b", N(img[0]), ref["bound_b"], BAR64),
            ess_b=hold(tag, "ess_b", N(img[1]), ref["ess_b"], BAR64),
            loss=hold(tag, "loss", N(loss), ref["loss"], BAR), rec=hold(tag, "rec", N(terms[0]), ref["rec"], BAR),
            kl=hold(tag, "kl", N(terms[1]), ref["kl"], BAR), bound=hold(tag, "bound", N(terms[2]), ref["bound"], BAR),
            ess=hold(tag, "ess", N(terms[3]), ref["ess"], BAR),
            g_rows=hold(tag, "g_rows", N(grads[0]), c["g_rows"], BAR),
            dmu=hold(tag, "dmu_" + est, dmu, want_dmu, BAR), dlogvar=hold(tag, "dlogvar_" + est, dlv, want_dlv, BAR))
        print(tag, est, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    # the estimator is live: with more than one sample the three gradients differ
    if K > 1:
        a, b, d = (c["grads"][e][0] for e in R.ESTIMATORS)
        assert rel(a, b) > 1e-3 and rel(b, d) > 1e-3
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))


def _combine(rows, lat, B, K, beta_rec=1.0, beta_kl=1.0):
    from hipvae import functional as HF
    sample = HF.IwaeSample(B, K, dev())
    loss, terms, img = HF.IwaeCombineFn.apply(G(np.asarray(rows, np.float32)), G(np.asarray(lat, np.float64)), sample,
                                              beta_rec, beta_kl, 0)
    return N(loss), N(terms), N(img), N(sample.weights)


def test_one_sample_dominates():
    """logw gaps of 1000 within an image: exp underflows for every other sample, so only a max-shifted logsumexp is finite."""
    B, K = 5, 65
    rows = np.full((K, B), 2000.0, dtype=np.float32)
    rows[np.arange(B) * 7 % K, np.arange(B)] = 1000.0 - np.arange(B)
    lat = np.zeros(K * B)
    loss, terms, img, w = _combine(rows.reshape(-1), lat, B, K)
    ref = R.combine(rows.reshape(-1), lat, B, 1.0, 1.0)
    assert np.isfinite(img).all() and np.isfinite(loss)
    assert rel(img[0], ref["bound_b"]) <= BAR64 and rel(img[0], -(1000.0 - np.arange(B)) - math.log(K)) <= 1e-14
    assert np.array_equal(img[1], np.ones(B)) and np.array_equal(np.sort(w)[-B:], np.ones(B)) and w.sum() == B
    assert rel(loss, ref["loss"]) <= BAR and rel(terms[0], ref["rec"]) <= BAR


@pytest.mark.parametrize("K", [3, 64, 65, 1000])
def test_equal_weights_give_ess_k_exactly(K):
    B = 4
    rows = np.repeat(np.float32([40.0, 41.5, 17.25, 300.0])[None], K, 0).reshape(-1)
    lat = np.repeat(np.float64([0.5, -2.0, 7.0, 0.0])[None], K, 0).reshape(-1)
    loss, terms, img, w = _combine(rows, lat, B, K, 0.75, 0.5)
    assert np.array_equal(img[1], np.full(B, float(K))) and terms[3] == K
    assert np.array_equal(w, np.full(K * B, 1.0 / K))
    assert rel(img[0], -(0.75 * rows[:B].astype(np.float64) + 0.5 * lat[:B])) <= 1e-15


def test_one_sample_is_the_elbo_exactly():
    B = 7
    rng = np.random.default_rng(3)
    rows, lat = rng.uniform(20, 60, B).astype(np.float32), rng.normal(size=B) * 3
    loss, terms, img, w = _combine(rows, lat, B, 1, 0.75, 0.5)
    logw = -(0.75 * rows.astype(np.float64) + 0.5 * lat)
    assert np.array_equal(img[0], logw) and np.array_equal(w, np.ones(B)) and np.array_equal(img[1], np.ones(B))
    assert terms[3] == 1.0 and rel(loss, -logw.mean()) <= BAR


# ---- 2. the broadcast reconstruction rows -------------------------------------------------------------------------------
# P at the float4 and the two-slice edges; the last two rows make a block take two rows of an image at once (K B slices fill
# the grid on their own) with an odd row left over, on the scalar and on the float4 path
ROWS = [(5, 1, 1), (5, 3, 1), (5, 3, 3), (5, 1, 1023), (5, 3, 1023), (5, 1, 1024), (5, 3, 1024), (5, 3, 1025), (4, 1, 3072),
        (4, 3, 3072), (1100, 3, 3), (2100, 5, 8)]


@pytest.mark.parametrize("loss_type", R.LOSS_TYPES)
@pytest.mark.parametrize("B, K, P", ROWS)
def test_broadcast_rows_equal_the_materialised_rows_bit_for_bit(B, K, P, loss_type):
    from hipvae import abi
    from hipvae import functional as HF
    lt = abi.LOSS_TYPES[loss_type]
    x, recon = R.make_images(B, K, P, 100 + P + K, loss_type)
    xd, rd = G(x), G(recon).requires_grad_(True)
    rows = HF.IwaeRowsFn.apply(xd, rd, lt)
    g = G(np.random.default_rng(5).normal(size=K * B).astype(np.float32))
    (d,) = torch.autograd.grad(rows, (rd,), g)
    r2 = G(recon).requires_grad_(True)
    want = HF.ReconRowsFn.apply(xd.repeat(K, 1), r2, lt)
    (d2,) = torch.autograd.grad(want, (r2,), g)
    assert rows.dtype == torch.float32 and rows.shape == (K * B,)
    assert torch.equal(rows, want), float((rows - want).abs().max())
    assert torch.equal(d, d2)
    ref = R.rows(recon, x, loss_type)
    e = hold((B, K, P, loss_type), "rows", N(rows), ref, BAR)
    dref = g.double().cpu().numpy()[:, None] * R.derr(recon, np.tile(x, (K, 1)), loss_type)
    e2 = hold((B, K, P, loss_type), "drecon", N(d), dref, BAR)
    print(B, K, P, loss_type, f"rows {e:.2e} drecon {e2:.2e}")
    if loss_type == "bce":
        assert N(rows)[0] >= 100.0 and np.isfinite(N(d)).all()          # the log clamp at recon = 0 under x = 1


def test_bound_op_reads_x_in_place():
    """ops.iwae_bound on [B, C, H, W] images: the loss of the restatement, the gradient into recon of the chain."""
    import ops
    B, K, D = 4, 3, 10
    mu, logvar, eps = R.make_inputs(B, K, D, 9)
    x, recon = R.make_images(B, K, 3 * 8 * 8, 10)
    z, lat = R.sample(mu, logvar, eps)
    for loss_type in R.LOSS_TYPES:
        sample = ops.iwae_sample(G(mu), G(logvar), K, eps=G(eps))
        rd = G(recon).reshape(K * B, 3, 8, 8).requires_grad_(True)
        loss, terms = ops.iwae_bound(G(x).reshape(B, 3, 8, 8), rd, sample, 0.75, 0.5, loss_type, with_terms=True)
        rows32 = N(ops.reconstruction_loss(G(x).repeat(K, 1), G(recon), loss_type, "none"))
        ref = R.combine(rows32, lat, B, 0.75, 0.5)
        assert rel(N(loss), ref["loss"]) <= BAR and rel(N(terms), [ref[k] for k in ("rec", "kl", "bound", "ess")]) <= BAR
        (d,) = torch.autograd.grad(loss, (rd,))
        g_rows, _ = R.combine_grads(ref["w"], B, 0.75, 0.5)
        want = g_rows[:, None] * R.derr(recon, np.tile(x, (K, 1)), loss_type)
        assert rel(N(d).reshape(K * B, -1), want) <= BAR


# ---- 3. the streaming form ------------------------------------------------------------------------------------------------
def test_accumulate_in_chunks_equals_the_one_shot_combine():
    from hipvae import functional as HF
    B, K = 5, 130
    rng = np.random.default_rng(5)
    rows, lat = rng.uniform(20, 60, K * B).astype(np.float32), rng.normal(size=K * B) * 3
    want = R.combine(rows, lat, B, 0.75, 0.5)
    _, _, img, _ = _combine(rows, lat, B, K, 0.75, 0.5)
    rd, ld = G(rows), G(lat)
    outs = {}
    for chunk in (1, 7, 64, 130):
        state = torch.zeros((5, B), dtype=torch.float64, device=dev())
        for k0 in range(0, K, chunk):
            k1 = min(K, k0 + chunk)
            HF.iwae_accumulate(rd[k0 * B:k1 * B], ld[k0 * B:k1 * B], state, 0.75, 0.5)
        assert np.array_equal(N(state[4]), np.full(B, float(K)))
        outs[chunk] = [N(t) for t in HF.iwae_finalize(state)]
        for name, got, ref in zip(("log_px", "elbo", "ess"), outs[chunk], (want["bound_b"], want["elbo_b"], want["ess_b"])):
            e = hold(("accumulate", chunk), "stream_" + name, got, ref, BAR64)
            print("chunk", chunk, name, f"{e:.2e}")
        assert rel(outs[chunk][0], img[0]) <= BAR64 and rel(outs[chunk][2], img[1]) <= BAR64     # the one-shot kernel
    for chunk in (1, 7, 64):
        for a, b in zip(outs[chunk], outs[130]):
            assert rel(a, b) <= BAR64


# ---- 4. the step against its expression tree ------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


HP = dict(beta_kl=0.5, beta_rec=0.75, lr=2e-4)
B_STEP = 4


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


def _model(state):
    import models
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    return model.to(dev()).train()


def _solver(state, dataset=None, **kw):
    import solvers
    model = _model(state)
    solver = solvers.IWAESolver(dataset or _DS(), model, B_STEP, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                                torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", HP["beta_kl"],
                                HP["beta_rec"], dev(), False, None, clip=None, **kw)
    assert solver.conv_math == "fp32"
    return solver, model


def _grads(model):
    out = []
    for p in model.parameters():
        out.append(torch.zeros(p.numel(), device=dev()) if p.grad is None else p.grad.detach().reshape(-1).clone())
    return torch.cat(out)


@pytest.mark.parametrize("estimator", R.ESTIMATORS)
@pytest.mark.parametrize("K", [1, 3])
def test_step_equals_its_expression_tree(K, estimator):
    """One eager ``train_step`` against the same objective assembled from ``model.encode`` / ``model.decode`` on a twin,
    with the sampling, the rows and the combine in torch fp64 arithmetic (iwae_ref.torch_loss: autograd of the bound for
    "iwae", of the stop-gradient formulation for "stl"; x is repeated K times there).  The decoder's BatchNorm couples the
    K B rows, so "dreg" is the form that holds for any decoder: the weight multiplies the gradient that arrives at row r
    (``dreg_by_row``; for independently decoded rows the host test shows it equal to the squared-weight surrogate)."""
    import ops
    from hipvae.functional import conv_math_scope
    state = _init_state()
    g = torch.Generator().manual_seed(1 + K)
    x = torch.rand(B_STEP, 3, 32, 32, generator=g)
    eps = torch.randn(K * B_STEP, TINY["zdim"], generator=g)
    solver, model = _solver(state, num_samples=K, estimator=estimator)
    with ops.noise_queue([eps.clone()]):
        got = solver.train_step(x, 0)
    grads = _grads(model)
    twin = _model(state)
    xd = x.to(dev())
    with conv_math_scope("fp32"):
        mu, logvar = twin.encode(xd)
        surrogate, value = R.torch_loss(mu.double(), logvar.double(), eps.to(dev()).double(), xd.flatten(1).double(),
                                        lambda z: twin.decode(z.float()).flatten(1).double(), HP["beta_rec"],
                                        HP["beta_kl"], "mse", estimator, dreg_by_row=True)
        (solver.scale * surrogate).backward()
    want = dict(loss_enc=solver.scale * float(value["loss"]), loss_dec=solver.scale * float(value["loss"]),
                loss_kl=float(value["kl"]), loss_rec=float(value["rec"]), bound=float(value["bound"]),
                ess=float(value["ess"]))
    print(K, estimator, {k: (got[k], want[k]) for k in want})
    assert got["L2"] is None and set(got) == set(want) | {"L2"}
    for k in want:
        assert abs(got[k] - want[k]) <= BAR * abs(want[k]), (k, got[k], want[k])
    assert 1.0 <= got["ess"] <= K and (K > 1 or got["ess"] == 1.0)
    ref = _grads(twin)
    err = float((grads - ref).abs().max() / ref.abs().max())
    print(K, estimator, "flat gradients", err)
    assert err <= BAR, err


def test_captured_step_replays_the_eager_step_and_recaptures_on_a_switch():
    import ops
    state = _init_state()
    g = torch.Generator().manual_seed(7)
    batches = [torch.rand(B_STEP, 3, 32, 32, generator=g).to(dev()) for _ in range(2)]
    K, steps = 3, 6
    captured, _ = _solver(state, num_samples=K, estimator="dreg")
    captured.enable_graph()
    torch.cuda.manual_seed(1234)
    got = [captured.train_step(batches[k % 2], k) for k in range(steps)]
    assert len(captured._graphs) == 1 and captured._graph is not None
    key = captured._graph_key
    eager, _ = _solver(state, num_samples=K, estimator="dreg")
    torch.cuda.manual_seed(1234)
    for k in range(steps):
        draw = torch.randn((K * B_STEP, TINY["zdim"]), device=dev())
        with ops.noise_queue([draw]):
            want = eager.train_step(batches[k % 2], k)
        assert not getattr(eager, "_graphs", None)
        for name in ("loss_enc", "loss_kl", "loss_rec", "bound", "ess"):
            assert abs(got[k][name] - want[name]) <= BAR * abs(want[name]), (k, name, got[k][name], want[name])
    captured.num_samples = 2
    for k in range(steps, steps + 2):
        captured.train_step(batches[k % 2], k)
    assert len(captured._graphs) == 2 and captured._graph_key != key
    key = captured._graph_key
    captured.estimator = "stl"
    for k in range(steps + 2, steps + 4):
        captured.train_step(batches[k % 2], k)
    assert len(captured._graphs) == 3 and captured._graph_key != key


# ---- 5. the likelihood ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    from hipvae.dataset import DeviceImageTable
    imgs = np.random.default_rng(4).integers(0, 256, size=(16, 32, 32, 3), dtype=np.uint8)
    return DeviceImageTable.from_arrays(imgs, None, dev())


def _restated_likelihood(model, table, K, seed):
    """The restatement on the device model's own reconstructions: the draw of compute_log_likelihood for one chunk, z and
    the combine in fp64, the decoder in eval mode."""
    x = table.gather(np.arange(16))
    was = model.training
    model.eval()
    with torch.no_grad():
        mu, logvar = model.encode(x)
        eps = torch.randn((K * 16, mu.shape[1]), generator=torch.Generator().manual_seed(seed))
        z, lat = R.sample(N(mu), N(logvar), eps.numpy())
        recon = model.decode(torch.from_numpy(z).float().to(dev()))
    model.train(was)
    rows = R.rows(N(recon.flatten(1)), N(x.flatten(1)), "mse")
    return R.combine(rows, lat, 16, 1.0, 1.0)


def test_log_likelihood(table):
    from hipvae.likelihood import compute_log_likelihood
    model = _model(_init_state())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    a = compute_log_likelihood(table, model, num_samples=64, batch_size=16, seed=3)
    b = compute_log_likelihood(table, model, num_samples=64, batch_size=16, seed=3)
    assert set(a) == {"log_px", "bits_per_dim", "elbo", "ess", "per_image"}
    for k in ("log_px", "elbo", "ess"):
        assert np.array_equal(a["per_image"][k], b["per_image"][k]) and a[k] == b[k] and a["per_image"][k].shape == (16,)
    assert a["bits_per_dim"] == -a["log_px"] / (3 * 32 * 32 * math.log(2.0))
    other = compute_log_likelihood(table, model, num_samples=64, batch_size=16, seed=4)
    assert other["log_px"] != a["log_px"]
    # the flag and every buffer as found; torch's generators untouched
    assert model.training
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(cpu_state, torch.get_rng_state()) and torch.equal(dev_state, torch.cuda.get_rng_state(dev()))
    # one sample: the estimate is the ELBO sample itself
    one = compute_log_likelihood(table, model, num_samples=1, batch_size=16, seed=3)
    assert np.array_equal(one["per_image"]["log_px"], one["per_image"]["elbo"])
    assert np.array_equal(one["per_image"]["ess"], np.ones(16))
    # against the restatement, and K = 64 above K = 1 on the mean over the images with the restatement as the yardstick
    ref64, ref1 = _restated_likelihood(model, table, 64, 3), _restated_likelihood(model, table, 1, 3)
    print("log_px K=64", a["log_px"], ref64["bound"], "K=1", one["log_px"], ref1["bound"])
    assert rel(a["per_image"]["log_px"], ref64["bound_b"]) <= BAR and rel(a["per_image"]["elbo"], ref64["elbo_b"]) <= BAR
    assert rel(one["per_image"]["log_px"], ref1["bound_b"]) <= BAR
    assert ref64["bound"] >= ref1["bound"] and a["log_px"] >= one["log_px"]
    assert a["log_px"] >= a["elbo"] and 1.0 <= a["ess"] <= 64.0
    # chunks and batches change the draws' shapes, not the estimator: K = 64 in chunks of 7 over batches of 5 stays close
    c = compute_log_likelihood(table, model, num_samples=64, chunk=7, batch_size=5, seed=3)
    assert c["per_image"]["log_px"].shape == (16,) and abs(c["elbo"] - a["elbo"]) <= 0.05 * abs(a["elbo"])
    sub = compute_log_likelihood(table, model, num_samples=2, indices=[3, 9], seed=3)
    assert sub["per_image"]["indices"].tolist() == [3, 9] and sub["per_image"]["log_px"].shape == (2,)


class _Recorder:
    def __init__(self):
        self.log = {}

    def add_scalar(self, tag, value, global_step=None):
        self.log[tag] = (float(value), global_step)

    def add_scalars(self, tag, values, global_step=None):
        self.log[tag] = ({k: float(v) for k, v in values.items()}, global_step)

    def flush(self):
        pass


def test_extra_scores_write_the_log_likelihood_record(table):
    from hipvae.likelihood import compute_log_likelihood
    solver, model = _solver(_init_state(), dataset=table, num_samples=2)
    solver.writer, solver.test_iter = _Recorder(), 5
    solver.extra_scores = ("log_likelihood",)
    solver.likelihood_params = dict(num_samples=4, seed=2)
    solver.write_disentanglemnt_scores(3)
    assert not solver.writer.log
    solver.write_disentanglemnt_scores(10)
    rec, step = solver.writer.log["log_likelihood"]
    want = compute_log_likelihood(table, model, num_samples=4, seed=2, batch_size=B_STEP, loss_type="mse",
                                  beta_rec=HP["beta_rec"])
    assert step == 10 and rec == {k: want[k] for k in ("log_px", "bits_per_dim", "elbo", "ess")} and model.training


# ---- 6. refusals leave the outputs alone ------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    from hipvae import abi
    B, K, D, P = 4, 3, 10, 64
    f32 = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=dev())          # noqa: E731
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=dev())          # noqa: E731
    mu, lv, eps, z, lat = f32(B, D), f32(B, D), f32(K * B, D), f32(K * B, D), f64(K * B)
    x, recon, rows, ws = f32(B, P), f32(K * B, P), f32(K * B), f64(K * B)
    wt, img, out, terms, state = f64(K * B), f64(4, B), f32(1), f32(4), f64(5, B)
    p = lambda t: t.data_ptr()                                                      # noqa: E731
    st = abi.stream()
    calls = [
        ("itcv_iwae_sample_fwd", p(mu), D, p(lv), D, p(eps), D, p(z), p(lat), B, 0, D, st),
        ("itcv_iwae_sample_fwd", p(mu), D - 1, p(lv), D, p(eps), D, p(z), p(lat), B, K, D, st),
        ("itcv_iwae_sample_fwd", p(mu), 513, p(lv), 513, p(eps), 513, p(z), p(lat), B, K, 513, st),
        ("itcv_iwae_sample_fwd", p(mu), D, None, D, p(eps), D, p(z), p(lat), B, K, D, st),
        ("itcv_iwae_sample_bwd", p(z), D, p(lat), None, p(mu), D, p(lv), D, p(eps), D, p(mu), p(lv), B, K, D, 2, st),
        ("itcv_iwae_sample_bwd", p(z), D, p(lat), p(wt), p(mu), D, p(lv), D, p(eps), D, p(mu), p(lv), B, 1025, D, 0, st),
        ("itcv_iwae_rows_fwd", p(x), p(recon), p(rows), B, K, P, 5, p(ws), ws.numel() * 8, st),
        ("itcv_iwae_rows_fwd", p(x), p(recon), p(rows), B, K, P, 0, p(ws), 8, st),
        ("itcv_iwae_rows_bwd", p(x), p(recon), p(rows), p(recon), B, 0, P, 0, st),
        ("itcv_iwae_combine_fwd", p(rows), p(lat), float("nan"), 1.0, p(wt), p(img), p(out), p(terms), B, K, st),
        ("itcv_iwae_combine_fwd", p(rows), p(lat), 1.0, 1.0, p(wt), p(img), p(out), p(terms), 1 << 15, 1024, st),
        ("itcv_iwae_combine_bwd", p(out), p(wt), 1.0, 1.0, p(rows), p(lat), B, 1025, st),
        ("itcv_iwae_accumulate", p(rows), p(lat), 1.0, float("inf"), p(state), B, K, st),
        ("itcv_iwae_finalize", p(state), p(lat), p(lat), None, B, st),
    ]
    for args in calls:
        assert getattr(abi.lib, args[0])(*args[1:]) != 0, args[0]
        assert abi.last_error().startswith(args[0])
    torch.cuda.synchronize()
    for t in (mu, lv, eps, z, lat, x, recon, rows, ws, wt, img, out, terms, state):
        assert bool((t == 7.0).all())
