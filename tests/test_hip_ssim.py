"""The SSIM kernels (csrc/ssim.hip) on the device against the numpy fp64 restatement tests/ssim_ref.py, within the a-priori
bound derived in that file's docstring (no tolerance here is taken from what the kernels give):

    |out - ref| <= ssim_bound + 2^-24 |ref|        (fp32 results: the loss and dy; the second term is their one rounding)
    |stats - ref| <= stats_bound                   (fp64 results)

tests/test_ssim_ref_host.py pins the restatement and holds every input used here to bound <= 1e-9 P per row and <= 1e-9
max |dy|, three orders of magnitude under what an fp32 evaluation of the map is off by.

Shapes: the table of the issue with its 32 replaced by the kernels' tile T = 16 (ssim_ref.SHAPES): one position; 2 x 7
positions; one row of positions three tiles wide; 17 x 16 positions (a one-row partial tile next to full ones); the tiny
model's and a c2 image; K = 3 and K = 15.  Inputs: uniform, smooth pairs, binary, a constant plane against noise, y = x.

alpha = 0 against ops.reconstruction_loss(.., "l1") is taken at reduction "none" and scale 1: the inputs are multiples of
2^-24, so the fp32 differences of the l1 kernel are exact and its row is the fp32 rounding of the same sum in another
order; with a scale that kernel rounds twice (the row, then scale * row), and its "sum" adds rounded rows, neither of which
the bound's single rounding covers.

Worst observed error / allowance on one MI355X, per quantity, over all cases (the tests print them): the fp64 statistics
0.039 of their bound (3.8e-15 absolute); the loss 0.973 and dy 0.999, which is the one fp32 rounding the allowance's second
term stands for (an error of half an ulp of fp32; the bound's own share is three orders of magnitude smaller); alpha = 0
against the l1 kernel: equal bits in every case; reconstruction_quality: ssim 2e-4, ms_ssim 5e-4, mse 2e-4 of their
bounds, psnr and l1 equal."""
import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
HP = dict(beta_kl=0.5, beta_rec=0.75, beta_neg=512.0, gamma_r=1e-8, clip=100.0, lr=2e-4)
WORST = {}


def dev():
    return torch.device("cuda")


def G(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=dev())


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def note(what, err, allowed):
    """Keeps the worst error / allowance (and the absolute error there) of a quantity and returns the violations."""
    err, allowed = np.asarray(err, dtype=np.float64).reshape(-1), np.asarray(allowed, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / allowed, 0.0)
    i = int(ratio.argmax())
    if ratio[i] >= WORST.get(what, (-1.0, 0.0))[0]:
        WORST[what] = (float(ratio[i]), float(err[i]))
    return int((err > allowed).sum())


def run_loss(x, y, alpha, reduction, scale, K, gup=None):
    import ops
    tx, ty = G(x), G(y).requires_grad_(gup is not None)
    out = ops.ssim_loss(tx, ty, reduction, scale, alpha=alpha, window=K)
    assert out.dtype == torch.float32 and out.shape == ((x.shape[0],) if reduction == "none" else ())
    if gup is None:
        return out, None
    out.backward(G(gup).reshape(out.shape))
    assert ty.grad.dtype == torch.float32 and ty.grad.shape == ty.shape
    return out, ty.grad


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_kernels_against_restatement(shape, kind):
    import ops
    from hipvae import functional as HF
    B, C, H, W, K = shape
    P = C * H * W
    x, y = R.make_pair(kind, (B, C, H, W))
    bad = 0
    for alpha in R.ALPHAS:
        for reduction in R.REDUCTIONS:
            gup = R.upstream(B, reduction)
            for scale in (1.0, 0.75 / P):
                out, dy = run_loss(x, y, alpha, reduction, scale, K, gup)
                ref, bound = R.loss(x, y, alpha, reduction, scale, K), R.ssim_bound(x, y, alpha, reduction, scale, K)
                bad += note("loss", np.abs(N(out) - ref), bound + 2.0 ** -24 * np.abs(ref))
                gref, gbound = R.grad(x, y, gup, alpha, reduction, scale, K), R.grad_bound(x, y, gup, alpha, reduction, scale, K)
                bad += note("dy", np.abs(N(dy) - gref), gbound + 2.0 ** -24 * np.abs(gref))
                if kind == "same":
                    assert (out == 0).all(), (alpha, reduction, scale, out)
        if alpha == 0.0:
            mine, _ = run_loss(x, y, 0.0, "none", 1.0, K)
            l1 = ops.reconstruction_loss(G(x), G(y), "l1", "none")
            ref = R.loss(x, y, 0.0, "none", 1.0, K)
            bad += note("l1", np.abs(N(mine) - N(l1)), R.ssim_bound(x, y, 0.0, "none", 1.0, K) + 2.0 ** -24 * np.abs(ref))
    st = HF.ssim_stats(G(x), G(y), K)
    assert st.dtype == torch.float64 and st.shape == (B, C, 2)
    bad += note("stats", np.abs(N(st) - R.stats(x, y, K)), R.stats_bound(x, y, K))
    if kind == "same":
        assert (st == 1.0).all()
    print("worst error / allowance (absolute error there):", {k: "%.3g (%.3g)" % v for k, v in WORST.items()})
    assert bad == 0, WORST


@pytest.mark.parametrize("shape", [(3, 1, 27, 26, 11), (3, 3, 32, 32, 11), (3, 2, 9, 20, 3)])
def test_bits(shape):
    """Two runs give the same bits; the rows of a batch of 3 are those of the same images one at a time, forward and
    backward; a forward under no_grad is the forward with a gradient."""
    from hipvae import functional as HF
    B, C, H, W, K = shape
    x, y = R.make_pair("smooth", (B, C, H, W))
    for alpha in (1.0, 0.84):
        gup = R.upstream(B, "none")
        out, dy = run_loss(x, y, alpha, "none", 0.75, K, gup)
        out2, dy2 = run_loss(x, y, alpha, "none", 0.75, K, gup)
        assert torch.equal(out, out2) and torch.equal(dy, dy2)
        with torch.no_grad():
            quiet, _ = run_loss(x, y, alpha, "none", 0.75, K)
        assert torch.equal(quiet, out) and not quiet.requires_grad
        for b in range(B):
            o1, d1 = run_loss(x[b:b + 1], y[b:b + 1], alpha, "none", 0.75, K, gup[b:b + 1])
            assert torch.equal(o1, out[b:b + 1]) and torch.equal(d1, dy[b:b + 1]), (alpha, b)
        for reduction in ("sum", "mean"):
            a, da = run_loss(x, y, alpha, reduction, 0.75, K, gup[:1])
            b_, db = run_loss(x, y, alpha, reduction, 0.75, K, gup[:1])
            assert torch.equal(a, b_) and torch.equal(da, db)
    st = HF.ssim_stats(G(x), G(y), K)
    assert torch.equal(st, HF.ssim_stats(G(x), G(y), K))
    for b in range(B):
        assert torch.equal(HF.ssim_stats(G(x[b:b + 1]), G(y[b:b + 1]), K), st[b:b + 1])


def test_contiguity_dtype_and_detach():
    import ops
    x, y = R.make_pair("uniform", (2, 3, 32, 32))
    tx, ty = G(x).requires_grad_(True), G(y).requires_grad_(True)
    want, dwant = run_loss(x, y, 0.84, "sum", 1.0, 11, np.ones(1, dtype=np.float32))
    wide = torch.zeros((2, 3, 32, 40), device=dev())
    wide[..., :32] = ty.detach()
    view = wide[..., :32].requires_grad_(True)                        # not contiguous
    out = ops.ssim_loss(tx, view, alpha=0.84)
    out.backward()
    assert torch.equal(out, want) and torch.equal(view.grad, dwant) and tx.grad is None       # x is a constant
    assert torch.equal(ops.reconstruction_loss(tx, ty, "ssim_l1"), want)
    assert torch.equal(ops.reconstruction_loss(tx, ty, "ssim"), ops.ssim_loss(tx, ty))
    from hipvae import abi
    with pytest.raises(abi.HipExtensionError):
        ops.ssim_loss(tx.double(), ty.double())


@pytest.mark.parametrize("shape, levels", [((2, 3, 32, 32), 2), ((1, 1, 176, 176), 5)])
def test_reconstruction_quality(shape, levels):
    from hipvae import quality as Q
    x, y = R.make_pair("smooth", shape, bits=16)                      # a grid on which four 2 x 2 means in a row are exact
    got = Q.reconstruction_quality(G(x), G(y))
    ref, bound = R.quality(x, y), R.quality_bound(x, y)
    assert R.levels_of(*shape[2:]) == levels and sorted(got) == sorted(ref)
    bad = 0
    for k in ref:
        assert got[k].dtype == torch.float64 and got[k].shape == (shape[0],) and got[k].is_cuda
        bad += note("quality." + k, np.abs(N(got[k]) - ref[k]), bound[k])
    print({k: "%.3g (%.3g)" % v for k, v in WORST.items() if k.startswith("quality.")})
    assert bad == 0, WORST
    one = Q.reconstruction_quality(G(x), G(y), levels=1)
    assert torch.equal(one["ms_ssim"], one["ssim"].clamp_min(0.0)) and torch.equal(one["ssim"], got["ssim"])
    same = Q.reconstruction_quality(G(x), G(x))
    assert (same["ssim"] == 1).all() and (same["ms_ssim"] == 1).all() and torch.isinf(same["psnr"]).all()
    assert (same["mse"] == 0).all() and (same["l1"] == 0).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------
class _Images:
    def __init__(self, t):
        self.t = t

    def __len__(self):
        return len(self.t)

    def __getitem__(self, i):
        return self.t[i]


class _Recorder:
    def __init__(self):
        self.log = {}

    def add_scalar(self, tag, value, global_step=None):
        self.log[tag] = (float(value), global_step)

    def add_scalars(self, tag, values, global_step=None):
        self.log[tag] = ({k: float(v) for k, v in values.items()}, global_step)

    def flush(self):
        pass


FIVE = ("psnr", "ssim", "ms_ssim", "mse", "l1")


@pytest.fixture(scope="module")
def bytes_u8():
    return np.random.default_rng(4).integers(0, 256, (40, 32, 32, 3), dtype=np.uint8)


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


def _solver(name, state, loss_type, dataset=None, writer=None, test_iter=1000):
    import models
    from solvers import IntroSolver, VAESolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    args = [dataset if dataset is not None else _Images(torch.zeros(1000, 1)), model, 8,
            torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]), torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]),
            loss_type, HP["beta_kl"], HP["beta_rec"]]
    if name == "intro":
        args += [HP["beta_neg"], HP["gamma_r"]]
    solver = (IntroSolver if name == "intro" else VAESolver)(*args, dev(), False, None, writer, test_iter, clip=HP["clip"])
    return solver, model


def test_compute_reconstruction_quality(bytes_u8):
    """From a dataset and from its device table: the same numbers; the means of the per-image vectors of the public
    function on the deterministic reconstruction; training flag and BatchNorm buffers untouched."""
    from hipvae import quality as Q
    from hipvae.dataset import DeviceImageTable
    _, model = _solver("vae", _init_state(), "ssim")
    images = torch.from_numpy(bytes_u8).permute(0, 3, 1, 2).float().div(255)
    ds, table = _Images(images), DeviceImageTable.from_arrays(bytes_u8, None, dev())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    a = Q.compute_reconstruction_quality(ds, model, batch_size=16)
    b = Q.compute_reconstruction_quality(table, model, batch_size=16)
    assert sorted(a) == sorted(FIVE + ("per_image", "indices")) and a["indices"].tolist() == list(range(40))
    assert all(isinstance(a[k], float) and np.isfinite(a[k]) for k in FIVE)
    assert {k: a[k] for k in FIVE} == {k: b[k] for k in FIVE}
    assert model.training and all(torch.equal(before[k], v) for k, v in model.state_dict().items())
    model.eval()
    with torch.no_grad():
        xs = images[:16].to(dev())
        want = Q.reconstruction_quality(xs, model.decode(model.encode(xs)[0]))
    model.train()
    for k in FIVE:
        assert a["per_image"][k].shape == (40,) and torch.equal(a["per_image"][k][:16], want[k])
        assert a[k] == float(a["per_image"][k].mean())
    sub = Q.compute_reconstruction_quality(ds, model, num=12, seed=1, levels=1)
    assert sub["indices"].tolist() == np.sort(np.random.RandomState(1).choice(40, 12, replace=False)).tolist()
    assert sub["ms_ssim"] != a["ms_ssim"] and sub["per_image"]["ssim"].shape == (12,)
    print({k: a[k] for k in FIVE})


@pytest.mark.parametrize("loss_type", ["ssim", "ssim_l1"])
@pytest.mark.parametrize("name", ["vae", "intro"])
def test_solver_hook_against_restatement(name, loss_type):
    """compute_rec_loss(x, r, "none" | "mean") is beta times the restatement, within the bound."""
    solver, _ = _solver(name, _init_state(), loss_type)
    alpha = {"ssim": 1.0, "ssim_l1": 0.84}[loss_type]
    x, y = R.make_pair("smooth", (8, 3, 32, 32))
    for reduction in ("none", "mean"):
        for beta in (None, 0.3):
            got = solver.compute_rec_loss(G(x), G(y), reduction, beta)
            s = HP["beta_rec"] if beta is None else beta
            ref, bound = R.loss(x, y, alpha, reduction, s), R.ssim_bound(x, y, alpha, reduction, s)
            assert note("hook", np.abs(N(got) - ref), bound + 2.0 ** -24 * np.abs(ref)) == 0, (reduction, beta, WORST["hook"])


@pytest.mark.parametrize("loss_type", ["ssim", "ssim_l1"])
@pytest.mark.parametrize("name", ["vae", "intro"])
def test_captured_steps_equal_eager_steps(name, loss_type):
    """Six steps from one seed, eagerly and with enable_graph() (three eager warm-up steps, then three replays of the one
    captured graph): identical dicts, identical parameters, everything finite."""
    state = _init_state()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(8, 3, 32, 32, generator=gen).to(dev()) for _ in range(2)]

    def trajectory(graph):
        solver, model = _solver(name, state, loss_type)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res = [solver.train_step(xs[k % 2], k) for k in range(6)]
        if graph:
            assert len(solver._graphs) == 1 and solver._graph is not None
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()

    (e, we), (g, wg) = trajectory(False), trajectory(True)
    for k, (a, b) in enumerate(zip(e, g)):
        assert set(a) == set(b) and all(np.isfinite(v) for v in a.values()), (k, a)
        print(name, loss_type, k, {n: (a[n], b[n]) for n in a if a[n] != b[n]} or "identical")
    print("parameters: max |eager - captured| =", float((we - wg).abs().max()), "checksum", float(we.double().sum()))
    assert e == g
    assert torch.equal(we, wg)
    # the loss type is live: the mse step from the same state and seed reports another reconstruction term
    plain, _ = _solver(name, state, "mse")
    torch.cuda.manual_seed(1234)
    d0 = plain.train_step(xs[0], 0)
    assert abs(d0["loss_rec"] - e[0]["loss_rec"]) > 1e-2 * abs(e[0]["loss_rec"]), (d0["loss_rec"], e[0]["loss_rec"])


def test_solver_writes_the_reconstruction_quality_record(bytes_u8):
    from hipvae import quality as Q
    from hipvae.dataset import DeviceImageTable
    table = DeviceImageTable.from_arrays(bytes_u8, None, dev())
    solver, model = _solver("vae", _init_state(), "ssim", dataset=table, writer=_Recorder(), test_iter=5)
    assert solver.reconstruction_params is None
    solver.extra_scores, solver.reconstruction_params = ("reconstruction_quality",), dict(num=24, seed=2)
    solver.write_disentanglemnt_scores(3)
    assert not solver.writer.log                                      # cur_iter % test_iter != 0: nothing
    solver.write_disentanglemnt_scores(10)
    assert list(solver.writer.log) == ["reconstruction_quality"]
    rec, step = solver.writer.log["reconstruction_quality"]
    want = Q.compute_reconstruction_quality(table, model, num=24, seed=2, batch_size=8)
    assert step == 10 and list(rec) == list(FIVE) and rec == {k: want[k] for k in FIVE} and model.training
    solver.extra_scores = ("reconstruction_quality", "nope")
    with pytest.raises(ValueError, match=r"unknown score\(s\) \['nope'\].*'reconstruction_quality'"):
        solver.write_disentanglemnt_scores(10)
