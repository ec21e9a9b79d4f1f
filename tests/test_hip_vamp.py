"""GPU tests of the VampPrior objective (csrc/vamp.hip, ops.vamp_latent / vamp_log_prob, solvers/vamp.py, the VampPrior
scores of hipvae.density / hipvae.quality) against the fp64 restatement tests/vamp_ref.py.

Bounds, all normwise: the loss and each of the three terms relative to the fp64 value; z, logq, logp, r and each gradient
tensor as max |err| / max |value|.  The ceiling is the project's fp32 bar, 1e-4; a quantity whose fp64 value is exactly
zero must come out exactly zero.  The stored inputs keep |mean KL| >= 5e-2 of the larger of |mean logq| and |mean logp|,
so the relative bound on the loss bounds its two parts to 5e-6, and every row's largest responsibility <= 0.9, so the
softmax is never a disguised arg-max.  The kernels are fp64 from the fp32 inputs; what is left is the fp32 rounding of the
stored results and of the sample z that L is formed from.  Worst values measured on an MI355X over every case of
test_kernel_against_restatement (printed by it):

    loss 8.8e-08, mean KL 8.8e-08, mean logq 4.2e-08, mean logp 5.1e-08, z 4.6e-08, logq 4.2e-16, logp 3.5e-08, r 9.1e-08,
    dmu 7.8e-08, dlogvar 7.7e-07, dp_mu 2.6e-07, dp_logvar 2.2e-07
"""
import os

import numpy as np
import pytest
import torch

import vamp_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
SHAPES = R.SHAPES
WORST = {}
QUANTITIES = ("z", "logq", "logp", "r", "dmu", "dlogvar", "dp_mu", "dp_logvar")


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())       # a copy: the stored cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "vamp.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def case(golden, B, K, D):
    """The stored inputs of a shape and the restatement's values, computed once per shape and never modified."""
    key = (B, K, D)
    if key not in _CASES:
        p = f"{B}x{K}x{D}:"
        beta = float(golden["beta"])
        ins = R.make_inputs(B, K, D, int(golden[p + "seed"]))
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in ins])
        ref = R.vamp(*ins, beta=beta)
        assert abs(ref["loss"] - float(golden[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        ratio, rmax = R.conditions(ref)
        assert ratio >= 5e-2 and (K < 2 or rmax <= 0.9), (ratio, rmax)
        for a in (*ins, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _CASES[key] = dict(ins=ins, ref=ref, beta=beta)
    return _CASES[key]


def place(x, layout):
    """A device tensor holding the values of ``x``: dense; "strided": the right part of a wider nan tensor that must not
    be read (row stride D + 3); "fc": one half of a [., 2D] tensor whose other half is nan (row stride 2D)."""
    if layout == "dense":
        return G(x)
    pad = 3 if layout == "strided" else x.shape[1]
    wide = np.full((x.shape[0], x.shape[1] + pad), np.nan, dtype=np.float32)
    wide[:, pad:] = x
    t = G(wide)[:, pad:]
    assert t.stride() == (x.shape[1] + pad, 1) or x.shape[0] == 1
    return t


def run(ins, beta, reduce="mean", layout="dense", g=None, gz=None, loss_only=False, z_only=False):
    """Everything ops.vamp_latent computes on the device, and the four gradients of  sum(g * loss) + sum(gz * z)."""
    import ops
    from hipvae import functional as HF
    mu, lv, eps, pm, pl = ins
    tm, tl, tpm, tpl = (place(a, layout).detach().requires_grad_(True) for a in (mu, lv, pm, pl))
    te = place(eps, layout)
    z, loss, terms = ops.vamp_latent(tm, tl, tpm, tpl, beta=beta, eps=te, reduce=reduce, with_terms=True)
    assert not terms.requires_grad and terms.shape == (3,) and z.shape == mu.shape
    assert loss.shape == ((mu.shape[0],) if reduce == "none" else ())
    obj = 0.0
    if not z_only:
        obj = obj + (loss if g is None else loss * (G(np.asarray(g, np.float32)) if np.ndim(g) else g)).sum()
    if gz is not None and not loss_only:
        obj = obj + (z * G(gz.astype(np.float32))).sum()
    dmu, dlv, dpm, dpl = torch.autograd.grad(obj, (tm, tl, tpm, tpl))
    _, (z2, out, rows, terms2, logq, logp, r) = HF.vamp_latent_forward(
        tm.detach(), tl.detach(), te, tpm.detach(), tpl.detach(), beta, HF.VAMP_REDUCES[reduce])
    assert torch.equal(z2, z.detach()) and torch.equal(terms2, terms)
    assert torch.equal(rows if reduce == "none" else out, loss.detach())
    assert r.shape == (mu.shape[0], pm.shape[0]) and r.dtype == logq.dtype == logp.dtype == torch.float64
    return dict(z=z.detach(), loss=loss.detach(), terms=terms, rows=rows, logq=logq, logp=logp, r=r, dmu=dmu, dlogvar=dlv,
                dp_mu=dpm, dp_logvar=dpl)


def rel(x, want):
    """Normwise error; a quantity that is exactly zero in fp64 must be exactly zero."""
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    if scale == 0.0:
        assert not x.any()
        return 0.0
    assert np.isfinite(x).all()
    return float(np.abs(x - want).max() / scale)


def errors(got, ref):
    e = dict(loss=rel(N(got["loss"]), ref["loss"]))
    t = N(got["terms"])
    for i, name in enumerate(("kl", "mean_logq", "mean_logp")):
        e[name] = rel(t[i], ref["terms"][i])
    for k in QUANTITIES:
        e[k] = rel(N(got[k]), ref[k])
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
@pytest.mark.parametrize("B, K, D", SHAPES)
def test_kernel_against_restatement(golden, B, K, D):
    c = case(golden, B, K, D)
    got = run(c["ins"], c["beta"])
    check(got, c["ref"], f"[{B}x{K}x{D}]")
    rows = N(got["r"]).sum(1)
    assert np.abs(rows - 1.0).max() <= 1e-12                 # the responsibilities of a row sum to one
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


# ---- 2. layouts and upstream gradients -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B, K, D", [(5, 7, 10), (33, 65, 130), (17, 15, 65)])
def test_layouts_and_upstream(golden, B, K, D):
    c = case(golden, B, K, D)
    ins, beta = c["ins"], c["beta"]
    dense = run(ins, beta)
    # the same bits from row-strided views read in place: the nan around them is not read
    same_bits(dense, run(ins, beta, layout="strided"))
    same_bits(dense, run(ins, beta, layout="fc"))
    rng = np.random.RandomState(B + K + D)
    # an upstream factor on the mean
    check(run(ins, beta, g=-0.375, layout="strided"), R.vamp(*ins, beta=beta, g=-0.375), f"[{B}x{K}x{D} g=-0.375]")
    # per-row upstream on reduce="none", with a gradient on z as well
    gb, gz = rng.randn(B), rng.randn(B, D)
    gb32, gz32 = gb.astype(np.float32), gz.astype(np.float32)
    got = run(ins, beta, reduce="none", g=gb32, gz=gz32, layout="fc")
    ref = R.vamp(*ins, beta=beta, reduce="none", g=gb32, gz=gz32)
    e = check(dict(got, loss=got["loss"].double().sum()), dict(ref, loss=ref["loss"].sum()), f"[{B}x{K}x{D} none]")
    assert rel(N(got["loss"]), ref["rows"]) <= BAR and e
    # the sum
    check(run(ins, beta, reduce="sum", g=0.5), R.vamp(*ins, beta=beta, reduce="sum", g=0.5), f"[{B}x{K}x{D} sum]")
    # gz on z alone: the components get an exactly zero gradient; the loss alone
    got = run(ins, beta, gz=gz32, z_only=True)
    check(got, R.vamp(*ins, beta=beta, g=0.0, gz=gz32), f"[{B}x{K}x{D} z alone]")
    assert not got["dp_mu"].any() and not got["dp_logvar"].any()
    check(run(ins, beta, gz=gz32, loss_only=True), R.vamp(*ins, beta=beta), f"[{B}x{K}x{D} loss alone]")
    # beta = 0: the term is gone, z still carries its gradient
    got = run(ins, 0.0, gz=gz32)
    ref0 = R.vamp(*ins, beta=0.0, gz=gz32)
    assert not got["dp_mu"].any() and not got["dp_logvar"].any() and float(got["loss"]) == 0.0
    for k in ("z", "dmu", "dlogvar", "logq", "logp", "r"):
        assert rel(N(got[k]), ref0[k]) <= BAR, k


# ---- 3. components astronomically far away ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B, K, D", [(9, 5, 10), (33, 40, 33)])
def test_far_components(B, K, D):
    mu, lv, eps, pm, pl = R.make_inputs(B, K, D, seed=11)
    pm = pm.copy()
    pm[1:] = 1e4                                             # L_bk ~ -1e7 D ... -1e9: exp underflows to exactly zero
    ins = (mu, lv, eps, pm, pl)
    ref = R.vamp(*ins, beta=1.5)
    assert ref["r"][:, 1:].max() == 0.0 and ref["r"][:, 0].min() == 1.0
    got = run(ins, 1.5, gz=np.ones((B, D), np.float32))
    ref = R.vamp(*ins, beta=1.5, gz=np.ones((B, D)))
    check(got, ref, f"[far {B}x{K}x{D}]")
    for k in got:
        assert torch.isfinite(got[k]).all(), k
    assert not got["r"][:, 1:].any() and bool((got["r"][:, 0] == 1.0).all())
    assert not got["dp_mu"][1:].any() and not got["dp_logvar"][1:].any()


# ---- 4. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, K, D", [(64, 500, 128), (33, 65, 130), (7, 9, 512), (257, 8, 2)])
def test_bitwise_reproducible_row_independent_and_log_prob(golden, B, K, D):
    import ops
    c = case(golden, B, K, D)
    ins, beta = c["ins"], c["beta"]
    mu, lv, eps, pm, pl = ins
    a = run(ins, beta, reduce="none")
    same_bits(a, run(ins, beta, reduce="none"))
    # row b does not depend on the rows around it: other rows changed, and other rows dropped
    keep = sorted({0, B // 2, B - 1})
    rng = np.random.RandomState(3)
    mu2, lv2, eps2 = (x.copy() for x in (mu, lv, eps))
    others = [i for i in range(B) if i not in keep]
    for x in (mu2, lv2, eps2):
        x[others] = rng.randn(len(others), D).astype(np.float32)
    changed = run((mu2, lv2, eps2, pm, pl), beta, reduce="none")
    alone = run((mu[keep], lv[keep], eps[keep], pm, pl), beta, reduce="none")
    for k in ("z", "logq", "logp", "rows", "r"):
        assert torch.equal(a[k][keep], changed[k][keep]), k
        assert torch.equal(a[k][keep], alone[k]), k
    # the forward-only entry on the returned sample gives the same logp bit for bit, dense or strided
    lp = ops.vamp_log_prob(a["z"], G(pm), G(pl))
    assert lp.dtype == torch.float64 and not lp.requires_grad and torch.equal(lp, a["logp"])
    assert torch.equal(ops.vamp_log_prob(place(N(a["z"]).astype(np.float32), "strided"), place(pm, "fc"), place(pl, "strided")),
                       a["logp"])


# ---- 5. training steps against the oracle ----------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


# beta_kl, beta_rec, beta_neg, gamma_r, clip, lr: the siblings' values but for lr, see test_two_steps_against_the_oracle
K_PSEUDO, LR_PRIOR = 6, 2e-5
HP = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-5]


def _init_state():
    import models
    torch.manual_seed(0)
    state = {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}
    raw = torch.rand(K_PSEUDO, 3, 32, 32, generator=torch.Generator().manual_seed(7))      # starts from "images"
    raw[0, 0, 0, 0], raw[1, 1, 2, 3] = 1.25, -0.5                # two entries outside [0, 1]: clamped, never moved
    return state, raw


def _hip_solver(state, raw, hp=HP, lr_prior=LR_PRIOR, **kw):
    import models
    from solvers import VampSolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    pseudo = models.PseudoInputs.from_images(raw).to(dev())
    solver = VampSolver(_DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
                        torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1], dev(), False, None,
                        clip=hp[4], pseudo_inputs=pseudo,
                        optimizer_prior=torch.optim.Adam(pseudo.parameters(), lr=lr_prior), **kw)
    assert solver.conv_math == "fp32"
    return solver, model, pseudo


def _oracle_trainer(state, raw, hp, lr_prior):
    from oracle.network import Net
    from oracle.steps import Trainer

    class VampTrainer(Trainer):
        """The oracle's VAE step in fp64 with the clamped pseudo-inputs as a third key group ("prior.raw"): the second
        encode in the solver's order, the torch restatement of the op, one backward over the three groups, the clip over
        encoder and decoder only, Adam on all three (the prior at its own learning rate)."""

        def _step_vae(self, real, draws):
            net = self.net
            mu, logvar = net.encode(real)
            p_mu, p_logvar = net.encode(net.sd["prior.raw"].clamp(0, 1))
            z, loss_kl, logq, logp = R.torch_vamp(mu, logvar, draws[0], p_mu, p_logvar, self.beta_kl)
            self.trace.setdefault("kl", []).append(loss_kl.detach().reshape(-1).clone())
            self.trace.update(log_q=float(logq.detach().mean()), log_p=float(logp.detach().mean()))
            rec = net.decode(z)
            loss_rec = self.rec_loss(real, rec, "mean")
            loss = self.scale * (loss_rec + loss_kl)
            self._backward(loss, ("decoder", "encoder", "prior"))
            norm = self._clip() if self.clip else None
            self._adam("encoder")
            self._adam("decoder")
            lr, self.lr = self.lr, lr_prior
            self._adam("prior")
            self.lr = lr
            return {"loss_enc": float(loss.detach()), "loss_dec": float(loss.detach()), "loss_kl": float(loss_kl.detach()),
                    "loss_rec": float(loss_rec.detach()), "L2": norm}

    state = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    tr = VampTrainer("vae", Net("conv", state=state, **TINY), dataset_size=1000, beta_kl=hp[0], beta_rec=hp[1],
                     beta_neg=hp[2], gamma_r=hp[3], clip=hp[4], lr=hp[5])
    tr.net.sd["prior.raw"] = raw.double().clone().requires_grad_(True)
    tr.keys["prior"] = ["prior.raw"]
    return tr


def test_two_steps_against_the_oracle():
    """Two training steps of the tiny model (B = 8, K = 6, fp32 arithmetic on the device, one recorded draw a step)
    against the fp64 CPU oracle whose step is restated in this file.  Tolerances: those of test_hip_mmd.py's step test --
    the returned dict to 1e-4 at step 0 and 3e-4 at step 1, the op's output to 3e-4 / 3e-3 of its scale -- and, for the
    weights and the pseudo-inputs after the two steps, those of test_hip_model.py's run_golden_steps (every element
    within the Adam limit 2.05 lr per step, all but 2e-3 of them within a quarter of it, the median within 0.02 lr).

    All three groups train at lr 2e-5, not the siblings' 2e-4.  Adam's first update is lr g / (|g| + eps): where |g| is at
    rounding level its sign differs between fp32 and fp64, and after step 0 about 90 of the weights differ from the
    oracle's by 2 lr (the same 92 weights at either lr; test_hip_model.py documents the effect).  Every sibling carries
    that into step 1; here the KL is logq - logp with |KL| = 0.06 |logq| for this model at its initial weights, so the
    same weight differences show 16 times larger in loss_kl and in the gradient norm.  Measured on an MI355X against the
    fp64 oracle at step 1, lr 2e-4: loss_kl 6.4e-4, L2 8.5e-4 (pseudo-inputs at 1e-3 or 2e-4 alike); lr 2e-5: loss_kl
    7.5e-5, L2 9.7e-5.  That this is the trajectory and not the step is checked here as well: the oracle restarted from
    the device's own state before step 1 (weights, BatchNorm buffers, pseudo-inputs; the returned dict does not depend
    on Adam's moments) has to give the device's dict to step 0's tolerance, 1e-4 (measured: 5e-7 at either lr).  fp32
    storage rounds a pseudo-input below 1 by up to 6e-8 and a weight of 0.05 by 4e-9, both well below 0.02 lr = 4e-7."""
    import ops
    state, raw = _init_state()
    tr = _oracle_trainer(state, raw, HP, LR_PRIOR)
    solver, model, pseudo = _hip_solver(state, raw)
    log, op0 = [], ops.vamp_latent
    ops.vamp_latent = lambda *a, **k: (log.append(op0(*a, **k)), log[-1])[1]
    keys = ("loss_enc", "loss_dec", "loss_kl", "loss_rec", "L2")
    g = torch.Generator().manual_seed(1)
    try:
        for s in range(2):
            x = torch.rand(8, 3, 32, 32, generator=g)
            eps = torch.randn(8, 10, generator=g)
            log.clear()
            if s == 1:
                forced = _oracle_trainer({k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                                         pseudo.raw.detach().cpu().clone(), HP, LR_PRIOR).step(x.double(), [eps.double()])
            with ops.noise_queue([eps.clone()]):
                got = solver.train_step(x, s)
                assert not ops._noise["queue"]                   # the one recorded draw was taken
            ref = tr.step(x.double(), [eps.double()])
            print(s, {k: (got[k], ref[k]) for k in keys}, got["log_q"], tr.trace["log_q"], got["log_p"], tr.trace["log_p"])
            gd, go = N(pseudo.raw.grad), tr.grads["prior.raw"].numpy()
            print(s, "pseudo-input gradient: normwise error", rel(gd, go), "median |g|", float(np.median(np.abs(go))),
                  "max |g|", float(np.abs(go).max()), "pseudo-inputs: max |difference| / lr",
                  float((pseudo.raw.detach().cpu().double() - tr.net.sd["prior.raw"].detach()).abs().max()) / LR_PRIOR)
            assert set(got) == set(keys) | {"log_q", "log_p"}
            np.testing.assert_allclose([got[k] for k in keys], [ref[k] for k in keys], rtol=1e-4 if s == 0 else 3e-4)
            if s == 1:
                print(s, "restarted from the device's state:", {k: (got[k], forced[k]) for k in keys})
                np.testing.assert_allclose([got[k] for k in keys], [forced[k] for k in keys], rtol=1e-4)
            tol = 3e-4 if s == 0 else 3e-3
            assert len(log) == len(tr.trace["kl"]) == 1
            want = tr.trace["kl"][0]
            assert float((log[0][1].detach().reshape(-1).cpu() - want).abs().max()) < tol * float(want.abs().max())
            for k in ("log_q", "log_p"):
                assert abs(got[k] - tr.trace[k]) <= tol * abs(tr.trace[k]), (s, k)
    finally:
        ops.vamp_latent = op0

    def bulk(diffs, lr, name):
        assert float(diffs.max()) <= 2.05 * lr * 2, (name, float(diffs.max()))
        assert float((diffs > 0.25 * lr * 2).float().mean()) < 2e-3, name
        assert float(diffs.median()) < 0.02 * lr, name

    sd = model.state_dict()
    bulk(torch.cat([(sd[k].detach().cpu().double() - v.detach()).abs().reshape(-1) for k, v in tr.net.sd.items()
                    if k in sd and v.dtype.is_floating_point and "running" not in k]), HP[5], "weights")
    after = pseudo.raw.detach().cpu()
    inside = (raw >= 0) & (raw <= 1)
    bulk((after.double() - tr.net.sd["prior.raw"].detach()).abs()[inside], LR_PRIOR, "pseudo-inputs")
    # they trained -- Adam's first two steps move an entry by about lr each -- except the two entries outside [0, 1]
    moved = (after - raw).abs()
    assert float(moved[inside].median()) > 0.5 * LR_PRIOR, float(moved[inside].median())
    assert int((~inside).sum()) == 2 and not moved[~inside].any()


# ---- 6. graph capture --------------------------------------------------------------------------------------------------
def test_captured_steps_equal_eager_steps_and_lr_change_recaptures():
    """With enable_graph() the trajectory follows the eager one from the same state through the capture; after the prior
    optimiser's lr is halved it still does, which it could not if the step replayed the graph captured with the old
    value: the key re-captures."""
    from hipvae.flat import fused_update
    state, raw = _init_state()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(8, 3, 32, 32, generator=gen).to(dev()) for _ in range(2)]

    def trajectory(graph):
        solver, model, pseudo = _hip_solver(state, raw)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], []
        for k in range(12):
            if k == 6:
                solver.optimizer_prior.param_groups[0]["lr"] /= 2
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8, 9, 10, 11) else None)
        flat = torch.cat([p.detach().reshape(-1) for p in list(model.parameters()) + [pseudo.raw]]).cpu()
        return res, flat, keys, fused_update(solver.optimizer_prior)

    (e, we, _, _), (gr, wg, keys, spec) = trajectory(False), trajectory(True)
    assert keys[3] is not None and keys[3] == keys[4] == keys[5]
    assert keys[7] is not None and keys[7] == keys[8] == keys[11] != keys[5]
    assert spec in keys[11] and spec not in keys[5]
    for x, y in zip(e, gr):
        for k in x:
            assert abs(x[k] - y[k]) <= 1e-5 * abs(x[k]) + 1e-9, (k, x[k], y[k])
    assert float((we - wg).abs().max()) < 1e-6
    assert float((we[-raw.numel():] - raw.reshape(-1)).abs().max()) > LR_PRIOR      # the pseudo-inputs are in the walk


# ---- 7. scores -----------------------------------------------------------------------------------------------------------
class _Images:
    """A dataset of 96 random images (no factors)."""

    def __init__(self):
        self.x = torch.rand(96, 3, 32, 32, generator=torch.Generator().manual_seed(9))

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i]


def test_scores_use_the_learned_prior():
    from hipvae import density, quality
    state, raw = _init_state()
    solver, model, pseudo = _hip_solver(state, raw)
    bn = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    prior = density.vamp_prior(model, pseudo, batch_size=4)
    assert model.training and all(torch.equal(v, model.state_dict()[k]) for k, v in bn.items())
    assert prior.means.shape == prior.logvars.shape == (K_PSEUDO, 10) and prior.means.dtype == torch.float32
    same = density.vamp_prior(model, pseudo, batch_size=64)
    assert rel(N(same.means), N(prior.means)) <= BAR            # eval mode: the chunking does not change a row
    # log-density against the restatement on the same encoded components
    x = torch.randn(300, 10, generator=torch.Generator().manual_seed(2)).to(dev())
    lp = density.vamp_log_prob(prior, x)
    want = R.torch_log_prob(x.double().cpu(), prior.means.double().cpu(), prior.logvars.double().cpu()).numpy()
    assert lp.dtype == torch.float64 and rel(N(lp), want) <= BAR
    # samples: seed-stable, the global generators untouched
    st = torch.random.get_rng_state(), torch.cuda.get_rng_state()
    s0, s1 = density.vamp_sample(prior, 33, seed=4), density.vamp_sample(prior, 33, seed=4)
    assert torch.equal(s0, s1) and s0.shape == (33, 10) and not torch.equal(s0, density.vamp_sample(prior, 33, seed=5))
    assert torch.equal(st[0], torch.random.get_rng_state()) and torch.equal(st[1], torch.cuda.get_rng_state())
    # compute_latent_density reports the mean of that log-density over its held-out latents
    ds = _Images()
    got = density.compute_latent_density(ds, model, num_fit=48, num_eval=32, batch_size=16, n_components=2, prior=prior)
    held = density.vamp_log_prob(prior, got["latents"]["heldout"]).mean().item()
    assert got["prior"] is prior and abs(got["loglik_prior"] - held) <= 1e-12 * abs(held)
    assert abs(got["gap"] - (got["loglik_heldout"] - held)) <= 1e-9 * abs(held)
    plain = density.compute_latent_density(ds, model, num_fit=48, num_eval=32, batch_size=16, n_components=2)
    assert "prior" not in plain and plain["loglik_prior"] != got["loglik_prior"]
    # sample quality decodes the prior's samples
    q = quality.compute_sample_quality(ds, model, num_real=64, batch_size=16, prior=prior, scores=("frechet", "prdc"))
    assert q["prior"] is prior and "gmm" not in q and np.isfinite(q["frechet"])
    q0 = quality.compute_sample_quality(ds, model, num_real=64, batch_size=16, scores=("frechet",))
    assert not torch.equal(q["features"]["fake"], q0["features"]["fake"])
    # the solver hands its own prior to the scores, and refuses the N(0, I) likelihood
    own = solver._eval_prior()
    assert torch.equal(own.means, density.vamp_prior(model, pseudo, 8).means)
    solver.extra_scores = ("log_likelihood",)
    with pytest.raises(NotImplementedError):
        solver.write_disentanglemnt_scores(0)
