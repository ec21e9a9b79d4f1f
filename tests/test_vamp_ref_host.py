"""Host: the fp64 restatement of the VampPrior op (tests/vamp_ref.py) against torch autograd and the analytic KL, the
stored cases, and what the op, the solver, the pseudo-inputs and the prior's sampler do before any kernel runs."""
import math
import os
import re

import numpy as np
import pytest
import torch

import vamp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(cdim=3, zdim=10, channels=(8, 16), image_size=16)        # the net of test_solver_hyper_host.py
ALL = ["VAESolver", "IntroSolver", "TCSovler", "IntroTCSovler", "DIPSolver", "IntroDIPSolver", "MMDSolver",
       "IntroMMDSolver", "FactorSolver", "AdaGVAESolver", "JointVAESolver", "AnnealedVAESolver"]


def rel(x, want):
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    return float(np.abs(x - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", R.REDUCES)
@pytest.mark.parametrize("B, K, D", [(2, 3, 3), (5, 7, 10), (33, 65, 130), (7, 1, 4)])
def test_restatement_against_fp64_autograd(B, K, D, reduce):
    ins = R.make_inputs(B, K, D, seed=B + K + D)
    rng = np.random.RandomState(1)
    g = rng.randn(B) if reduce == "none" else -0.375
    gz = rng.randn(B, D)
    ref = R.vamp(*ins, beta=0.75, reduce=reduce, g=g, gz=gz)
    mu, lv, eps, pm, pl = (torch.from_numpy(a.astype(np.float64)) for a in ins)
    leaves = [t.requires_grad_(True) for t in (mu, lv, pm, pl)]
    z, loss, logq, logp = R.torch_vamp(leaves[0], leaves[1], eps, leaves[2], leaves[3], 0.75, reduce)
    obj = (loss * torch.as_tensor(g)).sum() + (z * torch.from_numpy(gz)).sum()
    grads = torch.autograd.grad(obj, leaves)
    for name, got, want in (("z", ref["z"], z), ("loss", ref["loss"], loss), ("logq", ref["logq"], logq),
                            ("logp", ref["logp"], logp), ("dmu", ref["dmu"], grads[0]), ("dlogvar", ref["dlogvar"], grads[1]),
                            ("dp_mu", ref["dp_mu"], grads[2]), ("dp_logvar", ref["dp_logvar"], grads[3])):
        assert rel(got, want.detach().numpy()) <= 1e-12, name
    assert np.abs(ref["r"].sum(1) - 1.0).max() <= 1e-12        # |L| ~ 2e2: exp(L - lse) carries |L| 2^-53
    np.testing.assert_allclose(ref["terms"], [(ref["logq"] - ref["logp"]).mean(), ref["logq"].mean(), ref["logp"].mean()],
                               rtol=1e-14)
    lp = R.torch_log_prob(z.detach(), pm.detach(), pl.detach()).numpy()
    assert rel(lp, ref["logp"]) <= 1e-13


def test_single_standard_component_is_the_analytic_kl():
    """K = 1 with p_mu = 0, p_logvar = 0: logp_b = log N(z_b; 0, I), so E_eps rows_b is KL(q_b || N(0, I)).  N = 200000
    draws of one row; the standard error of the mean printed below is sd(rows) / sqrt(N) ~ 3e-3 for this row, and the
    mean has to land within five of them."""
    D, n = 6, 200000
    rng = np.random.RandomState(0)
    mu, lv = 0.5 * rng.randn(1, D), rng.uniform(-1.0, 0.5, (1, D))
    kl = -0.5 * (1.0 + lv - mu * mu - np.exp(lv)).sum()
    eps = rng.randn(n, D)
    ref = R.vamp(np.repeat(mu, n, 0), np.repeat(lv, n, 0), eps, np.zeros((1, D)), np.zeros((1, D)), reduce="none")
    z = ref["z"]
    assert rel(ref["logp"], -0.5 * (D * R.LOG2PI + (z * z).sum(1))) <= 1e-13 and (ref["r"] == 1.0).all()
    se = ref["rows"].std(ddof=1) / math.sqrt(n)
    print(f"analytic KL {kl:.5f}, Monte-Carlo mean {ref['rows'].mean():.5f}, standard error {se:.2e} ({n} draws)")
    assert se < 5e-3 and abs(ref["rows"].mean() - kl) <= 5.0 * se


def test_reduce_forms_are_consistent():
    ins = R.make_inputs(9, 4, 5, seed=3)
    none, mean, tot = (R.vamp(*ins, beta=1.5, reduce=r) for r in ("none", "mean", "sum"))
    assert none["loss"].shape == (9,) and np.array_equal(none["loss"], mean["rows"])
    assert abs(mean["loss"] - none["loss"].mean()) <= 1e-15 * abs(mean["loss"])
    assert abs(tot["loss"] - none["loss"].sum()) <= 1e-15 * abs(tot["loss"])
    for k in ("dmu", "dlogvar", "dp_mu", "dp_logvar"):
        assert rel(mean[k] * 9, tot[k]) <= 1e-14 and rel(none[k], tot[k]) <= 1e-14, k     # g = 1 per row is the sum


def test_stored_cases_hold_the_two_conditions():
    g = np.load(os.path.join(ROOT, "tests", "golden", "vamp.npz"))
    assert sorted(k for k in g.files if k != "beta") == sorted(f"{B}x{K}x{D}:{n}" for B, K, D in R.SHAPES
                                                                for n in ("seed", "checksum", "loss"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vamp.npz")) < 32 * 1024
    for B, K, D in [s for s in R.SHAPES if s[0] * s[1] * s[2] <= 1 << 18]:
        p = f"{B}x{K}x{D}:"
        ins = R.make_inputs(B, K, D, int(g[p + "seed"]))
        assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in ins])
        ref = R.vamp(*ins, beta=float(g["beta"]))
        assert abs(ref["loss"] - float(g[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        ratio, rmax = R.conditions(ref)
        assert ratio >= 5e-2 and (K < 2 or rmax <= 0.9), (B, K, D, ratio, rmax)


# ---- refusals on the host, before any launch -------------------------------------------------------------------------------
def test_op_refusals():
    import ops
    from hipvae import abi
    from hipvae import functional as HF
    assert (HF.VAMP_MAX_B, HF.VAMP_MAX_K, HF.VAMP_MAX_D, HF.VAMP_MAX_PAIRS) == (4096, 4096, 512, 1 << 22)
    z = torch.zeros
    ok = (z(4, 3), z(4, 3), z(5, 3), z(5, 3))
    with pytest.raises(ValueError, match="share one"):
        ops.vamp_latent(z(4, 3), z(4, 2), z(5, 3), z(5, 3))
    with pytest.raises(ValueError, match="share one"):
        ops.vamp_latent(z(4, 3), z(4, 3), z(5, 3), z(6, 3))
    with pytest.raises(ValueError, match="D = 3"):
        ops.vamp_latent(z(4, 3), z(4, 3), z(5, 4), z(5, 4))
    with pytest.raises(ValueError, match="eps"):
        ops.vamp_latent(*ok, eps=z(4, 2))
    with pytest.raises(ValueError, match="reduce"):
        ops.vamp_latent(*ok, reduce="batchmean")
    with pytest.raises(ValueError, match="finite"):
        ops.vamp_latent(*ok, beta=float("nan"))
    with pytest.raises(ValueError, match="K <= 4096"):
        ops.vamp_latent(z(4, 3), z(4, 3), z(4097, 3), z(4097, 3))
    with pytest.raises(ValueError, match="B <= 4096"):
        ops.vamp_latent(z(4097, 3), z(4097, 3), z(5, 3), z(5, 3))
    with pytest.raises(ValueError, match="D <= 512"):
        ops.vamp_latent(z(4, 513), z(4, 513), z(5, 513), z(5, 513))
    with pytest.raises(ValueError, match="D <= 512"):
        ops.vamp_latent(z(4, 0), z(4, 0), z(5, 0), z(5, 0))
    with pytest.raises(ValueError, match=r"2\^22"):
        ops.vamp_latent(z(2049, 3), z(2049, 3), z(2048, 3), z(2048, 3))
    with pytest.raises(ValueError, match=r"2\^22"):
        ops.vamp_log_prob(z(4096, 3), z(1025, 3), z(1025, 3))
    with pytest.raises(ValueError, match="share one"):
        ops.vamp_log_prob(z(4, 3), z(5, 3), z(5, 2))
    # valid shapes on the CPU reach the device check: there is no CPU path
    with pytest.raises(abi.HipExtensionError):
        ops.vamp_latent(*ok)
    with pytest.raises(abi.HipExtensionError):
        ops.vamp_log_prob(z(4, 3), z(5, 3), z(5, 3))


def _solver(pseudo=None, batch_size=4, **kw):
    import models
    from solvers import VampSolver
    m = models.SoftIntroVAE(arch="conv", **NET)

    class DS:
        def __len__(self):
            return 100

    pseudo = models.PseudoInputs(7, NET["cdim"], NET["image_size"]) if pseudo is None else pseudo
    return VampSolver(DS(), m, batch_size, torch.optim.Adam(m.encoder.parameters()), torch.optim.Adam(m.decoder.parameters()),
                      "mse", 0.5, 0.75, torch.device("cpu"), False, None, pseudo_inputs=pseudo,
                      optimizer_prior=torch.optim.Adam(pseudo.parameters(), lr=1e-3), **kw), m, pseudo


def test_solver_surface_and_refusals():
    import models
    import solvers
    from solvers import VAESolver, VampSolver
    assert solvers.__all__ == ALL and "VampSolver" not in solvers.__all__
    s, m, pseudo = _solver()
    assert s._updates == ("encoder", "decoder", "prior") and s._walk == ("decoder", "encoder", "prior")
    assert VAESolver._walk == ("decoder", "encoder") and VAESolver._updates == ("encoder", "decoder")
    assert s._module("prior") is pseudo and s._optimizer("prior") is s.optimizer_prior
    assert s._module("encoder") is m.encoder and s._optimizer("decoder") is s.optimizer_d
    assert len(s._params("prior")) == 1 and s._params("prior")[0] is pseudo.raw
    # one step and one train_step, VAESolver's
    assert VampSolver._device_step is VAESolver._device_step and VampSolver.train_step is VAESolver.train_step
    assert VampSolver._run is VAESolver._run and VampSolver._backward is VAESolver._backward
    assert VAESolver._eval_prior(s) is None
    # the prior optimiser's update is part of the graph key: a change of its lr re-captures
    k0 = s._graph_key_extra()
    s.optimizer_prior.param_groups[0]["lr"] = 5e-4
    assert s._graph_key_extra() != k0
    s.extra_scores = ("log_likelihood",)
    with pytest.raises(NotImplementedError):
        s.write_disentanglemnt_scores(0)
    # wrong geometry, too many components, too many pairs
    with pytest.raises(ValueError, match="cdim, image_size"):
        _solver(models.PseudoInputs(7, 1, NET["image_size"]))
    with pytest.raises(ValueError, match="cdim, image_size"):
        _solver(models.PseudoInputs(7, NET["cdim"], 32))
    with pytest.raises(ValueError, match="K <= 4096"):
        _solver(_Many(4097))
    with pytest.raises(ValueError, match=r"2\^22"):
        _solver(_Many(4096), batch_size=1025)
    with pytest.raises(TypeError):
        VampSolver(None, m, 4, None, None, "mse", 1.0, 1.0, torch.device("cpu"), False, None)


class _Many(torch.nn.Module):
    """The geometry of K pseudo-inputs without their storage."""

    def __init__(self, num):
        super().__init__()
        self.num, self.cdim, self.image_size = num, NET["cdim"], NET["image_size"]
        self.raw = torch.nn.Parameter(torch.zeros(1))


def test_pseudo_inputs_clamp_and_mask():
    import models
    torch.manual_seed(0)
    p = models.PseudoInputs(500, 3, 8)
    assert p.raw.shape == (500, 3, 8, 8) and [n for n, _ in p.named_parameters()] == ["raw"]
    assert abs(float(p.raw.detach().mean()) - 0.05) < 1e-3 and abs(float(p.raw.detach().std()) - 0.01) < 1e-3     # N(0.05, 0.01), 96000 draws
    assert models.PseudoInputs().raw.shape == (500, 3, 64, 64)
    x = torch.tensor([-0.5, 0.0, 0.25, 1.0, 1.5, float(np.nextafter(np.float32(1), np.float32(2)))]).reshape(6, 1, 1, 1)
    q = models.PseudoInputs.from_images(x)
    assert q.num == 6 and q.cdim == 1 and q.image_size == 1 and torch.equal(q.raw.detach(), x) and q.raw is not x
    out = q()
    assert torch.equal(out.detach().reshape(-1), torch.tensor([0.0, 0.0, 0.25, 1.0, 1.0, 1.0]))
    (out * torch.arange(1.0, 7.0).reshape(6, 1, 1, 1)).sum().backward()
    assert torch.equal(q.raw.grad.reshape(-1), torch.tensor([0.0, 2.0, 3.0, 4.0, 0.0, 0.0]))     # exactly zero outside
    for bad in (dict(num=0), dict(cdim=0), dict(image_size=-1), dict(std=-1.0)):
        with pytest.raises(ValueError):
            models.PseudoInputs(**bad)
    with pytest.raises(ValueError):
        models.PseudoInputs.from_images(torch.zeros(3, 8, 8))


def test_vamp_sample_is_seed_stable_and_private():
    from hipvae import density
    rng = np.random.RandomState(0)
    prior = density.VampPrior(torch.from_numpy(rng.randn(5, 4).astype(np.float32)),
                              torch.from_numpy(rng.uniform(-8.0, -7.0, (5, 4)).astype(np.float32)))
    assert prior.n_components == 5 and prior.dim == 4
    torch.manual_seed(123)
    state = torch.random.get_rng_state()
    a, b, c = density.vamp_sample(prior, 1000, seed=3), density.vamp_sample(prior, 1000, seed=3), \
        density.vamp_sample(prior, 1000, seed=4)
    assert torch.equal(state, torch.random.get_rng_state())
    assert torch.equal(a, b) and not torch.equal(a, c) and a.shape == (1000, 4) and a.dtype == torch.float32
    # narrow components: every sample sits on one of the five means, and all five are used about equally
    near = torch.cdist(a, prior.means).argmin(1)
    assert float(torch.cdist(a, prior.means).min(1).values.max()) < 0.2
    counts = torch.bincount(near, minlength=5)
    assert int(counts.min()) > 140 and int(counts.max()) < 260         # 200 +- 4.7 sd of Binomial(1000, 0.2)
    with pytest.raises(ValueError):
        density.vamp_sample(prior, 0)
    with pytest.raises(ValueError, match="VampPrior"):
        density.compute_latent_density([0, 1], None, prior="vamp")


# ---- the source ----------------------------------------------------------------------------------------------------------
def test_kernel_file_and_header():
    from hipvae import abi
    src = open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "vamp.hip")).read()
    assert '#include "objective.h"' in src and "#pragma clang fp contract(off)" in src
    assert "atomic" not in re.sub(r"//[^\n]*", "", src)
    for fn in ("posterior_sample(", "ordered_sum<", "row_grid("):
        assert fn in src, fn
    assert re.search(r"^SRCS\s*=.*\bvamp\.hip\b", open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "Makefile")).read(),
                     flags=re.M)
    assert "vamp.hip" in open(os.path.join(ROOT, "intro-tc-vae_amd", "csrc", "objective.h")).read().split("#pragma once")[0]
    for fn in ("itcv_vamp_workspace", "itcv_vamp_fwd", "itcv_vamp_bwd", "itcv_vamp_logprob"):
        assert fn in abi.SIGNATURES, fn
    assert abi.ABI_VERSION == 4
    ws = abi.lib.itcv_vamp_workspace
    assert ws(64, 500, 128) == (2 * 16 + 1) * 64 * 8 and ws(4096, 1024, 512) > 0
    assert ws(4097, 1, 1) == ws(1, 4097, 1) == ws(1, 1, 513) == ws(4096, 1025, 8) == ws(0, 1, 1) == 0
