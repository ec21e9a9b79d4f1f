"""GPU tests of the device-side beta-VAE and explicitness scores (csrc/logreg.hip, hipvae/logreg.py,
hipvae/disentangle.py) against the numpy fp64 restatement of tests/test_classify_host.py at the same inputs, and against
what was recorded from sklearn and the unmodified reference (golden/classify.npz).

Bounds.  Integers (predictions, pair counts, accuracies) are compared EXACTLY.  Column statistics: 1e-13 relative (of the
column's largest |x| for the mean, which may be near 0).  Value and gradient: with A = max_i,c (sum_d |x_id| |W_dc| +
|b_c|) the largest logit's sum of magnitudes, a logit of D + 1 products carries at most (D + 2) ulp of A however the
products are ordered (the MFMA adds four at a time, numpy in BLAS order); logsumexp and the probabilities inherit that
absolute error (d lse / d z and d p / d z are <= 1), and the means over the rows do not grow it.  D + 2 <= 130 here, so
  |f - ref| <= 512 ulp * max(1, A, f)          |grad - ref| <= 512 ulp * max(1, max|x|) * max(1, A)
with ulp = 2.2e-16.  Probabilities at a given theta: 512 ulp * max(1, A).  The converged solve: max|grad F_p| <= gtol is
reported for every problem; F - F* <= |grad|^2 / (2 lambda) plus the rounding of F above; probabilities within
PROBA_SOLVE_TOL (measured in the host test between restatement solves at gtol and gtol / 100, 10x margin: 5e-8).
Explicitness: 1e-9 of the restatement (an AUC moves only when a pair of probabilities swaps order) and the recorded
loose-solver distance of the reference's own value."""
import os

import numpy as np
import pytest
import torch

from test_classify_host import (GOLDEN, LOOSE_AUC_TOL, PROBA_SOLVE_TOL, offsets, ref_colstats, ref_factor_change_accuracy,
                                ref_pair_counts, ref_prepare, ref_present, ref_proba, ref_valgrad_all, ref_zdiff,
                                solved_pair)

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
ULP = 2.220446049250313e-16


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "classify.npz"))
    return {k: g[k] for k in g.files}


def case(golden, name):
    """(x as a device tensor (possibly strided), x numpy, y, sizes, cvalid) of the three shapes."""
    g = golden
    if name in ("full", "small"):
        n = 777 if name == "full" else 60
        sizes = [int(s) for s in g["sizes"]]
        y = g["v_train"][:n]
        cvalid = ref_present(y, sizes) & ref_present(g["v_test"][:n], sizes)
        return G(g["x_train"][:n]), g["x_train"][:n], y, sizes, cvalid
    rs = np.random.RandomState(11)                                      # N = 1030, D = 128, ld = 160, K = 1, 3 classes
    wide = rs.randn(1030, 160).astype(np.float32)
    y = rs.randint(3, size=(1030, 1)).astype(np.int32)
    wide[:, :128] += 0.5 * y
    xd = G(wide)[:, :128]
    assert xd.stride() == (160, 1)
    return xd, wide[:, :128], y, [3], np.ones(3, dtype=bool)


def test_column_statistics(golden):
    from hipvae import functional as HF
    for name in ("full", "strided"):
        xd, x, _, _, _ = case(golden, name)
        flags = HF.disent_flags(dev())
        mean, scale = HF.logreg_colstats(xd, flags)
        m, s = ref_colstats(x)
        em = np.abs(mean.cpu().numpy() - m) / np.abs(x).max(0)
        es = np.abs(scale.cpu().numpy() - s) / s
        print(name, "max relative error of mean", em.max(), "of scale", es.max())
        assert em.max() <= 1e-13 and es.max() <= 1e-13 and flags.tolist() == [0, 0]
        m2, s2 = HF.logreg_colstats(xd, flags)
        assert torch.equal(mean, m2) and torch.equal(scale, s2)
    xd = case(golden, "full")[0]
    mean, scale = HF.logreg_colstats(xd, HF.disent_flags(dev()))
    assert scale[-1].item() == 1.0 and mean[-1].item() == 1.25          # the constant column


@pytest.mark.parametrize("name", ["full", "small", "strided"])
def test_value_gradient_probabilities(golden, name):
    from hipvae import functional as HF
    xd, x, y, sizes, cvalid = case(golden, name)
    flags = HF.disent_flags(dev())
    standardise = name != "strided"
    stats_d = HF.logreg_colstats(xd, flags) if standardise else None
    X = ref_prepare(x, ref_colstats(x) if standardise else None)
    prob = HF.LogregProblem(xd, G(y), sizes, G(cvalid.astype(np.int32)), flags, stats=stats_d)
    off = offsets(sizes)
    rs = np.random.RandomState(3)
    for theta in (np.zeros((X.shape[1] + 1, off[-1])), 0.5 * rs.randn(X.shape[1] + 1, off[-1])):
        f, g = prob.valgrad(G(theta))
        f2, g2 = prob.valgrad(G(theta))
        assert torch.equal(f, f2) and torch.equal(g, g2)                # bitwise
        rf, rg = ref_valgrad_all(theta, X, y, sizes, cvalid)
        A = max(1.0, float((np.abs(X) @ np.abs(theta[:-1]) + np.abs(theta[-1])).max()))
        ef = np.abs(f.cpu().numpy() - rf).max()
        eg = np.abs(g.cpu().numpy() - rg).max()
        tf, tg = 512 * ULP * max(A, float(rf.max())), 512 * ULP * max(1.0, float(np.abs(X).max())) * A
        print(name, "A", A, "|f - ref|", ef, "bound", tf, "|grad - ref|", eg, "bound", tg)
        assert ef <= tf and eg <= tg
        assert not g.cpu().numpy()[:, ~cvalid].any()                    # exactly 0 at invalid classes
        P, pred = prob.proba(G(theta))
        for k in range(len(sizes)):
            sl = slice(off[k], off[k + 1])
            rP, rpred = ref_proba(theta[:, sl], X, y[:, k], cvalid[sl])
            assert np.abs(P.cpu().numpy()[:, sl] - rP).max() <= 512 * ULP * A
            if theta.any():                                             # at zero every logit ties: first valid class
                assert np.array_equal(pred.cpu().numpy()[:, k], rpred)
            else:
                assert (pred.cpu().numpy()[:, k] == np.flatnonzero(cvalid[sl])[0]).all()
    assert flags.tolist() == [0, 0]
    if name == "small":
        assert (~cvalid).any()


def test_pair_counts_exact(golden):
    from hipvae import functional as HF
    g = golden
    flags = HF.disent_flags(dev())
    ones = torch.ones(4, dtype=torch.int32, device=dev())
    c2, pos, neg = HF.logreg_auc(G(g["tie_scores"]), G(g["tie_y"].reshape(-1, 1)), [4], ones, flags)
    r2, rp, rn = ref_pair_counts(g["tie_scores"], g["tie_y"], np.ones(4, dtype=bool))
    assert c2.tolist() == r2.tolist() and pos.tolist() == rp.tolist() and neg.tolist() == rn.tolist()
    assert np.abs(c2.cpu().numpy() / (2.0 * rp * rn) - g["tie_auc"]).max() <= 1e-15
    for tag in ("small", "full"):                                       # 7 problems, invalid classes, several blocks
        n = 777 if tag == "full" else 60
        sizes = [int(s) for s in g["sizes"]]
        off = offsets(sizes)
        _, _, theta, cvalid, stats = solved_pair(g, tag)
        X, v = ref_prepare(g["x_test"][:n], stats), g["v_test"][:n]
        P = np.concatenate([ref_proba(theta[:, off[k]:off[k + 1]], X, v[:, k], cvalid[off[k]:off[k + 1]])[0]
                            for k in range(7)], 1)
        c2, pos, neg = HF.logreg_auc(G(P), G(v), sizes, G(cvalid.astype(np.int32)), flags)
        c2b = HF.logreg_auc(G(P), G(v), sizes, G(cvalid.astype(np.int32)), flags)[0]
        assert torch.equal(c2, c2b)
        for k in range(7):
            sl = slice(off[k], off[k + 1])
            r2, rp, rn = ref_pair_counts(P[:, sl], v[:, k], cvalid[sl])
            assert c2[sl].tolist() == r2.tolist() and pos[sl].tolist() == rp.tolist() and neg[sl].tolist() == rn.tolist()
    assert flags.tolist() == [0, 0]


def test_converged_solve_and_explicitness(golden):
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    off = offsets(sizes)
    for tag in ("small", "full"):
        n = 777 if tag == "full" else 60
        rtr, rte, rtheta, cvalid, stats = solved_pair(g, tag)
        xtr, vtr, xte, vte = G(g["x_train"][:n]), G(g["v_train"][:n]), G(g["x_test"][:n]), G(g["v_test"][:n])
        flags = HF.disent_flags(dev())
        prob, theta, info = DS.fit_softmax(xtr, vtr, sizes, G(cvalid.astype(np.int32)), stats=HF.logreg_colstats(xtr, flags),
                                           flags=flags)
        print(tag, "iterations", info["iterations"], "evaluations", info["evaluations"], "max|grad|", info["gmax"])
        assert max(info["gmax"]) <= 1e-9 and len(info["gmax"]) == 7
        f, grad = prob.valgrad(theta)
        X = ref_prepare(g["x_train"][:n], stats)
        fstar = ref_valgrad_all(rtheta, X, g["v_train"][:n], sizes, cvalid)[0]
        P = prob.proba(theta)[0].cpu().numpy()
        for k in range(7):
            sl = slice(off[k], off[k + 1])
            nk = int(cvalid[sl][g["v_train"][:n, k]].sum())
            lam = (2.0 if cvalid[sl].sum() == 2 else 1.0) / nk
            gap = float(f[k]) - fstar[k]
            bound = float((grad[:, sl] ** 2).sum()) / (2 * lam) + 512 * ULP * max(1.0, fstar[k])
            rP = ref_proba(rtheta[:, sl], X, g["v_train"][:n, k], cvalid[sl])[0]
            dp = np.abs(P[:, sl] - rP).max()
            print(tag, "problem", k, "F - F*", gap, "bound", bound, "max |P - P*|", dp)
            assert gap <= bound and dp <= PROBA_SOLVE_TOL
        tr, te = DS.explicitness(xtr, vtr, xte, vte, sizes)
        ref = g[f"expl_{tag}"]
        print(tag, "explicitness", (tr, te), "restatement", (rtr, rte), "reference", ref)
        assert abs(tr - rtr) <= 1e-9 and abs(te - rte) <= 1e-9
        assert abs(tr - ref[0]) <= LOOSE_AUC_TOL[tag] and abs(te - ref[1]) <= LOOSE_AUC_TOL[tag]


def test_accuracies_equal_the_reference_and_errors(golden):
    from hipvae import disentangle as DS
    g = golden
    xtr, xte = G(g["fc_x_train"]), G(g["fc_x_test"])
    ytr, yte = g["fc_y_train"].astype(np.int64), g["fc_y_test"].astype(np.int64)
    for scale in (0, 1):
        acc = DS.factor_change_accuracy(xtr, ytr, xte, yte, 5, scale=bool(scale))
        print("scale", scale, "accuracy", acc, float(g[f"fc_acc_{scale}"]))
        assert acc == float(g[f"fc_acc_{scale}"])
    # a test label unseen in training counts as wrong: train on the rows of classes 0..3 only
    keep = ytr < 4
    acc = DS.factor_change_accuracy(xtr[G(keep)], ytr[keep], xte, yte, 5)
    want = ref_factor_change_accuracy(g["fc_x_train"][keep], ytr[keep], g["fc_x_test"], yte, 5, False)[0]
    assert acc == want and acc < 1.0
    with pytest.raises(ValueError, match="at least 2 classes"):
        DS.factor_change_accuracy(xtr, np.zeros_like(ytr), xte, yte, 5)
    with pytest.raises(RuntimeError, match="problem 0"):
        DS.factor_change_accuracy(xtr, ytr, xte, yte, 5, max_iter=3)
    bad = ytr.copy()
    bad[7] = 5
    with pytest.raises(ValueError, match="factor value"):
        DS.factor_change_accuracy(xtr, bad, xte, yte, 5)
    xb = xtr.clone()
    xb[3, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        DS.factor_change_accuracy(xb, ytr, xte, yte, 5)
    torch.cuda.synchronize()


# ---- end to end (helpers copied from tests/test_hip_disent.py) -------------------------------------------------------
class StubWriter:
    def __init__(self):
        self.calls = []

    def add_images(self, tag, img_tensor, global_step=None):
        self.calls.append(("add_images", tag, None, global_step))

    def add_scalar(self, tag, value, global_step=None):
        self.calls.append(("add_scalar", tag, float(value), global_step))

    def add_scalars(self, tag, values, global_step=None):
        self.calls.append(("add_scalars", tag, {k: float(v) for k, v in values.items()}, global_step))

    def flush(self):
        self.calls.append(("flush",))

    def of(self, kind, tag):
        return [c for c in self.calls if c[0] == kind and c[1] == tag]


def make_dataset():
    from solvers.vae import DisentanglementDataset

    class Synthetic(DisentanglementDataset):
        """20 deterministic 3 x 32 x 32 images ordered by their factors (sizes 4, 1, 5; the middle one never varies)."""
        factor_sizes = [4, 1, 5]
        latent_indices = [0, 2]

        def __init__(self):
            g = torch.Generator().manual_seed(3)
            base = torch.rand(20, 3, 32, 32, generator=g)
            f0, f2 = torch.arange(20) // 5, torch.arange(20) % 5
            self.images = (0.5 * base + 0.1 * f0.view(-1, 1, 1, 1) + 0.05 * f2.view(-1, 1, 1, 1)).clamp(0, 1)

        def __len__(self):
            return 20

        def __getitem__(self, i):
            return self.images[i], 0

    return Synthetic()


class WalkingSeed:
    """A FactorSampler whose ``seed`` changes on every read, so that the reference's per-batch
    ``RandomState(latent_generator.seed).randint`` yields a deterministic sequence with more than one class."""

    def __init__(self, ds, seed):
        from hipvae.disentangle import FactorSampler
        self.inner, self.next_seed = FactorSampler(ds, dev(), seed=seed), 100

    @property
    def seed(self):
        self.next_seed += 1
        return self.next_seed

    def __getattr__(self, name):
        return getattr(self.inner, name)


def test_bvae_score_end_to_end():
    import models
    from hipvae import disentangle as DS
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_dataset()
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    got = DS.compute_bvae_score(DS.FactorSampler(ds, dev(), seed=42), model, num_samples=96, batch_size=8,
                                index_state=np.random.RandomState(5))
    assert model.training and before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    # the same draws, encoded by the test
    twin, idx = DS.FactorSampler(ds, dev(), seed=42), np.random.RandomState(5)
    model.eval()
    sets = []
    for _ in range(2):
        rows, ys = [], []
        for _ in range(12):
            k = idx.randint(2)
            v_li, v_lj = twin.sample_factors_of_variation(8), twin.sample_factors_of_variation(8)
            v_li[:, k] = v_lj[:, k]
            x_li, x_lj = twin.sample_observations_from_factors(v_li), twin.sample_observations_from_factors(v_lj)
            with torch.no_grad():
                mu = model.encode(torch.cat([x_li, x_lj], 0))[0].cpu().numpy()
            rows.append(ref_zdiff(mu[:8], mu[8:]))
            ys.append(k)
        sets.append((np.stack(rows), np.array(ys)))
    model.train()
    (xtr, ytr), (xte, yte) = sets
    assert len(set(ytr.tolist())) == 2
    z, y = DS.factor_change_rows(DS.FactorSampler(ds, dev(), seed=42), model, 96, 8, np.random.RandomState(5))
    assert np.allclose(z.cpu().numpy(), xtr, rtol=2e-7, atol=0) and np.array_equal(y, ytr) and z.dtype == torch.float32
    want = tuple(ref_factor_change_accuracy(xtr, ytr, xte, yte, 2, s)[0] for s in (False, True))
    print("bvae", got, want)
    assert got == want
    with pytest.raises(ValueError, match="at least 2 classes"):       # a seeded generator fixes the index, as the reference
        DS.compute_bvae_score(DS.FactorSampler(ds, dev(), seed=42), model, num_samples=32, batch_size=8)


def test_solver_writes_all_device_scores():
    import models
    from solvers import VAESolver
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_dataset()
    w = StubWriter()
    solver = VAESolver(dataset=ds, model=model, batch_size=2, optimizer_e=torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
                       optimizer_d=torch.optim.Adam(model.decoder.parameters(), lr=2e-4), recon_loss_type="mse", beta_kl=1.0,
                       beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)
    assert solver.device_scores is None
    solver.latent_generator = WalkingSeed(ds, seed=42)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    solver.write_disentanglemnt_scores(0)                               # unset: exactly today's two records
    assert [c[:2] for c in w.calls] == [("add_scalar", "mig_score"), ("add_scalars", "mod_expl")]
    assert list(w.calls[1][2]) == ["modularity_score"]
    solver.device_scores = "all"
    n = len(w.calls)
    solver.write_disentanglemnt_scores(0)
    new = w.calls[n:]
    assert [c[:2] for c in new] == [("add_scalars", "bvae_score"), ("add_scalar", "mig_score"), ("add_scalars", "mod_expl")]
    assert list(new[0][2]) == ["score", "scaled"] and list(new[2][2]) == ["modularity_score", "explicitness_score"]
    assert all(0.0 <= v <= 1.0 for v in new[0][2].values()) and 0.0 <= new[2][2]["explicitness_score"] <= 1.0
    assert all(c[3] == 0 for c in new) and model.training
    assert before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
