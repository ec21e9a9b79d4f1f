"""GPU tests of the device-side DCI score (csrc/gbt.hip, hipvae/gbt.py, hipvae/disentangle.py) against the numpy fp64
restatement of tests/test_gbt_host.py at the same inputs.

Bounds.  Everything integer is compared EXACTLY: bins, nbins, histogram tables, split feature / bin, node sums, accuracy
counts, predictions.  Leaf values are correctly rounded IEEE operations on exact integers: compared exactly.  Gains:
1e-15 relative.  Gradients: the device's ``exp`` and numpy's may differ in the last bit, so g, h agree to 1e-14 and the
quantised gq, hq to one unit; the end-to-end fixture satisfies the stability condition asserted in the host test, under
which such a difference cannot change a tree, so there the tree arrays are equal and importances and the DCI triple
agree to 1e-12."""
import numpy as np
import pytest
import torch

from test_gbt_host import (NODES, ONE_Q, RUNS, fixture_fit, load_fixture, offsets, ref_bin, ref_completeness, ref_cuts,
                           ref_dci, ref_disentanglement, ref_grad, ref_hist, ref_leaf, ref_present, ref_split)

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def flags():
    from hipvae import functional as HF
    return HF.disent_flags(dev())


# ---- bins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, max_bin", [(1000, 256), (1000, 4), (300, 256)])
def test_cuts_and_bins(N, max_bin):
    from hipvae import functional as HF
    rs = np.random.RandomState(N + max_bin)
    wide = rs.randn(N, 9).astype(np.float32)
    wide[:, 0] = np.float32(-2.5)                                        # constant: one bin
    wide[:, 1] = rs.choice([-1.0, 0.25, 7.0], size=N).astype(np.float32)  # three distinct values
    wide[:, 3] = np.round(wide[:, 3] * 4) / 4                            # heavy ties
    x = wide[:, :5]
    xd = G(wide)[:, :5]
    assert xd.stride() == (9, 1)
    other = rs.randn(77, 5).astype(np.float32) * 2                       # "test rows": binned with the training cuts
    cuts, nbins = ref_cuts(x, max_bin)
    f = flags()
    dc, dn = HF.gbt_cuts(xd, max_bin)
    assert np.array_equal(dn.cpu().numpy(), nbins) and nbins[0] == 1 and nbins[1] == 3 and nbins.max() <= max_bin
    for d in range(5):
        assert np.array_equal(dc[d, :nbins[d] - 1].cpu().numpy(), cuts[d]), d
    assert np.array_equal(HF.gbt_bin(xd, dc, dn, max_bin, f).cpu().numpy(), ref_bin(x, cuts))
    assert np.array_equal(HF.gbt_bin(G(other), dc, dn, max_bin, f).cpu().numpy(), ref_bin(other, cuts))
    assert f.tolist() == [0, 0]


# ---- gradients -------------------------------------------------------------------------------------------------------
def test_gradients():
    from hipvae import functional as HF
    rs = np.random.RandomState(4)
    N, sizes = 257, [2, 5]
    cvalid = np.array([1, 1, 1, 1, 1, 0, 1], dtype=bool)                 # class 3 of the second problem takes no part
    y = np.stack([rs.randint(2, size=N), rs.randint(5, size=N)], 1).astype(np.int32)
    F = rs.randn(7, N) * 3.0
    g, h, gq, hq = ref_grad(F, y, sizes, cvalid)
    f = flags()
    dgq, dhq, dg, dh = HF.gbt_grad(G(F), G(y), sizes, G(cvalid.astype(np.int32)), f, with_fp64=True)
    eg, eh = np.abs(dg.cpu().numpy() - g).max(), np.abs(dh.cpu().numpy() - h).max()
    print("max |g - ref|", eg, "max |h - ref|", eh)
    assert eg <= 1e-14 and eh <= 1e-14
    assert np.abs(dgq.cpu().numpy() - gq).max() <= 1 and np.abs(dhq.cpu().numpy() - hq).max() <= 1
    assert not dgq[5].any() and not dhq[5].any() and not dgq[2:, G(y[:, 1] == 3)].any()   # invalid class, invalid rows
    assert (dhq.cpu().numpy()[[0, 1]] > 0).all() and f.tolist() == [0, 0]


# ---- histogram -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, D, level, B, kind", [
    (1, 1, 0, 256, "random"), (4099, 3, 5, 256, "random"), (4099, 130, 0, 16, "random"), (4099, 130, 5, 256, "random"),
    (4099, 3, 0, 256, "onebin"), (20000, 3, 2, 64, "random")])
def test_histogram_tables_exact(N, D, level, B, kind):
    from hipvae import functional as HF
    rs = np.random.RandomState(N + D + level)
    nn, base = 1 << level, (1 << level) - 1
    bins = rs.randint(B, size=(D, N)).astype(np.uint8)
    bins[D // 2] = 0                                                     # a feature with one bin
    if kind == "onebin":
        bins[:] = 7                                                      # every row in one bin: maximal LDS contention
    node = (base + rs.randint(nn, size=(3, N))).astype(np.uint8)
    if nn > 2:
        node[node == base + 3] = base + 4                                # a node without rows
    if level:
        node[:, ::5] = 0                                                 # rows that stopped in a leaf above the level
    gq = rs.randint(-ONE_Q, ONE_Q + 1, size=(3, N)).astype(np.int64)
    hq = rs.randint(0, ONE_Q // 2 + 1, size=(3, N)).astype(np.int64)
    cvalid = np.array([1, 0, 1], dtype=np.int32)
    tab = HF.gbt_hist(G(bins), G(gq), G(hq), G(node), G(cvalid), level, B).cpu().numpy()
    assert tab.shape == (3, nn, D, B, 2) and not tab[1].any()            # an invalid class slot: cleared, not built
    for c in (0, 2):
        assert np.array_equal(tab[c], ref_hist(bins, gq[c], hq[c], node[c], level, B)), c
    part = HF.gbt_hist(G(bins), G(gq), G(hq), G(node), G(cvalid), level, B, c0=2, nc=1).cpu().numpy()   # a class chunk
    assert np.array_equal(part[0], tab[2])
    if nn > 2:
        assert not tab[0][3].any()


# ---- split -----------------------------------------------------------------------------------------------------------
def _split_case(name):
    """(tab [D][B][2] int64, nbins[D]) of one root node."""
    rs = np.random.RandomState(9)
    if name == "tie_features":                                            # feature 4 duplicates feature 1, the informative one
        N, D, B = 2000, 6, 256
        y = rs.randint(2, size=N)
        x = rs.randn(N, D).astype(np.float32)
        x[:, 1] += 1.5 * y
        x[:, 4] = x[:, 1]
        cuts, nbins = ref_cuts(x, B)
        bins = ref_bin(x, cuts)
        p = 0.5
        gq = np.rint((p - y) * 2.0 ** 24).astype(np.int64) + rs.randint(-1000, 1000, size=N)
        hq = np.full(N, ONE_Q // 2, dtype=np.int64)
        return ref_hist(bins, gq, hq, np.zeros(N, dtype=np.uint8), 0, B)[0], nbins
    tab = np.zeros((2, 8, 2), dtype=np.int64)
    if name == "empty_bin":                                               # bins 1..2 of feature 1 are empty: b = 0, 1, 2 tie
        tab[0, :4, 1] = ONE_Q
        tab[1, 0], tab[1, 3] = (-3 * ONE_Q, 2 * ONE_Q), (3 * ONE_Q, 2 * ONE_Q)
        return tab, np.array([4, 5], dtype=np.int32)
    if name == "min_child_weight":                                        # the best raw cut isolates a row of weight < 1
        tab[0, 0], tab[0, 1], tab[0, 2] = (-9 * ONE_Q, ONE_Q - 1), (ONE_Q, 3 * ONE_Q), (2 * ONE_Q, 3 * ONE_Q)
        tab[1, 0] = tab[0].sum(0)
        return tab, np.array([3, 2], dtype=np.int32)
    if name == "below_threshold":                                         # a real but tiny gain: stays a leaf
        tab[0, 0], tab[0, 1] = (-1500, 4 * ONE_Q), (1500, 4 * ONE_Q)
        tab[1, 0] = tab[0].sum(0)
        return tab, np.array([2, 1], dtype=np.int32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["tie_features", "empty_bin", "min_child_weight", "below_threshold"])
def test_split_from_given_tables(name):
    from hipvae import functional as HF
    tab, nbins = _split_case(name)
    D, B = tab.shape[:2]
    GP, HP = int(tab[0, :, 0].sum()), int(tab[0, :, 1].sum())
    want = ref_split(tab, nbins, GP, HP, 1.0)
    trees = tuple(t[0] for t in HF.gbt_tree_arrays(1, 1, dev()))
    nsum = torch.zeros((1, NODES, 2), dtype=torch.int64, device=dev())
    HF.gbt_split(G(tab[None, None]), G(nbins), G(np.ones(1, dtype=np.int32)), 0, trees, nsum, lam=1.0, eta=0.3)
    tfeat, tbin, tvalue, tgain = (t[0].cpu().numpy() for t in trees)
    nsum = nsum[0].cpu().numpy()
    assert tuple(nsum[0]) == (GP, HP) and tvalue[0] == ref_leaf(GP, HP, 1.0, 0.3)
    if name == "below_threshold":
        raw = 0.5 * ((1500 / 2.0 ** 24) ** 2 / 5.0 * 2)
        assert want is None and 0 < raw < 1e-6
    if want is None:
        assert (tfeat == -1).all() and tgain[0] == 0.0 and not tvalue[1:].any()
        return
    d, b, gain, GL, HL, _ = want
    print(name, "split", (d, b), "gain", gain, "device", tgain[0])
    assert (tfeat[0], tbin[0]) == (d, b)
    assert abs(tgain[0] - gain) <= 1e-15 * abs(gain)
    assert tuple(nsum[1]) == (GL, HL) and tuple(nsum[2]) == (GP - GL, HP - HL)
    assert tvalue[1] == ref_leaf(GL, HL, 1.0, 0.3) and tvalue[2] == ref_leaf(GP - GL, HP - HL, 1.0, 0.3)
    assert (tfeat[1:] == -1).all()
    if name == "tie_features":
        assert d == 1                                                     # not its duplicate, feature 4
    if name == "empty_bin":
        assert (d, b) == (1, 0)
    if name == "min_child_weight":
        assert (d, b) == (0, 1)                                           # b = 0 has the larger raw gain and HL < 1


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(RUNS)))
def test_fit_equals_the_restatement(i):
    from hipvae import disentangle as DS
    g, want = load_fixture(), fixture_fit(i)
    sizes = [int(s) for s in g["sizes"]]
    args = (G(g["x_train"]), G(g["y_train"]), G(g["x_test"]), G(g["y_test"]), sizes)
    got = DS.fit_boosted_trees(*args, **RUNS[i])
    tfeat, tbin, tvalue, tgain = (t.cpu().numpy() for t in got.trees)
    assert np.array_equal(got.nbins.cpu().numpy(), want["nbins"])
    assert np.array_equal(tfeat, want["tfeat"]) and np.array_equal(tbin, want["tbin"])
    assert np.array_equal(tvalue, want["tvalue"])
    rel = np.abs(tgain - want["tgain"]).max() / want["tgain"].max()
    err = np.abs(got.importance.cpu().numpy() - want["importance"]).max()
    print("splits", int((tfeat >= 0).sum()), "gain rel err", rel, "importance err", err)
    assert (np.abs(tgain - want["tgain"]) <= 1e-15 * np.abs(want["tgain"])).all()
    assert err <= 1e-12
    assert got.train_correct == want["correct"].tolist() and got.test_correct == want["correct_test"].tolist()
    assert np.array_equal(got.test_pred.cpu().numpy(), want["pred_test"])
    assert got.test_accuracy == [c / 300 for c in want["correct_test"]]
    assert np.abs(got.margins.cpu().numpy() - want["F"]).max() <= 1e-12
    triple, ref = DS.dci(*args, **RUNS[i]), ref_dci(want, 300)
    print("dci", triple, ref, "sklearn path of the reference (informational)", g["sklearn_dci"])
    assert all(abs(a - b) <= 1e-12 for a, b in zip(triple, ref))
    if i == 0:                                                            # two device runs: the same bits
        again = DS.fit_boosted_trees(*args, **RUNS[i])
        for a, b in zip(got.trees + (got.importance, got.margins, got.test_margins),
                        again.trees + (again.importance, again.margins, again.test_margins)):
            assert torch.equal(a, b)


def test_closed_forms_on_the_device():
    from hipvae import disentangle as DS
    g = load_fixture()
    for i in range(int(g["n_matrices"])):
        P = G(g[f"P{i}"], torch.float64)
        assert abs(float(DS.dci_completeness(P)) - float(g["completeness"][i])) <= 1e-12
        assert abs(float(DS.dci_disentanglement(P)) - float(g["disentanglement"][i])) <= 1e-12
        assert abs(ref_completeness(g[f"P{i}"]) - float(g["completeness"][i])) <= 1e-12
        assert abs(ref_disentanglement(g[f"P{i}"]) - float(g["disentanglement"][i])) <= 1e-12


# ---- flags -----------------------------------------------------------------------------------------------------------
def test_errors_and_unseen_test_labels():
    from hipvae import disentangle as DS
    g = load_fixture()
    sizes = [int(s) for s in g["sizes"]]
    small = dict(rounds=2, max_depth=2, max_bin=16)
    xtr, ytr, xte, yte = g["x_train"], g["y_train"], g["x_test"], g["y_test"]
    base = DS.fit_boosted_trees(G(xtr), G(ytr), G(xte), G(yte), sizes, **small)
    assert (base.test_pred[:, 2] != 3).all()                              # a class unseen in training is never predicted
    unseen = int((yte[:, 2] == 3).sum())
    assert unseen > 0 and base.test_correct[2] <= 300 - unseen
    moved = yte.copy()
    hit = np.nonzero(base.test_pred[:, 2].cpu().numpy() == yte[:, 2])[0][:10]
    moved[hit, 2] = 3                                                     # ten correct rows relabelled to the unseen class
    again = DS.fit_boosted_trees(G(xtr), G(ytr), G(xte), G(moved), sizes, **small)
    assert again.test_correct[2] == base.test_correct[2] - 10 and again.test_correct[:2] == base.test_correct[:2]
    assert again.test_accuracy[2] < base.test_accuracy[2] and again.train_correct == base.train_correct
    bad = xtr.copy()
    bad[17, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        DS.fit_boosted_trees(G(bad), G(ytr), G(xte), G(yte), sizes, **small)
    lab = ytr.copy()
    lab[5, 1] = 5
    with pytest.raises(ValueError, match="outside"):
        DS.fit_boosted_trees(G(xtr), G(lab), G(xte), G(yte), sizes, **small)
    one = ytr.copy()
    one[:, 0] = 1
    with pytest.raises(ValueError, match="at least 2 classes"):
        DS.fit_boosted_trees(G(xtr), G(one), G(xte), G(yte), sizes, **small)
    with pytest.raises(RuntimeError, match="max_depth = 7"):
        DS.fit_boosted_trees(G(xtr), G(ytr), G(xte), G(yte), sizes, rounds=1, max_depth=7)
    torch.cuda.synchronize()


# ---- compute_dci_score and the solver (helpers copied from tests/test_hip_classify.py) --------------------------------
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


SMALL = dict(informativeness_method="xgb",
             informativeness_params=dict(n_estimators=4, max_depth=3, tree_method="gpu_hist", gpu_id=0,
                                         eval_metric="mlogloss", use_label_encoder=False))


def test_compute_dci_score_end_to_end():
    import models
    from hipvae import disentangle as DS
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_dataset()
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    got = DS.compute_dci_score(WalkingSeed(ds, seed=42), model, num_samples=96, batch_size=8, params=SMALL)
    print("dci", got)
    assert len(got) == 3 and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in got)
    assert model.training and before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    assert got == DS.compute_dci_score(WalkingSeed(ds, seed=42), model, num_samples=96, batch_size=8, params=SMALL)
    # the same draws, encoded by the test, through dci()
    twin = DS.FactorSampler(ds, dev(), seed=42)
    (xtr, ytr), (xte, yte) = (DS.factor_representations(twin, model, 96, 8) for _ in range(2))
    assert got == DS.dci(xtr, ytr, xte, yte, [4, 5], rounds=4, max_depth=3)
    with pytest.raises(NotImplementedError):
        DS.compute_dci_score(WalkingSeed(ds, seed=42), model, num_samples=16, batch_size=8,
                             params=dict(informativeness_method="rf"))


def test_solver_writes_dci_from_the_device():
    import models
    from solvers import VAESolver
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_dataset()
    w = StubWriter()
    solver = VAESolver(dataset=ds, model=model, batch_size=2, optimizer_e=torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
                       optimizer_d=torch.optim.Adam(model.decoder.parameters(), lr=2e-4), recon_loss_type="mse", beta_kl=1.0,
                       beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)
    solver.latent_generator = WalkingSeed(ds, seed=42)
    solver.dci_params = SMALL
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    solver.device_scores = "all+dci"
    solver.write_disentanglemnt_scores(0)
    assert [c[:2] for c in w.calls] == [("add_scalars", "bvae_score"), ("add_scalar", "mig_score"),
                                        ("add_scalars", "mod_expl"), ("add_scalars", "dci")]
    assert list(w.calls[3][2]) == ["dci_informativeness_score", "dci_completeness_score", "dci_disentanglement_score"]
    assert all(0.0 <= v <= 1.0 for v in w.calls[3][2].values())
    assert list(w.calls[0][2]) == ["score", "scaled"] and list(w.calls[2][2]) == ["modularity_score", "explicitness_score"]
    solver.device_scores = "all"
    n = len(w.calls)
    solver.write_disentanglemnt_scores(0)
    assert [c[:2] for c in w.calls[n:]] == [("add_scalars", "bvae_score"), ("add_scalar", "mig_score"),
                                            ("add_scalars", "mod_expl")]
    assert all(c[3] == 0 for c in w.calls) and model.training
    assert before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
