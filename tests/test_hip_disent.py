"""GPU tests of the device-side disentanglement scores (csrc/disent.hip, hipvae/disentangle.py) against the numpy fp64
restatement of tests/test_disent_host.py and the results recorded from the unmodified reference (golden/disent.npz).

Bounds: integer tables and bin numbers are compared EXACTLY.  MI and H: 1e-10 absolute -- a pair's table has at most
32 x 256 non-zero cells, each term is a few ulp (2.2e-16) of an O(10) logarithm times c/N <= 1, and the weights c/N sum
to 1, so the sum's error stays near 1e-14 for any order of summation and below 32 * 256 * 10 * 4 ulp ~ 1e-11 in the
worst case.  Scores (a mean of differences / quotients of those): 1e-9.

What each shape launches (the histogram's plan is asked of the library through ``HF.disent_hist_tiling`` and restated in
tests/test_disent_host.py, which holds HIST_TIERS to these figures on the CPU; tc = columns per block, rp = 256 / tc rows
per step of a block, a row slice is 512 rows):

  case            N        D    factor sizes          bins  tc  column tiles      groups  LDS bytes  row slices
  tc64            1037     70   6 6 2 3 3             10    64  2, the last 6     1       51 280     3, the last 13 rows
  tc32            1037     70   6 6 2 3 3             20    32  3, the last 6     1       51 280     3
  tc4_dsprites    1037     10   3 6 40 32 32          20    4   3, the last 2     1       36 612     3
  tc2             1037     5    100 100               32    2   3, the last 1     1       52 000     3
  tc2_groups      1037     5    250 250 250           32    2   3, the last 1     3       65 000     3
  tc1_wide        1037     3    200 200               32    1   3                 1       52 800     3
  large_n         262 445  5    3 7                   20    8   1 (5 of 8 used)   1       6 440      513, the last 301 rows
  (earlier tests: tc 16 and 8 on the fixture, 2 on a single row, 1 everywhere else, 16 groups at tc 1)

1037 is a multiple of no 4 * rp, so every tier's last step of a slice is ragged.  large_n also doubles the min-max slices
to 512 rows (513 partials for the fold) and sends the binning kernel's capped grid of 4096 blocks on its second trip.
Largest errors on the MI355X over the seven cases: |MI - ref| 2.2e-16, |H - ref| 1.8e-15, MIG and modularity below 3e-16;
every integer table, marginal and bin number equal, every repeated call bit for bit."""
import os

import numpy as np
import pytest
import torch

from test_disent_host import GOLDEN, HIST_TIERS, ref_all, ref_bins, ref_mig, ref_modularity
from test_hip_extra_scores import strided

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
MI_TOL, SCORE_TOL = 1e-10, 1e-9


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(dev())


def close(a, b, tol):
    """|a - b| <= tol elementwise, nan / inf only where both have the same one."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(np.isfinite(a), fin) and \
        np.array_equal(a[~fin], b[~fin], equal_nan=True) and bool((np.abs(a[fin] - b[fin]) <= tol).all())


def check_against_restatement(mu, v, sizes, bins, x_np=None):
    """Everything the device computes for one (input, bins) against the restatement; returns (device MI, H, ref MI, H)."""
    from hipvae import disentangle as DS
    x_np = mu.cpu().numpy() if x_np is None else x_np
    b, joint, marg, mi, h = ref_all(x_np, v.cpu().numpy(), sizes, bins)
    assert np.array_equal(DS.discretize(mu, bins).cpu().numpy(), b)
    dj, dm = DS.factor_counts(mu, v, sizes, bins)
    for k in range(len(sizes)):
        assert np.array_equal(dj[k].cpu().numpy().astype(np.int64), joint[k]), k
        assert np.array_equal(dm[k].cpu().numpy().astype(np.int64), marg[k]), k
    dmi, dh = DS.mutual_info(mu, v, sizes, bins)
    assert dmi.dtype == dh.dtype == torch.float64 and dmi.is_cuda
    print("bins", bins, "max |MI - ref|", np.abs(dmi.cpu().numpy() - mi).max(), "max |H - ref|",
          np.abs(dh.cpu().numpy() - h).max())
    assert close(dmi.cpu().numpy(), mi, MI_TOL) and close(dh.cpu().numpy(), h, MI_TOL)
    return dmi, dh, mi, h


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "disent.npz"))
    return {k: g[k] for k in g.files}


def test_fixture_against_restatement_and_reference(golden):
    from hipvae import disentangle as DS
    g = golden
    sizes = [int(s) for s in g["sizes"]]
    mu, v = G(g["x"]), G(g["v"])
    for bins in (10, 20):
        dmi, dh, mi, h = check_against_restatement(mu, v, sizes, bins, g["x"])
        assert np.array_equal(DS.discretize(mu, bins).cpu().numpy(), g[f"bins{bins}"])    # the reference's, exactly
        assert close(dmi.cpu().numpy(), g[f"MI{bins}"], 1e-9) and close(dh.cpu().numpy(), g["H"], 1e-9)
    mig = DS.mig_score(mu, v, sizes)
    mod = DS.modularity_score(mu, v, sizes)
    both = DS.scores(mu, v, sizes)
    print("mig", mig, float(g["mig"]), "modularity", mod, float(g["modularity"]))
    assert abs(mig - float(g["mig"])) <= SCORE_TOL and both["mig"] == mig
    # the constant column: theta = 0, 0 / 0 -- nan exactly where the reference's numpy gives nan
    assert np.isnan(mod) and np.isnan(float(g["modularity"])) and np.isnan(both["modularity"])
    # the nine informative columns, as a row-strided view of the same tensor
    mod9 = DS.modularity_score(mu[:, :9], v, sizes)
    print("modularity of the informative columns", mod9, float(g["modularity_informative"]))
    assert abs(mod9 - float(g["modularity_informative"])) <= SCORE_TOL
    assert abs(DS.mig_score(mu, v, sizes, bins=10) - ref_mig(*ref_all(g["x"], g["v"], sizes, 10)[3:])) <= SCORE_TOL
    assert abs(mod9 - ref_modularity(ref_all(g["x"][:, :9], g["v"], sizes, 20)[3])) <= SCORE_TOL


def test_edge_hits_and_smallest_shapes():
    from hipvae import disentangle as DS
    # integers 0..10 with 10 bins: the edges 0, 1, ..., 9 are exact in fp64; x = j lands in bin j + 1, the maximum in bin 10
    x = G(np.arange(11, dtype=np.float32).reshape(11, 1))
    got = DS.discretize(x, 10).cpu().numpy()[:, 0]
    assert got.tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10]
    v = G(np.arange(11, dtype=np.int32).reshape(11, 1) % 3)
    check_against_restatement(x, v, [3], 10)
    # N = 3, D = 1, K = 1
    x3, v3 = G(np.array([[0.5], [-1.0], [2.0]], dtype=np.float32)), G(np.array([[0], [1], [1]], dtype=np.int32))
    for bins in (1, 2, 32):
        check_against_restatement(x3, v3, [2], bins)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert close(DS.modularity_score(x3, v3, [2]), ref_modularity(ref_all(x3.cpu().numpy(), v3.cpu().numpy(), [2], 20)[3]),
                     SCORE_TOL)                                       # K = 1: 0 / 0 as in numpy
    with pytest.raises(IndexError):
        DS.mig_score(x3, v3, [2])                                     # one latent has no second-largest MI
    # N = 1: lo == hi, the single sample sits in the middle bin of [x - 0.5, x + 0.5]; MI = H = 0
    x1, v1 = G(np.array([[3.0, -7.5]], dtype=np.float32)), G(np.array([[1, 0]], dtype=np.int32))
    dmi, dh, _, _ = check_against_restatement(x1, v1, [2, 1], 10)
    assert DS.discretize(x1, 10).cpu().tolist() == [[6, 6]] and not dmi.any() and not dh.any()
    assert np.isnan(DS.mig_score(x1, v1, [2, 1]))                     # H = 0: 0 / 0


@pytest.fixture(scope="module")
def tiling_case():
    """The top of every supported range at once: N = 4100 (9 row slices, the last one short), D = 129 (no multiple of any
    column tile), K = 16 with one factor of 256 values, bins = 32, and mu the right half of an [N, 2 D] tensor."""
    rs = np.random.RandomState(7)
    N, D = 4100, 129
    sizes = [2, 3, 256, 5, 1, 7, 4, 9, 2, 6, 3, 8, 2, 5, 4, 3]
    v = np.stack([rs.randint(s, size=N) for s in sizes], 1).astype(np.int32)
    W = rs.randn(len(sizes), D) * (rs.rand(len(sizes), D) < 0.2)
    wide = np.zeros((N, 2 * D), dtype=np.float32)
    wide[:, D:] = ((v / np.array(sizes)) @ W + 0.2 * rs.randn(N, D)).astype(np.float32)
    wide[:, :D] = rs.randn(N, D).astype(np.float32) * 100.0           # must not be read
    return wide, v, sizes, ref_all(wide[:, D:], v, sizes, 32)


def test_tiling_top_of_every_range_strided(tiling_case):
    from hipvae import disentangle as DS
    wide, v, sizes, (b, joint, marg, mi, h) = tiling_case
    D = wide.shape[1] // 2
    mu = G(wide)[:, D:]
    assert mu.stride() == (2 * D, 1)
    vv = G(v)
    assert np.array_equal(DS.discretize(mu, 32).cpu().numpy(), b)
    dj, dm = DS.factor_counts(mu, vv, sizes, 32)
    for k in range(16):
        assert np.array_equal(dj[k].cpu().numpy().astype(np.int64), joint[k]), k
        assert np.array_equal(dm[k].cpu().numpy().astype(np.int64), marg[k]), k
    dmi, dh = DS.mutual_info(mu, vv, sizes, 32)
    print("max |MI - ref|", np.abs(dmi.cpu().numpy() - mi).max(), "max |H - ref|", np.abs(dh.cpu().numpy() - h).max())
    assert close(dmi.cpu().numpy(), mi, MI_TOL) and close(dh.cpu().numpy(), h, MI_TOL)
    got = DS.scores(mu, vv, sizes, mig_bins=32, modularity_bins=32)
    assert close(got["mig"], ref_mig(mi, h), SCORE_TOL) and close(got["modularity"], ref_modularity(mi), SCORE_TOL)


def test_factor_groups_when_one_table_exceeds_the_lds_budget():
    """16 factors of 256 values at 32 bins: one column's table is 512 KB, so the factors go out in groups of consecutive
    factors (a path of its own in the launch plan); counts and MI against the restatement."""
    from hipvae import disentangle as DS
    rs = np.random.RandomState(9)
    N, D, sizes = 600, 3, [256] * 16
    v = np.stack([rs.randint(s, size=N) for s in sizes], 1).astype(np.int32)
    x = (v[:, :D] / 256.0 + 0.1 * rs.randn(N, D)).astype(np.float32)
    check_against_restatement(G(x), G(v), sizes, 32, x)


# ---- every tier of the histogram's launch plan, and the large-N trips ------------------------------------------------
def planted_case(N, D, sizes, seed):
    """Latents that depend on the factors (no flat tables), as the right part of a wider NaN-padded tensor."""
    rs = np.random.RandomState(seed)
    v = np.stack([rs.randint(s, size=N) for s in sizes], 1).astype(np.int32)
    W = rs.randn(len(sizes), D) * (rs.rand(len(sizes), D) < 0.5)
    x = ((v / np.array(sizes, dtype=np.float64)) @ W + 0.2 * rs.randn(N, D)).astype(np.float32)
    return x, v


def check_tier(name, x, v):
    """The plan is the one the case is named for; then bins, tables, marginals (exact), MI, H, MIG and modularity of the
    strided input against the restatement, every call made twice and compared bit for bit."""
    from hipvae import disentangle as DS
    from hipvae import functional as HF
    D, sizes, bins, tc, tiles, last, groups, lds = HIST_TIERS[name]
    assert x.shape[1] == D and HF.disent_hist_tiling(D, sizes, bins) == dict(tc=tc, column_tiles=tiles, groups=groups,
                                                                              lds_bytes=lds)
    sizes = list(sizes)
    mu, vv = strided(x), G(v)
    dmi, dh, mi, h = check_against_restatement(mu, vv, sizes, bins, x)
    got = DS.scores(mu, vv, sizes, mig_bins=bins, modularity_bins=bins)
    want_mig, want_mod = ref_mig(mi, h), ref_modularity(mi)
    print(name, "mig", got["mig"], want_mig, "modularity", got["modularity"], want_mod)
    assert np.isfinite([want_mig, want_mod]).all()
    assert close(got["mig"], want_mig, SCORE_TOL) and close(got["modularity"], want_mod, SCORE_TOL)
    dj, dm = DS.factor_counts(mu, vv, sizes, bins)
    first = torch.cat([t.reshape(-1) for t in dj + dm]).clone()
    dj, dm = DS.factor_counts(mu, vv, sizes, bins)
    assert torch.equal(first, torch.cat([t.reshape(-1) for t in dj + dm]))
    mi2, h2 = DS.mutual_info(mu, vv, sizes, bins)
    assert torch.equal(dmi, mi2) and torch.equal(dh, h2)
    assert torch.equal(DS.discretize(mu, bins), DS.discretize(mu, bins))
    assert DS.scores(mu, vv, sizes, mig_bins=bins, modularity_bins=bins) == got


@pytest.mark.parametrize("name", ["tc64", "tc32", "tc4_dsprites", "tc2", "tc2_groups", "tc1_wide"])
def test_histogram_column_tile_tiers(name):
    """N = 1037: three row slices, the last of 13 rows, a multiple of no 4 * (256 / tc).  tc2_groups is the only way factor
    groups and tc > 1 combine: a second group is opened only when the largest group holds more than half of the words one
    column may use, which leaves room for two columns at the most (the host tests sweep that)."""
    D, sizes = HIST_TIERS[name][:2]
    x, v = planted_case(1037, D, sizes, seed=21 + D)
    check_tier(name, x, v)


def test_large_n_doubled_minmax_slices_second_bins_trip_and_513_row_slices():
    """N = 262 144 + 301: the min-max slices double to 512 rows (513 partials, the last of 301 rows), the binning kernel's
    capped grid takes a second trip (N D = 1 312 225 > 4096 * 256) and the histogram runs 513 row slices at tc = 8.  The
    extremes of columns 0 and 3 sit in row 0 and in the last 301 rows: a dropped slice moves the range."""
    from hipvae import abi
    N, (D, sizes) = 262144 + 301, HIST_TIERS["large_n"][:2]
    assert abi.lib.itcv_disent_minmax_workspace(N, D) == 2 * 513 * D * 4 and N - 512 * 512 == 301
    assert N * D > 4096 * 256 and -(-N // 512) == 513
    x, v = planted_case(N, D, sizes, seed=5)
    x[0, 0], x[N - 7, 0] = 12.0, -11.5
    x[N - 300, 3], x[0, 3] = 12.5, -13.25
    for c, (lo, hi) in ((0, (N - 7, 0)), (3, (0, N - 300))):
        assert int(x[:, c].argmin()) == lo and int(x[:, c].argmax()) == hi
    check_tier("large_n", x, v)


def test_refusals(golden):
    from hipvae import disentangle as DS
    sizes = [int(s) for s in golden["sizes"]]
    mu, v = G(golden["x"]), G(golden["v"])
    with pytest.raises(RuntimeError, match="bins = 33"):
        DS.mutual_info(mu, v, sizes, 33)
    with pytest.raises(RuntimeError, match="bins = 33"):
        DS.discretize(mu, 33)
    with pytest.raises(RuntimeError, match="size 257"):
        DS.mutual_info(mu, v, sizes[:-1] + [257], 10)
    with pytest.raises(RuntimeError, match="K = 17"):
        DS.mutual_info(mu, torch.zeros((777, 17), dtype=torch.int32, device=dev()), [2] * 17, 10)
    bad = mu.clone()
    bad[5, 3] = float("nan")
    for fn in (DS.mig_score, DS.modularity_score, DS.scores):
        with pytest.raises(ValueError, match="non-finite"):
            fn(bad, v, sizes)
    bad[5, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        DS.discretize(bad, 10)
    vb = v.clone()
    vb[700, 2] = sizes[2]                                             # a factor value equal to its size
    for fn in (DS.mig_score, DS.scores):
        with pytest.raises(ValueError, match="factor value"):
            fn(mu, vb, sizes)
    vb[700, 2] = -1
    with pytest.raises(ValueError, match="factor value"):
        DS.factor_counts(mu, vb, sizes, 10)
    torch.cuda.synchronize()                                          # no fault behind any of them
    assert abs(DS.mig_score(mu, v, sizes) - float(golden["mig"])) <= SCORE_TOL


def test_bit_identical_runs(tiling_case):
    from hipvae import disentangle as DS
    wide, v, sizes, _ = tiling_case
    D = wide.shape[1] // 2
    mu, vv = G(wide)[:, D:], G(v)
    runs = []
    for _ in range(2):
        dj, dm = DS.factor_counts(mu, vv, sizes, 32)
        dmi, dh = DS.mutual_info(mu, vv, sizes, 32)
        runs.append((torch.cat([t.reshape(-1) for t in dj + dm]).clone(), dmi.clone(), dh.clone(),
                     DS.scores(mu, vv, sizes, 32, 32)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])
    assert np.array_equal(list(runs[0][3].values()), list(runs[1][3].values()), equal_nan=True)


# ---- end to end: the solvers' TensorBoard side channel ---------------------------------------------------------------
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


class CountingSampler:
    """A FactorSampler that counts how often it is asked for data."""

    def __init__(self, ds, seed):
        from hipvae.disentangle import FactorSampler
        self.inner, self.calls = FactorSampler(ds, dev(), seed=seed), 0
        self.factor_sizes, self.latent_indices = self.inner.factor_sizes, self.inner.latent_indices

    def generate(self, *a, **kw):
        self.calls += 1
        return self.inner.generate(*a, **kw)


@pytest.mark.parametrize("name", ["vae", "intro_tc"])
def test_solver_writes_device_scores(name):
    import models
    from hipvae.disentangle import FactorSampler
    from solvers import VAESolver
    from solvers.intro_tc import IntroTCSovler
    from utils import SingletonWriter
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_dataset()
    w = StubWriter()
    kw = dict(dataset=ds, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters(), lr=2e-4),
              optimizer_d=torch.optim.Adam(model.decoder.parameters(), lr=2e-4), recon_loss_type="mse", beta_kl=1.0,
              beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)
    if name == "intro_tc":
        kw.update(beta_neg=256.0, gamma_r=1e-8)
    solver = (IntroTCSovler if name == "intro_tc" else VAESolver)(**kw)
    assert solver.device_scores is None and solver.latent_generator is None      # no `evaluation` package next to us
    solver.latent_generator = sampler = CountingSampler(ds, seed=42)
    SingletonWriter().writer, SingletonWriter().cur_iter, SingletonWriter().test_iter = w, 0, 1
    x = torch.stack([ds[i][0] for i in range(16)])
    try:
        solver.train_step(x, 0)
    finally:
        SingletonWriter().writer = None
    assert model.training and sampler.calls == 1
    (mig,) = w.of("add_scalar", "mig_score")
    (mod,) = w.of("add_scalars", "mod_expl")
    assert mig[3] == 0 and mod[3] == 0 and list(mod[2]) == ["modularity_score"] and w.calls[-1] == ("flush",)
    # the same draws, encoded by the test: len(ds) // 2 = 10 samples, one short batch of the 16
    twin = FactorSampler(ds, dev(), seed=42)
    (f, obs), = list(twin.generate(10, 16))
    assert obs.shape == (10, 3, 32, 32)
    model.eval()
    with torch.no_grad():
        mu = model.encode(obs)[0]
    model.train()
    sizes = [4, 5]
    x_np = mu.cpu().numpy()
    want_mig = ref_mig(*ref_all(x_np, f, sizes, 10)[3:])
    want_mod = ref_modularity(ref_all(x_np, f, sizes, 20)[3])
    print(name, "mig", mig[2], want_mig, "modularity", mod[2]["modularity_score"], want_mod)
    assert close(mig[2], want_mig, SCORE_TOL) and close(mod[2]["modularity_score"], want_mod, SCORE_TOL)
    # scoring alone: train mode restored, running buffers and torch's RNG streams untouched
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    n = len(w.calls)
    solver.write_disentanglemnt_scores(0)
    assert len(w.calls) == n + 2 and sampler.calls == 2 and model.training
    assert before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    # nothing runs off the test iteration, without a writer, or for a dataset without factors
    solver.test_iter = 2
    solver.write_disentanglemnt_scores(1)
    solver.test_iter, solver.writer = 1, None
    solver.write_disentanglemnt_scores(0)
    solver.train_step(x, 1)
    solver.writer, solver.dataset = w, list(range(20))
    solver.write_disentanglemnt_scores(0)
    solver.dataset = ds
    assert len(w.calls) == n + 2 and sampler.calls == 2
    # a solver without a generator builds its own sampler
    solver.latent_generator = None
    solver.write_disentanglemnt_scores(0)
    assert isinstance(solver.latent_generator, FactorSampler) and len(w.of("add_scalar", "mig_score")) == 3
