"""GPU tests of the device-resident image tables (csrc/dataset.hip, hipvae/dataset.py).

Every comparison is EXACT (``torch.equal`` / bit patterns): the gather's value rule is the correctly rounded fp32 division
by 255, which numpy's and torch's fp32 division are too, so the restatement ``ref_gather`` of tests/test_dataset_host.py,
the reference datasets' recorded ``__getitem__`` tensors (golden/dataset.npz) and ``FactorSampler``'s host lookups all
have to agree with it bit for bit; scores computed from equal observations by the same kernels are equal floats.

Shapes: the 16-byte path needs W % 16 == 0 (1 x 4 x 16, 3 x 4 x 32); everything else takes the scalar form, including
images whose byte size is a multiple of 16 (8 x 8) and 90-byte images whose starts are unaligned (3 x 5 x 6).  n = 130
images of 3 x 4 x 32 are 3120 chunks = 13 blocks, n = 1 is less than one block.  No out-of-range device index is run here:
the kernel's guard is four lines to read, and the ``IndexError`` path of host indices is covered without a device."""
import numpy as np
import pytest
import torch

from test_dataset_host import GOLDEN, StandIn, ref_gather  # noqa: F401

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py
N = 37
SHAPES = [(1, 8, 8), (3, 8, 8), (3, 5, 6), (1, 4, 16), (3, 4, 32)]


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    b = torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(bits(a), bits(b))


def host_images(shape, n=N, seed=0):
    """uint8 ``[n, H, W]`` (C == 1) or ``[n, H, W, C]`` with every byte value present."""
    C, H, W = shape
    rng = np.random.RandomState(seed + 131 * C + 17 * H + W)
    a = rng.randint(0, 256, size=(n, H, W, C)).astype(np.uint8)
    a.reshape(-1)[:256] = rng.permutation(256).astype(np.uint8)
    return a[..., 0] if C == 1 else a


def index_sets():
    rng = np.random.RandomState(5)
    return {"edges": np.array([N - 1, 0, 7, 7, 0, N - 1, 20, 7], dtype=np.int64), "one": np.array([N - 1], dtype=np.int64),
            "many": rng.randint(0, N, size=130).astype(np.int64)}


def hflip(x, flip):
    from hipvae import abi
    y = torch.empty_like(x)
    f = torch.as_tensor(np.asarray(flip), dtype=torch.uint8).to(x.device)
    B, C, H, W = x.shape
    abi.call("itcv_hflip", abi.ptr(x), abi.ptr(y), abi.ptr(f), B, C * H, W, abi.stream())
    return y


# ---- the kernel against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edges", "one", "many"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_equals_restatement_bitwise(shape, which):
    from hipvae.dataset import DeviceImageTable
    imgs, idx = host_images(shape), index_sets()[which]
    table = DeviceImageTable.from_arrays(imgs, device=dev())
    assert table.image_shape == shape and table.num_images == N and table.images.dtype == torch.uint8
    planar = imgs[:, None] if imgs.ndim == 3 else imgs.transpose(0, 3, 1, 2)
    assert np.array_equal(table.images.cpu().numpy(), planar)                  # HWC -> planar on the device
    n = len(idx)
    plain = table.gather(idx)
    assert plain.shape == (n,) + shape and same_bits(plain, ref_gather(imgs, idx))
    mixed = (np.arange(n) % 3 != 1).astype(np.uint8)
    for flip in (np.zeros(n, np.uint8), np.ones(n, np.uint8), mixed):
        got = table.gather(idx, flip=flip)
        assert same_bits(got, ref_gather(imgs, idx, flip)), (shape, which, flip[:4])
    assert torch.equal(table.gather(idx, flip=mixed), hflip(plain, mixed))     # == itcv_hflip of the unflipped gather
    assert torch.equal(table.gather(idx, flip=torch.as_tensor(mixed).to(dev())), hflip(plain, mixed))
    table.check()


def test_gather_covers_every_byte_value_on_both_paths():
    from hipvae.dataset import DeviceImageTable
    want = torch.arange(256, dtype=torch.uint8).float().div(255)
    for W in (16, 8):          # 16-byte chunks, scalar form
        u8 = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 256 // W, W).to(dev())
        got = DeviceImageTable.from_device_tensor(u8).gather([0])
        assert same_bits(got.reshape(-1), want), W


def test_out_slice_leaves_the_rest_untouched():
    from hipvae.dataset import DeviceImageTable
    for shape in ((3, 4, 32), (3, 5, 6)):
        imgs = host_images(shape)
        table = DeviceImageTable.from_arrays(imgs, device=dev())
        buf = torch.full((12,) + shape, float("nan"), device=dev())
        idx = np.array([5, 36, 0, 5], dtype=np.int64)
        ret = table.gather(idx, out=buf[3:7], flip=[0, 1, 0, 1])
        assert ret.data_ptr() == buf[3:7].data_ptr()
        assert same_bits(buf[3:7], ref_gather(imgs, idx, [0, 1, 0, 1]))
        assert bool(torch.isnan(buf[:3]).all()) and bool(torch.isnan(buf[7:]).all())
        with pytest.raises(ValueError):
            table.gather(idx, out=buf[3:8])


def test_fixture_items_bitwise():
    from hipvae.dataset import DeviceImageTable
    g = np.load(GOLDEN + "/dataset.npz")
    for name, shape in (("dsprites", (1, 8, 8)), ("mpi3d", (3, 8, 8))):
        ds = StandIn(g[name + "_imgs"], 8, g[name + "_latents_values"])
        table = DeviceImageTable.from_dataset(ds, dev())
        assert table.image_shape == shape and table.factor_sizes is None
        got = table.gather(np.arange(40))
        assert same_bits(got, g[name + "_items"]), name
        lab = table.labels(np.arange(40))
        assert lab.is_cuda and np.array_equal(lab.cpu().numpy(), g[name + "_labels"])
        assert lab.dtype == torch.from_numpy(g[name + "_labels"]).dtype
        assert np.array_equal(table.labels([39, 0]).cpu().numpy(), g[name + "_labels"][[39, 0]])


def test_offsets_past_2_to_31():
    """A 4.3 GB table (allocated, not filled): image 10 923 is the first that lies wholly past byte 2^31."""
    from hipvae.dataset import DeviceImageTable
    n_img, shape = 22000, (3, 256, 256)
    per = int(np.prod(shape))
    assert 10923 * per > 2 ** 31 > 10922 * per and n_img * per > 2 ** 32
    free, _ = torch.cuda.mem_get_info(dev())
    assert free > n_img * per + (1 << 30)
    u8 = torch.empty((n_img,) + shape, dtype=torch.uint8, device=dev())
    table = DeviceImageTable.from_device_tensor(u8)
    assert table.images.data_ptr() == u8.data_ptr()                            # nothing copied
    g = torch.Generator().manual_seed(11)
    pat = torch.randint(0, 256, (3,) + shape, generator=g, dtype=torch.uint8)
    where = [10923, n_img - 2, n_img - 1]
    for k, i in enumerate(where):
        u8[i].copy_(pat[k])
    want = pat.float().div(255)
    got = table.gather(np.array(where, dtype=np.int64))
    assert same_bits(got, want)
    got = table.gather(torch.tensor(where[::-1], device=dev()), flip=[0, 1, 0], check=True)
    assert same_bits(got[0], want[2]) and same_bits(got[1], want[1].flip(-1)) and same_bits(got[2], want[0])
    del table, u8, got
    torch.cuda.empty_cache()


def test_device_indices_in_range_pass_the_check():
    from hipvae.dataset import DeviceImageTable
    imgs = host_images((3, 4, 32))
    table = DeviceImageTable.from_arrays(imgs, labels=np.arange(N), device=dev())
    idx = index_sets()["many"]
    d = torch.from_numpy(idx).to(dev())
    got = table.gather(d, check=True)
    assert same_bits(got, ref_gather(imgs, idx))
    table.gather(d, check=False)
    table.check()                                                              # nothing was out of range
    assert torch.equal(table.labels(d).cpu(), torch.from_numpy(idx))
    with pytest.raises(TypeError):
        table.gather(d.to(torch.int32))
    assert table.gather(np.zeros(0, np.int64)).shape == (0, 3, 4, 32)


# ---- sampler ---------------------------------------------------------------------------------------------------------
def make_factor_dataset(shape):
    """24 asymmetric images ordered by their factors (sizes 1, 3, 2, 4; the first never varies), stored as the reference
    classes store them (uint8 ``imgs``, ``resize``, ``latents_values``); ``__getitem__`` is ``imgs[i] / 255`` as
    ``ToTensor`` makes it."""
    from solvers.vae import DisentanglementDataset
    C, H, W = shape

    class Synthetic(DisentanglementDataset):
        factor_sizes = [1, 3, 2, 4]
        latent_indices = [1, 2, 3]

        def __init__(self):
            rng = np.random.RandomState(9)
            a = rng.randint(0, 256, size=(24, H, W, C)).astype(np.uint8)
            a[:, :, : W // 2] //= 2                                           # left half darker: no image is its own mirror
            a += (np.arange(24, dtype=np.uint8) * 3)[:, None, None, None]    # wraps, like the reference's * 255
            self.imgs = a[..., 0] if C == 1 else a
            self.resize = H
            self.latents_values = np.stack(np.unravel_index(np.arange(24), self.factor_sizes), 1)

        def __len__(self):
            return 24

        def __getitem__(self, i):
            a = self.imgs[i]
            a = a[None] if a.ndim == 2 else a.transpose(2, 0, 1)
            return torch.from_numpy(np.ascontiguousarray(a)).float().div(255), self.latents_values[i]

    return Synthetic()


def test_sampler_equals_factor_sampler():
    from hipvae.dataset import DeviceFactorSampler, DeviceImageTable
    from hipvae.disentangle import FactorSampler
    ds = make_factor_dataset((1, 8, 8))
    a, b = FactorSampler(ds, dev(), seed=3), DeviceFactorSampler(ds, dev(), seed=3)
    assert b.table.image_shape == (1, 8, 8) and b.table.factor_sizes == [1, 3, 2, 4] and b.num_latents == 3

    def same(x, y):
        (fa, oa), (fb, ob) = x, y
        assert np.array_equal(fa, fb) and oa.shape == ob.shape and oa.device == ob.device
        assert ob.dtype == torch.float32 and torch.equal(bits(oa), bits(ob))

    same(a.sample(50), b.sample(50))
    same(a.sample_fixed_factor(8, 1), b.sample_fixed_factor(8, 1))
    ga, gb = list(a.generate(130, 64)), list(b.generate(130, 64))
    assert [len(f) for f, _ in gb] == [64, 64, 2]
    for x, y in zip(ga, gb):
        same(x, y)
    # a sampler over a table that was built earlier
    c = DeviceFactorSampler(DeviceImageTable.from_dataset(ds, dev()), dev(), seed=3)
    same(FactorSampler(ds, dev(), seed=3).sample(50), c.sample(50))


def nan_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_scores_are_identical_on_both_samplers():
    """The scores' encoder is the tiny model of the other score tests, which takes 3 x 32 x 32 images: the dataset has
    the factor structure above at that size."""
    import models
    from hipvae import disentangle as DS
    from hipvae.dataset import DeviceFactorSampler
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_factor_dataset((3, 32, 32))
    fv = dict(num_train=20, num_eval=10, num_variance_estimate=64, batch_size=8)
    got = []
    for cls in (DS.FactorSampler, DeviceFactorSampler):
        s = cls(ds, dev(), seed=3)
        sc = DS.compute_scores(s, model, num_samples=200)
        f1 = DS.compute_factor_vae_score(s, model, **fv)
        f2 = DS.compute_factor_vae_score(s, model, params=dict(threshold=1e-6), **fv)   # every dimension active
        got.append([sc["mig"], sc["modularity"], *f1, *f2])
        assert all(isinstance(v, float) for v in got[-1])
    print("FactorSampler", got[0], "DeviceFactorSampler", got[1])
    assert nan_equal(got[0], got[1])
    assert got[0][0] == got[0][0] and 0.0 <= got[0][4] <= 1.0 and 0.0 <= got[0][5] <= 1.0


# ---- loader ----------------------------------------------------------------------------------------------------------
LN, LB, LSHAPE = 70, 16, (3, 4, 16)


@pytest.fixture(scope="module")
def loader_table():
    from hipvae.dataset import DeviceImageTable
    imgs = host_images(LSHAPE, n=LN, seed=3)
    table = DeviceImageTable.from_arrays(imgs, labels=np.arange(LN), device=dev())
    unit = torch.from_numpy(ref_gather(imgs, np.arange(LN)))
    assert all(not torch.equal(u, u.flip(-1)) for u in unit)
    return table, unit


def epoch(loader):
    xs, ys = zip(*[(x, y) for x, y in loader])
    assert all(x.is_cuda and x.dtype == torch.float32 and y.is_cuda for x, y in zip(xs, ys))
    return [x.shape[0] for x in xs], torch.cat(xs).cpu(), torch.cat(ys).cpu()


def test_loader_epochs(loader_table):
    from hipvae.dataset import DeviceLoader
    table, unit = loader_table
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    loader = DeviceLoader(table, LB, seed=4)
    assert len(loader) == 5
    sizes, x1, y1 = epoch(loader)
    assert sizes == [16, 16, 16, 16, 6]
    assert sorted(y1.tolist()) == list(range(LN)) and y1.tolist() != list(range(LN))     # each index once, shuffled
    assert torch.equal(bits(x1), bits(unit[y1]))                                         # each image == its row / 255
    _, x2, y2 = epoch(loader)
    assert sorted(y2.tolist()) == list(range(LN)) and y2.tolist() != y1.tolist()         # two epochs differ
    assert torch.equal(bits(x2), bits(unit[y2]))
    again = DeviceLoader(table, LB, seed=4)
    _, _, z1 = epoch(again)
    _, _, z2 = epoch(again)
    assert torch.equal(z1, y1) and torch.equal(z2, y2)                                   # the same seed repeats
    assert not torch.equal(epoch(DeviceLoader(table, LB, seed=5))[2], y1)
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    # drop_last, no shuffle, a table without labels (the labels are then the indices)
    dropped = DeviceLoader(table, LB, seed=4, drop_last=True)
    sizes, x3, y3 = epoch(dropped)
    assert len(dropped) == 4 and sizes == [16] * 4 and torch.equal(y3, y1[:64]) and torch.equal(x3, x1[:64])
    from hipvae.dataset import DeviceImageTable
    bare = DeviceImageTable.from_device_tensor(table.images)
    _, x4, y4 = epoch(DeviceLoader(bare, LB, shuffle=False))
    assert y4.tolist() == list(range(LN)) and torch.equal(bits(x4), bits(unit))


def test_loader_flips_and_pre_process(loader_table):
    from hipvae.dataset import DeviceLoader
    table, unit = loader_table
    _, x, y = epoch(DeviceLoader(table, LB, seed=4, flip_p=1.0))
    assert sorted(y.tolist()) == list(range(LN)) and torch.equal(bits(x), bits(unit[y].flip(-1)))   # all mirrored
    _, x, y = epoch(DeviceLoader(table, 64, seed=4, flip_p=0.5, drop_last=True))
    assert x.shape[0] == 64 and len(set(y.tolist())) == 64
    straight = torch.tensor([torch.equal(a, unit[i]) for a, i in zip(x, y.tolist())])
    mirrored = torch.tensor([torch.equal(a, unit[i].flip(-1)) for a, i in zip(x, y.tolist())])
    assert bool((straight ^ mirrored).all()) and bool(straight.any()) and bool(mirrored.any())
    seen = []

    def pre(xb, yb):
        seen.append(int(xb.shape[0]))
        return xb * 2.0, yb + 1000, "tag"

    out = list(DeviceLoader(table, LB, seed=4, pre_process=pre))
    assert seen == [16, 16, 16, 16, 6] and all(len(o) == 3 and o[2] == "tag" for o in out)
    xs, ys = torch.cat([o[0] for o in out]).cpu(), torch.cat([o[1] for o in out]).cpu() - 1000
    assert torch.equal(xs, unit[ys] * 2.0)


# ---- solver ----------------------------------------------------------------------------------------------------------
def test_solver_opt_in():
    import models
    from hipvae.dataset import DeviceFactorSampler, DeviceImageTable
    from hipvae.disentangle import FactorSampler
    from solvers import VAESolver
    from test_hip_disent import StubWriter
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_factor_dataset((3, 32, 32))
    w = StubWriter()
    solver = VAESolver(dataset=ds, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                       optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                       beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=1, clip=100.0)
    assert solver.latent_generator is None                      # as today: no `evaluation` package next to the solver
    solver.extra_scores = ("factor_vae",)
    solver.factor_vae_params = dict(num_train=8, num_eval=4, num_variance_estimate=64, batch_size=8, threshold=1e-6)
    solver.latent_generator = FactorSampler(ds, dev(), seed=0)
    solver.write_disentanglemnt_scores(0)
    host_records = list(w.calls)
    assert [(c[0], c[1]) for c in host_records] == [("add_scalar", "mig_score"), ("add_scalars", "mod_expl"),
                                                    ("add_scalars", "factor_vae")]
    w.calls.clear()
    table = solver.use_device_dataset(seed=0)
    assert isinstance(table, DeviceImageTable) and table.image_shape == (3, 32, 32) and table.num_images == 24
    assert isinstance(solver.latent_generator, DeviceFactorSampler) and solver.latent_generator.table is table
    solver.write_disentanglemnt_scores(0)
    print(host_records, w.calls)
    assert len(w.calls) == 3 and all(a[:2] == b[:2] and a[3] == b[3] and nan_equal(
        list(a[2].values()) if isinstance(a[2], dict) else a[2],
        list(b[2].values()) if isinstance(b[2], dict) else b[2]) for a, b in zip(host_records, w.calls))
    # an earlier table is taken as it is
    assert solver.use_device_dataset(table=table, seed=1) is table and solver.latent_generator.table is table
    assert model.training
