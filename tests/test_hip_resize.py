"""GPU tests of the device resize (csrc/resize.hip, hipvae/resize.py, hipvae/dataset.py).

Every comparison is EXACT: the kernel's bytes against Pillow's recorded bytes (golden/resize.npz) and against the
restatement of tests/resize_ref.py; the fused fp32 form against restatement / 255 as int32 bit patterns and against the
plain gather of the materialised table.  Pillow is never imported here.

Shapes (resize_ref.SHAPES): the reference's 64 -> 128 upscale (5-wide windows), 64 -> 32 (9), 256 -> 64 (17, the largest LDS
footprint) and 256 -> 128; 64 -> 256, whose 256 output rows are cut into several bands per image (band seams);
non-integer ratios; tiny images whose widths are no multiple of 16 or of 4 (the scalar load and store forms, unaligned
image starts); and the two single-pass cases.  Each case has a random image holding every byte value and a 0/255 image
whose overshoot reaches both clamps.  No out-of-range device index is launched (the guard is the one of the gather, four
lines to read; host indices are range-checked before any launch)."""
import numpy as np
import pytest
import torch

import resize_ref as R
from test_dataset_host import GOLDEN, StandIn
from test_hip_dataset import TINY, bits, dev, hflip, nan_equal, same_bits

pytestmark = pytest.mark.gpu

CASES = [(Hin, Win, Hout, Wout, C) for Hin, Win, Hout, Wout, chans in R.SHAPES for C in chans]
REPEAT = 3          # the table of a case: its two images, three times over (6 images)
EDGES = np.array([5, 0, 2, 2, 0, 5, 3, 2], dtype=np.int64)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN + "/resize.npz")
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def want():
    """The restatement's bytes per case, computed once."""
    memo = {}

    def get(case, x):
        if case not in memo:
            memo[case] = R.resize(x, case[2], case[3])
        return memo[case]

    return get


def case_table(golden, case):
    from hipvae.dataset import DeviceImageTable
    x = golden[R.case_name(*case) + "_in"]
    planar = np.concatenate([x] * REPEAT)
    return DeviceImageTable.from_device_tensor(torch.from_numpy(planar).to(dev())), x


@pytest.mark.parametrize("case", CASES, ids=lambda c: R.case_name(*c))
def test_resized_table_and_fused_gather(golden, want, case):
    Hin, Win, Hout, Wout, C = case
    table, x = case_table(golden, case)
    y = want(case, x)
    assert np.array_equal(y, golden[R.case_name(*case) + "_out"])             # restatement == Pillow, on these very inputs
    full = np.concatenate([y] * REPEAT)

    small = table.resized((Hout, Wout))
    assert small.image_shape == (C, Hout, Wout) and small.num_images == 2 * REPEAT and small.images.dtype == torch.uint8
    got = small.images.cpu().numpy()
    print(R.case_name(*case), "table mismatches:", int((got != full).sum()))
    assert np.array_equal(got, full)

    view = table.view_resized((Hout, Wout))
    assert view.image_shape == (C, Hout, Wout) and view.images is table.images
    for idx in (np.array([5], dtype=np.int64), EDGES):
        n = len(idx)
        plain = view.gather(idx)
        ref = R.unit(full[idx])
        print(R.case_name(*case), "n =", n, "fused mismatches:", int((plain.cpu().numpy().view(np.int32) != ref.view(np.int32)).sum()))
        assert plain.shape == (n, C, Hout, Wout) and same_bits(plain, ref)
        assert torch.equal(bits(plain), bits(small.gather(idx)))
        assert same_bits(view.gather(torch.from_numpy(idx).to(dev())), ref)  # device indices
        mixed = (np.arange(n) % 3 != 1).astype(np.uint8)
        for flip in (np.zeros(n, np.uint8), np.ones(n, np.uint8), mixed):
            mirrored = hflip(plain, flip)
            assert torch.equal(view.gather(idx, flip=flip), mirrored), flip[:4]
            assert torch.equal(view.gather(idx, flip=torch.as_tensor(flip).to(dev())), mirrored)
        assert same_bits(view.gather(idx, flip=mixed), np.where(mixed[:, None, None, None] != 0, ref[..., ::-1], ref))
    view.check()
    small.check()


def test_more_blocks_than_one_wave_of_the_grid(golden, want):
    case = (8, 8, 12, 12, 3)
    table, x = case_table(golden, case)
    full = np.concatenate([want(case, x)] * REPEAT)
    idx = np.random.RandomState(5).randint(0, 2 * REPEAT, size=300).astype(np.int64)
    view = table.view_resized(12)
    got = view.gather(idx)
    assert same_bits(got, R.unit(full[idx])) and torch.equal(got, table.resized(12).gather(idx))
    flip = (np.arange(300) % 2).astype(np.uint8)
    assert torch.equal(view.gather(idx, flip=flip), hflip(got, flip))
    view.check()


def test_out_slice_leaves_the_rest_untouched(golden, want):
    for case in ((64, 64, 32, 32, 3), (7, 9, 13, 4, 3), (5, 6, 10, 12, 3)):
        table, x = case_table(golden, case)
        full = np.concatenate([want(case, x)] * REPEAT)
        view = table.view_resized(case[2:4])
        buf = torch.full((12,) + view.image_shape, float("nan"), device=dev())
        idx = np.array([5, 1, 0, 5], dtype=np.int64)
        ret = view.gather(idx, out=buf[3:7], flip=[0, 1, 0, 1])
        assert ret.data_ptr() == buf[3:7].data_ptr()
        ref = R.unit(full[idx])
        ref[[1, 3]] = ref[[1, 3]][..., ::-1]
        assert same_bits(buf[3:7], ref)
        assert bool(torch.isnan(buf[:3]).all()) and bool(torch.isnan(buf[7:]).all())
        with pytest.raises(ValueError):
            view.gather(idx, out=buf[3:8])
        view.check()


def test_resized_table_carries_labels_and_factors_and_chunks(monkeypatch):
    from hipvae import dataset as D
    rng = np.random.RandomState(2)
    imgs = rng.randint(0, 256, size=(24, 8, 8, 3)).astype(np.uint8)
    ds = StandIn(imgs, 12, np.arange(48).reshape(24, 2))
    table = D.DeviceImageTable.from_dataset(StandIn(imgs, 8, ds.latents_values), dev())
    table.factor_sizes, table.latent_indices = [1, 3, 2, 4], [1, 2, 3]
    monkeypatch.setattr(D, "UPLOAD_CHUNK_BYTES", 5 * 3 * 12 * 12)             # 5 images a launch: 5 launches, the last of 4
    small = table.resized(12)
    assert np.array_equal(small.images.cpu().numpy(), R.resize(imgs.transpose(0, 3, 1, 2), 12, 12))
    view = table.view_resized(12)
    for t in (small, view):
        assert t.label_table is table.label_table and t.factor_sizes == [1, 3, 2, 4] and t.latent_indices == [1, 2, 3]
        assert np.array_equal(t.labels([23, 0]).cpu().numpy(), ds.latents_values[[23, 0]])
    for mode, kind in (("table", D.DeviceImageTable), ("gather", D.ResizedView), ("auto", D.DeviceImageTable)):
        t = D.DeviceImageTable.from_dataset(ds, dev(), device_resize=mode)
        assert type(t) is kind and t.image_shape == (3, 12, 12) and t.num_images == 24
        assert same_bits(t.gather([7, 23]), R.unit(R.resize(imgs[[7, 23]].transpose(0, 3, 1, 2), 12, 12)))
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (1000, 1 << 40))
    with pytest.raises(MemoryError):
        table.resized(12)
    assert type(table.view_resized(12)) is D.ResizedView


# ---- sampler, scores, loader ---------------------------------------------------------------------------------------------
def make_resizing_dataset(shape, resize):
    """The factor dataset of tests/test_hip_dataset.py stored at ``shape`` and served at ``resize``: ``__getitem__`` is the
    restatement of the reference's ``img.resize((resize, resize), Image.BICUBIC)`` followed by ``ToTensor``."""
    from test_hip_dataset import make_factor_dataset
    base = make_factor_dataset(shape)

    class Resizing(type(base)):
        def __init__(self):
            self.imgs, self.latents_values, self.resize = base.imgs, base.latents_values, resize
            a = self.imgs[:, None] if self.imgs.ndim == 3 else self.imgs.transpose(0, 3, 1, 2)
            self.served = torch.from_numpy(R.unit(R.resize(a, resize, resize)))

        def __getitem__(self, i):
            return self.served[i], self.latents_values[i]

    return Resizing()


@pytest.mark.parametrize("mode", ["table", "gather"])
def test_sampler_equals_factor_sampler(mode):
    from hipvae.dataset import DeviceFactorSampler
    from hipvae.disentangle import FactorSampler
    ds = make_resizing_dataset((1, 8, 8), 12)
    a, b = FactorSampler(ds, dev(), seed=3), DeviceFactorSampler(ds, dev(), seed=3, device_resize=mode)
    assert b.table.image_shape == (1, 12, 12) and b.table.factor_sizes == [1, 3, 2, 4]

    def same(x, y):
        (fa, oa), (fb, ob) = x, y
        assert np.array_equal(fa, fb) and oa.shape == ob.shape and oa.device == ob.device
        assert ob.dtype == torch.float32 and torch.equal(bits(oa), bits(ob))

    same(a.sample(50), b.sample(50))
    same(a.sample_fixed_factor(8, 1), b.sample_fixed_factor(8, 1))
    for x, y in zip(a.generate(130, 64), b.generate(130, 64)):
        same(x, y)
    b.table.check()


def test_mig_is_the_same_float_from_both_tables():
    import models
    from hipvae import disentangle as DS
    from hipvae.dataset import DeviceFactorSampler
    from solvers import VAESolver
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_resizing_dataset((3, 16, 16), 32)
    got = []
    for mode in ("table", "gather"):
        s = DeviceFactorSampler(ds, dev(), seed=3, device_resize=mode)
        got.append(DS.compute_scores(s, model, num_samples=200)["mig"])
        s.table.check()
    got.append(DS.compute_scores(DS.FactorSampler(ds, dev(), seed=3), model, num_samples=200)["mig"])
    print("mig: table, gather, host", got)
    assert all(isinstance(v, float) for v in got) and nan_equal(got[:1] * 2, got[1:]) and got[0] == got[0]
    solver = VAESolver(dataset=ds, model=model, batch_size=16, optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                       optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                       beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=None, test_iter=1, clip=100.0)
    with pytest.raises(NotImplementedError):
        solver.use_device_dataset(seed=0)
    table = solver.use_device_dataset(seed=0, device_resize="gather")
    assert table.image_shape == (3, 32, 32) and solver.latent_generator.table is table


def test_loader_over_the_view_equals_the_loader_over_the_table(golden):
    from hipvae.dataset import DeviceLoader
    case = (16, 16, 5, 5, 3)
    table, _ = case_table(golden, case)
    small, view = table.resized(5), table.view_resized(5)
    for kw in (dict(seed=4), dict(seed=4, flip_p=0.5), dict(shuffle=False, drop_last=True)):
        a, b = list(DeviceLoader(small, 4, **kw)), list(DeviceLoader(view, 4, **kw))
        assert [x.shape for x, _ in b] == ([(4, 3, 5, 5)] if kw.get("drop_last") else [(4, 3, 5, 5), (2, 3, 5, 5)])
        for (xa, ya), (xb, yb) in zip(a, b):
            assert torch.equal(bits(xa), bits(xb)) and torch.equal(ya, yb)
    view.check()
    small.check()
