"""CPU-only checks of the device-resident image tables (csrc/dataset.hip, hipvae/dataset.py): the boundary of
``itcv_gather_u8`` (header, ctypes table, library, argument checks before any launch), the numpy restatement of its value
rule against the reference datasets' recorded ``__getitem__`` tensors (golden/dataset.npz, bit for bit), and the host
logic that needs no device: what ``from_dataset`` refuses, the host index range check, the sampler's index arithmetic
and the loader's batch arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def ref_gather(imgs, idx, flip=None):
    """The rule of itcv_gather_u8 restated: ``imgs`` uint8 ``[N, H, W]`` or ``[N, H, W, C]`` -> fp32 ``[n, C, H, W]``,
    ``imgs[idx] / 255`` in fp32 (numpy's fp32 division is the IEEE one), image j mirrored along W where ``flip[j]``."""
    imgs = np.asarray(imgs)
    assert imgs.dtype == np.uint8
    planar = imgs[:, None] if imgs.ndim == 3 else imgs.transpose(0, 3, 1, 2)
    out = planar[np.asarray(idx, dtype=np.int64)].astype(np.float32) / np.float32(255)
    if flip is not None:
        f = np.asarray(flip).astype(bool)
        out[f] = out[f][..., ::-1]
    return np.ascontiguousarray(out)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "dataset.npz"))
    return {k: g[k] for k in g.files}


def test_gather_symbol_in_header_table_and_library():
    from hipvae import abi
    text = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    assert int(re.search(r"#define ITCV_ABI_VERSION (\d+)", text).group(1)) == 4 == abi.ABI_VERSION
    assert abi.lib.itcv_abi_version() == 4
    decl = re.search(r"int itcv_gather_u8\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == 10
    kinds = [abi.p if "*" in a else (abi.i64 if a.startswith("long long") else abi.i32) for a in args]
    assert abi.SIGNATURES["itcv_gather_u8"] == (abi.i32, kinds)
    assert hasattr(ctypes.CDLL(abi.LIB_PATH), "itcv_gather_u8")


def test_gather_argument_checks_need_no_gpu():
    from hipvae import abi
    fake = 4096       # never dereferenced: every call below is refused before a launch
    ok = dict(table=fake, num_images=5, rows=4, W=16, idx=fake, n=2, flip=None, out=fake, flags=fake)
    for bad in (dict(table=None), dict(idx=None), dict(out=None), dict(flags=None), dict(num_images=0),
                dict(num_images=-3), dict(rows=0), dict(W=0), dict(W=-16), dict(n=0), dict(n=-1),
                dict(rows=1 << 16, W=1 << 15)):
        a = dict(ok, **bad)
        rc = abi.lib.itcv_gather_u8(a["table"], a["num_images"], a["rows"], a["W"], a["idx"], a["n"], a["flip"], a["out"],
                                    a["flags"], None)
        assert rc != 0 and "itcv_gather_u8" in abi.last_error(), bad
    with pytest.raises(RuntimeError, match="itcv_gather_u8"):
        abi.call("itcv_gather_u8", None, 1, 1, 1, None, 1, None, None, None, None)


def test_restatement_matches_the_reference_items(golden):
    for name in ("dsprites", "mpi3d"):
        imgs, items = golden[name + "_imgs"], golden[name + "_items"]
        assert imgs.dtype == np.uint8 and items.dtype == np.float32 and len(imgs) == 40
        assert np.array_equal(imgs, golden[name + "_raw"] * 255)                 # the constructor's wrap, as stored
        got = ref_gather(imgs, np.arange(40))
        assert got.shape == items.shape and np.array_equal(got.view(np.uint32), items.view(np.uint32)), name
        assert np.array_equal(golden[name + "_labels"], golden[name + "_latents_values"])
    assert len(np.unique(golden["dsprites_imgs"])) == 256                        # every byte value is pinned
    # the division is not a product with 1/255: the two differ for 126 byte values
    b = np.arange(256, dtype=np.uint8)
    div = torch.from_numpy(b).float().div(255).numpy()
    assert np.array_equal(ref_gather(b.reshape(1, 1, 256), [0]).ravel().view(np.uint32), div.view(np.uint32))
    assert int((b.astype(np.float32) * np.float32(1 / 255.0) != div).sum()) == 126
    flipped = ref_gather(golden["mpi3d_imgs"], [3, 3], [0, 1])
    assert np.array_equal(flipped[1], flipped[0][:, :, ::-1]) and not np.array_equal(flipped[0], flipped[1])


class StandIn:
    """What from_dataset reads of a reference dataset."""

    def __init__(self, imgs, resize, latents_values=None):
        self.imgs, self.resize, self.latents_values = imgs, resize, latents_values


def test_from_dataset_refuses_before_any_device_use(golden, monkeypatch):
    from hipvae.dataset import DeviceImageTable

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    imgs = golden["dsprites_imgs"]
    with pytest.raises(TypeError, match="uint8"):
        DeviceImageTable.from_dataset(StandIn(imgs.astype(np.float32) / 255, 8), "cuda:0")
    with pytest.raises(TypeError, match="uint8"):
        DeviceImageTable.from_dataset(StandIn(imgs.astype(np.int64), 8), "cuda:0")
    with pytest.raises(NotImplementedError, match="resize"):
        DeviceImageTable.from_dataset(StandIn(imgs, 64), "cuda:0")
    with pytest.raises(NotImplementedError, match="resize"):
        DeviceImageTable.from_dataset(StandIn(golden["mpi3d_imgs"], 4), "cuda:0")
    with pytest.raises(TypeError):
        DeviceImageTable.from_arrays(imgs.astype(np.int32), device="cuda:0")


def test_host_indices_are_range_checked_before_any_launch(monkeypatch):
    from hipvae import abi
    from hipvae.dataset import DeviceImageTable
    table = DeviceImageTable(torch.zeros(5, 1, 4, 16, dtype=torch.uint8), torch.arange(5))   # host memory: no launch can work
    assert len(table) == 5 and table.image_shape == (1, 4, 16)

    def no_launch(*a, **k):
        raise AssertionError("a kernel was launched")

    monkeypatch.setattr(abi, "call", no_launch)
    for bad in ([-1], [5], np.array([0, 4, 5]), torch.tensor([2, -1])):
        with pytest.raises(IndexError, match="outside"):
            table.gather(bad)
        with pytest.raises(IndexError):
            table.labels(bad)
    with pytest.raises(TypeError):
        table.gather(np.array([0.5]))
    with pytest.raises(abi.HipExtensionError):
        DeviceImageTable.from_device_tensor(torch.zeros(5, 1, 4, 16, dtype=torch.uint8))
    with pytest.raises(TypeError):
        DeviceImageTable(torch.zeros(5, 1, 4, 16))


def test_in_range_host_gather_refuses_host_memory():
    """No CPU fallback: a table in host memory reaches the binding and is refused there."""
    from hipvae import abi
    from hipvae.dataset import DeviceImageTable
    table = DeviceImageTable(torch.zeros(5, 1, 4, 16, dtype=torch.uint8))
    with pytest.raises(abi.HipExtensionError):
        table.gather([0, 4], out=torch.empty(2, 1, 4, 16))


class Factors:
    factor_sizes = [1, 3, 2, 4]
    latent_indices = [1, 2, 3]


def test_device_sampler_draws_the_same_indices():
    from hipvae.dataset import DeviceFactorSampler, DeviceImageTable
    from hipvae.disentangle import FactorSampler
    table = DeviceImageTable(torch.zeros(24, 1, 8, 8, dtype=torch.uint8))
    table.factor_sizes, table.latent_indices = Factors.factor_sizes, Factors.latent_indices
    a, b = FactorSampler(Factors(), "cpu", seed=3), DeviceFactorSampler(table, "cpu", seed=3)
    c = DeviceFactorSampler(Factors(), "cpu", seed=3, table=table)
    assert b.factor_sizes == a.factor_sizes and b.latent_indices == a.latent_indices and b.factor_bases == a.factor_bases
    for n in (50, 1, 130):
        fa, fb, fc = (s.sample_factors_of_variation(n) for s in (a, b, c))
        assert np.array_equal(fa, fb) and np.array_equal(fa, fc)
        ia, ib, ic = a.indices_from_factors(fa), b.indices_from_factors(fb), c.indices_from_factors(fc)
        assert np.array_equal(ia, ib) and np.array_equal(ia, ic) and ia.min() >= 0 and ia.max() < 24
    with pytest.raises(ValueError, match="holds"):
        DeviceFactorSampler(Factors(), "cpu", table=DeviceImageTable(torch.zeros(23, 1, 8, 8, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="factor_sizes"):
        DeviceFactorSampler(DeviceImageTable(torch.zeros(24, 1, 8, 8, dtype=torch.uint8)), "cpu")


@pytest.mark.parametrize("drop_last", [False, True])
def test_loader_batch_arithmetic(drop_last):
    from torch.utils.data import DataLoader
    from hipvae.dataset import DeviceImageTable, DeviceLoader
    N, B = 37, 8
    loader = DeviceLoader(DeviceImageTable(torch.zeros(N, 1, 4, 4, dtype=torch.uint8)), B, drop_last=drop_last)
    torch_loader = DataLoader(list(range(N)), B, shuffle=True, drop_last=drop_last)
    sizes = DeviceLoader.batch_sizes(N, B, drop_last)
    assert sizes == [len(b) for b in torch_loader] == ([8, 8, 8, 8] if drop_last else [8, 8, 8, 8, 5])
    assert len(loader) == len(torch_loader) == len(sizes)
    assert DeviceLoader.batch_sizes(16, 8, False) == DeviceLoader.batch_sizes(16, 8, True) == [8, 8]
    assert DeviceLoader.batch_sizes(3, 8, True) == [] and DeviceLoader.batch_sizes(3, 8, False) == [3]
    with pytest.raises(ValueError):
        DeviceLoader(loader.table, 0)
