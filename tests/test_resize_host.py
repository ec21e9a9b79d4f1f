"""CPU-only checks of the device resize (csrc/resize.hip, hipvae/resize.py, hipvae/dataset.py): the restatement of
Pillow's 8-bit bicubic resize (tests/resize_ref.py) against Pillow's recorded bytes (golden/resize.npz) and, where
Pillow is installed, against Pillow live; ``bicubic_plan`` against the restatement's plan; the int32 bound; the boundary
of ``itcv_resize_u8`` (header, ctypes table, library, argument checks before any launch); the host half of
``from_image_files``; and what the new keywords refuse before any device use.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import resize_ref as R
from test_dataset_host import StandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(Hin, Win, Hout, Wout, C) for Hin, Win, Hout, Wout, chans in R.SHAPES for C in chans]
AXES = sorted({(s[0], s[2]) for s in R.SHAPES} | {(s[1], s[3]) for s in R.SHAPES})


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "resize.npz"))
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize("case", CASES, ids=lambda c: R.case_name(*c))
def test_restatement_equals_pillows_recorded_bytes(golden, case):
    Hin, Win, Hout, Wout, C = case
    name = R.case_name(*case)
    x, y = golden[name + "_in"], golden[name + "_out"]
    assert x.shape == (2, C, Hin, Win) and y.shape == (2, C, Hout, Wout) and x.dtype == y.dtype == np.uint8
    assert np.array_equal(x, R.case_images(Hin, Win, C))                     # the inputs are the documented ones
    assert len(np.unique(x[0])) == min(256, x[0].size) and set(np.unique(x[1])) <= {0, 255}
    assert np.array_equal(R.resize(x, Hout, Wout), y)


def test_golden_upscales_reach_both_clamps(golden):
    y = golden[R.case_name(64, 64, 128, 128, 1) + "_out"][1]
    assert int((y == 0).sum()) > 1000 and int((y == 255).sum()) > 1000
    assert str(golden["pillow_version"])


@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_bicubic_plan_equals_the_restatement_and_fits_int32(axis):
    from hipvae.resize import bicubic_plan
    bounds, coef = bicubic_plan(*axis)
    rb, rc = R.plan(*axis)
    assert bounds.dtype == coef.dtype == np.int32 and bounds.shape == (axis[1], 2) and coef.shape == rc.shape
    assert np.array_equal(bounds, rb) and np.array_equal(coef, rc)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= axis[0]).all()
    assert (bounds[:, 1] <= coef.shape[1]).all()
    assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()     # what the band staging relies on
    # sum |k| reaches 1.25 * 2^22 exactly (the 2:3 upscales) and never passes it: 255 * 1.25 * 2^22 + 2^21 = 1.34e9 < 2^31
    assert np.abs(rc).sum(1).max() <= 1.25 * (1 << 22) and R.max_accumulator(rc) < 2 ** 31


def test_bicubic_plan_refuses_bad_sizes():
    from hipvae.resize import bicubic_plan
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            bicubic_plan(*bad)
    b, c = bicubic_plan(8, 8)                                               # a plan exists; ResizePlan never asks for it
    assert b.shape == (8, 2) and c.shape == (8, 5)


def test_plan_and_restatement_equal_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    from hipvae.resize import bicubic_plan
    rng = np.random.RandomState(12)
    shapes = [(int(a), int(b), int(c), int(d)) for a, b, c, d in rng.randint(1, 41, size=(10, 4))] + [(33, 47, 33, 11)]
    for Hin, Win, Hout, Wout in shapes:
        for C in (1, 3):
            x = rng.randint(0, 256, size=(C, Hin, Win)).astype(np.uint8)
            img = Image.fromarray(x[0], "L") if C == 1 else Image.fromarray(np.ascontiguousarray(x.transpose(1, 2, 0)), "RGB")
            y = np.asarray(img.resize((Wout, Hout), Image.BICUBIC))
            y = y[None] if C == 1 else y.transpose(2, 0, 1)
            assert np.array_equal(R.resize(x, Hout, Wout), y), (Hin, Win, Hout, Wout, C)
        for a, b in ((Hin, Hout), (Win, Wout)):
            got, want = bicubic_plan(a, b), R.plan(a, b)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (a, b)


def test_resize_symbol_in_header_table_and_library():
    from hipvae import abi
    text = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    decl = re.search(r"int itcv_resize_u8\((.*?)\);", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == 20
    kinds = [abi.p if "*" in a else (abi.i64 if a.startswith("long long") else abi.i32) for a in args]
    assert abi.SIGNATURES["itcv_resize_u8"] == (abi.i32, kinds)
    assert hasattr(ctypes.CDLL(abi.LIB_PATH), "itcv_resize_u8")
    assert "resize.hip" in open(os.path.join(abi.CSRC, "Makefile")).read()


def test_resize_argument_checks_need_no_gpu():
    from hipvae import abi
    fake = 4096       # never dereferenced: every call below is refused before a launch
    ok = dict(table=fake, num_images=5, planes=3, Hin=8, Win=8, idx=fake, n=2, flip=None, xb=fake, xc=fake, kx=5, yb=fake,
              yc=fake, ky=5, Hout=12, Wout=12, out=fake, f32=1, flags=fake)
    order = ("table", "num_images", "planes", "Hin", "Win", "idx", "n", "flip", "xb", "xc", "kx", "yb", "yc", "ky", "Hout",
             "Wout", "out", "f32", "flags")
    for bad in (dict(table=None), dict(out=None), dict(flags=None), dict(num_images=0), dict(planes=0), dict(Hin=0),
                dict(Win=-8), dict(Hout=0), dict(Wout=0), dict(n=0), dict(n=-1),
                dict(idx=None, n=6),                                        # images 0..n-1 of a table of 5
                dict(xc=None), dict(kx=0), dict(yc=None), dict(ky=0),
                dict(xb=None, xc=None),                                     # no horizontal pass, yet the width changes
                dict(yb=None, yc=None),
                dict(xb=None),                                              # coefficients without bounds
                dict(xb=None, xc=None, yb=None, yc=None, Hout=8, Wout=8),   # fp32 copy: that is itcv_gather_u8
                dict(Hin=1 << 15, Win=1 << 15), dict(Hout=1 << 15, Wout=1 << 15)):
        a = dict(ok, **bad)
        rc = abi.lib.itcv_resize_u8(*[a[k] for k in order], None)
        assert rc != 0 and "itcv_resize_u8" in abi.last_error(), bad
    with pytest.raises(RuntimeError, match="itcv_resize_u8"):
        abi.call("itcv_resize_u8", *([None, 1, 1, 1, 1, None, 1] + [None] * 3 + [0, None, None, 0, 1, 1, None, 0, None, None]))


def test_host_half_of_from_image_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from hipvae.dataset import DeviceImageTable
    rng = np.random.RandomState(4)
    paths = []
    for k, (h, w, mode) in enumerate(((16, 16, "RGB"), (12, 20, "RGB"), (16, 16, "L"))):
        a = rng.randint(0, 256, size=(h, w, 3) if mode == "RGB" else (h, w)).astype(np.uint8)
        paths.append(str(tmp_path / f"im{k}.png"))
        Image.fromarray(a, mode).save(paths[-1])
    host = DeviceImageTable.decode_image_files(paths, input_height=16)
    assert host.shape == (3, 16, 16, 3) and host.dtype == np.uint8
    got = R.resize(host.transpose(0, 3, 1, 2), 8, 8)
    for p, g in zip(paths, got):
        want = Image.open(p).convert("RGB").resize((16, 16), Image.BICUBIC).resize((8, 8), Image.BICUBIC)
        assert np.array_equal(g, np.asarray(want).transpose(2, 0, 1)), p
    assert np.array_equal(host[0], np.asarray(Image.open(paths[0])))          # a same-size resize changes nothing


class FileBacked:
    """What from_dataset reads of a UkiyoE-shaped dataset."""

    def __init__(self, root, entries, resize):
        self.root, self.entries, self.resize = root, entries, resize


def test_new_keywords_refuse_before_any_device_use(monkeypatch):
    from hipvae.dataset import DeviceFactorSampler, DeviceImageTable

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch, "empty", no_device)
    imgs = np.zeros((24, 8, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="device_resize"):
        DeviceImageTable.from_dataset(StandIn(imgs, 64), "cuda:0", device_resize="bogus")
    with pytest.raises(ValueError, match="device_resize"):
        DeviceImageTable.from_dataset(StandIn(imgs, 8), "cuda:0", device_resize=True)
    with pytest.raises(ValueError, match="device_resize"):
        DeviceFactorSampler(StandIn(imgs, 64), "cuda:0", device_resize="bogus")
    with pytest.raises(NotImplementedError, match="resize"):
        DeviceImageTable.from_dataset(StandIn(imgs, 64), "cuda:0")           # no keyword: as before
    with pytest.raises(NotImplementedError, match="device_resize"):
        DeviceImageTable.from_dataset(FileBacked("/nowhere", [("a.jpg", 0)], 64), "cuda:0")
    with pytest.raises(TypeError, match="uint8"):
        DeviceImageTable.from_dataset(StandIn(imgs.astype(np.float32), 64), "cuda:0", device_resize="table")
    table = DeviceImageTable(torch.zeros(5, 1, 8, 8, dtype=torch.uint8))     # host memory: no launch can work
    for bad in (0, -3, (8, 0), (8, 8, 8), 2.5):
        with pytest.raises(ValueError, match="size"):
            table.view_resized(bad)
        with pytest.raises(ValueError, match="size"):
            table.resized(bad)
    assert table.view_resized(8) is table and table.resized((8, 8)) is table
    view = table.view_resized((12, 4))
    assert view.image_shape == (1, 12, 4) and view.num_images == 5 and view.images is table.images
    with pytest.raises(IndexError, match="outside"):                        # the host range check, before any launch
        view.gather([5])
