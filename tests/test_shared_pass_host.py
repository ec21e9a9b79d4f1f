"""Host side of the shared decoder pass (no GPU): the entries added for it are declared in include/itcv_hip.h, bound in
hipvae.abi with matching argument counts and exported by the library; their argument validation answers before any launch;
the replay descriptor is the documented 56-byte record; the solver attribute exists and enters the graph key."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("itcv_bn_finalize_uv", "itcv_bn_train_fwd_uv", "itcv_bn_replay_desc_bytes", "itcv_bn_replay_desc",
       "itcv_bn_replay_many", "itcv_bn_replay_max_descs")


def _declaration(name):
    text = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/itcv_hip.h"
    args = m.group(1).strip()
    return [] if args == "void" else [a.strip() for a in args.split(",")]


def test_new_entries_are_declared_bound_and_exported():
    from hipvae import abi
    cdll = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert hasattr(cdll, name), name
        assert len(_declaration(name)) == len(abi.SIGNATURES[name][1]), name
    # the _uv forms are the existing entries plus ONE pointer; the existing signatures did not move
    for old, new in (("itcv_bn_train_fwd", "itcv_bn_train_fwd_uv"), ("itcv_bn_finalize", "itcv_bn_finalize_uv")):
        a, b = abi.SIGNATURES[old][1], abi.SIGNATURES[new][1]
        assert len(b) == len(a) + 1 and len(_declaration(old)) == len(a)
        k = next(i for i, d in enumerate(_declaration(new)) if "unbiased_var" in d)
        assert b[k] is abi.p and list(b[:k]) + list(b[k + 1:]) == list(a)
    assert abi.lib.itcv_abi_version() == 4


def test_replay_descriptor_validation_needs_no_gpu():
    from hipvae import abi
    lib = abi.lib
    nb = lib.itcv_bn_replay_desc_bytes()
    assert nb == 56 and lib.itcv_bn_replay_max_descs() == 64
    buf = (ctypes.c_uint8 * nb)()
    rm, rv, nbt, mean, uv = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20          # never dereferenced on the host
    assert lib.itcv_bn_replay_desc(ctypes.byref(buf), rm, rv, nbt, mean, uv, 64, 2, 0.1, 0) == 1
    assert lib.itcv_bn_replay_desc(ctypes.byref(buf), rm, rv, nbt, mean, uv, 257, 1, 1.0, 5) == 2
    raw = bytes(buf)
    assert [int.from_bytes(raw[i:i + 8], "little") for i in range(0, 40, 8)] == [rm, rv, nbt, mean, uv]
    assert [int.from_bytes(raw[i:i + 4], "little") for i in (40, 44, 52)] == [257, 1, 5]
    # track_running_stats=False: nothing to replay, the layer is left out
    assert lib.itcv_bn_replay_desc(ctypes.byref(buf), None, None, None, mean, uv, 64, 2, 0.1, 0) == 0
    # one of the two buffers alone is replayed on its own
    assert lib.itcv_bn_replay_desc(ctypes.byref(buf), None, rv, None, None, uv, 64, 2, 0.1, 0) == 1
    for bad in ((None, rm, rv, nbt, mean, uv, 64, 2, 0.1, 0),            # no descriptor
                (1, rm, rv, nbt, None, uv, 64, 2, 0.1, 0),               # running_mean without the saved mean
                (1, rm, rv, nbt, mean, None, 64, 2, 0.1, 0),             # running_var without the saved variance
                (1, rm, rv, nbt, mean, uv, 0, 2, 0.1, 0),                # C
                (1, rm, rv, nbt, mean, uv, 64, 0, 0.1, 0),               # groups
                (1, rm, rv, nbt, mean, uv, 64, 2, 1.5, 0),               # momentum
                (1, rm, rv, nbt, mean, uv, 64, 2, 0.1, -1)):             # block0
        args = list(bad)
        args[0] = ctypes.byref(buf) if args[0] else None
        assert lib.itcv_bn_replay_desc(*args) == -1, bad
        assert "itcv_bn_replay_desc" in abi.last_error()
    for bad in ((None, 1, 1, None), (1 << 20, 0, 1, None), (1 << 20, 1, 0, None), (1 << 20, 65, 65, None)):
        assert lib.itcv_bn_replay_many(*bad) != 0
        assert "itcv_bn_replay_many" in abi.last_error()
    # the _uv forms validate like the entries they extend
    assert lib.itcv_bn_finalize_uv(None, 1.0, 1e-5, 0.1, None, None, None, None, None, None, 4, None) != 0
    assert "itcv_bn_finalize" in abi.last_error()
    assert lib.itcv_bn_train_fwd_uv(*([None] * 6 + [0, 1, 8, 4, 4, 0.2, 0, 1e-5, 0.1] + [None] * 7 + [0, 0, None, 0, 0, 1, None])) != 0
    assert "itcv_bn_train_fwd" in abi.last_error()


def test_replay_without_records_launches_nothing():
    from hipvae import functional as HF
    HF.replay_bn_running([])                                                # no device, no error
    HF.replay_bn_running([(None, None, None, torch.zeros(1, 4), torch.zeros(1, 4), 0.1)])
    with pytest.raises(Exception):                                          # CPU tensors are refused, not computed on
        HF.replay_bn_running([(torch.zeros(4), torch.ones(4), None, torch.zeros(1, 4), torch.zeros(1, 4), 0.1)])


def test_solver_attribute_and_graph_key():
    import models
    from solvers import IntroSolver, VAESolver
    from solvers.intro_tc import IntroTCSovler

    class DS:
        def __len__(self):
            return 100

    m = models.SoftIntroVAE(arch="conv", cdim=3, zdim=4, channels=(8, 16), image_size=16)
    mk = lambda cls, **kw: cls(DS(), m, 4, torch.optim.Adam(m.encoder.parameters()), torch.optim.Adam(m.decoder.parameters()),
                               "mse", 1.0, 1.0, device=torch.device("cpu"), use_amp=False, grad_scaler=None, **kw)
    s = mk(IntroTCSovler, beta_neg=1.0, gamma_r=1e-8)
    assert isinstance(s, IntroSolver) and s.share_decoder_pass is True and s.batch_passes is True
    assert s._schedule_key() == (True, True)
    s.share_decoder_pass = False
    assert s._schedule_key() == (True, False)
    s.share_decoder_pass = True
    s.batch_passes = False                                   # the literal 13-pass schedule never shares
    assert s._schedule_key() == (False, False)
    s.batch_passes = True
    h = m.decoder.main.predict.register_forward_hook(lambda *a: None)
    assert s._schedule_key() == (True, False)                # a hooked decoder takes the repeated schedule
    h.remove()
    assert s._schedule_key() == (True, True)
    assert mk(VAESolver)._schedule_key() == ()
