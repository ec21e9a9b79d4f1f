"""CPU-only checks of the fused optimiser updates: the new entry points are declared, bound and exported alike, their
host-side argument checks fail loudly before any launch, and ``fused_update`` picks the fused update exactly for the
optimiser configurations it reproduces (everything else keeps torch's own ``opt.step()``)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("itcv_adamx_step_dev", "itcv_sgd_step_dev", "itcv_adagrad_step_dev", "itcv_rmsprop_step_dev")


def test_new_symbols_in_header_table_and_library():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert abi.ABI_VERSION == 4 == lib.itcv_abi_version()
    for flag, value in (("MAXIMIZE", 0x1), ("NESTEROV", 0x2), ("AMSGRAD", 0x4), ("DECOUPLED_WD", 0x8),
                        ("CENTERED", 0x10)):
        assert re.search(r"#define ITCV_OPT_%s 0x%x\b" % (flag, value), header), flag
        assert getattr(abi, "OPT_" + flag) == value


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
A, B, C, D, STEP = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


@pytest.mark.parametrize("args, msg", [
    (("itcv_sgd_step_dev", None, B, None, None, 8, 0.1, 0.0, 0.0, 0.0, 0, STEP, None), "itcv_sgd_step_dev"),
    (("itcv_sgd_step_dev", A, B, None, None, 8, 0.1, 0.9, 0.0, 0.0, 0, STEP, None), "momentum_buffer"),
    (("itcv_sgd_step_dev", A, B, C, None, 8, 0.1, 0.9, 0.1, 0.0, 2, STEP, None), "nesterov"),
    (("itcv_sgd_step_dev", A, B, None, None, 6, 0.1, 0.0, 0.0, 0.0, 0, STEP, None), "n % 4 == 0"),
    (("itcv_sgd_step_dev", A + 4, B, None, None, 8, 0.1, 0.0, 0.0, 0.0, 0, STEP, None), "aligned16"),
    (("itcv_sgd_step_dev", A, B, None, None, 8, -0.1, 0.0, 0.0, 0.0, 0, STEP, None), "lr >= 0.0"),
    (("itcv_sgd_step_dev", A, B, None, None, 8, 0.1, 0.0, 0.0, 0.0, 0x4, STEP, None), "flags"),
    (("itcv_sgd_step_dev", A, B, None, None, 8, 0.1, 0.0, 0.0, 0.0, 0, None, None), "step_dev"),
    (("itcv_adamx_step_dev", A, B, C, D, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0x4, STEP, None), "amsgrad"),
    (("itcv_adamx_step_dev", A, B, C, D, None, None, 8, 1e-3, 1.0, 0.999, 1e-8, 0.01, 0, STEP, None), "beta1"),
    (("itcv_adamx_step_dev", A, B, C, D, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, -0.01, 8, STEP, None),
     "weight_decay >= 0.0"),
    (("itcv_adamx_step_dev", A, B, None, D, None, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, STEP, None), "exp_avg"),
    (("itcv_adagrad_step_dev", A, B, None, None, 8, 1e-2, 0.0, 0.0, 1e-10, 0, STEP, None), "sum"),
    (("itcv_adagrad_step_dev", A, B, C, None, 8, 1e-2, -1.0, 0.0, 1e-10, 0, STEP, None), "lr_decay"),
    (("itcv_rmsprop_step_dev", A, B, C, None, None, None, 8, 1e-2, 0.99, 1e-8, 0.0, 0.9, 0, STEP, None),
     "momentum_buffer"),
    (("itcv_rmsprop_step_dev", A, B, C, None, None, None, 8, 1e-2, 0.99, 1e-8, 0.0, 0.0, 0x10, STEP, None),
     "grad_avg"),
    (("itcv_rmsprop_step_dev", A, B, None, None, None, None, 8, 1e-2, 0.99, 1e-8, 0.0, 0.0, 0, STEP, None),
     "square_avg"),
    (("itcv_rmsprop_step_dev", A, B, C, None, None, None, 8, 1e-2, -0.5, 1e-8, 0.0, 0.0, 0, STEP, None), "alpha"),
])
def test_host_side_argument_checks(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(RuntimeError):
        abi.call(*args)


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


def test_fused_update_table():
    from hipvae import abi
    from hipvae.flat import fused_update
    O = torch.optim
    ps = _params()
    # plain Adam (and AdamW without decay) maps to the existing kernel, with the hyper-parameters passed through as-is
    assert fused_update(O.Adam(ps, lr=2e-4)) == ("adam", 0, (2e-4, (0.9, 0.999), 1e-8))
    assert fused_update(O.AdamW(ps, lr=1e-3, weight_decay=0.0)) == ("adam", 0, (1e-3, (0.9, 0.999), 1e-8))
    assert fused_update(O.Adam(ps, lr=1e-3, weight_decay=0.1)) == ("adamx", 0, (1e-3, 0.9, 0.999, 1e-8, 0.1))
    assert fused_update(O.Adam(ps, lr=1e-3, weight_decay=0.1, decoupled_weight_decay=True)) == (
        "adamx", abi.OPT_DECOUPLED_WD, (1e-3, 0.9, 0.999, 1e-8, 0.1))
    assert fused_update(O.AdamW(ps)) == ("adamx", abi.OPT_DECOUPLED_WD, (1e-3, 0.9, 0.999, 1e-8, 0.01))
    assert fused_update(O.Adam(ps, amsgrad=True)) == ("adamx", abi.OPT_AMSGRAD, (1e-3, 0.9, 0.999, 1e-8, 0.0))
    assert fused_update(O.Adam(ps, maximize=True))[:2] == ("adamx", abi.OPT_MAXIMIZE)
    assert fused_update(O.AdamW(ps, amsgrad=True, maximize=True))[1] == (
        abi.OPT_AMSGRAD | abi.OPT_MAXIMIZE | abi.OPT_DECOUPLED_WD)
    assert fused_update(O.SGD(ps, lr=0.1)) == ("sgd", 0, (0.1, 0.0, 0.0, 0.0))
    assert fused_update(O.SGD(ps, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4, maximize=True)) == (
        "sgd", abi.OPT_NESTEROV | abi.OPT_MAXIMIZE, (0.1, 0.9, 0.0, 1e-4))
    assert fused_update(O.SGD(ps, lr=0.1, momentum=0.9, dampening=0.5)) == ("sgd", 0, (0.1, 0.9, 0.5, 0.0))
    assert fused_update(O.Adagrad(ps, lr=0.01, lr_decay=1e-3, weight_decay=1e-4, initial_accumulator_value=0.1,
                                  eps=1e-9)) == ("adagrad", 0, (0.01, 1e-3, 1e-4, 1e-9))
    assert fused_update(O.Adagrad(ps, maximize=True))[1] == abi.OPT_MAXIMIZE
    assert fused_update(O.RMSprop(ps, lr=0.01, alpha=0.9, eps=1e-7, weight_decay=1e-4, momentum=0.5,
                                  centered=True)) == ("rmsprop", abi.OPT_CENTERED, (0.01, 0.9, 1e-7, 1e-4, 0.5))
    assert fused_update(O.RMSprop(ps, maximize=True)) == ("rmsprop", abi.OPT_MAXIMIZE, (0.01, 0.99, 1e-8, 0.0, 0.0))
    hash(fused_update(O.AdamW(ps)))


def test_fused_update_fallbacks():
    from hipvae.flat import fused_update
    O = torch.optim
    ps = _params()

    class MySGD(O.SGD):
        pass

    assert fused_update(O.Adamax(ps)) is None
    assert fused_update(O.NAdam(ps)) is None
    assert fused_update(MySGD(ps, lr=0.1)) is None
    assert fused_update(O.SGD([{"params": ps[:1]}, {"params": ps[1:]}], lr=0.1)) is None
    assert fused_update(O.Adam(ps, capturable=True)) is None
    assert fused_update(O.AdamW(ps, capturable=True)) is None
    assert fused_update(O.RMSprop(ps, capturable=True)) is None
    assert fused_update(O.SGD(ps, lr=0.1, differentiable=True)) is None
    assert fused_update(O.Adam(ps, lr=torch.tensor(1e-3))) is None
    # a scheduler changing lr changes the spec (the captured graph's key)
    opt = O.SGD(ps, lr=0.1, momentum=0.9)
    a = fused_update(opt)
    opt.param_groups[0]["lr"] = 0.05
    assert fused_update(opt) != a


def test_grad_free_parameters_are_conv_expand_of_conv_blocks():
    import models
    cfg = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
    m = models.SoftIntroVAE(arch="conv", **cfg)
    free = {id(p) for p in models.grad_free_parameters(m)}
    names = sorted(k for k, p in m.named_parameters() if id(p) in free)
    assert names and all(k.endswith("conv_expand.weight") for k in names)
    assert len(names) == len([k for k in m.state_dict() if "conv_expand" in k])
    assert not models.grad_free_parameters(models.SoftIntroVAE(arch="res", **cfg))
