"""Host side of the live-range backward (SharedPass.live, IntroSolver.skip_dead_half): defaults, what blocks it, and the
graph key.  No GPU."""
import torch


class _DS:
    def __len__(self):
        return 100


def _solver():
    import models
    from solvers.intro_tc import IntroTCSovler
    model = models.SoftIntroVAE(arch="conv", cdim=3, zdim=8, channels=(16, 32), image_size=16)
    return IntroTCSovler(_DS(), model, 4, torch.optim.Adam(model.encoder.parameters()),
                         torch.optim.Adam(model.decoder.parameters()), "mse", 0.5, 0.75, 512.0, 1e-8, torch.device("cpu"),
                         False, None)


def test_switch_defaults_and_graph_key():
    from solvers.vae import VAESolver
    s = _solver()
    assert s.skip_dead_half is True and s._shared_pass.live is None and s._shared_pass.live_blockers == []
    assert s._schedule_key() == (True, True)                  # what tests/test_shared_pass_host.py pins stays
    assert s._graph_key_extra() == (True,)
    s.skip_dead_half = False
    assert s._graph_key_extra() == (False,) and s._schedule_key() == (True, True)
    assert VAESolver._graph_key_extra(s) == ()


def test_live_images_conditions():
    from hipvae import functional as HF

    class Ctx:
        pass

    sp, ctx = HF.SharedPass(), Ctx()
    ctx.shared = sp
    assert HF._live_images(ctx, 8) is None                    # off by default
    sp.live = (1, 2)
    assert HF._live_images(ctx, 8) is None                    # a backward that takes parameter gradients walks everything
    sp.param_grads = False
    assert HF._live_images(ctx, 8) == (4, 4)
    sp.live_blockers.append("residual add")                   # one function without a sub-range form: the whole pass
    assert HF._live_images(ctx, 8) is None
    with sp.record():
        pass
    assert sp.live is None and sp.live_blockers == [] and sp.param_grads
    ctx.shared = None
    assert HF._live_images(ctx, 8) is None


def test_blockers_are_recorded_once_per_reason():
    from hipvae import functional as HF
    sp = HF.SharedPass()
    with sp.record():
        HF._block_live("residual add")
        HF._block_live("residual add")
    assert sp.live_blockers == ["residual add"]
    HF._block_live("outside a recorded pass")                 # no pass is being recorded: nothing to note
    assert sp.live_blockers == ["residual add"]


def test_abi_has_the_sub_range_entries():
    from hipvae import abi
    assert abi.lib.itcv_abi_version() == abi.ABI_VERSION == 4
    assert hasattr(abi.lib, "itcv_bn_train_bwd_live") and hasattr(abi.lib, "itcv_conv2d_fwd_bf16p_sub")
