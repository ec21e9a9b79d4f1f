"""CPU-only checks around the SSIM loss (csrc/ssim.hip): the numpy restatement tests/ssim_ref.py is pinned against an
independent torch fp64 statement (grouped conv2d + autograd) and against known answers; every input of the GPU tests
keeps the kernels' a-priori bound (derived in tests/ssim_ref.py) under 1e-9 P per row and under 1e-9 of the gradient's
max-norm, so that tests/test_hip_ssim.py cannot be passed by an fp32 implementation (about 4e-6 P); the C entry points
refuse what they do not support before any launch; and the Python surface routes and refuses as documented."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops
import ssim_ref as R
from hipvae import abi
from hipvae import functional as HF

F64 = torch.float64
HOST_SHAPES = ((2, 3, 12, 17, 11), (1, 2, 27, 26, 11), (2, 2, 9, 20, 3), (1, 1, 40, 40, 15))


def torch_maps(x, y, K, sigma):
    """(S, cs) [B, C, H', W'] from five grouped convolutions in fp64: the independent statement."""
    C = x.shape[1]
    g = torch.tensor(R.window(K, sigma), dtype=F64)
    w = (g[:, None] * g[None, :]).expand(C, 1, K, K).contiguous()
    f = lambda t: F.conv2d(t, w, groups=C)                                          # noqa: E731
    mx, my = f(x), f(y)
    sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    cs = (2 * sxy + R.C2) / (sx + sy + R.C2)
    return (2 * mx * my + R.C1) / (mx * mx + my * my + R.C1) * cs, cs


def torch_loss(x, y, alpha, reduction, scale, K, sigma=1.5):
    P = x[0].numel()
    S, _ = torch_maps(x, y, K, sigma)
    rows = P * alpha * (1 - S.flatten(1).mean(1)) + (1 - alpha) * (y - x).abs().flatten(1).sum(1)
    s = float(np.float32(scale))
    return s * rows if reduction == "none" else s * (rows.mean() if reduction == "mean" else rows.sum())


def normwise(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("shape", HOST_SHAPES)
@pytest.mark.parametrize("alpha", (1.0, 0.84))
def test_restatement_equals_torch_fp64(shape, alpha):
    B, C, H, W, K = shape
    P = C * H * W
    for kind in ("uniform", "smooth", "binary", "constant"):
        x, y = R.make_pair(kind, (B, C, H, W))
        for reduction, scale in (("none", 1.0), ("sum", 0.75 / P), ("mean", 1.0)):
            gup = R.upstream(B, reduction)
            tx = torch.tensor(x, dtype=F64)
            ty = torch.tensor(y, dtype=F64, requires_grad=True)
            out = torch_loss(tx, ty, alpha, reduction, scale, K)
            out.backward(torch.tensor(gup, dtype=F64).reshape(out.shape))
            assert normwise(R.loss(x, y, alpha, reduction, scale, K), out.detach().numpy()) <= 1e-12
            assert normwise(R.grad(x, y, gup, alpha, reduction, scale, K), ty.grad.numpy()) <= 1e-12


def test_stats_and_ms_ssim_equal_torch_fp64():
    for shape, K, levels in (((2, 3, 32, 32), 11, 2), ((1, 1, 176, 176), 11, 5), ((2, 2, 9, 20), 3, 1)):
        x, y = R.make_pair("smooth", shape, bits=16)
        assert R.levels_of(shape[2], shape[3], K) == (levels if K == 11 else 2)
        tx, ty = torch.tensor(x), torch.tensor(y)
        S, cs = torch_maps(tx.double(), ty.double(), K, 1.5)
        st = torch.stack([S.flatten(2).mean(2), cs.flatten(2).mean(2)], 2)
        assert normwise(R.stats(x, y, K), st.numpy()) <= 1e-12
        w = torch.tensor(R.MS_WEIGHTS[:levels], dtype=F64)
        w = w / w.sum()
        ms = 1.0
        for lev in range(levels):
            if lev:
                tx, ty = F.avg_pool2d(tx, 2), F.avg_pool2d(ty, 2)
            S, cs = torch_maps(tx.double(), ty.double(), K, 1.5)
            ms = ms * (S if lev == levels - 1 else cs).flatten(2).mean(2).clamp_min(0) ** w[lev]
        got = R.quality(x, y, K, levels=levels)
        assert normwise(got["ms_ssim"], ms.mean(1).numpy()) <= 1e-12
        d = torch.tensor(y).double() - torch.tensor(x).double()
        assert normwise(got["mse"], (d * d).flatten(1).mean(1).numpy()) <= 1e-12
        assert normwise(got["psnr"], (10 * torch.log10(1 / (d * d).flatten(1).mean(1))).numpy()) <= 1e-12
        assert np.array_equal(R.halve(x), F.avg_pool2d(torch.tensor(x), 2).numpy())


def test_known_answers():
    for shape in ((2, 3, 12, 17, 11), (2, 2, 9, 20, 3), (1, 1, 40, 40, 15)):
        B, C, H, W, K = shape
        x, y = R.make_pair("same", (B, C, H, W))
        for alpha in R.ALPHAS:
            assert np.all(R.rows(x, y, alpha, K) == 0.0)
        assert np.all(R.stats(x, y, K) == 1.0)
        q = R.quality(x, y, K)
        assert np.all(q["ssim"] == 1.0) and np.all(q["ms_ssim"] == 1.0) and np.all(np.isinf(q["psnr"]))
        a, b = 0.25, 0.625
        xa, yb = np.full((B, C, H, W), a, dtype=np.float32), np.full((B, C, H, W), b, dtype=np.float32)
        want = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
        assert np.abs(R.stats(xa, yb, K)[:, :, 0] - want).max() <= 1e-12
        P = C * H * W
        assert np.abs(R.rows(xa, yb, 1.0, K) / P - (1 - want)).max() <= 1e-12
    for K in (3, 11, 15):
        g = R.window(K)
        assert np.array_equal(g, g[::-1]) and abs(g.sum() - 1.0) <= K * 2.0 ** -53
        assert HF.ssim_window_host(K, 1.5) == g.tolist()                  # the kernels are handed the restatement's bits


@pytest.mark.parametrize("shape", R.SHAPES)
def test_gpu_inputs_keep_the_bound_sharp(shape):
    """ssim_bound <= 1e-9 P per row and the gradient bound <= 1e-9 max |dy| for every input of tests/test_hip_ssim.py.  At
    y = x the gradient is exactly zero (SSIM is at its maximum, sign(0) = 0) and has no max-norm to hold a bound against:
    there the bound is held against the upstream gradient's own size, |g| scale [/ B], the gradient of a row that moved
    by as much as its images did."""
    B, C, H, W, K = shape
    P = C * H * W
    for kind in R.KINDS:
        x, y = R.make_pair(kind, (B, C, H, W))
        for alpha in R.ALPHAS:
            assert (R.ssim_bound(x, y, alpha, K=K, rows_only=True) / P).max() <= 1e-9, (kind, alpha)
            for reduction, scale in (("none", 1.0), ("sum", 0.75 / P), ("mean", 1.0)):
                gup = R.upstream(B, reduction)
                gb = R.grad_bound(x, y, gup, alpha, reduction, scale, K)
                norm = np.abs(R.grad(x, y, gup, alpha, reduction, scale, K)).max()
                if kind == "same":
                    assert norm <= gb.max()                   # the restatement gives rounding noise for the exact 0
                    norm = np.abs(gup).max() * float(np.float32(scale)) / (B if reduction == "mean" else 1)
                assert gb.max() <= 1e-9 * norm, (kind, alpha, reduction, gb.max() / norm)
    sb = R.stats_bound(*R.make_pair("uniform", (B, C, H, W)), K)
    assert sb.max() <= 1e-9


def test_an_fp32_evaluation_misses_the_bound():
    """The same map in fp32 (grouped conv2d) is off by far more than the bound allows: the GPU test is sharp."""
    B, C, H, W, K = 2, 3, 32, 32, 11
    x, y = R.make_pair("uniform", (B, C, H, W))
    P = C * H * W
    g = torch.tensor(R.window(K), dtype=torch.float32)
    w = (g[:, None] * g[None, :]).expand(C, 1, K, K).contiguous()
    tx, ty = torch.tensor(x), torch.tensor(y)
    f = lambda t: F.conv2d(t, w, groups=C)                                          # noqa: E731
    mx, my = f(tx), f(ty)
    sx, sy, sxy = f(tx * tx) - mx * mx, f(ty * ty) - my * my, f(tx * ty) - mx * my
    S = (2 * mx * my + R.C1) * (2 * sxy + R.C2) / ((mx * mx + my * my + R.C1) * (sx + sy + R.C2))
    per_position = np.abs(S.double().numpy() - R.maps(x, y, K)["S"]).max()
    assert per_position > 1e-7
    assert np.all(R.ssim_bound(x, y, 1.0, K=K, rows_only=True) < 1e-3 * P * per_position)
    # the mean over a plane averages some of it away, and still misses the statistics' bound by orders of magnitude
    miss = np.abs(S.double().flatten(2).mean(2).numpy() - R.stats(x, y, K)[:, :, 0])
    assert np.all(miss > 100.0 * R.stats_bound(x, y, K)[:, :, 0])


# ---- the C entry points refuse on the host --------------------------------------------------------------------------------
def _fwd(B=1, C=1, H=16, W=16, K=11, alpha=1.0, reduction=1, null=False):
    one = ctypes.c_void_p(16)              # never dereferenced: every refusal comes before a launch
    return abi.lib.itcv_ssim_loss_fwd(None if null else one, one, one, one, B, C, H, W, K, alpha, reduction, 1.0, one, 0, None)


@pytest.mark.parametrize("kw, named", [
    (dict(K=10), "K = 10"), (dict(K=17, H=32, W=32), "K = 17"), (dict(H=10), "H = 10"), (dict(W=9), "W = 9"),
    (dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(null=True), "pointer is NULL"),
    (dict(B=1 << 11, C=1 << 10), "B * C = 2097152"), (dict(reduction=3), "reduction = 3"), (dict(B=0), "B = 0"),
    (dict(H=4097), "H = 4097"),
])
def test_c_entries_refuse_before_any_launch(kw, named):
    assert _fwd(**kw) != 0
    msg = abi.last_error()
    assert msg.startswith("itcv_ssim_loss_fwd:") and named in msg, msg


def test_backward_and_stats_refuse_too():
    one = ctypes.c_void_p(16)
    assert abi.lib.itcv_ssim_loss_bwd(one, one, one, one, one, 1, 1, 16, 16, 12, 1.0, 1, 1.0, None) != 0
    assert "itcv_ssim_loss_bwd" in abi.last_error() and "K = 12" in abi.last_error()
    assert abi.lib.itcv_ssim_loss_bwd(one, one, one, None, one, 1, 1, 16, 16, 11, 1.0, 1, 1.0, None) != 0
    assert "pointer is NULL" in abi.last_error()
    assert abi.lib.itcv_ssim_stats(one, one, one, one, 1, 1, 8, 16, 11, one, 0, None) != 0
    assert "itcv_ssim_stats" in abi.last_error() and "H = 8" in abi.last_error()
    assert abi.lib.itcv_ssim_stats(one, one, one, one, 1, 1, 16, 16, 11, one, 0, None) != 0
    assert "workspace" in abi.last_error()


def test_workspace_answers_on_the_host():
    ws = abi.lib.itcv_ssim_workspace
    assert ws(1, 1, 11, 11, 11) == 3 * 8
    assert ws(2, 3, 32, 32, 11) == 3 * 8 * 6 * 2 * 2                      # 22 x 22 positions: 2 x 2 tiles of 16
    assert ws(1, 1, 27, 26, 11) == 3 * 8 * 2
    assert ws(128, 3, 128, 128, 11) == 3 * 8 * 384 * 8 * 8
    for bad in ((1, 1, 16, 16, 10), (1, 1, 32, 32, 17), (1, 1, 10, 16, 11), (0, 1, 16, 16, 11), (1 << 11, 1 << 10, 16, 16, 11),
                (1, 1, 4097, 16, 11), (1, 1, 16, 16, 1)):
        assert ws(*bad) == 0, bad


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def test_routing_reaches_the_kernels():
    x, y = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    for name in ("ssim", "ssim_l1"):
        with pytest.raises(abi.HipExtensionError):                        # NotImplementedError without the feature
            ops.reconstruction_loss(x, y, name)
        with pytest.raises(ValueError):
            ops.reconstruction_loss(x.flatten(1), y.flatten(1), name)
    with pytest.raises(abi.HipExtensionError):
        ops.ssim_loss(x, y)
    with pytest.raises(abi.HipExtensionError):
        HF.ssim_stats(x, y)
    assert ops.SSIM_LOSS_ALPHA == {"ssim": 1.0, "ssim_l1": 0.84}


def test_what_stays_as_it_was():
    x, y = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        ops.reconstruction_loss(x, y, "huber")
    with pytest.raises(NotImplementedError):
        ops.reconstruction_loss(x, y, "ssim", reduction="max")
    assert abi.LOSS_TYPES == {"mse": 0, "l1": 1, "bce": 2}
    assert not [k for k in abi.DEFINES if k.startswith("ITCV_LOSS_") and "SSIM" in k]
    for name in ("ssim", "ssim_l1"):
        with pytest.raises(NotImplementedError):
            ops.iwae_bound(x, y, None, 1.0, 1.0, loss_type=name)
        from hipvae import likelihood
        with pytest.raises(NotImplementedError):
            likelihood.compute_log_likelihood([x[0]], None, num_samples=2, loss_type=name)


@pytest.mark.parametrize("kw", [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(window=10),
                                dict(window=17), dict(window=1), dict(window=13)])
def test_ssim_loss_refuses_bad_arguments(kw):
    x, y = torch.rand(2, 3, 12, 16), torch.rand(2, 3, 12, 16)                       # H = 12 < 13
    with pytest.raises(ValueError):
        ops.ssim_loss(x, y, **kw)


def test_ssim_loss_refuses_bad_shapes():
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(ValueError):
        ops.ssim_loss(x.flatten(1), x.flatten(1))
    with pytest.raises(ValueError):
        ops.ssim_loss(x, x[:, :2])
    with pytest.raises(NotImplementedError):
        ops.ssim_loss(x, x, reduction="max")


def test_levels():
    from hipvae import quality
    for side, want in ((11, 1), (21, 1), (22, 2), (32, 2), (44, 3), (64, 3), (88, 4), (175, 4), (176, 5), (1024, 5)):
        assert quality.ms_ssim_levels(side, side + 3) == want == R.levels_of(side, side + 3)
    assert quality.MS_SSIM_WEIGHTS == R.MS_WEIGHTS
    with pytest.raises(ValueError):
        quality.ms_ssim_levels(10, 64)
    with pytest.raises(ValueError):
        quality.reconstruction_quality(torch.rand(1, 1, 32, 32), torch.rand(1, 1, 32, 32), levels=3)
