"""The kernels a training step runs around the convolutions against the fp64 restatement tests/tail_ref.py, on every
path their host dispatch can take: the loss heads, the scalar algebra, the gradient norm / clip pair, the flip and the
fill of csrc/loss_optim.hip, the skinny fp32 GEMMs and the bias gradient of csrc/conv_igemm.hip, the pointwise /
resampling kernels of csrc/norm_act.hip.  Kernel-level inputs through hipvae.functional / ops / hipvae.flat and
abi.call: no model and no solver.  tests/test_tail_ref_host.py shows, without a GPU, that the shapes below get the plans
they are listed for and that each of 14 plausible kernel mistakes moves a checked quantity by more than 100x the bar.

What the shapes launch (tail_ref's tables):
  recon_partial_kernel (B, P): (3, 7) scalar, one slice; (5, 2048) float4, one slice; (4, 2049) scalar, 2 slices of
      1028, the last short; (4, 4100) float4, 3 slices of 1368, the last 1364; (2, 4099) scalar, 3 slices; (1, 6148)
      float4, 4 slices of 1540; (300, 192) second trip of the finish kernel's ``b += 256``; (1100, 12) B > 1024, one
      slice; (8, 12288) 6 full slices.  BCE rows carry 8 planted (recon, target) pairs -- recon 0, 1, 2^-149, 1 - 2^-24
      against target 0, 1, 0.3 -- on the row's ends and on both sides of the first slice boundary; L1 rows exact ties
      there.  A view one float into its storage (P % 4 == 0) takes the scalar path.
  gemm64_kernel / gemm64_reduce (B, K, N): every row of tail_ref.LINEAR_PLANS; bias and ``accumulate`` each through the
      kernel (no split-K) and through the reduce (split-K; for ``accumulate`` that is (200, 70, 40) and (130, 1, 9));
      all four <A_KC, B_KC> instances -- the weight gradient of (3, 1, 5) / (130, 1, 9) is <false, true>, of (5, 7, 1)
      <true, false> (tail_ref.gemm_instances).
  bias_grad_partial: HW = 1 and > 1, one split and several, C = 1 and 257, accumulate on and off.
  sumsq_partial / scale_by_dev: n = 1, 3 (n4 == 0), 4, 1027 (tail by block 0), 2^21 + 3 (sumsq's 1024-block cap: two
      trips; exactly one trip of scale_by_dev's 2048 blocks) and, for scale_by_dev, 4 * 524289 + 2 (its second trip).
  pointwise: 1, 255 and 524288 + 77 elements (one grid pass and 77); pool / upsample at W % 4 == 0 and 2, H = W = 2,
      BC = 1 and at exactly 524288 outputs each way.

Error measure: rel_err = max |got - ref| / max |ref| per array; bars in tail_ref (TOL_*), bit equality where a kernel
does one exact fp32 operation.  The largest rel_err per family measured on the MI355X is in DESIGN.md.
"""
import pytest
import torch

import tail_ref as R

pytestmark = pytest.mark.gpu

REDUCTION = {"none": 0, "sum": 1, "mean": 2}
ERRORS = {}          # (family, quantity) -> (largest rel_err seen in this run, case)


@pytest.fixture(scope="module")
def HF():
    from hipvae import functional
    yield functional
    print("\nlargest rel_err per family and quantity:")
    for (fam, q), (e, sid) in sorted(ERRORS.items()):
        print(f"  TAIL_ERR {fam:8s} {q:14s} {e:.3e}  {sid}")


def dev():
    return torch.device("cuda:0")


def record(fam, q, sid, e):
    if e >= ERRORS.get((fam, q), (-1.0, ""))[0]:
        ERRORS[(fam, q)] = (e, str(sid))


def check(fam, q, sid, got, ref, tol):
    """rel_err(got, ref) < tol, recorded; nothing of the result may be NaN or infinite."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (q, sid, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), (q, sid)
    e = float((got - ref).abs().max() / (ref.abs().max() + 1e-30)) if ref.numel() else 0.0
    record(fam, q, sid, e)
    assert e < tol, (q, sid, e)


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def dleaf(t):
    return t.detach().float().to(dev()).requires_grad_(True)


# ---- reconstruction losses -------------------------------------------------------------------------------------------
def check_recon_grad(q, sid, got, ref, planted, loss):
    """The unplanted elements on their own scale; a planted element on its own magnitude or on the scale of the
    unplanted ones, whichever is larger -- a gradient of 1e12 hides neither the rest nor its planted neighbours."""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), (q, sid)
    un = ~planted
    check("recon", q, sid, got[un], ref[un], R.TOL_LOSS)
    if loss == "l1":
        assert float(got[planted].abs().max()) == 0.0, (q, sid)          # the subgradient at a tie
    elif loss == "bce":
        scale = torch.clamp(ref[planted].abs(), min=float(ref[un].abs().max()))
        e = float(((got[planted] - ref[planted]).abs() / scale).max())
        record("recon", q + "_plant", sid, e)
        assert e < R.TOL_LOSS, (q, sid, e)


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("B, P", R.RECON_SHAPES)
def test_reconstruction(HF, B, P, loss):
    import ops
    from hipvae.abi import LOSS_TYPES, lib
    assert lib.itcv_recon_workspace(B, P) == B * R.RECON_PLANS[(B, P)][0] * 8
    sid = f"{loss}-{B}x{P}"
    x, r, planted = R.recon_inputs(B, P, loss)
    x64, r64 = x.double(), r.double()
    w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    xd, wd = x.to(dev()), w.float().to(dev())
    rg = dleaf(r)
    rows = HF.ReconRowsFn.apply(xd, rg, LOSS_TYPES[loss])
    check("recon", "rows", sid, rows, R.recon_rows(x64, r64, loss), R.TOL_LOSS)
    got, = torch.autograd.grad((wd * rows).sum(), rg)
    check_recon_grad("rows_d", sid, got, R.recon_loss_grad(x64, r64, w, loss, "none"), planted, loss)
    for red in R.REDUCTIONS:
        for scale in (1.0, 0.25):
            out = ops.reconstruction_loss(xd, rg, loss, red, scale=scale)
            check("recon", "loss_" + red, sid, out, R.recon_loss(x64, r64, loss, red, scale), R.TOL_LOSS)
            g = w if red == "none" else torch.tensor(1.7, dtype=torch.float64)
            got, = torch.autograd.grad((g.float().to(dev()) * out).sum(), rg)
            check_recon_grad("loss_d_" + red, sid, got, R.recon_loss_grad(x64, r64, g, loss, red, scale), planted, loss)
            direct = HF.ReconLossFn.apply(xd, rg, LOSS_TYPES[loss], REDUCTION[red], scale)
            assert torch.equal(direct, out)


@pytest.mark.parametrize("which", ["x", "recon", "both"])
@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("B, P", [(5, 2048), (4, 4100)])
def test_reconstruction_misaligned_rows(HF, B, P, loss, which):
    """P % 4 == 0 and an operand that starts one float into its storage: no float4 read of it, the same values."""
    import ops
    from hipvae.abi import LOSS_TYPES
    sid = f"{loss}-{B}x{P}-{which}"
    x, r, _ = R.recon_inputs(B, P, loss)

    def shifted(t):
        base = torch.zeros(B * P + 4, device=dev())
        v = base[1:1 + B * P].view(B, P)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    xa, ra = x.to(dev()), r.to(dev())
    assert xa.data_ptr() % 16 == 0 and ra.data_ptr() % 16 == 0
    xm = shifted(x) if which in ("x", "both") else xa
    rm = (shifted(r) if which in ("recon", "both") else ra).detach().requires_grad_(True)
    ra = ra.requires_grad_(True)
    w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    ref = R.recon_rows(x.double(), r.double(), loss)
    rows_a, rows_m = (HF.ReconRowsFn.apply(a, b, LOSS_TYPES[loss]) for a, b in ((xa, ra), (xm, rm)))
    check("recon", "unaligned", sid, rows_m, ref, R.TOL_LOSS)
    check("recon", "unaligned_eq", sid, rows_m, rows_a.detach().double().cpu(), R.TOL_LOSS)
    ga, = torch.autograd.grad((w.float().to(dev()) * rows_a).sum(), ra)
    gm, = torch.autograd.grad((w.float().to(dev()) * rows_m).sum(), rm)
    assert bits_equal(ga, gm)                                   # the backward kernel is scalar either way
    for red in R.REDUCTIONS:
        out_a, out_m = (ops.reconstruction_loss(a, b, loss, red, scale=0.25) for a, b in ((xa, ra), (xm, rm)))
        check("recon", "unaligned", sid, out_m, R.recon_loss(x.double(), r.double(), loss, red, 0.25), R.TOL_LOSS)
        check("recon", "unaligned_eq", sid, out_m, out_a.detach().double().cpu(), R.TOL_LOSS)


# ---- nn.Linear -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B, K, N", R.LINEAR_SHAPES)
def test_linear_fn(HF, B, K, N, bias):
    from hipvae.abi import lib
    assert lib.itcv_linear_workspace(B, K, N) == R.linear_workspace(B, K, N)
    sid = f"{B}x{K}x{N}"
    x, w, b, dy, into, into_b = R.linear_inputs(B, K, N)
    x64, w64, b64, dy64 = x.double(), w.double(), b.double() if bias else None, dy.double()
    xd, wd, dyd = dleaf(x), dleaf(w), dy.to(dev())
    bd = dleaf(b) if bias else None
    y = HF.LinearFn.apply(xd, wd, bd)
    check("linear", "y", sid, y, R.linear_fwd(x64, w64, b64), R.TOL_LINEAR)
    got = torch.autograd.grad(y, (xd, wd) + ((bd,) if bias else ()), dyd)
    check("linear", "dx", sid, got[0], R.linear_dgrad(dy64, w64), R.TOL_LINEAR)
    check("linear", "dw", sid, got[1], R.linear_wgrad(dy64, x64), R.TOL_LINEAR)
    if bias:
        check("linear", "db", sid, got[2], R.bias_grad(dy64), R.TOL_LINEAR)
    # accumulated into non-zero targets: the kernels add into .grad and hand autograd nothing
    wd.grad = into.to(dev())
    if bias:
        bd.grad = into_b.to(dev())
    held = wd.grad.data_ptr()
    with HF.direct_grad_accumulation():
        HF.LinearFn.apply(xd, wd, bd).backward(dyd)
    assert wd.grad.data_ptr() == held
    check("linear", "dw_acc", sid, wd.grad, R.linear_wgrad(dy64, x64, into.double()), R.TOL_LINEAR)
    if bias:
        check("linear", "db_acc", sid, bd.grad, R.bias_grad(dy64, into_b.double()), R.TOL_LINEAR)
    check("linear", "dx", sid, xd.grad, R.linear_dgrad(dy64, w64), R.TOL_LINEAR)


@pytest.mark.parametrize("B, K, N", R.LINEAR_SHAPES)
def test_linear_raw_entry_points(HF, B, K, N):
    from hipvae.abi import call, lib, ptr, stream
    sid = f"{B}x{K}x{N}"
    nws = lib.itcv_linear_workspace(B, K, N)
    assert nws == max(R.gemm_workspace(*g) for g in R.linear_gemms(B, K, N).values())
    d = dev()
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=d)
    x, w, b, dy, into, _ = R.linear_inputs(B, K, N)
    x64, w64, b64, dy64 = x.double(), w.double(), b.double(), dy.double()
    xd, wd, bd, dyd = (t.to(d) for t in (x, w, b, dy))
    for bias in (bd, None):
        y = torch.full((B, N), float("nan"), device=d)
        call("itcv_linear_fwd", ptr(xd), ptr(wd), ptr(bias), ptr(y), B, K, N, ptr(ws), nws, stream())
        check("linear", "raw_y", sid, y, R.linear_fwd(x64, w64, b64 if bias is not None else None), R.TOL_LINEAR)
    dx = torch.full((B, K), float("nan"), device=d)
    call("itcv_linear_dgrad", ptr(dyd), ptr(wd), ptr(dx), B, K, N, ptr(ws), nws, stream())
    check("linear", "raw_dx", sid, dx, R.linear_dgrad(dy64, w64), R.TOL_LINEAR)
    for acc in (0, 1):
        dw = into.to(d) if acc else torch.full((N, K), float("nan"), device=d)
        call("itcv_linear_wgrad", ptr(dyd), ptr(xd), ptr(dw), B, K, N, acc, ptr(ws), nws, stream())
        check("linear", "raw_dw_acc" if acc else "raw_dw", sid, dw,
              R.linear_wgrad(dy64, x64, into.double() if acc else None), R.TOL_LINEAR)


@pytest.mark.parametrize("B, C, HW", list(R.BIAS_SHAPES))
def test_bias_grad(HF, B, C, HW):
    from hipvae.abi import lib
    assert lib.itcv_bias_grad_workspace(B, C, HW) == R.BIAS_SHAPES[(B, C, HW)] * C * 8
    sid = f"{B}x{C}x{HW}"
    g = torch.Generator().manual_seed(B + C + HW)
    dy, into = torch.randn(B, C, HW, generator=g), torch.randn(C, generator=g) * HW ** 0.5
    db = HF.bias_grad_raw(dy.to(dev()), B, C, HW)
    check("linear", "bias_grad", sid, db, R.bias_grad(dy.double()), R.TOL_LINEAR)
    tgt = into.to(dev())
    assert HF.bias_grad_raw(dy.to(dev()), B, C, HW, tgt) is None
    check("linear", "bias_grad_acc", sid, tgt, R.bias_grad(dy.double(), into.double()), R.TOL_LINEAR)


# ---- gradient norm and clip ------------------------------------------------------------------------------------------
def guarded(t, pad=4):
    """``t`` on the device with ``pad`` sentinels behind it: (the view of t's elements, the sentinels)."""
    buf = torch.full((t.numel() + pad,), 7.0, device=dev())
    buf[:t.numel()].copy_(t.reshape(-1))
    return buf[:t.numel()], buf[t.numel():]


@pytest.mark.parametrize("recipe", ["span", "tail"])
@pytest.mark.parametrize("n", R.SUMSQ_SIZES)
def test_sumsq(HF, n, recipe):
    from hipvae.abi import call, lib, ptr, stream
    v = R.sumsq_input(n, recipe)
    if recipe == "span" and n >= 2:
        assert float(v.abs().max()) >= 9.99e11 and float(v.abs().min()) <= 1.001e-12
    vd, _ = guarded(v)
    nws = lib.itcv_sumsq_workspace(n)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev())
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev())
    call("itcv_sumsq", ptr(vd), n, ptr(out), ptr(ws), nws, stream())
    check("norm", "sumsq_" + recipe, n, out[0], R.sumsq(v), R.TOL_SUMSQ)
    check("norm", "norm_" + recipe, n, out[0].sqrt(), R.sumsq(v).sqrt(), R.TOL_NORM)


@pytest.mark.parametrize("n", R.SCALE_SIZES)
def test_scale_by_device_coefficient(HF, n):
    """Every element, the n % 4 tail included, is multiplied exactly once; nothing behind the range is touched."""
    from hipvae.abi import call, ptr, stream
    v = R.sumsq_input(n, "span")
    vd, sentinels = guarded(v)
    coef = torch.tensor([0.37], device=dev())
    call("itcv_scale_by_dev", ptr(vd), n, ptr(coef), stream())
    assert bits_equal(vd, v * torch.tensor(0.37))
    assert bool((sentinels == 7.0).all())


@pytest.mark.parametrize("nparts", [1, 3])
def test_clip_coefficient_on_both_sides(HF, nparts):
    from hipvae.abi import call, ptr, stream
    parts = [3.0, 1e-12, 2.5e7][:nparts]
    norm = sum(parts) ** 0.5
    sq = torch.tensor(parts, dtype=torch.float64, device=dev())
    for side, clip in (("below", norm * (1 + 1e-4)), ("above", norm * (1 - 1e-4))):
        out = torch.full((2,), float("nan"), device=dev())
        call("itcv_clip_coef", ptr(sq), nparts, float(clip), ptr(out[0:1]), ptr(out[1:2]), stream())
        check("norm", "clip_norm", f"{nparts}-{side}", out[0], torch.tensor(norm, dtype=torch.float64), R.TOL_NORM)
        if side == "below":
            assert float(out[1]) == 1.0
        else:
            assert float(out[1]) < 1.0
            check("norm", "clip_coef", f"{nparts}-{side}", out[1], torch.tensor(R.clip_coef(norm, clip), dtype=torch.float64), R.TOL_NORM)


GROUP_SHAPES = [[(7, 3, 3, 3), (13,), (5, 11), (1,)], [(1027,)], [(3,), (2, 2, 2), (258, 5)]]


@pytest.mark.parametrize("ngroups", [1, 3])
def test_clip_grad_norm_over_flat_groups(HF, ngroups):
    """norm just below the clip value: coefficient exactly 1, gradients bit-unchanged; just above: every element is the
    fp32 product of its value and the coefficient -- scaled exactly once -- and the padding between tensors stays 0."""
    from hipvae.abi import call, ptr, stream
    from hipvae.flat import FlatGroup, clip_grad_norm
    g = torch.Generator().manual_seed(6 + ngroups)
    groups, grads = [], []
    for shapes in GROUP_SHAPES[:ngroups]:
        ps = [torch.nn.Parameter(torch.randn(*s, generator=g).to(dev())) for s in shapes]
        groups.append(FlatGroup(ps))
        grads.append([torch.randn(*s, generator=g) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=g)) for s in shapes])
    norm = R.total_norm([t for gs in grads for t in gs])
    for side, clip in (("below", norm * (1 + 1e-4)), ("above", norm * (1 - 1e-4))):
        for grp, gs in zip(groups, grads):
            grp.zero_grad()
            for p, t in zip(grp.params, gs):
                p.grad.copy_(t.to(dev()))
        # the coefficient clip_grad_norm will apply, from the same two kernels on the same buffers
        sq = torch.empty(ngroups, dtype=torch.float64, device=dev())
        for i, grp in enumerate(groups):
            grp.sumsq_into(sq[i:i + 1])
        nc = torch.full((2,), float("nan"), device=dev())
        call("itcv_clip_coef", ptr(sq), ngroups, float(clip), ptr(nc[0:1]), ptr(nc[1:2]), stream())
        coef = nc[1].cpu()
        n = clip_grad_norm(groups, clip)
        assert bits_equal(n, nc[0:1])
        check("norm", "flat_norm", f"{ngroups}-{side}", n[0], torch.tensor(norm, dtype=torch.float64), R.TOL_NORM)
        if side == "below":
            assert float(coef) == 1.0
        else:
            check("norm", "flat_coef", f"{ngroups}-{side}", coef, torch.tensor(R.clip_coef(norm, clip), dtype=torch.float64),
                  R.TOL_NORM)
            assert float(coef) < 1.0
        for grp, gs in zip(groups, grads):
            for p, t in zip(grp.params, gs):
                assert bits_equal(p.grad, t if side == "below" else t * coef), (side, tuple(t.shape))
            assert float(grp.flat_g.double().pow(2).sum()) == pytest.approx(
                float(sum((t.double() * (1.0 if side == "below" else float(coef))).pow(2).sum() for t in gs)), rel=1e-6)


# ---- scalar heads ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.ELBO_COEFS)
@pytest.mark.parametrize("B", R.ELBO_SIZES)
def test_exp_elbo(HF, B, c):
    g = torch.Generator().manual_seed(1 + B)
    a, b = 30.0 * torch.rand(B, generator=g), 5.0 * torch.rand(B, generator=g)
    ag, bg = dleaf(a), dleaf(b)
    out = HF.ExpElboFn.apply(ag, bg, c)
    sid = f"{B}-{c:.2g}"
    check("heads", "elbo", sid, out, R.exp_elbo(a.double(), b.double(), c), R.TOL_SCALAR)
    da, db = torch.autograd.grad(3.0 * out, (ag, bg))
    want = R.exp_elbo_grad(a.double(), b.double(), c, 3.0)
    check("heads", "elbo_d", sid, da, want, R.TOL_LOSS)
    assert bits_equal(da, db)


@pytest.mark.parametrize("n", [1, 8])
def test_lincomb(HF, n):
    g = torch.Generator().manual_seed(20 + n)
    terms = [torch.randn((), generator=g) for _ in range(n)]
    wts = [0.5, -1.25, 3.0, 1.0 / 12288, 0.0, 2.0, -7.0, 1e-3][:n]
    tg = [dleaf(t) for t in terms]
    out = HF.LinCombFn.apply(wts, *tg)
    check("heads", "lincomb", n, out, R.lincomb(wts, [t.double() for t in terms]), R.TOL_SCALAR)
    grads = torch.autograd.grad(2.0 * out, tg)
    want = torch.tensor([2.0 * wk for wk in wts], dtype=torch.float64)
    check("heads", "lincomb_d", n, torch.stack(grads), want, R.TOL_SCALAR)


def test_lincomb_refuses_nine_terms(HF):
    terms = [torch.ones((), device=dev()) for _ in range(9)]
    with pytest.raises(HF.abi.HipExtensionError):
        HF.LinCombFn.apply([1.0] * 9, *terms)
    assert "itcv_lincomb_fwd" in HF.abi.last_error()


# ---- pointwise / resampling ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.POINT_SIZES)
def test_pointwise(HF, n):
    from hipvae.abi import call, ptr, stream
    g = torch.Generator().manual_seed(n)
    x, dy, other = (torch.randn(n, generator=g) * 4 for _ in range(3))
    special = torch.tensor([0.0, -0.0, 30.0, -30.0, 100.0, -100.0])
    if n >= special.numel():
        x[:6] = special
        x[-6:] = special.flip(0)
    else:
        x[0] = 0.0
    xg = dleaf(x)
    y = HF.LeakyReluFn.apply(xg, 0.2)
    assert bits_equal(y, torch.nn.functional.leaky_relu(x, 0.2))
    dx, = torch.autograd.grad(y, xg, dy.to(dev()))
    assert bits_equal(dx, torch.where(x > 0, dy, dy * 0.2))
    y = HF.SigmoidFn.apply(xg)
    check("point", "sigmoid", n, y, R.sigmoid(x.double()), R.TOL_POINT)
    dx, = torch.autograd.grad(y, xg, dy.to(dev()))
    check("point", "sigmoid_d", n, dx, R.sigmoid_grad(x.double(), dy.double()), R.TOL_POINT)
    sat = ((y == 0) | (y == 1)).cpu()
    if n >= special.numel():
        assert int(sat.sum()) >= 6                               # +-100 and 30 saturate in fp32
    assert float(dx.cpu()[sat].abs().max() if bool(sat.any()) else 0.0) == 0.0
    assert bits_equal(HF.AddFn.apply(xg.detach(), other.to(dev())), x + other)
    for value in (0.1, -0.0):
        buf, sentinels = guarded(x)
        call("itcv_fill", ptr(buf), n, value, stream())
        assert bits_equal(buf, torch.full((n,), value)) and bool((sentinels == 7.0).all())


#              shape, runs the pool, runs the upsample
RESAMPLE_SHAPES = [((3, 5, 8, 12), True, True),          # W % 4 == 0
                   ((2, 3, 4, 6), True, True),           # W % 4 == 2
                   ((2, 3, 2, 2), True, True),           # one window per plane
                   ((1, 1, 6, 10), True, True),          # BC = 1
                   ((8, 16, 128, 128), True, False),     # pool forward: exactly 524288 outputs
                   ((8, 16, 64, 64), True, True),        # pool backward and upsample backward: exactly 524288 outputs
                   ((8, 16, 32, 32), False, True)]       # upsample forward: exactly 524288 outputs


@pytest.mark.parametrize("shape, pool, up", RESAMPLE_SHAPES, ids=[str(s[0]) for s in RESAMPLE_SHAPES])
def test_resampling(HF, shape, pool, up):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g)
    sid = "x".join(str(s) for s in shape)
    if pool:
        xg = dleaf(x)
        y = HF.AvgPool2Fn.apply(xg)
        check("point", "pool", sid, y, R.avgpool2(x.double()), R.TOL_POINT)
        dy = torch.randn(*y.shape, generator=g)
        dx, = torch.autograd.grad(y, xg, dy.to(dev()))
        check("point", "pool_d", sid, dx, R.avgpool2_adjoint(dy.double()), R.TOL_POINT)
    if up:
        xg = dleaf(x)
        y = HF.Upsample2Fn.apply(xg)
        assert bits_equal(y, R.upsample2(x))
        dy = torch.randn(*y.shape, generator=g)
        dx, = torch.autograd.grad(y, xg, dy.to(dev()))
        check("point", "up_d", sid, dx, R.upsample2_adjoint(dy.double()), R.TOL_POINT)


@pytest.mark.parametrize("H, W", [(3, 4), (4, 3), (1, 1)])
def test_avgpool_refuses_odd_sizes(HF, H, W):
    with pytest.raises(HF.abi.HipExtensionError):
        HF.AvgPool2Fn.apply(torch.zeros(2, 2, H, W, device=dev()))


@pytest.mark.parametrize("B, rows, W", R.FLIP_SHAPES)
def test_hflip(HF, B, rows, W):
    from hipvae.abi import call, ptr, stream
    x, flip = R.flip_input(B, rows, W)
    xd, fd = x.to(dev()), flip.to(dev())
    y, sentinels = guarded(torch.full((B * rows * W,), float("nan")))
    call("itcv_hflip", ptr(xd), ptr(y), fd.data_ptr(), B, rows, W, stream())
    assert bits_equal(y.view(B, rows, W), R.hflip(x, flip)) and bool((sentinels == 7.0).all())
    assert bits_equal(xd, x)
