"""Host-only checks of the fp64 restatement tests/tail_ref.py, which tests/test_hip_tail.py holds the loss, linear and
pointwise kernels to: (1) it reproduces the recorded reconstruction losses of the original program
(tests/golden/ops.npz, rec_*) to 1e-5 and agrees with torch's fp64 autograd everywhere else; (2) its plan arithmetic is
the library's, through the host-callable workspace queries, on every shape of the case tables, and every shape gets the
plan it is in the table for; (3) each mistake a kernel could plausibly make (tail_ref.DEFECTS) moves a checked quantity
by more than 100x the GPU tolerance on a named case, so a kernel with that mistake cannot pass."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD_TOL = 1e-5
AUTOGRAD_TOL = 1e-12


def T(a):
    return torch.from_numpy(np.asarray(a))


def dbl(*ts):
    return [t.double() for t in ts]


# ---- 1. the restatement against recorded values and torch fp64 -------------------------------------------------------
def test_reconstruction_against_recorded_outputs():
    G = np.load(os.path.join(GOLDEN, "ops.npz"))
    x, r = T(G["rec_x"]).double(), T(G["rec_xr"]).double()
    B = x.shape[0]
    x, r = x.reshape(B, -1), r.reshape(B, -1)
    for loss in R.LOSSES:
        for red in R.REDUCTIONS:
            assert R.rel_err(R.recon_loss(x, r, loss, red), T(G[f"rec_{loss}_{red}"])) < GOLD_TOL, (loss, red)
        w = T(G[f"rec_{loss}_w"]).double()
        d = R.recon_loss_grad(x, r, w, loss, "none")
        assert R.rel_err(d, T(G[f"rec_{loss}_dxr"]).reshape(B, -1)) < GOLD_TOL, loss


TORCH_LOSS = {"mse": F.mse_loss, "l1": F.l1_loss, "bce": F.binary_cross_entropy}


@pytest.mark.parametrize("loss", R.LOSSES)
@pytest.mark.parametrize("B, P", [(3, 7), (4, 2049), (300, 192)])
def test_reconstruction_against_torch_fp64(B, P, loss):
    """ATen's own clamps and subgradient, on the planted inputs: both BCE clamps fire, the L1 ties are exact."""
    x, r, planted = R.recon_inputs(B, P, loss)
    x, r = dbl(x, r)
    if loss == "bce":
        assert bool((torch.log(r[planted]) < -100).any()) and bool((((1 - r) * r)[planted] < 1e-12).any())
    if loss == "l1":
        assert bool((r[planted] == x[planted]).all()) and int(planted.sum()) == B * min(8, P // 2)
    w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    for red in R.REDUCTIONS:
        for scale in (1.0, 0.25):
            rg = r.clone().requires_grad_(True)
            rows = TORCH_LOSS[loss](rg, x, reduction="none").sum(1)
            ref = scale * {"none": rows, "sum": rows.sum(), "mean": rows.mean()}[red]
            g = w if red == "none" else torch.tensor(1.7, dtype=torch.float64)
            (g * ref).sum().backward()
            assert R.rel_err(R.recon_loss(x, r, loss, red, scale), ref) < AUTOGRAD_TOL
            got = R.recon_loss_grad(x, r, g, loss, red, scale)
            assert float((got - rg.grad).abs().max()) <= AUTOGRAD_TOL * float(rg.grad.abs().max())
            if loss == "l1":
                assert float(got[planted].abs().max()) == 0.0


def test_scalar_heads_against_torch_fp64():
    g = torch.Generator().manual_seed(1)
    for B in R.ELBO_SIZES:
        a, b = dbl(30 * torch.rand(B, generator=g), 5 * torch.rand(B, generator=g))
        for c in R.ELBO_COEFS:
            ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            ref = torch.exp(c * (ar + br)).mean()
            (3.0 * ref).backward()
            assert R.rel_err(R.exp_elbo(a, b, c), ref) < AUTOGRAD_TOL
            assert R.rel_err(R.exp_elbo_grad(a, b, c, 3.0), ar.grad) < AUTOGRAD_TOL and torch.equal(ar.grad, br.grad)
    terms = [torch.randn((), generator=g, dtype=torch.float64) for _ in range(8)]
    wts = [0.5, -1.25, 3.0, 1.0 / 12288, 0.0, 2.0, -7.0, 1e-3]
    assert float(R.lincomb(wts, terms)) == pytest.approx(sum(w * float(t) for w, t in zip(wts, terms)), rel=1e-14)


def test_clip_against_torch_fp64():
    g = torch.Generator().manual_seed(2)
    parts = [torch.randn(n, generator=g, dtype=torch.float64) for n in (7, 1027, 13)]
    norm = R.total_norm(parts)
    for clip in (norm * 0.5, norm * 2.0):
        ps = [torch.nn.Parameter(p.clone()) for p in parts]
        for p, v in zip(ps, parts):
            p.grad = v.clone()
        ref = float(torch.nn.utils.clip_grad_norm_(ps, clip))
        assert norm == pytest.approx(ref, rel=1e-14)
        coef = R.clip_coef(norm, clip)
        assert (coef == 1.0) == (clip > norm)
        for p, v in zip(ps, parts):
            assert R.rel_err(R.scale_by(v, coef), p.grad) < AUTOGRAD_TOL


@pytest.mark.parametrize("B, K, N", [(3, 31, 5), (7, 351, 40), (200, 70, 40)])
def test_linear_against_torch_fp64(B, K, N):
    g = torch.Generator().manual_seed(3)
    x, w, b, dy, into = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((B, K), (N, K), (N,), (B, N), (N, K)))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.linear(xr, wr, br)
    y.backward(dy)
    assert R.rel_err(R.linear_fwd(x, w, b), y) < AUTOGRAD_TOL and R.rel_err(R.linear_fwd(x, w), F.linear(x, w)) < AUTOGRAD_TOL
    assert R.rel_err(R.linear_dgrad(dy, w), xr.grad) < AUTOGRAD_TOL
    assert R.rel_err(R.linear_wgrad(dy, x), wr.grad) < AUTOGRAD_TOL
    assert R.rel_err(R.linear_wgrad(dy, x, into), into + wr.grad) < AUTOGRAD_TOL
    assert R.rel_err(R.bias_grad(dy), br.grad) < AUTOGRAD_TOL and R.rel_err(R.bias_grad(dy, b), b + br.grad) < AUTOGRAD_TOL
    d3 = torch.randn(B, N, 5, generator=g, dtype=torch.float64)
    assert R.rel_err(R.bias_grad(d3), d3.sum((0, 2))) < AUTOGRAD_TOL


def test_pointwise_against_torch_fp64():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 4, 6, generator=g, dtype=torch.float64)
    for fn, adj, ref in ((R.avgpool2, R.avgpool2_adjoint, lambda t: F.avg_pool2d(t, 2)),
                         (R.upsample2, R.upsample2_adjoint, lambda t: F.interpolate(t, scale_factor=2, mode="nearest"))):
        xr = x.clone().requires_grad_(True)
        yr = ref(xr)
        dy = torch.randn(*yr.shape, generator=g, dtype=torch.float64)
        yr.backward(dy)
        assert R.rel_err(fn(x), yr) < AUTOGRAD_TOL and R.rel_err(adj(dy), xr.grad) < AUTOGRAD_TOL
    v = torch.cat([torch.randn(50, generator=g, dtype=torch.float64), torch.tensor([0.0, -0.0, 30.0, -30.0])])
    dy = torch.randn(54, generator=g, dtype=torch.float64)
    for fn, grad, ref in ((R.sigmoid, R.sigmoid_grad, torch.sigmoid),
                          (lambda t: R.lrelu(t, 0.2), lambda t, d: R.lrelu_grad(t, d, 0.2), lambda t: F.leaky_relu(t, 0.2))):
        vr = v.clone().requires_grad_(True)
        yr = ref(vr)
        yr.backward(dy)
        assert R.rel_err(fn(v), yr) < AUTOGRAD_TOL and R.rel_err(grad(v, dy), vr.grad) < AUTOGRAD_TOL
    for B, rows, W in R.FLIP_SHAPES[:2]:
        xf, flip = R.flip_input(B, rows, W)
        want = torch.stack([xf[b].flip(-1) if int(flip[b]) else xf[b] for b in range(B)])
        assert torch.equal(R.hflip(xf, flip), want)
        assert len({int(f) for f in flip}) >= min(B, 3)


# ---- 2. plan restatements against the library ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hipvae import abi
    return abi.lib


@pytest.mark.parametrize("B, P", R.RECON_SHAPES)
def test_recon_plan_is_the_librarys(lib, B, P):
    assert lib.itcv_recon_workspace(B, P) == B * R.recon_splits(B, P) * 8
    assert (R.recon_splits(B, P), R.recon_chunk(B, P)) == R.RECON_PLANS[(B, P)]
    # every float4 group of a rounded slice of a P % 4 == 0 row lies inside the row
    splits, chunk = R.RECON_PLANS[(B, P)]
    if P % 4 == 0:
        assert chunk % 4 == 0 and all(min(s * chunk + chunk, P) % 4 == 0 for s in range(splits))


@pytest.mark.parametrize("B, K, N", R.LINEAR_SHAPES)
def test_linear_plans_are_the_librarys(lib, B, K, N):
    gemms = R.linear_gemms(B, K, N)
    need = [R.gemm_plan(*g)[3] * g[0] * g[1] * 4 if R.gemm_plan(*g)[3] > 1 else 0 for g in gemms.values()]
    assert lib.itcv_linear_workspace(B, K, N) == max(need) == R.linear_workspace(B, K, N)
    for name, plan in R.LINEAR_PLANS.get((B, K, N), {}).items():
        assert R.gemm_plan(*gemms[name]) == plan, name
    for g in gemms.values():
        mt, nt, ktiles, splits, kps = R.gemm_plan(*g)
        assert 1 <= splits <= 32 and (splits - 1) * kps < ktiles <= splits * kps     # no empty split, none missing


def test_linear_table_reaches_every_route():
    """Bias and accumulate each go through the kernel (no split-K) and through the reduce (split-K); a short last split,
    the cap, one K-tile with a tail, M = 1, N = 1."""
    plans = {s: {k: R.gemm_plan(*g) for k, g in R.linear_gemms(*s).items()} for s in R.LINEAR_SHAPES}
    fwd = [p["fwd"][3] for p in plans.values()]
    wg = [p["wgrad"][3] for p in plans.values()]
    assert 1 in fwd and max(fwd) == 32 and 1 in wg and max(wg) > 1
    assert any(p["fwd"][3] * p["fwd"][4] > p["fwd"][2] for p in plans.values())
    assert plans[(200, 70, 40)]["wgrad"][3] == 3 and all(p["wgrad"][3] == 1 for s, p in plans.items() if s[0] < 128)
    # all four gemm64_kernel<A_KC, B_KC> instances, and <false, true> with split-K
    inst = {s: R.gemm_instances(*s) for s in R.LINEAR_SHAPES}
    assert {i for v in inst.values() for i in v.values()} == {(a, b) for a in (True, False) for b in (True, False)}
    for s, want in R.LINEAR_INSTANCES.items():
        assert all(inst[s][k] == v for k, v in want.items()), s
    assert inst[(130, 1, 9)]["wgrad"] == (False, True) and plans[(130, 1, 9)]["wgrad"][3] == 2


@pytest.mark.parametrize("B, C, HW", list(R.BIAS_SHAPES))
def test_bias_plan_is_the_librarys(lib, B, C, HW):
    assert lib.itcv_bias_grad_workspace(B, C, HW) == R.bias_splits(B, C, HW) * C * 8
    assert R.bias_splits(B, C, HW) == R.BIAS_SHAPES[(B, C, HW)]


# ---- 3. every mistake moves a named case by more than 100x the tolerance ---------------------------------------------
def recon_case(B, P, loss):
    x, r, planted = R.recon_inputs(B, P, loss)
    return x.double(), r.double(), planted


def test_unrounded_chunk_moves_4100_and_6148():
    """(4, 4100): slices of 1367 read as 342 float4 -- element 1367 and 2734 of every row twice; (1, 6148): 3 elements
    at each of 3 boundaries.  The BCE plants sit on those boundaries."""
    for B, P in ((4, 4100), (1, 6148)):
        x, r, _ = recon_case(B, P, "bce")
        for red in R.REDUCTIONS:
            ref, bad = R.recon_loss(x, r, "bce", red), R.recon_loss(x, r, "bce", red, defect="chunk_unrounded")
            assert R.moved(bad, ref) > 100 * R.TOL_LOSS, (B, P, red)
    x, r, _ = recon_case(2, 4099, "bce")                # the scalar path has exact bounds: nothing to round
    assert R.moved(R.recon_rows(x, r, "bce", "chunk_unrounded"), R.recon_rows(x, r, "bce")) < 1e-12


@pytest.mark.parametrize("B, P, loss", [(4, 2049, "mse"), (4, 2049, "l1"), (4, 2049, "bce"), (2, 4099, "bce"), (4, 4100, "bce")])
def test_unclamped_end_moves_the_next_rows_head(B, P, loss):
    """(4, 2049): the last slice ends at 2056, seven elements into the next row -- 3e-3 of a row for every loss.
    (2, 4099) and (4, 4100): five and four elements, about 1e-3 of a row of uniform errors, too little for mse and l1;
    there it is the BCE plant on the next row's first element (an error of 100 in a row of errors near 1) that counts."""
    x, r, _ = recon_case(B, P, loss)
    ref, bad = R.recon_rows(x, r, loss), R.recon_rows(x, r, loss, "end_unclamped")
    assert R.moved(bad, ref) > 100 * R.TOL_LOSS


def test_dropped_and_doubled_tails_move_the_norm_and_the_scaled_values():
    for n in (1, 3, 1027, 2 * 1048576 + 3):
        v = R.sumsq_input(n, "tail")
        ref = R.total_norm([v])
        assert abs(R.total_norm([v], "sumsq_tail_dropped") - ref) > 100 * R.TOL_NORM * ref, n
        bad, good = R.scale_by(v.double(), 0.5, "scale_tail_twice"), R.scale_by(v.double(), 0.5)
        assert not torch.equal(bad, good) and R.moved(bad, good) > 0.1      # the scaled values are held to bit equality
    v = R.sumsq_input(4, "tail")
    assert R.total_norm([v], "sumsq_tail_dropped") == R.total_norm([v])     # n = 4 has no tail: why 3 and 1027 are there


def test_missing_bce_clamps_move_every_shape():
    for B, P in R.RECON_SHAPES:
        x, r, planted = recon_case(B, P, "bce")
        assert R.moved(R.recon_rows(x, r, "bce", "bce_fwd_unclamped"), R.recon_rows(x, r, "bce")) > 100 * R.TOL_LOSS
        w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64) if B > 1 else torch.ones(1, dtype=torch.float64)
        ref = R.recon_loss_grad(x, r, w, "bce", "none")
        bad = R.recon_loss_grad(x, r, w, "bce", "none", defect="bce_bwd_unclamped")
        assert R.moved(bad[planted], ref[planted]) > 100 * R.TOL_LOSS, (B, P)
        assert torch.equal(bad[~planted], ref[~planted])
        # the unplanted gradients are six to ten orders below the planted ones: they are held to their own scale
        assert float(ref[~planted].abs().max()) < 1e-6 * float(ref[planted].abs().max())


def test_mean_over_the_row_length_moves_every_shape():
    for B, P in R.RECON_SHAPES:
        x, r, _ = recon_case(B, P, "mse")
        g = torch.tensor(1.7, dtype=torch.float64)
        assert R.moved(R.recon_loss(x, r, "mse", "mean", defect="mean_over_P"), R.recon_loss(x, r, "mse", "mean")) > 100 * R.TOL_LOSS
        assert R.moved(R.recon_loss_grad(x, r, g, "mse", "mean", defect="mean_over_P"),
                       R.recon_loss_grad(x, r, g, "mse", "mean")) > 100 * R.TOL_LOSS


def test_l1_tie_sign_moves_every_shape():
    for B, P in R.RECON_SHAPES:
        x, r, planted = recon_case(B, P, "l1")
        w = torch.ones(B, dtype=torch.float64)
        ref, bad = R.recon_loss_grad(x, r, w, "l1", "none"), R.recon_loss_grad(x, r, w, "l1", "none", defect="l1_tie_sign")
        assert R.moved(bad, ref) > 0.5 and float(ref[planted].abs().max()) == 0.0


def linear_case(B, K, N):
    return dbl(*R.linear_inputs(B, K, N)[:5])


@pytest.mark.parametrize("B, K, N", [(5, 283, 70), (7, 351, 40), (64, 2049, 48), (64, 2048, 64), (64, 8192, 40)])
def test_bias_per_split_moves_the_split_forward(B, K, N):
    x, w, b, _, _ = linear_case(B, K, N)
    assert R.moved(R.linear_fwd(x, w, b, "bias_per_split"), R.linear_fwd(x, w, b)) > 100 * R.TOL_LINEAR


def test_ignored_accumulate_moves_200_70_40():
    x, w, b, dy, into = linear_case(200, 70, 40)
    assert R.moved(R.linear_wgrad(dy, x, into, "accumulate_ignored"), R.linear_wgrad(dy, x, into)) > 100 * R.TOL_LINEAR
    x, w, b, dy, into = linear_case(130, 1, 9)
    assert R.moved(R.linear_wgrad(dy, x, into, "accumulate_ignored"), R.linear_wgrad(dy, x, into)) > 100 * R.TOL_LINEAR
    # the weight gradient of every shape with B <= 127 has no split-K: there the defect has nothing to act on
    assert all(R.gemm_plan(N, K, B)[3] == 1 for B, K, N in R.LINEAR_SHAPES if B <= 127)


@pytest.mark.parametrize("B, K, N", [(3, 31, 5), (64, 33, 64), (65, 97, 65), (5, 283, 70), (7, 351, 40), (64, 2049, 48),
                                     (200, 70, 40)])
def test_kept_k_tail_moves_every_gemm_with_one(B, K, N):
    x, w, b, dy, _ = linear_case(B, K, N)
    assert K % 32 and R.moved(R.linear_fwd(x, w, b, "k_tail_kept"), R.linear_fwd(x, w, b)) > 100 * R.TOL_LINEAR
    if N % 32:
        assert R.moved(R.linear_dgrad(dy, w, "k_tail_kept"), R.linear_dgrad(dy, w)) > 100 * R.TOL_LINEAR
    if B % 32:
        assert R.moved(R.linear_wgrad(dy, x, None, "k_tail_kept"), R.linear_wgrad(dy, x)) > 100 * R.TOL_LINEAR


def test_full_last_split_moves_the_short_split_cases():
    for B, K, N in ((7, 351, 40), (64, 2049, 48)):
        x, w, b, _, _ = linear_case(B, K, N)
        assert R.moved(R.linear_fwd(x, w, b, "full_last_split"), R.linear_fwd(x, w, b)) > 100 * R.TOL_LINEAR
    x, w, b, dy, _ = linear_case(200, 70, 40)
    assert R.moved(R.linear_wgrad(dy, x, None, "full_last_split"), R.linear_wgrad(dy, x)) > 100 * R.TOL_LINEAR
    x, w, b, _, _ = linear_case(64, 2048, 64)             # 32 full splits: nothing short
    assert R.moved(R.linear_fwd(x, w, b, "full_last_split"), R.linear_fwd(x, w, b)) == 0.0


@pytest.mark.parametrize("B, rows, W", R.FLIP_SHAPES)
def test_flip_off_by_one_moves_every_width(B, rows, W):
    x, flip = R.flip_input(B, rows, W)
    assert R.moved(R.hflip(x, flip, "flip_off_by_one"), R.hflip(x, flip)) > 0.1     # held to bit equality


def test_elbo_weight_without_the_batch_moves_every_size_but_one():
    g = torch.Generator().manual_seed(1)
    for B in R.ELBO_SIZES:
        a, b = dbl(30 * torch.rand(B, generator=g), 5 * torch.rand(B, generator=g))
        m = R.moved(R.exp_elbo_grad(a, b, -0.05, 3.0, "elbo_weight_no_B"), R.exp_elbo_grad(a, b, -0.05, 3.0))
        assert (m > 100 * R.TOL_LOSS) if B > 1 else (m == 0.0)
