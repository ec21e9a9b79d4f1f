"""The latent-space kernels of csrc/latent.hip against the fp64 restatement tests/latent_ref.py, at every latent-size
tier and every ragged edge: kernel-level inputs, no model and no solver.

Shapes (Bt, D, row_offset, Bl) -- latent_ref.SHAPES -- and what they launch.  ``tc_fwd_part_kernel<DL, VROW, EPS,
MWS>``: test_forward_every_flag_combination runs all eight (VROW, EPS, MWS) combinations on every shape, so
  DL = 1: s1 (2, 1)  one lane; s2 (3, 64)  DL = 1 exactly full, one chunk of 3 columns; s10 (261, 40)  17 chunks and
          the second trip of the joint terms' max / sum loops;
  DL = 2: s3 (17, 65)  one live lane in the second slice, a last chunk of one column;
  DL = 4: s4 (37, 130, off 28, Bl 9)  last chunk of 5, the shard holds global row M - 1 = 35; s5: the same batch, rows
          0-8;
  DL = 8: s6 (19, 257)  one lane in the fifth slice; s7 (21, 512)  full, second trip of every ``l += 256`` loop;
          s8 (50, 293) and s9 (33, 300, off 16, Bl 17): the column-variance forms need more than 64 KB of LDS
-- 4 x 8 = 32 instances.  ``tc_bwd_rows/cols_kernel``: test_live_backward on s2-s7 and s10 (lch = 1, 2, 3, 5, 8);
``tc_full_bwd_rows/cols_kernel``: test_full_decomposition on s3, s4, s6, s8, s9 (lch = 2, 3, 5), dense and packed.

Error measure: rel_err = max |got - ref| / max |ref| per array; tolerance latent_ref.TOL.

Largest observed rel_err on the MI355X (every case, both dataset sizes; the maximum over the listed shapes):
  forward, all eight flag combinations, s1-s10:  prodm 1.5e-7 (s8)  logqz 1.5e-7 (s9)  lse 1.2e-7 (s3)  sjoint 1.3e-7 (s6)
  live backward, s2-s7 and s10:  rows / loss 1.2e-6 (s2)  dz 1.9e-6 (s3)  dmu_all 1.8e-6 (s3), outside the shard
      3.7e-7 (s5)  dlogvar 6.6e-7 (s3)
  full decomposition, s3 s4 s6 s8 s9:  loss 4.1e-7 (s8)  components 1.1e-7 (s8)  dz 5.3e-7 (s4)  dmu_all 2.8e-7 (s9),
      outside the shard 5.3e-7 (s4)  dlogvar_all 9.5e-6 (s9; s3 4.9e-6, else < 3e-7), outside the shard 1.2e-5 (s4)
  helpers:  density and its gradients 2.4e-7, samplers 1.9e-7 (dlp of the weighted sampler at 7 x 70: 1.2e-6),
      KL rows / loss and gradients 1.3e-7, diagonal densities 8.1e-8, reparameterisation 5.5e-8
  weight probe (every density 0), s4 s5 s9, on the weights' scale:  sjoint 4.0e-6  prodm 8.1e-6
The largest, 1.2e-5, is d/dlogvar_all of the full form (1 - d^2 / var cancels in fp32); it is not below 1e-5, so the
tolerance stays at the 1e-4 ceiling.
"""
import pytest
import torch

import latent_ref as R
from oracle import latent_math as lm

pytestmark = pytest.mark.gpu

REDUCTION = {"none": 0, "sum": 1, "mean": 2}
ERRORS = {}          # (quantity, case) -> largest rel_err seen in this run


@pytest.fixture(scope="module")
def HF():
    from hipvae import functional
    yield functional
    print("\nlargest rel_err per quantity and case:")
    for (q, sid), e in sorted(ERRORS.items()):
        print(f"  LATENT_ERR {q:12s} {sid:10s} {e:.3e}")


def dev():
    return torch.device("cuda:0")


def check(q, sid, got, ref, scale_of=None):
    """rel_err(got, ref) < TOL, recorded; ``scale_of``: the array whose maximum is the scale (a slice's parent)."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    scale = float((ref if scale_of is None else scale_of.detach().double()).abs().max()) + 1e-30
    e = float((got - ref).abs().max()) / scale if ref.numel() else 0.0
    ERRORS[(q, sid)] = max(ERRORS.get((q, sid), 0.0), e)
    assert e < R.TOL, (q, sid, e)


def leaves(*ts):
    return [t.detach().double().clone().requires_grad_(True) for t in ts]


def dleaves(*ts):
    return [t.detach().float().to(dev()).requires_grad_(True) for t in ts]


def check_dmu(q, sid, got, ref):
    """d/dmu_all on the shard's own rows and, separately, on the rows outside it (where the analytic KL and the
    diagonal density add nothing), both on the scale of the whole array."""
    Bt, D, off, Bl = R.SHAPES[sid]
    own = torch.zeros(Bt, dtype=torch.bool)
    own[off:off + Bl] = True
    check(q, sid, got.detach().cpu()[own], ref[own], scale_of=ref)
    check(q + "_out", sid, got.detach().cpu()[~own], ref[~own], scale_of=ref)


# ---- a. forward, all eight flag combinations -------------------------------------------------------------------------
@pytest.mark.parametrize("flags", R.ALL_FLAGS)
@pytest.mark.parametrize("sid", list(R.SHAPES))
def test_forward_every_flag_combination(HF, sid, flags):
    Bt, D, off, Bl = R.SHAPES[sid]
    z, mu, lv = R.check_case(sid, flags)
    zg, mg, lg = (t.float().to(dev()) for t in (z, mu, lv))
    for N in R.dataset_sizes(Bt):
        ref = R.estimator(z, mu, lv, N, off, flags)
        got = HF.tc_components(zg, mg, lg, N, off, flags, with_joint=True)
        for name, g, r in zip(("prodm", "logqz", "lse", "sjoint"), got, ref):
            assert g.shape == r.shape and bool(torch.isfinite(g).all()), (name, sid, flags)
            check(name, sid, g, r)


@pytest.mark.parametrize("flags", [R.LIVE, 0])
@pytest.mark.parametrize("sid", ["s4", "s5", "s9"])
def test_importance_weights_on_shards(HF, sid, flags):
    """latent_ref.weight_probe: every density is 0, so the joint terms are the shard's rows of the log importance
    weights themselves (row M - 1 with its own column-0 entry, in a partial chunk at a nonzero offset).  The weights of
    a row sum to about 1, so lse, prodm and logqz are near 0: all four are held to TOL on the weights' scale."""
    Bt, D, off, Bl = R.SHAPES[sid]
    z, mu, lv = R.weight_probe(sid, flags)
    zg, mg, lg = (t.float().to(dev()) for t in (z, mu, lv))
    for N in R.dataset_sizes(Bt):
        ref = R.estimator(z, mu, lv, N, off, flags)
        got = HF.tc_components(zg, mg, lg, N, off, flags, with_joint=True)
        for name, g, r in zip(("w_prodm", "w_logqz", "w_lse", "w_sjoint"), got, ref):
            check(name, sid, g, r, scale_of=ref[3])


# ---- b. a shard equals the same rows of the full batch, bit for bit --------------------------------------------------
@pytest.mark.parametrize("flags", [R.LIVE, 0])
@pytest.mark.parametrize("sid", ["s4", "s5", "s9"])
def test_shard_rows_equal_full_batch_bitwise(HF, sid, flags):
    Bt, D, off, Bl = R.SHAPES[sid]
    z, mu, lv = (t.to(dev()) for t in R.case_inputs(sid))
    for N in R.dataset_sizes(Bt):
        full = HF.tc_components(z, mu, lv, N, 0, flags, with_joint=True)
        lvs = lv[off:off + Bl].contiguous() if flags & R.VAR_FROM_ROW else lv
        part = HF.tc_components(z[off:off + Bl].contiguous(), mu, lvs, N, off, flags, with_joint=True)
        for name, p, f in zip(("prodm", "logqz", "lse", "sjoint"), part, full):
            assert torch.equal(p, f[off:off + Bl]), (name, sid, flags, N)


# ---- c. the live backward --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["s2", "s3", "s4", "s5", "s6", "s7", "s10"])
def test_live_backward(HF, sid):
    Bt, D, off, Bl = R.SHAPES[sid]
    ops = R.check_case(sid, R.LIVE)
    w = torch.linspace(-1.0, 2.0, Bl, dtype=torch.float64)
    wg = w.float().to(dev())
    for N in R.dataset_sizes(Bt):
        zr, mr, lr = leaves(*ops)
        prodm, logqz, _, _ = R.estimator(zr, mr, lr, N, off, R.LIVE)
        tc, kl = logqz - prodm, lm.kl_rows(lr, mr[off:off + Bl])
        zg, mg, lg = dleaves(*ops)

        def compare(tag, out, ref):
            check(tag, sid, out, ref)
            so, sr = ((wg * out).sum(), (w * ref).sum()) if ref.dim() else (out, ref)
            got = torch.autograd.grad(so, (zg, mg, lg))
            want = torch.autograd.grad(sr, (zr, mr, lr), retain_graph=True)
            check(tag + "_dz", sid, got[0], want[0])
            check_dmu(tag + "_dmu", sid, got[1], want[1])
            check(tag + "_dlv", sid, got[2], want[2])

        compare("tcrows", HF.TcRowsFn.apply(zg, mg, lg, N, off), tc)
        for ctc in (511.0, -0.5):
            for ckl in (0.0, 1.0):
                for red in ("none", "sum", "mean"):
                    out = HF.TcKlFn.apply(zg, mg, lg, N, off, ctc, ckl, REDUCTION[red])
                    compare("tckl", out, R.reduce_rows(ctc * tc + ckl * kl, red))


# ---- d. the full decomposition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("sid", ["s3", "s4", "s6", "s8", "s9"])
def test_full_decomposition(HF, sid, packed):
    Bt, D, off, Bl = R.SHAPES[sid]
    ops = R.check_case(sid, 0)
    w = torch.linspace(-1.0, 2.0, Bl, dtype=torch.float64)
    wg = w.float().to(dev())
    for N in R.dataset_sizes(Bt):
        zr, mr, lr = leaves(*ops)
        comps = R.full_components(zr, mr, lr, N, off)
        zg, = dleaves(ops[0])
        if packed:                      # the halves of one [Bt, 2D] tensor; their gradients are the halves of one too
            pk, = dleaves(torch.cat([ops[1], ops[2]], 1))
            mg, lg, wrt = pk[:, :D], pk[:, D:], (zg, pk)
        else:
            mg, lg = dleaves(ops[1], ops[2])
            wrt = (zg, mg, lg)
        for a, b, c in ((0.3, -2.0, 1.7), (1.0, 4.0, 1.0)):
            for red in ("none", "sum", "mean"):
                ref = R.reduce_rows(a * comps[0] + b * comps[1] + c * comps[2], red)
                out, cg = HF.TcFullFn.apply(zg, mg, lg, N, off, a, b, c, REDUCTION[red])
                check("full", sid, out, ref)
                check("full_comps", sid, cg, comps)
                so, sr = ((wg * out).sum(), (w * ref).sum()) if red == "none" else (out, ref)
                got = torch.autograd.grad(so, wrt)
                want = torch.autograd.grad(sr, (zr, mr, lr), retain_graph=True)
                if packed:
                    assert got[1].shape == (Bt, 2 * D)
                    got = (got[0], got[1][:, :D], got[1][:, D:])
                check("full_dz", sid, got[0], want[0])
                check_dmu("full_dmu", sid, got[1], want[1])
                check_dmu("full_dlv", sid, got[2], want[2])


# ---- e. the materialising helpers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("var_of", ["row", "column"])
@pytest.mark.parametrize("eps_density", [True, False])
def test_gauss_log_density(HF, eps_density, var_of):
    """[B,1,D] x [1,B,D] operands, the variance as [B,1,D] or [1,B,D], the means a non-contiguous view."""
    B, D = 7, 70
    flags = (R.VAR_FROM_ROW if var_of == "row" else 0) | (R.EPS_DENSITY if eps_density else 0)
    z, mu, lv = R.make_inputs(B, D, 1000)
    R.check_preconditions(z, mu, lv, flags)
    g = torch.randn(B, B, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ax = 1 if var_of == "row" else 0
    zr, mr, lr = leaves(z, mu, lv)
    ref = R.pairwise(zr, mr, lr, flags)
    want = torch.autograd.grad((g * ref).sum(), (zr, mr, lr))
    zg, lg = dleaves(z, lv)
    wide, = dleaves(torch.stack([mu, -mu], 2).reshape(B, 2 * D))       # mu in the even columns
    mview = wide[:, ::2]
    assert not mview.is_contiguous()
    out = HF.GaussLogDensityFn.apply(zg.unsqueeze(1), mview.unsqueeze(0), lg.unsqueeze(ax), eps_density)
    sid = f"{'eps' if eps_density else 'plain'}-{var_of}"
    check("gld", sid, out, ref)
    got = torch.autograd.grad((g.float().to(dev()) * out).sum(), (zg, wide, lg))
    check("gld_dx", sid, got[0], want[0])
    check("gld_dmu", sid, got[1][:, ::2], want[1])
    assert float(got[1][:, 1::2].abs().max()) == 0.0
    check("gld_dlv", sid, got[2], want[2])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B, D", [(7, 70), (5, 300)])
def test_sampling(HF, B, D, weighted):
    z, mu, lv = R.make_inputs(B, D, 1000)
    lp = R.pairwise(z, mu, lv, R.LIVE)                    # fp32 values, some at the clamp
    N = B + 3
    gen = torch.Generator().manual_seed(4)
    gp, gq = torch.randn(B, generator=gen, dtype=torch.float64), torch.randn(B, generator=gen, dtype=torch.float64)
    lr, = leaves(lp)
    pm, lq = (lm.weighted if weighted else lm.stratified)(lr, N)
    want, = torch.autograd.grad((gp * pm).sum() + (gq * lq).sum(), lr)
    lg, = dleaves(lp)
    a, b = HF.SamplingFn.apply(lg, N, weighted)
    sid = f"{'mws' if weighted else 'mss'}-{B}x{D}"
    check("samp_prodm", sid, a, pm)
    check("samp_logqz", sid, b, lq)
    got, = torch.autograd.grad((gp.float().to(dev()) * a).sum() + (gq.float().to(dev()) * b).sum(), lg)
    check("samp_dlp", sid, got, want)


@pytest.mark.parametrize("m", [9, 1])
def test_on_off_diag(HF, m):
    x = torch.randn(m, 9, generator=torch.Generator().manual_seed(5))
    dg, off = HF.on_off_diag(x.to(dev()))
    assert torch.equal(dg.cpu(), torch.diagonal(x)) and torch.equal(off.cpu(), x - torch.diag_embed(x))


def test_row_kernels_walk_their_loops_twice(HF):
    """(B, D) = (35, 300): 35 rows are three trips of kl_loss_fwd's 16 waves with a tail, D = 300 the second trip of
    the ``l += 256`` loops of kl_rows_fwd and diag_logdensity."""
    B, D = 35, 300
    z, mu, lv = R.make_inputs(B, D, 1000)
    sid = "35x300"
    w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    wg = w.float().to(dev())
    a, b = HF.diag_logdensity_rows(*(t.to(dev()) for t in (z, mu, lv)))
    zd, md, ld = z.double(), mu.double(), lv.double()
    check("diag_logq", sid, a, lm.log_density_plain(zd, md, ld).sum(1))
    check("diag_logp", sid, b, lm.log_density_plain(zd, torch.zeros_like(zd), torch.zeros_like(zd)).sum(1))
    mr, lr = leaves(mu, lv)
    rows = lm.kl_rows(lr, mr)
    mg, lg = dleaves(mu, lv)
    out = HF.KlRowsFn.apply(lg, mg)
    check("klrows", sid, out, rows)
    got = torch.autograd.grad((wg * out).sum(), (lg, mg))
    want = torch.autograd.grad((w * rows).sum(), (lr, mr), retain_graph=True)
    check("klrows_dlv", sid, got[0], want[0])
    check("klrows_dmu", sid, got[1], want[1])
    for red in ("none", "sum", "mean"):
        for scale in (1.0, 0.37):
            ref = scale * R.reduce_rows(rows, red)
            out = HF.KlLossFn.apply(lg, mg, REDUCTION[red], scale)
            check("klloss", sid, out, ref)
            so, sr = ((wg * out).sum(), (w * ref).sum()) if red == "none" else (out, ref)
            got = torch.autograd.grad(so, (lg, mg))
            want = torch.autograd.grad(sr, (lr, mr), retain_graph=True)
            check("klloss_dlv", sid, got[0], want[0])
            check("klloss_dmu", sid, got[1], want[1])


def test_reparam_grid_tail(HF):
    n = 2049                                              # eight blocks of 256 and one element
    gen = torch.Generator().manual_seed(6)
    mu, lv, eps, dz = (torch.randn(1, n, generator=gen) for _ in range(4))
    mr, lr = leaves(mu, lv)
    ref = lm.reparameterize(mr, lr, eps.double())
    want = torch.autograd.grad((dz.double() * ref).sum(), (mr, lr))
    mg, lg = dleaves(mu, lv)
    out = HF.ReparamFn.apply(mg, lg, eps.to(dev()))
    got = torch.autograd.grad((dz.to(dev()) * out).sum(), (mg, lg))
    check("reparam", "2049", out, ref)
    check("reparam_dmu", "2049", got[0], want[0])
    check("reparam_dlv", "2049", got[1], want[1])


# ---- f. refusals: an error, and nothing launched ---------------------------------------------------------------------
def _tc_fwd_refused(HF, Bl, Bt, off, D, N):
    from hipvae.abi import HipExtensionError, call, lib, ptr, stream
    d = dev()
    z, mu, lv = torch.zeros(Bl, D, device=d), torch.zeros(Bt, D, device=d), torch.zeros(max(Bl, Bt), D, device=d)
    outs = [torch.full(s, 7.0, device=d) for s in ((Bl,), (Bl,), (Bl, D), (Bl, Bt))]
    nws = lib.itcv_tc_fwd_workspace(Bl, Bt, D) + 1024
    ws = torch.full((nws,), 7, dtype=torch.uint8, device=d)
    with pytest.raises(HipExtensionError):
        call("itcv_tc_fwd", ptr(z), ptr(mu), ptr(lv), *(ptr(t) for t in outs), Bl, Bt, off, D, N, R.LIVE, ptr(ws), nws,
             stream())
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs + [ws])


@pytest.mark.parametrize("Bl, Bt, off, D, N", [(4, 4, 0, 513, 100), (1, 1, 0, 8, 100), (3, 4, 2, 8, 100), (4, 4, 0, 8, 0)],
                         ids=["D=513", "Bt=1", "rows-past-the-batch", "N=0"])
def test_forward_refusals(HF, Bl, Bt, off, D, N):
    _tc_fwd_refused(HF, Bl, Bt, off, D, N)
    z, mu = torch.zeros(Bl, D, device=dev()), torch.zeros(Bt, D, device=dev())
    with pytest.raises(HF.abi.HipExtensionError):
        HF.tc_components(z, mu, z, N, off)
    with pytest.raises(HF.abi.HipExtensionError):
        HF.TcKlFn.apply(z, mu, z, N, off, 1.0, 1.0, 2)
    with pytest.raises(HF.abi.HipExtensionError):
        HF.TcFullFn.apply(z, mu, mu.clone(), N, off, 1.0, 1.0, 1.0, 2)


def test_backward_refuses_other_than_live_flags(HF):
    from hipvae.abi import HipExtensionError, call, lib, ptr, stream
    d = dev()
    B, D = 4, 8
    ins = [torch.zeros(s, device=d) for s in ((B,), (B, D), (B, D), (B, D), (B,), (B, D), (B, B))]
    outs = [torch.full((B, D), 7.0, device=d) for _ in range(3)]
    nws = lib.itcv_tc_bwd_workspace(B, B)
    ws = torch.full((nws,), 7, dtype=torch.uint8, device=d)
    for flags in (0, R.VAR_FROM_ROW, R.EPS_DENSITY, R.LIVE | R.WEIGHTED):
        with pytest.raises(HipExtensionError):
            call("itcv_tc_bwd", *(ptr(t) for t in ins), *(ptr(t) for t in outs), B, B, 0, D, 100, flags, ptr(ws), nws,
                 stream())
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs + [ws])
