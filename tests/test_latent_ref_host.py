"""Host-only checks of the fp64 restatement tests/latent_ref.py, which tests/test_hip_latent.py holds the latent kernels
to: (1) it reproduces the recorded outputs of the original program (tests/golden/ops.npz and tc_full.npz, tags a and c)
to 1e-5 of the array maximum -- what fp32 rounding of the stored values allows; (2) the inputs of every GPU case meet
the three conditions the cases rely on; (3) each mistake a kernel could plausibly make (latent_ref.DEFECTS and the
swapped variance source) moves a checked quantity by at least 100x the GPU tolerance on the shapes that claim to catch
it, so a kernel with that mistake cannot pass."""
import os

import numpy as np
import pytest
import torch

import latent_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD_TOL = 1e-5
MOVE = 100 * R.TOL


def T(a):
    return torch.from_numpy(np.asarray(a))


def leaves(*ts):
    return [t.double().clone().requires_grad_(True) for t in ts]


@pytest.fixture(scope="module", params=["a", "c"])
def gold(request):
    tag = request.param
    G = np.load(os.path.join(GOLDEN, "ops.npz"))
    F = np.load(os.path.join(GOLDEN, "tc_full.npz"))
    z, mu, lv = (T(G[f"{tag}_{k}"]) for k in ("z", "mu", "logvar"))
    return tag, G, F, (z, mu, lv), int(G[f"{tag}_BDN"][2])


def test_estimator_against_recorded_outputs(gold):
    tag, G, _, (z, mu, lv), N = gold
    zd, md, ld = (t.double() for t in (z, mu, lv))
    g = lambda k: T(G[f"{tag}_{k}"])  # noqa: E731
    pm, lq, _, _ = R.estimator(zd, md, ld, N, 0, R.LIVE)
    assert R.rel_err(pm, g("mss_prodm")) < GOLD_TOL and R.rel_err(lq, g("mss_logqz")) < GOLD_TOL
    assert R.rel_err(lq - pm, g("tc_none")) < GOLD_TOL
    pm, lq, _, _ = R.estimator(zd, md, ld, N, 0, R.LIVE | R.WEIGHTED)
    assert R.rel_err(pm, g("mws_prodm")) < GOLD_TOL and R.rel_err(lq, g("mws_logqz")) < GOLD_TOL
    comps = R.full_components(zd, md, ld, N, 0)
    for k, name in enumerate(("full_mi", "full_tc", "full_dwkl")):
        assert R.rel_err(comps[k], g(name)) < GOLD_TOL, name


def test_tc_kl_gradients_against_recorded_outputs(gold):
    tag, G, _, (z, mu, lv), N = gold
    zr, mr, lr = leaves(z, mu, lv)
    loss = R.tc_kl(zr, mr, lr, N, 0, 511.0, 1.0, "mean")
    loss.backward()
    assert R.rel_err(loss, T(G[f"{tag}_tckl_b512p0"])) < GOLD_TOL
    for k, t in (("dz", zr), ("dmu", mr), ("dlogvar", lr)):
        assert R.rel_err(t.grad, T(G[f"{tag}_tckl_b512p0_{k}"])) < GOLD_TOL, k


def test_full_loss_against_recorded_outputs(gold):
    tag, _, F, (z, mu, lv), N = gold
    st = int(F[f"{tag}_stride"])
    for beta, bt in ((512.0, "512p0"), (0.5, "0p5"), (1.0, "1p0")):
        zr, mr, lr = leaves(z, mu, lv)
        loss, _ = R.full_loss(zr, mr, lr, N, 0, 1.0, beta, 1.0, "mean")
        loss.backward()
        assert R.rel_err(loss, T(F[f"{tag}_b{bt}"])) < GOLD_TOL
        for k, t in (("dz", zr), ("dmu", mr), ("dlogvar", lr)):
            assert R.rel_err(t.grad.reshape(-1)[::st], T(F[f"{tag}_b{bt}_{k}"])) < GOLD_TOL, (bt, k)
    zr, mr, lr = leaves(z, mu, lv)
    rows, _ = R.full_loss(zr, mr, lr, N, 0, 1.0, 512.0, 1.0, "none")
    assert R.rel_err(rows, T(F[f"{tag}_w_rows"])) < GOLD_TOL
    (T(F[f"{tag}_w"]).double() * rows).sum().backward()
    for k, t in (("dz", zr), ("dmu", mr), ("dlogvar", lr)):
        assert R.rel_err(t.grad.reshape(-1)[::st], T(F[f"{tag}_w_{k}"])) < GOLD_TOL, k


@pytest.mark.parametrize("sid", list(R.SHAPES))
def test_case_inputs_meet_the_preconditions(sid):
    """Clamp share in [0.005, 0.25], >= 1 % floored variances, no element within 1e-3 of the clamp -- for all four
    (density, variance source) forms, the diagonal terms of the full form included, and fp32 decides every clamp as fp64
    does.  s1 holds four elements, of which the recipe clamps two or three: its share is only required to lie strictly
    between 0 and 1."""
    from oracle import latent_math as lm
    Bt, D, off, Bl = R.SHAPES[sid]
    for flags in range(4):
        z, mu, lv = R.check_case(sid, flags)
        r32 = R.pairwise_unclamped(z.float(), mu.float(), lv.float(), flags)
        r64 = R.pairwise_unclamped(z, mu, lv, flags)
        assert torch.equal(r32 <= -50, r64 <= -50)
    z, mu, lv = R.shard_operands(sid, 0)
    diag = -0.5 * ((z - mu[off:off + Bl]) ** 2 * torch.exp(-lv[off:off + Bl]) + lv[off:off + Bl] + lm.LOG_2PI)
    prior = -0.5 * (z * z + lm.LOG_2PI)
    assert float((diag + 50).abs().min()) >= 1e-3 and float((prior + 50).abs().min()) >= 1e-3
    # the near rows: their largest joint term is a column of the last chunk
    sj = R.estimator(*R.shard_operands(sid, R.LIVE), Bt + 3, off, R.LIVE)[3]
    assert int(sj[0].argmax()) >= Bt - max(Bt % R.CHUNK, 1)


def moved(got, ref):
    """The largest rel_err over the paired arrays."""
    return max(R.rel_err(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("sid", ["s3", "s4", "s6", "s9"])
@pytest.mark.parametrize("flags", [R.LIVE, 0])
def test_dropping_the_tail_chunk_moves_the_forward(sid, flags):
    Bt, D, off, Bl = R.SHAPES[sid]
    ops = R.shard_operands(sid, flags)
    for N in R.dataset_sizes(Bt):
        ref = R.estimator(*ops, N, off, flags)
        bad = R.estimator(*ops, N, off, flags, "drop_tail")
        assert R.rel_err(bad[0], ref[0]) > MOVE and R.rel_err(bad[1], ref[1]) > MOVE, (N,)
        assert R.rel_err(bad[2], ref[2]) > MOVE
        assert R.rel_err(bad[3], ref[3][:, :bad[3].shape[1]]) == 0.0      # the joint terms that are computed are right


@pytest.mark.parametrize("flags", [R.LIVE, 0])
def test_local_row_index_moves_the_weights_on_s4(flags):
    """Row M - 1 = 35 of s4 is local row 7: with the local index no row of the shard gets the special column-0 weight.
    At N = Bt + 3 that is 2.2 in one joint term -- on the recipe's inputs 7e-3 of prodm's scale and less of the other
    arrays', because the densities there are of order 100 to 6000.  The weight probe of the same shape (every density
    0) is what holds the kernel to it: there the joint terms move by a third of their scale."""
    Bt, D, off, Bl = R.SHAPES["s4"]
    N = Bt + 3
    ops = R.shard_operands("s4", flags)
    ref, bad = R.estimator(*ops, N, off, flags), R.estimator(*ops, N, off, flags, "local_row")
    assert abs(float(bad[3][7, 0] - ref[3][7, 0])) > 1.0
    ops = R.weight_probe("s4", flags)
    ref, bad = R.estimator(*ops, N, off, flags), R.estimator(*ops, N, off, flags, "local_row")
    assert float(ref[3].abs().max()) < 7.0                           # the joint terms are the log weights
    for k in range(4):
        assert R.rel_err(bad[k], ref[k]) > MOVE, k
    # s5 holds no special row: there the two indexings agree, which is why s4 is in the list
    ops = R.weight_probe("s5", flags)
    assert moved(R.estimator(*ops, N, 0, flags, "local_row"), R.estimator(*ops, N, 0, flags)) == 0.0


@pytest.mark.parametrize("flags", R.ALL_FLAGS)
def test_swapped_variance_source_moves_the_forward_on_s3(flags):
    Bt, D, off, Bl = R.SHAPES["s3"]
    z, mu, lv = R.shard_operands("s3", flags)
    for N in R.dataset_sizes(Bt):
        ref = R.estimator(z, mu, lv, N, off, flags)
        bad = R.estimator(z, mu, lv, N, off, flags ^ R.VAR_FROM_ROW)
        assert min(R.rel_err(b, r) for b, r in zip(bad, ref)) > MOVE


@pytest.mark.parametrize("sid", list(R.SHAPES))
def test_missing_weighted_constant_moves_the_forward(sid):
    """prodm loses D log(Bt N) on every shape; logqz loses one log(Bt N), which is above 100x the tolerance of its own
    scale (about D) on the shapes with D <= 130: s1-s5 and s10 are the ones that hold the finish kernel to it."""
    Bt, D, off, Bl = R.SHAPES[sid]
    for flags in (f for f in R.ALL_FLAGS if f & R.WEIGHTED):
        ops = R.shard_operands(sid, flags)
        for N in R.dataset_sizes(Bt):
            ref, bad = R.estimator(*ops, N, off, flags), R.estimator(*ops, N, off, flags, "no_const")
            assert R.rel_err(bad[0], ref[0]) > MOVE
            assert R.rel_err(bad[1], ref[1]) > MOVE or D > 130


def test_inactive_clamp_moves_the_gradients_on_s4():
    Bt, D, off, Bl = R.SHAPES["s4"]
    N = Bt + 3
    w = torch.linspace(-1.0, 2.0, Bl, dtype=torch.float64)
    grads = {}
    for defect in (None, "clamp_through"):
        zr, mr, lr = leaves(*R.shard_operands("s4", R.LIVE))
        (w * R.tc_rows(zr, mr, lr, N, off, R.LIVE, defect)).sum().backward()
        za, ma, la = leaves(*R.shard_operands("s4", 0))
        R.full_loss(za, ma, la, N, off, 0.3, -2.0, 1.7, "mean", defect)[0].backward()
        grads[defect] = [t.grad for t in (zr, mr, lr, za, ma, la)]
    for bad, ref in zip(grads["clamp_through"], grads[None]):
        assert R.rel_err(bad, ref) > MOVE
