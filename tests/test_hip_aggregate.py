"""GPU tests of the dataset-scale aggregate-posterior kernel (csrc/aggregate.hip: itcv_aggregate_logdensity), of the
decomposition built on it (hipvae/aggregate.py) and of the solver switch, against the fp64 restatement of
tests/aggregate_ref.py.  Error measure and tolerance are the project's: rel_err = max |got - ref| / max |ref| per array,
TOL = 1e-4 (tests/latent_ref.py).

What each shape (S, N, D) launches.  P = lanes per component (next_pow2(D), 64 above), G = 64 / P components per wave step,
DL = values of l per lane, R = rows per wave (a block holds 4 R rows), chunk = components staged in LDS at a time.  With
splits = 0 the library cuts N into min(ceil(512 / row tiles), N / (4 chunk)) slices, at least one:
  1x1x1        P 1   G 64  R 8  chunk 1024  1 slice:    one component in a wave step of 64 slots, per-row joint terms (P < R)
  3x5x10       P 16  G 4   R 8  chunk 64    1 slice:    two wave steps, the second with one component and three empty groups
  9x1000x10    P 16  G 4   R 8  chunk 64    3 slices:   334 + 334 + 332 components, partial last chunks; rows in two waves
  33x4099x32   P 32  G 2   R 8  chunk 32    32 slices:  two row tiles (32 + 1 rows); 129-component slices end in a chunk of
                                                        one component (a step with an empty group), the last slice holds 100
  9x2051x33    P 64  G 1   R 8  chunk 16    32 slices:  the first D above a power of two: 31 idle lanes per component
  9x1500x64    P 64  G 1   R 8  chunk 16    23 slices:  every lane busy, no padding in l
  9x777x65     P 64  DL 2  R 8  chunk 8     24 slices:  the first D of the two-values-per-lane tier; 63 of 64 second values idle
  5x300x130    P 64  DL 4  R 4  chunk 8     9 slices:   the four-values tier (32 KB chunk); rows split 4 + 1 over two waves
  5x200x512    P 64  DL 8  R 2  chunk 4     12 slices:  the largest D; rows over three waves
  2x300001x10  P 16  G 4   R 8  chunk 64    512 slices, and ONE slice (splits = 1): 75 001 wave steps per lane, 4688 chunks
  9x131x2, 9x131x3, 9x131x7: P 2, 4, 8 (G 32, 16, 8), the lane groups the shapes above do not reach; P 2 and 4 keep the joint
               terms per row, P 8 = R is the narrowest tier in which lane r of a group keeps row r's
test_splits pins 1 and 3 slices; test_rows_do_not_depend_on_the_call 1, 2, 3 and 5.

Largest errors: not recorded yet -- every test prints its figures (rel_err per quantity and shape), and the figures of a run
on the MI355X belong here.
"""
import functools
import math

import numpy as np
import pytest
import torch

import aggregate_ref as R

pytestmark = pytest.mark.gpu

TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)      # the model of tests/test_hip_model.py


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(shape):
    """fp32 inputs of a shape and their fp64 references (uniform weights, log_softmax weights), computed once."""
    z, rows, mu, lv, lw = R.make_inputs(*shape)
    z64, mu64, lv64 = z.double(), mu.double(), lv.double()
    return dict(z=z, rows=rows, mu=mu, lv=lv, lw=lw, ref={False: R.log_density(z64, mu64, lv64, None),
                                                         True: R.log_density(z64, mu64, lv64, lw.double())})


def on_device(c, *names):
    return tuple(c[n].to(dev()) for n in names)


def check(tag, got, ref):
    errs = [R.rel_err(g, r) for g, r in zip(got, ref)]
    print(tag, "rel_err logqz %.2e lse %.2e" % tuple(errs))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert max(errs) <= R.TOL, (tag, errs)
    return errs


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "softmax"])
@pytest.mark.parametrize("shape", R.SHAPES + R.NARROW, ids=R.sid)
def test_against_fp64(shape, weighted):
    from hipvae import functional as HF
    c = case(shape)
    z, mu, lv, lw = on_device(c, "z", "mu", "lv", "lw")
    for splits in (0, 1) if shape == R.LONG else (0,):     # the long stream also as ONE slice: 75 001 steps per lane
        got = HF.aggregate_logdensity(z, mu, lv, lw if weighted else None, splits)
        assert got[0].shape == (shape[0],) and got[1].shape == (shape[0], shape[2])
        check("%s %s splits %d" % (R.sid(shape), "softmax" if weighted else "uniform", splits), got, c["ref"][weighted])


@pytest.mark.parametrize("shape,a,b,splits", [((33, 4099, 32), 5, 21, 3), ((33, 4099, 32), 32, 33, 1), ((9, 777, 65), 2, 7, 2),
                                               ((9, 1000, 10), 1, 9, 5)], ids=str)
def test_rows_do_not_depend_on_the_call(shape, a, b, splits):
    """Rows [a, b) computed alone (other places in the tile, another S) equal the full call's bit for bit at equal splits;
    so do two identical calls."""
    from hipvae import functional as HF
    z, mu, lv, lw = on_device(case(shape), "z", "mu", "lv", "lw")
    full = HF.aggregate_logdensity(z, mu, lv, lw, splits)
    again = HF.aggregate_logdensity(z, mu, lv, lw, splits)
    part = HF.aggregate_logdensity(z[a:b].contiguous(), mu, lv, lw, splits)
    for f, g, p in zip(full, again, part):
        assert torch.equal(f.view(torch.int32), g.view(torch.int32))
        assert torch.equal(f[a:b].view(torch.int32), p.view(torch.int32))


@pytest.mark.parametrize("splits", [1, 3, 0])
@pytest.mark.parametrize("shape", [(33, 4099, 32), (9, 777, 65)], ids=R.sid)
def test_splits(shape, splits):
    from hipvae import functional as HF
    c = case(shape)
    z, mu, lv, lw = on_device(c, "z", "mu", "lv", "lw")
    check("%s splits %d" % (R.sid(shape), splits), HF.aggregate_logdensity(z, mu, lv, lw, splits), c["ref"][True])


@pytest.mark.parametrize("n,D", [(37, 130), (50, 10)])
def test_agrees_with_the_training_kernel(n, D):
    """Uniform weights over the batch are the minibatch-weighted sampler of itcv_tc_fwd up to its constant log(Bt Nd):
    logqz_new = logqz_old + log Nd, sum_l lse_new = prodm_old + D log Nd."""
    from hipvae import abi
    from hipvae import functional as HF
    Nd = 10000
    z, _, mu, lv, _ = R.make_inputs(n, n, D)
    z, mu, lv = z.to(dev()), mu.to(dev()), lv.to(dev())
    prodm, logqz_old, _ = HF.tc_components(z, mu, lv, Nd, 0, flags=abi.TC_WEIGHTED)
    logqz, lse = HF.aggregate_logdensity(z, mu, lv)
    e1 = R.rel_err(logqz, logqz_old.double() + math.log(Nd))
    e2 = R.rel_err(lse.double().sum(1), prodm.double() + D * math.log(Nd))
    print("vs itcv_tc_fwd at %d x %d x %d: logqz %.2e prodm %.2e" % (n, n, D, e1, e2))
    assert max(e1, e2) <= R.TOL


def check_scores(tag, got, ref):
    """Every key of the decomposition.  The per-sample arrays meet TOL relative to their largest magnitude, so a mean of
    differences of two of them is held to TOL times the sum of the two magnitudes."""
    from hipvae import aggregate
    ps = ref["per_sample"]
    mag = {k: float(ps[k].abs().max()) for k in ("logqcx", "logpz", "logqz")}
    mag["prodm"], mag["lse"] = float(ps["lse"].sum(1).abs().max()), float(ps["lse"].abs().max())
    bound = dict(mi=mag["logqcx"] + mag["logqz"], tc=mag["logqz"] + mag["prodm"], dwkl=mag["prodm"] + mag["logpz"],
                 kl=mag["logqcx"] + mag["logpz"] + 2 * (mag["logqz"] + mag["prodm"]), joint_entropy=mag["logqz"],
                 kl_analytic=abs(ref["kl_analytic"]), marginal_entropies=mag["lse"], dimwise_kl=mag["lse"] + 50.0)
    assert sorted(got) == sorted(aggregate.KEYS)
    for k in aggregate.KEYS:
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(ref[k])).max())
        print(tag, k, "ref", np.asarray(ref[k]).ravel()[:3], "abs err %.2e of bound %.2e" % (err, R.TOL * bound[k]))
        assert np.isfinite(np.asarray(got[k])).all() and err <= R.TOL * bound[k], (tag, k)
    assert isinstance(got["kl"], float) and abs(got["kl"] - (got["mi"] + got["tc"] + got["dwkl"])) <= 4e-16 * bound["kl"]
    assert got["marginal_entropies"].dtype == np.float64 and got["marginal_entropies"].shape == got["dimwise_kl"].shape


@pytest.mark.parametrize("shape", [(33, 4099, 32), (9, 2051, 33)], ids=R.sid)
def test_elbo_decomposition(shape):
    from hipvae import aggregate
    c = case(shape)
    z, rows, mu, lv, lw = on_device(c, "z", "rows", "mu", "lv", "lw")
    for w_dev, w in ((None, None), (lw, c["lw"])):
        check_scores(R.sid(shape), aggregate.elbo_decomposition(z, rows, mu, lv, w_dev),
                     R.decomposition(c["z"], c["rows"], c["mu"], c["lv"], w))
    bad = z.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(ValueError):
        aggregate.elbo_decomposition(bad, rows, mu, lv)
    with pytest.raises(ValueError):
        aggregate.elbo_decomposition(z, rows + shape[1], mu, lv)


def test_end_to_end_on_a_tiny_model():
    import models
    from hipvae import aggregate
    from hipvae.dataset import DeviceImageTable
    from solvers import VAESolver
    from test_hip_dataset import make_factor_dataset
    from test_hip_disent import StubWriter
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = make_factor_dataset((3, 32, 32))
    table = DeviceImageTable.from_dataset(ds, dev())
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    rng_dev, rng_host = torch.cuda.get_rng_state(), torch.get_rng_state()
    kw = dict(num_samples=50, batch_size=7, seed=11, return_inputs=True)
    (s_t, in_t), (s_d, in_d) = (aggregate.compute_elbo_decomposition(src, model, **kw) for src in (table, ds))
    assert all(torch.equal(a, b) for a, b in zip(in_t, in_d))               # the same inputs from both sources
    z, rows, mu, lv = in_t
    assert z.shape == (50, 10) and mu.shape == lv.shape == (24, 10) and rows.dtype == torch.int64
    assert model.training and before and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.cuda.get_rng_state(), rng_dev) and torch.equal(torch.get_rng_state(), rng_host)
    ref = R.decomposition(z.cpu(), rows.cpu(), mu.cpu(), lv.cpu())
    check_scores("tiny model (table)", s_t, ref)
    check_scores("tiny model (dataset)", s_d, ref)
    assert s_t["mi"] <= math.log(24) + 1e-3                                 # a sample's own component is in the mixture
    # a subset of the components, the documented draws
    sub, (z2, rows2, mu2, _) = aggregate.compute_elbo_decomposition(table, model, num_samples=9, num_components=5, seed=3,
                                                                    return_inputs=True)
    comps, rows_h, _ = aggregate.draw_plan(24, 9, 5, 3)
    assert mu2.shape == (5, 10) and sorted(comps.tolist()) == comps.tolist() and len(set(comps.tolist())) == 5
    assert np.array_equal(rows2.cpu().numpy(), rows_h) and rows_h.max() < 5 and torch.equal(mu2, mu[torch.from_numpy(comps)])
    assert sorted(sub) == sorted(aggregate.KEYS)
    model.eval()
    aggregate.dataset_posteriors(ds, model, np.arange(3), 2)
    assert not model.training
    model.train()

    # the solver switch: one record at a test iteration, none off it, for a table and for a dataset without factors
    class Plain:
        def __len__(self):
            return len(ds)

        def __getitem__(self, i):
            return ds[i]

    for dataset, use_table in ((ds, True), (Plain(), False)):
        w = StubWriter()
        solver = VAESolver(dataset=dataset, model=model, batch_size=16,
                           optimizer_e=torch.optim.Adam(model.encoder.parameters()),
                           optimizer_d=torch.optim.Adam(model.decoder.parameters()), recon_loss_type="mse", beta_kl=1.0,
                           beta_rec=1.0, device=dev(), use_amp=False, grad_scaler=None, writer=w, test_iter=2, clip=100.0)
        assert solver.elbo_params is None
        if use_table:
            assert solver.use_device_dataset(table) is table
        solver.device_scores, solver.extra_scores = False, ("elbo_decomposition",)
        solver.elbo_params = dict(num_samples=50, seed=11, batch_size=7)
        solver.write_disentanglemnt_scores(0)
        solver.write_disentanglemnt_scores(1)
        assert [(c[0], c[1], c[3]) for c in w.calls] == [("add_scalars", "aggregate_decomp", 0)]
        rec = w.calls[0][2]
        assert list(rec) == ["mi", "tc", "dwkl", "kl", "kl_analytic"]
        assert all(rec[k] == s_t[k] for k in rec)            # the same draws, the same batches: the same scores
        assert model.training
        solver.extra_scores = ("elbo_decomposition", "mig")
        with pytest.raises(ValueError, match="elbo_decomposition"):
            solver.write_disentanglemnt_scores(0)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
