"""Host tests of the importance-weighted bound: the fp64 restatement tests/iwae_ref.py against torch fp64 autograd (the plain
bound for "iwae", the stop-gradient formulations for "stl" and "dreg"), its edge cases, the stored vectors, the solver's and
the ops' surface, and the refusals of the C entry points, which fire in host code before any launch.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import iwae_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NET = dict(cdim=3, zdim=10, channels=(8, 16), image_size=16)
NEW = ("itcv_iwae_sample_fwd", "itcv_iwae_sample_bwd", "itcv_iwae_rows_workspace", "itcv_iwae_rows_fwd",
       "itcv_iwae_rows_bwd", "itcv_iwae_combine_fwd", "itcv_iwae_combine_bwd", "itcv_iwae_accumulate", "itcv_iwae_finalize")
BAR = 1e-12


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def _problem(B, K, D, P, seed, loss_type):
    mu, logvar, eps = R.make_inputs(B, K, D, seed)
    rng = np.random.default_rng(seed + 7)
    x = rng.uniform(0.05, 0.95, size=(B, P))
    W = rng.normal(size=(D, P)) * 0.4                        # the linear stand-in decoder
    return mu.astype(np.float64), logvar.astype(np.float64), eps.astype(np.float64), x, W


# ---- the restatement against autograd ----------------------------------------------------------------------------------
@pytest.mark.parametrize("estimator", R.ESTIMATORS)
@pytest.mark.parametrize("loss_type", R.LOSS_TYPES)
@pytest.mark.parametrize("B, K, D, P", [(3, 1, 5, 7), (3, 4, 5, 7), (1, 6, 2, 3), (4, 2, 1, 1)])
def test_restatement_equals_torch_float64_autograd(B, K, D, P, loss_type, estimator):
    beta_rec, beta_kl, g = 0.75, 0.5, 1.7
    mu, logvar, eps, x, W = _problem(B, K, D, P, 11 + B + K, loss_type)
    ref = R.full(mu, logvar, eps, x, W, beta_rec, beta_kl, loss_type, estimator, g=g)
    tm, tl, tw = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (mu, logvar, W))

    def decode(z):
        pre = z @ tw
        return torch.sigmoid(pre) if loss_type == "bce" else pre

    surrogate, value = R.torch_loss(tm, tl, torch.tensor(eps), torch.tensor(x), decode, beta_rec, beta_kl, loss_type,
                                    estimator)
    dmu, dlv, dw = torch.autograd.grad(g * surrogate, (tm, tl, tw))
    for k in ("loss", "rec", "kl", "bound", "ess"):
        assert rel(ref[k], float(value[k])) <= BAR, (k, ref[k], float(value[k]))
    assert rel(ref["dmu"], dmu.numpy()) <= BAR
    assert rel(ref["dlogvar"], dlv.numpy()) <= BAR
    assert rel(ref["ddecoder"], dw.numpy()) <= BAR        # the decoder's gradient keeps the single weight under all three
    if estimator == "dreg":          # rows decoded independently: the weight-by-row form is the same gradient
        tm2, tl2 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (mu, logvar))
        s2, _ = R.torch_loss(tm2, tl2, torch.tensor(eps), torch.tensor(x), decode, beta_rec, beta_kl, loss_type, "dreg",
                             dreg_by_row=True)
        dmu2, dlv2, dw2 = torch.autograd.grad(g * s2, (tm2, tl2, tw))
        assert rel(dmu2.numpy(), dmu.numpy()) <= BAR and rel(dlv2.numpy(), dlv.numpy()) <= BAR
        assert rel(dw2.numpy(), dw.numpy()) <= BAR
    if estimator != "iwae":
        plain = R.full(mu, logvar, eps, x, W, beta_rec, beta_kl, loss_type, "iwae", g=g)
        assert np.array_equal(plain["ddecoder"], ref["ddecoder"]) and plain["loss"] == ref["loss"]
        if K > 1:
            assert rel(plain["dmu"], ref["dmu"]) > 1e-6


def test_restatement_edges():
    mu, logvar, eps, x, W = _problem(3, 1, 5, 7, 3, "mse")
    a = R.full(mu, logvar, eps, x, W, 0.75, 0.5, "mse", "stl")
    b = R.full(mu, logvar, eps, x, W, 0.75, 0.5, "mse", "dreg")
    assert np.array_equal(a["dmu"], b["dmu"]) and np.array_equal(a["dlogvar"], b["dlogvar"])      # K = 1: they coincide
    out = R.combine(a["rows"], a["lat"], 3, 0.75, 0.5)
    assert np.array_equal(out["bound_b"], out["logw"]) and np.array_equal(out["w"], np.ones(3))
    assert np.array_equal(out["ess_b"], np.ones(3))
    # K = 1 with "iwae" is the beta-VAE step with a sampled KL: the mean over eps of lat is the analytic KL
    m, l = mu[:1], logvar[:1]
    e = np.random.default_rng(0).normal(size=(200000, 5))
    _, lat = R.sample(np.repeat(m, 200000, 0), np.repeat(l, 200000, 0), e)
    kl = -0.5 * (1.0 + l - m * m - np.exp(l)).sum()
    assert abs(lat.mean() - kl) <= 0.02 * abs(kl)
    # equal weights: ess = K; one dominating sample with gaps above 800: a max-shifted logsumexp is needed and gives it
    rows = np.full(12, 40.0)
    eq = R.combine(rows, np.zeros(12), 3, 1.0, 1.0)
    assert np.allclose(eq["ess_b"], 4.0, rtol=1e-15) and np.allclose(eq["bound_b"], -40.0, rtol=1e-15)
    rows = np.full(12, 2000.0)
    rows[:3] = 1000.0
    dom = R.combine(rows, np.zeros(12), 3, 1.0, 1.0)
    assert np.isfinite(dom["bound_b"]).all() and np.allclose(dom["bound_b"], -1000.0 - np.log(4.0))
    assert np.allclose(dom["ess_b"], 1.0) and dom["w"][:3].tolist() == [1.0] * 3
    # the bound never decreases in K in expectation; on one draw it is at least the mean of logw (Jensen), per image
    rows = np.random.default_rng(1).uniform(20, 60, 64 * 5)
    full = R.combine(rows, np.zeros(64 * 5), 5, 1.0, 1.0)
    assert (full["bound_b"] >= full["elbo_b"]).all()


def test_streaming_form_equals_the_one_shot_combine():
    B, K = 5, 130
    rng = np.random.default_rng(5)
    rows, lat = rng.uniform(20, 60, K * B), rng.normal(size=K * B) * 3
    want = R.combine(rows, lat, B, 0.75, 0.5)
    for chunk in (1, 7, 64, 130):
        state = None
        for k0 in range(0, K, chunk):
            k1 = min(K, k0 + chunk)
            state = R.accumulate(state, rows[k0 * B:k1 * B], lat[k0 * B:k1 * B], B, 0.75, 0.5)
        log_px, elbo, ess = R.finalize(state)
        assert (state["n"] == K).all()
        assert rel(log_px, want["bound_b"]) <= 1e-13 and rel(ess, want["ess_b"]) <= 1e-12
        assert rel(elbo, want["elbo_b"]) <= 1e-13


def test_stored_vectors():
    import sys
    sys.path.insert(0, GOLDEN)
    keep, sys.dont_write_bytecode = sys.dont_write_bytecode, True         # no cache directory next to the stored vectors
    try:
        import make_golden_iwae as M
    finally:
        sys.path.remove(GOLDEN)
        sys.dont_write_bytecode = keep
    g = np.load(os.path.join(GOLDEN, "iwae.npz"))
    assert g["shapes"].tolist() == [list(s) for s in M.SHAPES] and g["hp"].tolist() == [M.BETA_REC, M.BETA_KL]
    assert os.path.getsize(os.path.join(GOLDEN, "iwae.npz")) < 1 << 20
    full = 0
    for B, K, D in M.SHAPES:
        p = f"{B}x{K}x{D}:"
        seed = int(g[p + "seed"])
        mu, logvar, eps = R.make_inputs(B, K, D, seed)
        rows = M.make_rows(B, K, seed)
        assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in (mu, logvar, eps, rows)])
        _, lat = R.sample(mu, logvar, eps)
        ref = R.combine(rows, lat, B, M.BETA_REC, M.BETA_KL)
        for k in ("loss", "rec", "kl", "bound", "ess"):
            assert rel(ref[k], g[p + k]) <= BAR, (p, k)
        if p + "mu" in g.files:
            full += 1
            assert np.array_equal(g[p + "mu"], mu) and np.array_equal(g[p + "rows"], rows)
            assert rel(lat, g[p + "lat"]) <= BAR and rel(ref["w"], g[p + "w"]) <= BAR
    assert full >= 5
    ks, bs, ds = ({s[i] for s in M.SHAPES} for i in (1, 0, 2))
    assert {1, 2, 3, 63, 64, 65, 1024} <= ks and {1, 3, 4, 5, 65} <= bs and {1, 31, 32, 33, 64, 65, 512} <= ds


# ---- the solver's surface -------------------------------------------------------------------------------------------------
def _solver(**kw):
    import models
    import solvers
    m = models.SoftIntroVAE(arch="conv", **NET)

    class DS:
        def __len__(self):
            return 100

    return solvers.IWAESolver(DS(), m, 4, torch.optim.Adam(m.encoder.parameters()),
                              torch.optim.Adam(m.decoder.parameters()), "mse", 0.5, 0.75, torch.device("cpu"), False, None,
                              **kw)


def test_solver_class_defaults_and_graph_key():
    import solvers
    from solvers.hyper import Choice
    from solvers.iwae import IWAE_ESTIMATORS, IWAESolver
    assert solvers.IWAESolver is IWAESolver and IWAESolver.__mro__[1] is solvers.VAESolver
    assert IWAE_ESTIMATORS == ("iwae", "stl", "dreg") and isinstance(IWAESolver.estimator, Choice)
    assert IWAESolver.train_step is solvers.VAESolver.train_step
    assert IWAESolver._device_step is solvers.VAESolver._device_step
    assert IWAESolver._total_loss is not solvers.VAESolver._total_loss
    doc = " ".join(solvers.iwae.__doc__.split())
    assert "``compute_kl_loss``" in doc and "are not called by this step" in doc
    s = _solver()
    assert (s.num_samples, s.estimator) == (8, "iwae")
    base = solvers.VAESolver._graph_key_extra(s)
    assert s._graph_key_extra() == base + (8, "iwae")
    s.num_samples, s.estimator = 3, "dreg"
    assert s._graph_key_extra() == base + (3, "dreg")
    assert s._extra_results(1.5, 2.5) == dict(bound=1.5, ess=2.5)
    # the seam's default is today's sum
    v = solvers.VAESolver._total_loss(s, torch.tensor(2.0), torch.tensor(3.0))
    assert float(v) == pytest.approx(s.scale * 5.0)


def test_solver_refusals():
    for bad in (0, -1, 1025, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="num_samples"):
            _solver(num_samples=bad)
    for bad in ("vimco", None, 1):
        with pytest.raises(ValueError, match="estimator"):
            _solver(estimator=bad)
    s = _solver()
    with pytest.raises(ValueError, match="estimator"):
        s.estimator = "path"


def test_unknown_extra_score_lists_log_likelihood():
    s = _solver()

    class W:
        pass

    s.writer, s.extra_scores, s.test_iter = W(), ("log_likelihood", "nope"), 1
    with pytest.raises(ValueError, match=r"unknown score\(s\) \['nope'\].*'log_likelihood'"):
        s.write_disentanglemnt_scores(0)


# ---- the ops refuse before any device call --------------------------------------------------------------------------------
def test_op_value_errors_come_before_any_device_call():
    import ops
    from hipvae import abi
    from hipvae import functional as HF
    assert ops.IWAE_ESTIMATORS == ("iwae", "stl", "dreg")
    mu = torch.zeros(4, 10)
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="1 <= K <= 1024"):
            ops.iwae_sample(mu, mu, bad)
    with pytest.raises(ValueError, match="share one"):
        ops.iwae_sample(mu, torch.zeros(4, 9), 2)
    with pytest.raises(ValueError, match="1 <= D <= 512"):
        ops.iwae_sample(torch.zeros(2, 513), torch.zeros(2, 513), 2)
    with pytest.raises(ValueError, match=r"eps must be \[K B, D\] = \(8, 10\)"):
        ops.iwae_sample(mu, mu, 2, eps=torch.zeros(4, 10))
    with pytest.raises(abi.HipExtensionError, match="device tensors"):
        ops.iwae_sample(mu, mu, 2)
    sample = HF.IwaeSample.__new__(HF.IwaeSample)
    sample.B, sample.K = 4, 2
    x, recon = torch.zeros(4, 3, 2, 2), torch.zeros(8, 3, 2, 2)
    with pytest.raises(ValueError, match="estimator must be one of"):
        ops.iwae_bound(x, recon, sample, 1.0, 1.0, estimator="vimco")
    with pytest.raises(NotImplementedError):
        ops.iwae_bound(x, recon, sample, 1.0, 1.0, loss_type="huber")
    with pytest.raises(ValueError, match="what iwae_sample returned"):
        ops.iwae_bound(x, recon, object(), 1.0, 1.0)
    with pytest.raises(ValueError, match="K B = 8"):
        ops.iwae_bound(x, recon[:4], sample, 1.0, 1.0)
    with pytest.raises(ValueError, match="finite"):
        ops.iwae_bound(x, recon, sample, float("nan"), 1.0)
    with pytest.raises(abi.HipExtensionError, match="device tensors"):
        ops.iwae_bound(x, recon, sample, 1.0, 1.0)
    from hipvae import likelihood
    with pytest.raises(ValueError, match="num_samples"):
        likelihood.compute_log_likelihood([], None, num_samples=0)
    with pytest.raises(NotImplementedError):
        likelihood.compute_log_likelihood([], None, loss_type="huber")
    assert "only" in likelihood.compute_log_likelihood.__doc__.lower() and "bce" in likelihood.compute_log_likelihood.__doc__


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_library_and_makefile():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert abi.ABI_VERSION == 4 and abi.lib.itcv_abi_version() == 4
    makefile = open(os.path.join(abi.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\biwae\.hip\b", makefile, re.M)
    src = open(os.path.join(abi.CSRC, "iwae.hip")).read()
    assert "atomic" not in src.split("namespace itcv")[1].lower()
    ws = abi.lib.itcv_iwae_rows_workspace
    # one fp64 partial per row and slice, the slicing of itcv_recon_workspace at K B rows
    assert ws(4, 3, 3072) == abi.lib.itcv_recon_workspace(12, 3072) and ws(1, 1, 1) == 8
    assert ws(64, 8, 12288) == abi.lib.itcv_recon_workspace(512, 12288)
    assert ws(0, 1, 8) == ws(1, 0, 8) == ws(1, 1025, 8) == ws(1 << 15, 1024, 8) == ws(2, 2, 0) == 0


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
P = [0x10000 * (k + 1) for k in range(12)]
INF, NAN = float("inf"), float("nan")


def _sfwd(mu=P[0], ldm=10, lv=P[1], ldl=10, eps=P[2], lde=10, z=P[3], lat=P[4], B=4, K=3, D=10):
    return ("itcv_iwae_sample_fwd", mu, ldm, lv, ldl, eps, lde, z, lat, B, K, D, None)


def _sbwd(dz=P[0], ldz=10, h=P[1], wt=P[2], mu=P[3], ldm=10, lv=P[4], ldl=10, eps=P[5], lde=10, dmu=P[6], dlv=P[7], B=4, K=3,
          D=10, est=0):
    return ("itcv_iwae_sample_bwd", dz, ldz, h, wt, mu, ldm, lv, ldl, eps, lde, dmu, dlv, B, K, D, est, None)


def _rfwd(x=P[0], recon=P[1], rows=P[2], B=4, K=3, Pn=64, lt=0, ws=P[3], nws=1 << 20):
    return ("itcv_iwae_rows_fwd", x, recon, rows, B, K, Pn, lt, ws, nws, None)


def _rbwd(x=P[0], recon=P[1], g=P[2], d=P[3], B=4, K=3, Pn=64, lt=0):
    return ("itcv_iwae_rows_bwd", x, recon, g, d, B, K, Pn, lt, None)


def _cfwd(rows=P[0], lat=P[1], br=1.0, bk=1.0, wt=P[2], img=P[3], out=P[4], terms=P[5], B=4, K=3):
    return ("itcv_iwae_combine_fwd", rows, lat, br, bk, wt, img, out, terms, B, K, None)


def _cbwd(g=P[0], wt=P[1], br=1.0, bk=1.0, gr=P[2], gl=P[3], B=4, K=3):
    return ("itcv_iwae_combine_bwd", g, wt, br, bk, gr, gl, B, K, None)


def _acc(rows=P[0], lat=P[1], br=1.0, bk=1.0, state=P[2], B=4, K=3):
    return ("itcv_iwae_accumulate", rows, lat, br, bk, state, B, K, None)


def _fin(state=P[0], a=P[1], b=P[2], c=P[3], B=4):
    return ("itcv_iwae_finalize", state, a, b, c, B, None)


@pytest.mark.parametrize("args, msg", [
    (_sfwd(mu=None), "NULL"), (_sfwd(lv=None), "NULL"), (_sfwd(eps=None), "NULL"), (_sfwd(z=None), "NULL"),
    (_sfwd(lat=None), "NULL"), (_sfwd(B=0), "B = 0"), (_sfwd(K=0), "K = 0 samples is outside 1..1024"),
    (_sfwd(K=1025), "K = 1025"), (_sfwd(B=1 << 15, K=1024), "exceed 2^24"), (_sfwd(D=0), "D = 0 is outside 1..512"),
    (_sfwd(D=513, ldm=513, ldl=513, lde=513), "D = 513"), (_sfwd(ldm=9), "mu's row stride of 9 is below D = 10"),
    (_sfwd(ldl=9), "logvar's row stride of 9"), (_sfwd(lde=9), "eps's row stride of 9"),
    (_sbwd(dz=None), "NULL"), (_sbwd(h=None), "NULL"), (_sbwd(wt=None, est=2), "NULL"), (_sbwd(dmu=None), "NULL"),
    (_sbwd(dlv=None), "NULL"), (_sbwd(K=1025), "K = 1025"), (_sbwd(D=513, ldm=513, ldl=513, lde=513, ldz=513), "D = 513"),
    (_sbwd(ldz=9), "dz's row stride of 9"), (_sbwd(ldm=3), "mu's row stride of 3"), (_sbwd(est=3), "estimator 3"),
    (_sbwd(est=-1), "estimator -1"), (_sbwd(B=1 << 20, K=17), "exceed 2^24"),
    (_rfwd(x=None), "NULL"), (_rfwd(recon=None), "NULL"), (_rfwd(rows=None), "NULL"), (_rfwd(ws=None), "NULL"),
    (_rfwd(nws=8 * 11), "workspace"), (_rfwd(Pn=0), "P = 0"), (_rfwd(lt=3), "unknown loss type 3"), (_rfwd(K=0), "K = 0"),
    (_rfwd(B=-1), "B = -1"), (_rbwd(x=None), "NULL"), (_rbwd(g=None), "NULL"), (_rbwd(d=None), "NULL"),
    (_rbwd(lt=-1), "unknown loss type -1"), (_rbwd(K=2000), "K = 2000"), (_rbwd(Pn=0), "P = 0"),
    (_cfwd(rows=None), "NULL"), (_cfwd(lat=None), "NULL"), (_cfwd(wt=None), "NULL"), (_cfwd(img=None), "NULL"),
    (_cfwd(out=None), "NULL"), (_cfwd(terms=None), "NULL"), (_cfwd(br=NAN), "finite"), (_cfwd(bk=INF), "finite"),
    (_cfwd(K=0), "K = 0"), (_cfwd(B=0), "B = 0"), (_cbwd(g=None), "NULL"), (_cbwd(gr=None), "NULL"), (_cbwd(gl=None), "NULL"),
    (_cbwd(br=INF), "finite"), (_cbwd(K=1025), "K = 1025"),
    (_acc(rows=None), "NULL"), (_acc(state=None), "NULL"), (_acc(bk=NAN), "finite"), (_acc(K=1025), "K = 1025"),
    (_acc(B=0), "B = 0"), (_fin(state=None), "NULL"), (_fin(c=None), "NULL"), (_fin(B=0), "B = 0"),
])
def test_refusals_fire_before_any_launch(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(abi.HipExtensionError):
        abi.call(*args)


def test_weights_are_asked_for_by_dreg_alone():
    from hipvae import abi
    for est in (0, 1):
        args = _sbwd(wt=None, est=est, ldz=9)
        assert getattr(abi.lib, args[0])(*args[1:]) != 0
        assert "row stride of 9" in abi.last_error()
