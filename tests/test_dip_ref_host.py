"""CPU-only tests of the DIP-VAE KL hook: the fp64 restatement (tests/dip_ref.py) against central differences and against
its own E[mu mu^T] - m m^T form, the stored vectors (golden/dip.npz), the surface of DIPSolver / IntroDIPSolver, and what
the new entry points refuse before any launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
NEW = ("itcv_dip_kl_workspace", "itcv_dip_kl_fwd", "itcv_dip_kl_bwd")


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("beta, off, Bl", [(0.0, 0, None), (0.5, 0, None), (0.5, 2, 3)])
def test_gradients_agree_with_central_differences(kind, beta, off, Bl):
    mu, lv = R.make_inputs(7, 5, seed=3)
    ref = R.dip(mu, lv, kind, 3.0, 7.0, beta, off, Bl)
    dmu, dlv = R.central_differences(mu, lv, kind, 3.0, 7.0, beta, off, Bl)
    e_mu, e_lv = np.abs(ref["dmu"] - dmu).max(), np.abs(ref["dlogvar"] - dlv).max()
    print(kind, beta, "dmu", e_mu, "dlogvar", e_lv)
    assert e_mu <= 1e-7 and e_lv <= 1e-7
    assert np.array_equal(ref["W"], ref["W"].T)
    if kind == "i" and beta == 0.0:
        assert not ref["dlogvar"].any()


@pytest.mark.parametrize("kind", R.KINDS)
def test_centred_and_moment_forms_agree_in_fp64(kind):
    mu, lv = R.make_inputs(64, 16, seed=4)
    mu, lv = mu.astype(np.float64), lv.astype(np.float64)
    a, b = R.covariance(mu, lv, kind, True), R.covariance(mu, lv, kind, False)
    print(kind, np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-12
    la = R.dip(mu, lv, kind, 3.0, 7.0, 0.5, centred=True)["loss"]
    lb = R.dip(mu, lv, kind, 3.0, 7.0, 0.5, centred=False)["loss"]
    assert abs(la - lb) <= 1e-12 * abs(la)


def test_moment_form_cancels_in_fp32():
    """Why the kernel uses the centred form: with a column offset of 1000 standard deviations the squares are 10^6 times
    the covariance, 2^-24 of them is several percent of it and the fp32 moment form loses it; the centred form keeps fp32
    accuracy."""
    rng = np.random.default_rng(0)
    mu = (rng.normal(size=(64, 4)) * 0.001 + 1.0).astype(np.float32)
    want = R.covariance(mu, mu, "i")
    m = mu.mean(0, dtype=np.float32)
    moment = (mu.T @ mu / np.float32(64) - np.outer(m, m)).astype(np.float32)
    X = mu - m
    centred = (X.T @ X / np.float32(64)).astype(np.float32)
    scale = np.abs(want).max()
    assert np.abs(centred - want).max() <= 1e-5 * scale < 1e-2 * scale < np.abs(moment - want).max()


def test_torch_form_equals_numpy_form():
    mu, lv = R.make_inputs(9, 6, seed=5)
    for kind in R.KINDS:
        ref = R.dip(mu, lv, kind, 3.0, 7.0, 0.5)
        tm, tl = (torch.from_numpy(a).double().requires_grad_(True) for a in (mu, lv))
        loss = R.torch_hook(tm, tl, kind, 3.0, 7.0, 0.5)
        loss.backward()
        assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
        assert np.abs(tm.grad.numpy() - ref["dmu"]).max() <= 1e-12 * np.abs(ref["dmu"]).max()
        assert np.abs(tl.grad.numpy() - ref["dlogvar"]).max() <= 1e-12 * max(np.abs(ref["dlogvar"]).max(), 1e-300)


def test_shard_algebra_of_the_restatement():
    """The mean over equal shards of (global regulariser + shard KL) is the single-rank hook, in value and gradients."""
    mu, lv = R.make_inputs(64, 16, seed=6)
    one = R.dip(mu, lv, "ii", 3.0, 7.0, 0.5)
    parts = [R.dip(mu, lv, "ii", 3.0, 7.0, 0.5, 8 * r, 8) for r in range(8)]
    assert abs(np.mean([p["loss"] for p in parts]) - one["loss"]) <= 1e-12 * abs(one["loss"])
    for k in ("dmu", "dlogvar"):
        assert np.abs(np.mean([p[k] for p in parts], 0) - one[k]).max() <= 1e-12 * np.abs(one[k]).max()


def test_stored_vectors():
    g = np.load(os.path.join(GOLDEN, "dip.npz"))
    lam_od, lam_d, beta = g["hp"]
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    for must in [(2, 1), (2, 3), (3, 64), (35, 10), (64, 128), (33, 130), (65, 65), (512, 128), (16, 300), (7, 512)]:
        assert must in shapes
    full = 0
    for Bt, D in shapes:
        for kind in R.KINDS:
            p = f"{Bt}x{D}:{kind}:"
            mu, lv = R.make_inputs(Bt, D, int(g[p + "seed"]))
            assert mu.dtype == lv.dtype == np.float32
            assert np.array_equal(g[p + "checksum"], [mu.astype(np.float64).sum(), lv.astype(np.float64).sum()])
            ref = R.dip(mu, lv, kind, lam_od, lam_d, beta)
            assert abs(ref["loss"] - float(g[p + "loss"])) <= 1e-12 * abs(ref["loss"])
            assert np.abs(ref["terms"] - g[p + "terms"]).max() <= 1e-12 * np.abs(ref["terms"]).max()
            if p + "mu" in g.files:
                full += 1
                assert np.array_equal(g[p + "mu"], mu) and np.array_equal(g[p + "logvar"], lv)
                for k in ("W", "dmu", "dlogvar"):
                    assert np.abs(ref[k] - g[p + k]).max() <= 1e-12 * max(np.abs(ref[k]).max(), 1e-300), (p, k)
            # the offsets make the columns' means several standard deviations: the case the centred form is for
            if D >= 3 and Bt >= 16:
                assert np.abs(mu.mean(0)).max() > 2 * mu.std(0).min()
    assert full >= 8


# ---- the solvers' surface -------------------------------------------------------------------------------------------
def _solver(cls, **kw):
    import models
    torch.manual_seed(0)
    m = models.SoftIntroVAE(arch="conv", **TINY)

    class DS:
        def __len__(self):
            return 100

    args = [DS(), m, 8, torch.optim.Adam(m.encoder.parameters()), torch.optim.Adam(m.decoder.parameters()), "mse",
            0.5, 0.75]
    if cls.__name__.startswith("Intro"):
        args += [512.0, 1e-8]
    return cls(*args, torch.device("cpu"), False, None, **kw)


def _classes():
    from solvers.dip import DIPSolver, IntroDIPSolver
    return DIPSolver, IntroDIPSolver


def test_solver_defaults_and_lambda_d_convention():
    from solvers import IntroSolver, VAESolver
    DIPSolver, IntroDIPSolver = _classes()
    assert issubclass(DIPSolver, VAESolver) and issubclass(IntroDIPSolver, IntroSolver)
    for cls in _classes():
        for name, default in (("dip_type", "i"), ("lambda_od", 10.0), ("lambda_d", None)):
            p = inspect.signature(cls.__init__).parameters[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
        sig = inspect.signature(cls.compute_kl_loss)
        assert list(sig.parameters) == ["self", "z", "mu", "logvar", "reduce", "beta", "write"]
        s = _solver(cls)
        assert (s.dip_type, s.lambda_od, s.lambda_d) == ("i", 10.0, 100.0)      # the library's sweep: 10 lambda_od for "i"
        s = _solver(cls, dip_type="ii", lambda_od=4)
        assert (s.dip_type, s.lambda_od, s.lambda_d) == ("ii", 4.0, 4.0)        # ... and lambda_od for "ii"
        s.lambda_od = 6
        assert s.lambda_d == 6.0                                                # None follows lambda_od
        s.dip_type = "i"
        assert s.lambda_d == 60.0
        s.lambda_d = 2.5
        s.lambda_od = 1.0
        assert (s.lambda_od, s.lambda_d) == (1.0, 2.5)
        s.lambda_d = None
        assert s.lambda_d == 10.0


def test_solver_validation_on_every_assignment():
    for cls in _classes():
        for bad in ("I", "iii", "", None, 1):
            with pytest.raises(ValueError, match="dip_type"):
                _solver(cls, dip_type=bad)
        for bad in (-1.0, float("nan"), float("inf"), "3", None, True):
            with pytest.raises(ValueError, match="lambda_od"):
                _solver(cls, lambda_od=bad)
        for bad in (-0.5, float("nan"), float("-inf"), "3"):
            with pytest.raises(ValueError, match="lambda_d"):
                _solver(cls, lambda_d=bad)
        s = _solver(cls, dip_type="ii", lambda_od=2.0, lambda_d=3.0)
        with pytest.raises(ValueError, match="dip_type"):
            s.dip_type = "II"
        with pytest.raises(ValueError, match="lambda_od"):
            s.lambda_od = -2.0
        with pytest.raises(ValueError, match="lambda_d"):
            s.lambda_d = float("nan")
        assert (s.dip_type, s.lambda_od, s.lambda_d) == ("ii", 2.0, 3.0)


def test_graph_key_holds_the_kind_and_both_lambdas():
    from solvers import IntroSolver, VAESolver
    for cls, step in zip(_classes(), (VAESolver, IntroSolver)):
        s = _solver(cls, lambda_od=2.0)
        base = tuple(step._graph_key_extra(s))
        assert s._graph_key_extra() == base + ("i", 2.0, 20.0)
        s.lambda_od *= 2
        assert s._graph_key_extra() == base + ("i", 4.0, 40.0)
        s.dip_type = "ii"
        assert s._graph_key_extra() == base + ("ii", 4.0, 4.0)


def test_reduce_none_and_sum_dispatch_to_the_base_hook(monkeypatch):
    from solvers.vae import VAESolver
    calls = []
    monkeypatch.setattr(VAESolver, "compute_kl_loss",
                        lambda self, z, mu, logvar, reduce="mean", beta=None, write=False:
                        calls.append((reduce, beta, write)) or "base")
    mu, lv = torch.zeros(4, 10), torch.zeros(4, 10)
    for cls in _classes():
        s = _solver(cls)
        assert s.compute_kl_loss(None, mu, lv, reduce="none", beta=512.0) == "base"
        assert s.compute_kl_loss(None, mu, lv, "sum") == "base"
    assert calls == [("none", 512.0, False), ("sum", None, False)] * 2


def test_cpu_tensors_raise():
    import ops
    from hipvae import abi
    mu, lv = torch.zeros(4, 10), torch.zeros(4, 10)
    with pytest.raises(abi.HipExtensionError):
        ops.dip_kl_loss(mu, lv, 1.0, 1.0, 1.0)
    with pytest.raises(abi.HipExtensionError):
        ops.dip_regularizer(mu, lv, 1.0, 1.0, "ii")
    for cls in _classes():
        with pytest.raises(abi.HipExtensionError):
            _solver(cls).compute_kl_loss(None, mu, lv)
    with pytest.raises(ValueError, match="kind"):
        ops.dip_kl_loss(mu, lv, 1.0, 1.0, 1.0, kind="iii")
    with pytest.raises(ValueError, match="together"):
        ops.dip_kl_loss(mu, lv, 1.0, 1.0, 1.0, mu_all=mu)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_library_and_makefile():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert abi.ABI_VERSION == 4 and abi.lib.itcv_abi_version() == 4
    assert re.search(r"#define\s+ITCV_ABI_VERSION\s+4\b", header)
    makefile = open(os.path.join(abi.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bdip\.hip\b", makefile, re.M)
    assert os.path.exists(os.path.join(abi.CSRC, "dip.hip"))
    # the workspace holds two fp64 partials per 32 x 32 tile of C and does not depend on the batch
    assert abi.lib.itcv_dip_kl_workspace(64, 128) == abi.lib.itcv_dip_kl_workspace(4096, 128) == 4 * 4 * 2 * 8
    assert abi.lib.itcv_dip_kl_workspace(64, 512) == 16 * 16 * 2 * 8
    assert abi.lib.itcv_dip_kl_workspace(64, 1) == abi.lib.itcv_dip_kl_workspace(64, 32) == 16
    assert abi.lib.itcv_dip_kl_workspace(64, 33) == 64
    assert abi.lib.itcv_dip_kl_workspace(64, 513) == abi.lib.itcv_dip_kl_workspace(1, 8) == 0


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
P = [0x10000 * (k + 1) for k in range(10)]
INF, NAN = float("inf"), float("nan")


def _fwd(mu=P[0], lv=P[1], ld=8, out=P[2], terms=P[3], W=P[4], mean=P[5], Bl=4, Bt=8, off=0, D=8, kind=1, lod=1.0, ld_=1.0,
         ckl=1.0, ws=P[9], nws=1 << 20):
    return ("itcv_dip_kl_fwd", mu, lv, ld, out, terms, W, mean, Bl, Bt, off, D, kind, lod, ld_, ckl, ws, nws, None)


def _bwd(g=P[0], mu=P[1], lv=P[2], ld=8, W=P[3], mean=P[4], dmu=P[5], dlv=P[6], Bl=4, Bt=8, off=0, D=8, kind=1, ckl=1.0):
    return ("itcv_dip_kl_bwd", g, mu, lv, ld, W, mean, dmu, dlv, Bl, Bt, off, D, kind, ckl, None)


@pytest.mark.parametrize("args, msg", [
    (_fwd(mu=None), "NULL"), (_fwd(lv=None), "NULL"), (_fwd(out=None), "NULL"), (_fwd(terms=None), "NULL"),
    (_fwd(W=None), "NULL"), (_fwd(mean=None), "NULL"), (_fwd(ws=None), "workspace"), (_fwd(nws=8), "workspace"),
    (_fwd(Bt=1, Bl=1), "Bt = 1 rows"), (_fwd(Bt=0, Bl=0), "Bt = 0 rows"),
    (_fwd(D=0, ld=0), "D = 0 is outside 1..512"), (_fwd(D=513, ld=513), "D = 513 is outside 1..512"),
    (_fwd(D=-3, ld=-3), "D = -3"),
    (_fwd(off=5), "inside the global batch"), (_fwd(off=-1), "inside the global batch"),
    (_fwd(Bl=9), "inside the global batch"), (_fwd(Bl=0), "inside the global batch"),
    (_fwd(off=2 ** 31 - 1), "inside the global batch"),
    (_fwd(kind=0), "kind 0"), (_fwd(kind=3), "kind 3"),
    (_fwd(lod=-1.0), "lambda"), (_fwd(lod=NAN), "lambda"), (_fwd(lod=INF), "lambda"),
    (_fwd(ld_=-1e-30), "lambda"), (_fwd(ld_=NAN), "lambda"), (_fwd(ld_=INF), "lambda"),
    (_fwd(ckl=NAN), "coef_kl"), (_fwd(ckl=-INF), "coef_kl"),
    (_fwd(ld=9), "row stride 9"), (_fwd(ld=7), "row stride 7"), (_fwd(ld=24), "row stride 24"), (_fwd(ld=0), "row stride 0"),
    (_bwd(g=None), "NULL"), (_bwd(mu=None), "NULL"), (_bwd(lv=None), "NULL"), (_bwd(W=None), "NULL"),
    (_bwd(mean=None), "NULL"), (_bwd(dmu=None), "NULL"), (_bwd(dlv=None), "NULL"),
    (_bwd(Bt=1, Bl=1), "Bt = 1 rows"), (_bwd(D=513, ld=1026), "D = 513"), (_bwd(D=0, ld=0), "D = 0"),
    (_bwd(off=5), "inside the global batch"), (_bwd(Bl=9), "inside the global batch"), (_bwd(kind=4), "kind 4"),
    (_bwd(ckl=NAN), "coef_kl"), (_bwd(ld=12), "row stride 12"),
])
def test_refusals_fire_before_any_launch(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(abi.HipExtensionError):
        abi.call(*args)
