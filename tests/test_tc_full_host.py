"""CPU-only checks of the full beta-TC decomposition loss (solvers/tc.py:91-144): the hook's surface, the ``kl_loss``
option, the host-side argument checks of its C-ABI entries, and the data-parallel packed gather of (mu, logvar) with its
reduce-scatter adjoint on a gloo world of 2 (one collective each way)."""
import inspect
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
NEW = ("itcv_tc_full_fwd", "itcv_tc_full_fwd_workspace", "itcv_tc_full_bwd", "itcv_tc_full_bwd_workspace")


def test_full_hook_surface():
    from solvers.intro_tc import IntroTCSovler
    from solvers.tc import TCSovler
    sig = inspect.signature(TCSovler._compute_kl_loss_full)
    # the reference's parameter list and defaults (solvers/tc.py:91-99)
    assert list(sig.parameters) == ["self", "z", "mu", "logvar", "reduce", "beta", "write"]
    assert [sig.parameters[k].default for k in ("reduce", "beta", "write")] == ["mean", None, False]
    for cls in (TCSovler, IntroTCSovler):
        p = inspect.signature(cls.__init__).parameters["kl_loss"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "simple"
    with pytest.raises(ValueError, match="z"):
        TCSovler._compute_kl_loss_full(object(), None, torch.zeros(2, 3), torch.zeros(2, 3))


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


def test_kl_loss_option_validation():
    from solvers.intro_tc import IntroTCSovler
    from solvers.tc import TCSovler
    for cls in (TCSovler, IntroTCSovler):
        assert _solver(cls).kl_loss == "simple"
        s = _solver(cls, kl_loss="full")
        assert s.kl_loss == "full"
        s.kl_loss = "simple"
        assert s.kl_loss == "simple"
        with pytest.raises(ValueError, match="kl_loss"):
            s.kl_loss = "Full"
        assert s.kl_loss == "simple"
        for bad in ("", "none", None, 1):
            with pytest.raises(ValueError, match="kl_loss"):
                _solver(cls, kl_loss=bad)


def test_new_symbols_in_header_table_and_library():
    import ctypes
    import re
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert abi.lib.itcv_tc_full_fwd_workspace(64, 512, 128) == abi.lib.itcv_tc_fwd_workspace(64, 512, 128) > 0
    assert abi.lib.itcv_tc_full_bwd_workspace(64, 512) == 64 * 512 * 4
    assert abi.lib.itcv_tc_full_bwd_workspace(0, 512) == 0


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
P = [0x10000 * (k + 1) for k in range(12)]


def _fwd(z=P[0], mu=P[1], lv=P[2], ld=8, out=P[3], rows=P[4], Bl=4, Bt=8, off=0, D=8, red=2, ws=P[11]):
    return ("itcv_tc_full_fwd", z, mu, lv, ld, out, rows, None, P[5], P[6], P[7], P[8], P[9], Bl, Bt, off, D, 100,
            1.0, 2.0, 1.0, red, ws, 1 << 20, None)


def _bwd(g=P[0], dz=P[8], ld=8, Bl=4, Bt=8, off=0, D=8, red=2, ws=P[11]):
    return ("itcv_tc_full_bwd", g, P[1], P[2], P[3], ld, P[4], P[5], P[6], P[7], dz, P[9], P[10], Bl, Bt, off, D, 100,
            1.0, 2.0, 1.0, red, ws, 1 << 20, None)


@pytest.mark.parametrize("args, msg", [
    (_fwd(z=None), "NULL"), (_fwd(mu=None), "NULL"), (_fwd(lv=None), "NULL"), (_fwd(out=None), "NULL"),
    (_fwd(rows=None), "NULL"), (_fwd(ws=None), "NULL"),
    (_fwd(D=520, ld=520), "latent size 520 > 512"), (_fwd(Bl=0), "must be positive"),
    (_fwd(off=6), "inside the global batch"), (_fwd(off=-1), "inside the global batch"),
    (_fwd(ld=7), "row stride 7"), (_fwd(red=3), "reduction 3"), (_fwd(red=-1), "reduction -1"),
    (_bwd(g=None), "NULL"), (_bwd(dz=None), "NULL"), (_bwd(D=513, ld=1026), "latent size 513"),
    (_bwd(Bl=9), "inside the global batch"), (_bwd(ld=4), "row stride 4"), (_bwd(red=5), "reduction 5"),
    (_bwd(ws=None), "workspace"), (_bwd(Bt=1, Bl=1), "batch size must be >= 2"),
])
def test_host_side_argument_checks(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(RuntimeError):
        abi.call(*args)


def test_reduce_none_with_null_rows_passes_the_checks_it_needs():
    """rows[] is scratch of the reduced forms only: a NULL rows with reduction 0 is not an argument error (checked up to
    the workspace test, which a NULL workspace then fails -- still before any launch)."""
    from hipvae import abi
    args = list(_fwd(rows=None, red=0, ws=None))
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    assert "NULL" in abi.last_error()
    args = list(_fwd(rows=None, red=0))
    args[-2] = 0                                    # ws_bytes below the workspace query
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    assert "workspace" in abi.last_error()


# ---- data parallelism: one packed all-gather of (mu, logvar), reduce-scatter adjoint -----------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _full_rows(z, mu_all, lv_all, N, off, a, b, c):
    """Rows [off, off + len(z)) of the global batch's a*mi + b*tc + c*dwkl (solvers/tc.py:104-121 with weights), built
    from the oracle's pieces: ops.py:24-29 density with the variance of component i, stratified sampler."""
    from oracle import latent_math as lm
    Bl = z.shape[0]
    mu_d, lv_d = mu_all[off:off + Bl], lv_all[off:off + Bl]
    lcx = lm.log_density_plain(z, mu_d, lv_d).sum(1)
    lpz = lm.log_density_plain(z, torch.zeros_like(z), torch.zeros_like(z)).sum(1)
    lp = lm.log_density_plain(z.unsqueeze(1), mu_all.unsqueeze(0), lv_all.unsqueeze(0))
    lw = lm.log_importance_weights(mu_all.shape[0], N, z.dtype)[off:off + Bl]
    prodm = torch.logsumexp(lw.unsqueeze(2) + lp, 1).sum(1)
    logqz = torch.logsumexp(lw + lp.sum(2), 1)
    return a * (lcx - logqz) + b * (logqz - prodm) + c * (prodm - lpz)


def _dp_worker(rank, world, port, out):
    for p in (os.path.join(ROOT, "intro-tc-vae_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hipvae import ddp
    from oracle import latent_math as lm
    ddp.init(sync_bn=False)
    torch.manual_seed(0)
    B, D, N = 12, 7, 500
    a, b, c = 1.0, 6.0, 1.0
    mu = torch.randn(B, D, dtype=torch.float64)
    lv = -2 + 2 * torch.randn(B, D, dtype=torch.float64)
    z = mu + torch.randn(B, D, dtype=torch.float64) * (0.5 * lv).exp()
    z[0, :3] += 40.0                                    # rows where the -50 clamp is active
    Bl = B // world
    sl = slice(rank * Bl, (rank + 1) * Bl)
    zf, mf, lf = (t.clone().requires_grad_(True) for t in (z, mu, lv))
    full = _full_rows(zf, mf, lf, N, 0, a, b, c)
    full.mean().backward()
    # with a = c = 1 the rows are the oracle's own decomposition, recombined as the reference does
    mi, tc, dw = lm.decomposition(z, mu, lv, N)
    ok = torch.allclose(_full_rows(z, mu, lv, N, 0, 1.0, b, 1.0), mi + b * tc + dw, rtol=1e-12, atol=1e-9)
    calls = {"gather": 0, "reduce": 0}
    ag, ar = dist.all_gather, dist.all_reduce

    def count(name, f):
        def g(*x, **k):
            calls[name] += 1
            return f(*x, **k)
        return g

    dist.all_gather, dist.all_reduce = count("gather", ag), count("reduce", ar)
    try:
        zl, ml, ll = (t[sl].clone().requires_grad_(True) for t in (z, mu, lv))
        mu_all, lv_all = ddp.all_gather_mu_logvar(ml, ll)
        assert calls == {"gather": 1, "reduce": 0}
        assert mu_all.shape == lv_all.shape == (B, D) and ddp.row_offset(Bl) == rank * Bl
        loc = _full_rows(zl, mu_all, lv_all, N, ddp.row_offset(Bl), a, b, c)
        loc.mean().backward()
        assert calls == {"gather": 1, "reduce": 1}      # one collective each way for mu AND logvar
    finally:
        dist.all_gather, dist.all_reduce = ag, ar
    ok = ok and torch.allclose(loc, full[sl].detach(), rtol=1e-12, atol=1e-9)
    # d(global mean)/d(local leaf) = (1/world) * d(sum_r local mean_r)/d leaf
    for got, ref in ((zl.grad, zf.grad[sl]), (ml.grad, mf.grad[sl]), (ll.grad, lf.grad[sl])):
        ok = ok and torch.allclose(got / world, ref, rtol=1e-10, atol=1e-12)
    out[rank] = bool(ok)
    ddp.shutdown()
    dist.destroy_process_group()


def test_packed_gather_reproduces_full_batch_loss_and_gradients():
    world, port = 2, _free_port()
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_dp_worker, args=(world, port, out), nprocs=world, join=True)
        assert dict(out) == {0: True, 1: True}


def test_single_rank_gather_is_the_identity():
    from hipvae import ddp
    assert ddp.get() is None
    mu, lv = torch.zeros(3, 4), torch.ones(3, 4)
    m2, l2 = ddp.all_gather_mu_logvar(mu, lv)
    assert m2 is mu and l2 is lv
