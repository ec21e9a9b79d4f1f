"""CPU-only tests of the sliced-Wasserstein KL hook (SWAE): the fp64 restatement (tests/sw_ref.py) against its torch form
and central differences, its closed forms (equal sets, a shift, a scaling, a permutation, duplicated rows), the stored
vectors (golden/sw.npz), the surface of SWAESolver / IntroSWAESolver, and what the new entry points refuse before any
launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import sw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
NEW = ("itcv_sw_lds_rows", "itcv_sw_workspace", "itcv_sw_kl_fwd", "itcv_sw_kl_bwd")


# ---- the restatement against itself ----------------------------------------------------------------------------------
def test_torch_form_equals_numpy_form():
    z, prior, t, mu, lv = R.make_inputs(9, 6, 7, seed=5)
    ref = R.sw(z, prior, t, mu, lv, 3.0, 0.5)
    tz, tp, tt, tm, tl = (torch.from_numpy(a).double().requires_grad_(True) for a in (z, prior, t, mu, lv))
    loss = R.torch_hook(tz, tp, tt, tm, tl, 3.0, 0.5)
    loss.backward()
    assert tp.grad is None and tt.grad is None
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    for got, k in ((tz.grad, "dz"), (tm.grad, "dmu"), (tl.grad, "dlogvar")):
        assert np.abs(got.numpy() - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), k


@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_gradients_agree_with_central_differences(beta):
    """The value is piecewise quadratic in z: inside one cell of the sort the central difference of a quadratic is exact
    up to rounding.  The step is far below the smallest projection gap, so no order changes."""
    z, prior, t, mu, lv = R.make_inputs(7, 5, 6, seed=3)
    mu, lv = mu[:4], lv[:4]                                         # the local rows need not be the whole batch
    u = R.projections(z, prior, t)[0]
    gap = R.min_gap(z, prior, t) * np.abs(u).max()
    step = 1e-6
    assert step <= 1e-3 * gap, gap
    ref = R.sw(z, prior, t, mu, lv, 3.0, beta)
    dz, dmu, dlv = R.central_differences(z, prior, t, mu, lv, 3.0, beta, step)
    errs = [np.abs(ref["dz"] - dz).max(), np.abs(ref["dmu"] - dmu).max(), np.abs(ref["dlogvar"] - dlv).max()]
    print(beta, "gap %.2e dz %.2e dmu %.2e dlogvar %.2e" % (gap, *errs))
    assert max(errs) <= 1e-8
    if beta == 0.0:
        assert not ref["dmu"].any() and not ref["dlogvar"].any()


# ---- closed forms --------------------------------------------------------------------------------------------------------
def test_equal_sets_give_zero_exactly():
    z, _, t, mu, lv = R.make_inputs(33, 6, 5, seed=7)
    ref = R.sw(z, z.copy(), t, mu, lv, 3.0, 0.0)
    assert ref["terms"][1] == 0.0 and ref["loss"] == 0.0 and not ref["per"].any() and not ref["G"].any()
    assert not ref["dz"].any()


def test_shift_identity():
    """z = prior + c moves every projection of direction l by theta_l . c and keeps every order: SW^2 = mean_l
    (theta_l . c)^2."""
    _, prior, t, mu, lv = R.make_inputs(40, 6, 9, seed=8)
    c = np.linspace(-0.5, 0.75, 6)
    d = R.distance(prior.astype(np.float64) + c, prior, t)
    want = ((R.directions(t) @ c) ** 2).mean()
    assert abs(d["sw2"] - want) <= 1e-12 * want
    assert np.abs(d["G"] - (R.directions(t) @ c)[:, None]).max() <= 1e-12


def test_scaling_both_sets_scales_the_value_by_the_square():
    z, prior, t, _, _ = R.make_inputs(21, 4, 6, seed=9)
    base = R.distance(z, prior, t)["sw2"]
    for s in (0.5, 3.0, -2.0):
        got = R.distance(s * z.astype(np.float64), s * prior.astype(np.float64), t)["sw2"]
        assert abs(got - s * s * base) <= 1e-12 * s * s * base


def test_row_permutation_keeps_the_value_and_permutes_the_gradient():
    z, prior, t, mu, lv = R.make_inputs(19, 5, 6, seed=10)
    perm = np.random.default_rng(0).permutation(19)
    a, b = R.sw(z, prior, t, mu, lv, 3.0, 0.5), R.sw(z[perm], prior, t, mu, lv, 3.0, 0.5)
    assert abs(a["loss"] - b["loss"]) <= 1e-13 * abs(a["loss"])
    assert np.abs(a["dz"][perm] - b["dz"]).max() <= 1e-13 * np.abs(a["dz"]).max()
    assert np.abs(a["G"][:, perm] - b["G"]).max() <= 1e-13 * np.abs(a["G"]).max()


def test_duplicated_rows_are_ranked_by_row_index():
    z, prior, t, _, _ = R.make_inputs(8, 3, 4, seed=11)
    z[5] = z[2]
    z[7] = z[2]
    d = R.distance(z, prior, t)
    for l in range(4):
        pos = {int(r): k for k, r in enumerate(d["order"][l])}
        assert pos[5] == pos[2] + 1 and pos[7] == pos[2] + 2          # adjacent, in row order
        vs = np.sort(R.projections(z, prior, t)[1][l])
        u2 = R.projections(z, prior, t)[0][l, 2]
        assert np.array_equal(d["G"][l, [2, 5, 7]], u2 - vs[pos[2]:pos[2] + 3])
    # all rows equal: the order is the identity, whatever the direction
    same = np.repeat(z[:1], 8, axis=0)
    assert np.array_equal(R.distance(same, prior, t)["order"], np.tile(np.arange(8), (4, 1)))


def test_zero_direction_contributes_nothing():
    z, prior, t, _, _ = R.make_inputs(6, 3, 3, seed=12)
    t[1] = 0.0
    d = R.distance(z, prior, t)
    assert not d["Theta"][1].any() and d["per"][1] == 0.0 and not d["G"][1].any()
    assert np.isfinite(d["sw2"]) and d["sw2"] > 0


def test_shard_algebra_of_the_restatement():
    """The mean over equal shards of (global distance + shard KL) is the single-rank hook, in value and gradients."""
    z, prior, t, mu, lv = R.make_inputs(64, 16, 10, seed=6)
    one = R.sw(z, prior, t, mu, lv, 3.0, 0.5)
    parts = [R.sw(z, prior, t, mu[8 * r:8 * r + 8], lv[8 * r:8 * r + 8], 3.0, 0.5) for r in range(8)]
    assert abs(np.mean([p["loss"] for p in parts]) - one["loss"]) <= 1e-12 * abs(one["loss"])
    assert np.abs(np.mean([p["dz"] for p in parts], 0) - one["dz"]).max() <= 1e-12 * np.abs(one["dz"]).max()
    for k in ("dmu", "dlogvar"):
        got = np.concatenate([p[k] for p in parts]) / 8
        assert np.abs(got - one[k]).max() <= 1e-12 * np.abs(one[k]).max()


# ---- the stored vectors ----------------------------------------------------------------------------------------------
def test_stored_vectors():
    g = np.load(os.path.join(GOLDEN, "sw.npz"))
    lam, beta = g["hp"]
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    for must in [(1, 1, 1), (2, 1, 1), (2, 3, 2), (3, 64, 5), (64, 128, 50), (512, 128, 50), (65, 130, 33), (4096, 8, 3),
                 (4097, 8, 3), (12, 6, 257), (3, 2048, 2)]:
        assert must in shapes
    full = 0
    for Bt, D, L in shapes:
        p = f"{Bt}x{D}x{L}:"
        z, prior, t, mu, lv = R.make_inputs(Bt, D, L, int(g[p + "seed"]))
        assert z.dtype == prior.dtype == t.dtype == mu.dtype == lv.dtype == np.float32
        assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in (z, prior, t, mu, lv)])
        ref = R.sw(z, prior, t, mu, lv, lam, beta)
        assert abs(ref["loss"] - float(g[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        assert np.abs(ref["terms"] - g[p + "terms"]).max() <= 1e-12 * np.abs(ref["terms"]).max()
        # the condition on the inputs under which an fp64 evaluation sorts as the restatement does
        assert R.min_gap(z, prior, t) >= float(g["gap"]) == 1e-11, p
        assert float(g[p + "gmax"]) > 1e-6                                         # far from fp32 underflow
        if p + "dz" in g.files:
            full += 1
            for k in ("dz", "G", "per"):
                assert np.abs(ref[k] - g[p + k]).max() <= 1e-12 * np.abs(ref[k]).max(), (p, k)
    assert full >= 2


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
    from solvers.swae import IntroSWAESolver, SWAESolver
    return SWAESolver, IntroSWAESolver


def test_solver_defaults_and_exports():
    import solvers
    from solvers import IntroSolver, VAESolver, scores
    SWAESolver, IntroSWAESolver = _classes()
    assert solvers.SWAESolver is SWAESolver and solvers.IntroSWAESolver is IntroSWAESolver
    assert issubclass(SWAESolver, VAESolver) and issubclass(IntroSWAESolver, IntroSolver)
    # imported by name: the list of solvers that train from images alone and the score table stay as they were
    assert solvers.__all__ == ["VAESolver", "IntroSolver", "TCSovler", "IntroTCSovler", "DIPSolver", "IntroDIPSolver",
                               "MMDSolver", "IntroMMDSolver", "FactorSolver", "AdaGVAESolver", "JointVAESolver",
                               "AnnealedVAESolver"]
    assert not any("sw" in name or "sliced" in name for name in scores.KNOWN)
    for cls in _classes():
        for name, default in (("lambda_sw", 10.0), ("num_projections", 50)):
            p = inspect.signature(cls.__init__).parameters[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
        sig = inspect.signature(cls.compute_kl_loss)
        assert list(sig.parameters) == ["self", "z", "mu", "logvar", "reduce", "beta", "write"]
        s = _solver(cls)
        assert (s.lambda_sw, s.num_projections) == (10.0, 50)
        s = _solver(cls, lambda_sw=4, num_projections=7)
        assert (s.lambda_sw, s.num_projections) == (4.0, 7)
        assert isinstance(s.lambda_sw, float) and isinstance(s.num_projections, int)


def test_solver_validation_on_every_assignment():
    for cls in _classes():
        for bad in (-1.0, float("nan"), float("inf"), "3", None, True):
            with pytest.raises(ValueError, match="lambda_sw"):
                _solver(cls, lambda_sw=bad)
        for bad in (0, -1, 4097, 2.0, "3", None, True, float("nan")):
            with pytest.raises(ValueError, match="num_projections"):
                _solver(cls, num_projections=bad)
        s = _solver(cls, lambda_sw=2.0, num_projections=4096)
        with pytest.raises(ValueError, match="lambda_sw"):
            s.lambda_sw = -2.0
        with pytest.raises(ValueError, match="num_projections"):
            s.num_projections = 0
        assert (s.lambda_sw, s.num_projections) == (2.0, 4096)
        s.lambda_sw = 0                                                           # zero switches the distance off
        s.num_projections = 1
        assert (s.lambda_sw, s.num_projections) == (0.0, 1)


def test_graph_key_holds_the_pair():
    from solvers import IntroSolver, VAESolver
    for cls, step in zip(_classes(), (VAESolver, IntroSolver)):
        s = _solver(cls, lambda_sw=2.0)
        base = tuple(step._graph_key_extra(s))
        assert s._graph_key_extra() == base + (2.0, 50)
        s.lambda_sw *= 2
        assert s._graph_key_extra() == base + (4.0, 50)
        s.num_projections = 20
        assert s._graph_key_extra() == base + (4.0, 20)


def test_reduce_none_and_sum_dispatch_to_the_base_hook(monkeypatch):
    import ops
    from solvers.vae import VAESolver
    calls = []
    monkeypatch.setattr(VAESolver, "compute_kl_loss",
                        lambda self, z, mu, logvar, reduce="mean", beta=None, write=False:
                        calls.append((reduce, beta, write)) or "base")
    mu, lv = torch.zeros(4, 10), torch.zeros(4, 10)
    for cls in _classes():
        s = _solver(cls)
        with ops.noise_queue([]):                                                 # a draw would raise: none is made
            assert s.compute_kl_loss(None, mu, lv, reduce="none", beta=512.0) == "base"
            assert s.compute_kl_loss(mu, mu, lv, "sum") == "base"
    assert calls == [("none", 512.0, False), ("sum", None, False)] * 2


def test_mean_needs_z_and_draws_the_prior_then_the_directions():
    import ops
    from hipvae import abi
    mu, lv = torch.zeros(4, 10), torch.zeros(4, 10)
    for cls in _classes():
        s = _solver(cls, num_projections=6)
        with pytest.raises(ValueError, match="sampled latents"):
            s.compute_kl_loss(None, mu, lv)
        # the two draws of the call are taken from the queue -- the prior in the shape of z, then the directions [L, D]
        # (the queue asserts the shapes) -- before the kernels refuse the CPU tensors
        q = [torch.ones(4, 10), torch.ones(6, 10), torch.ones(4, 10)]
        with ops.noise_queue(q):
            with pytest.raises(abi.HipExtensionError):
                s.compute_kl_loss(mu, mu, lv)
            assert len(ops._noise["queue"]) == 1
        with ops.noise_queue([torch.ones(6, 10), torch.ones(4, 10)]):              # the other order is not the contract
            with pytest.raises(AssertionError):
                s.compute_kl_loss(mu, mu, lv)


def test_cpu_tensors_and_bad_arguments_raise():
    import ops
    from hipvae import abi, quality
    z, p, t, mu, lv = torch.zeros(4, 10), torch.zeros(4, 10), torch.ones(3, 10), torch.zeros(4, 10), torch.zeros(4, 10)
    with pytest.raises(abi.HipExtensionError):
        ops.sw_kl_loss(z, mu, lv, p, t, 1.0, 1.0)
    with pytest.raises(abi.HipExtensionError):
        ops.sw_regularizer(z, p, t, 1.0)
    with pytest.raises(abi.HipExtensionError):
        ops.sliced_wasserstein(z, p, t)
    with pytest.raises(ValueError, match="together"):
        ops.sw_kl_loss(z, mu, lv, p, t, 1.0, 1.0, z_all=z)
    with pytest.raises(ValueError, match="together"):
        ops.sw_kl_loss(z, mu, lv, p, t, 1.0, 1.0, prior_all=p)
    for bad in (dict(p=torch.zeros(6, 10)), dict(p=torch.zeros(4, 9)), dict(t=torch.ones(3, 9)), dict(t=torch.ones(10)),
                dict(mu=torch.zeros(4, 9)), dict(lv=torch.zeros(3, 10))):
        a = {**dict(z=z, p=p, t=t, mu=mu, lv=lv), **bad}
        with pytest.raises(ValueError, match="shape"):
            ops.sw_kl_loss(a["z"], a["mu"], a["lv"], a["p"], a["t"], 1.0, 1.0)
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_sw"):
            ops.sw_kl_loss(z, mu, lv, p, t, 1.0, lam)
    with pytest.raises(ValueError, match="beta"):
        ops.sw_kl_loss(z, mu, lv, p, t, float("nan"), 1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.sliced_wasserstein(z, torch.zeros(5, 10), t)
    with pytest.raises(ValueError, match="shape"):
        ops.sliced_wasserstein(z, p, torch.ones(3, 11))
    with pytest.raises(ValueError, match="equal counts"):
        quality.sliced_wasserstein_distance(z, torch.zeros(5, 10))
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="num_projections"):
            quality.sliced_wasserstein_distance(z, p, num_projections=bad)
    with pytest.raises(ValueError, match="space"):
        quality.compute_sliced_wasserstein(None, None, space="pixels")
    with pytest.raises(ValueError, match="prior"):
        quality.compute_sliced_wasserstein(None, None, prior="uniform")


def test_score_directions_come_from_a_private_generator():
    from hipvae import quality
    torch.manual_seed(3)
    before = torch.get_rng_state()
    a = quality.sliced_wasserstein_directions(5, 7, seed=4)
    assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(a, quality.sliced_wasserstein_directions(5, 7, seed=4))
    assert not torch.equal(a, quality.sliced_wasserstein_directions(5, 7, seed=5))
    assert a.shape == (5, 7) and a.dtype == torch.float32


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_library_and_makefile():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    i32, f64, p, sz = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    declared = {"itcv_sw_lds_rows": (i32, []),
                "itcv_sw_workspace": (sz, [i32, i32, i32]),
                "itcv_sw_kl_fwd": (i32, [p, sz, p, sz] + [p] * 8 + [i32] * 4 + [f64] * 2 + [p, sz, p]),
                "itcv_sw_kl_bwd": (i32, [p] * 8 + [i32] * 4 + [f64] * 2 + [p])}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES and hasattr(lib, name), name
        fn = getattr(abi.lib._cdll, name)                 # the ctypes function behind the memoising wrapper
        assert (fn.restype, list(fn.argtypes)) == declared[name], name
    assert abi.lib.itcv_abi_version() == abi.ABI_VERSION == 4                     # symbols were only added
    makefile = open(os.path.join(abi.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bsw\.hip\b", makefile, re.M)
    assert os.path.exists(os.path.join(abi.CSRC, "sw.hip"))
    assert "sw.hip" in open(os.path.join(abi.CSRC, "objective.h")).read().split("#pragma once")[0]
    # the keys of every training batch sit in LDS; above that one slice of 20 bytes a row (rounded up to 16 bytes) per
    # resident block, the grid capped at 256 blocks
    rows = abi.lib._cdll.itcv_sw_lds_rows()
    ws = abi.lib._cdll.itcv_sw_workspace
    assert rows >= 4096
    assert ws(1, 1, 1) == ws(rows, 4096, 2048) == 0
    assert ws(rows + 1, 3, 8) == 3 * ((rows + 1) * 20 + 15) // 16 * 16
    assert ws(rows + 1, 257, 8) == ws(rows + 1, 4096, 8) == 256 * (((rows + 1) * 20 + 15) // 16 * 16)
    assert ws(0, 1, 1) == ws(2 ** 20 + 1, 1, 1) == ws(8, 0, 1) == ws(8, 4097, 1) == ws(8, 1, 0) == ws(8, 1, 2049) == 0


def test_options_default_to_off_and_check_their_range():
    from hipvae import abi
    from hipvae import functional as HF
    lib = abi.lib._cdll
    rows = lib.itcv_sw_lds_rows()
    for name, hi in (("sw_lds_rows", 4096), ("sw_max_blocks", 1024)):
        assert HF.get_option(name) == 0
        for bad in (-1, hi + 1):
            with pytest.raises(abi.HipExtensionError, match=name):
                HF.set_option(name, bad)
        assert HF.get_option(name) == 0
    try:
        with HF.option_scope("sw_lds_rows", 1):
            assert lib.itcv_sw_lds_rows() == 1 and abi.lib.itcv_sw_workspace(2, 3, 8) == 3 * 48
            with HF.option_scope("sw_max_blocks", 2):
                assert abi.lib.itcv_sw_workspace(2, 3, 8) == 2 * 48
        assert lib.itcv_sw_lds_rows() == rows and abi.lib.itcv_sw_workspace(2, 3, 8) == 0
    finally:
        HF.set_option("sw_lds_rows", 0)
        HF.set_option("sw_max_blocks", 0)


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
P = [0x10000 * (k + 1) for k in range(12)]
INF, NAN = float("inf"), float("nan")


def _fwd(z=P[0], ldz=8, pr=P[1], ldp=8, t=P[2], mu=P[3], lv=P[4], out=P[5], terms=P[6], per=P[7], Th=P[8], G=P[9], Bl=4,
         Bt=8, L=3, D=8, lam=1.0, ckl=1.0, ws=P[10], nws=1 << 20):
    return ("itcv_sw_kl_fwd", z, ldz, pr, ldp, t, mu, lv, out, terms, per, Th, G, Bl, Bt, L, D, lam, ckl, ws, nws, None)


def _bwd(g=P[0], mu=P[1], lv=P[2], G=P[3], Th=P[4], dz=P[5], dmu=P[6], dlv=P[7], Bl=4, Bt=8, L=3, D=8, lam=1.0, ckl=1.0):
    return ("itcv_sw_kl_bwd", g, mu, lv, G, Th, dz, dmu, dlv, Bl, Bt, L, D, lam, ckl, None)


@pytest.mark.parametrize("args, msg", [
    (_fwd(z=None), "NULL"), (_fwd(pr=None), "NULL"), (_fwd(t=None), "NULL"), (_fwd(mu=None), "NULL"),
    (_fwd(lv=None), "NULL"), (_fwd(mu=None, lv=None), "NULL"), (_fwd(mu=None, ckl=0.0), "NULL"),
    (_fwd(out=None), "NULL"), (_fwd(terms=None), "NULL"), (_fwd(per=None), "NULL"), (_fwd(Th=None), "NULL"),
    (_fwd(Bt=4097, ws=None), "workspace"), (_fwd(Bt=4097, nws=4097 * 20 * 3 - 1), "workspace"),
    (_fwd(Bt=5000, L=300, nws=256 * 100000 - 1), "workspace"),
    (_fwd(Bt=0), "Bt = 0 rows"), (_fwd(Bt=-5), "Bt = -5"), (_fwd(Bt=2 ** 20 + 1), "Bt = 1048577 rows is outside 1..2^20"),
    (_fwd(L=0), "L = 0 projections"), (_fwd(L=4097), "L = 4097 projections is outside 1..4096"), (_fwd(L=-1), "L = -1"),
    (_fwd(D=0), "D = 0 is outside 1..2048"), (_fwd(D=2049), "D = 2049 is outside 1..2048"), (_fwd(D=-3), "D = -3"),
    (_fwd(Bl=0), "Bl = 0 local rows"), (_fwd(Bl=-1), "Bl = -1"), (_fwd(Bl=2 ** 24 + 1), "Bl = 16777217"),
    (_fwd(Bt=2 ** 20, L=65), "L * Bt = 68157440 is above 2^26"), (_fwd(Bt=2 ** 14 + 1, L=4096), "above 2^26"),
    (_fwd(lam=-1e-30), "lambda_sw"), (_fwd(lam=NAN), "lambda_sw"), (_fwd(lam=INF), "lambda_sw"),
    (_fwd(ckl=NAN), "coef_kl"), (_fwd(ckl=-INF), "coef_kl"),
    (_fwd(ldz=7), "z_all's row stride of 7 is below D = 8"), (_fwd(ldp=0), "prior's row stride of 0 is below D = 8"),
    (_bwd(g=None), "NULL"), (_bwd(mu=None), "NULL"), (_bwd(lv=None), "NULL"), (_bwd(G=None), "NULL"),
    (_bwd(Th=None), "NULL"), (_bwd(dz=None), "NULL"), (_bwd(dmu=None), "NULL"), (_bwd(dlv=None), "NULL"),
    (_bwd(Bt=0), "Bt = 0 rows"), (_bwd(Bt=2 ** 20 + 1), "Bt = 1048577"), (_bwd(L=0), "L = 0"), (_bwd(L=4097), "L = 4097"),
    (_bwd(Bl=0), "Bl = 0"), (_bwd(Bl=2 ** 24 + 1), "Bl = 16777217"), (_bwd(D=2049), "D = 2049"), (_bwd(D=0), "D = 0"),
    (_bwd(Bt=2 ** 20, L=65), "above 2^26"),
    (_bwd(lam=-1.0), "lambda_sw"), (_bwd(lam=NAN), "lambda_sw"), (_bwd(ckl=NAN), "coef_kl"), (_bwd(ckl=INF), "coef_kl"),
])
def test_refusals_fire_before_any_launch(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(abi.HipExtensionError):
        abi.call(*args)
