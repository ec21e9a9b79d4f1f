"""CPU-only tests of the MMD KL hook (InfoVAE / MMD-VAE, WAE-MMD): the fp64 restatement (tests/mmd_ref.py) against central
differences, its symmetry and translation identities, why d^2 is not taken in the fp32 Gram form, the stored vectors
(golden/mmd.npz), the surface of MMDSolver / IntroMMDSolver, and what the new entry points refuse before any launch."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import mmd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
NEW = ("itcv_mmd_kl_workspace", "itcv_mmd_kl_fwd", "itcv_mmd_kl_bwd")


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", R.KERNELS)
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_gradients_agree_with_central_differences(kernel, beta):
    z, prior, mu, lv = R.make_inputs(7, 5, 5, seed=3)
    mu, lv = mu[:4], lv[:4]                                         # the local rows need not be the whole batch
    ref = R.mmd(z, prior, mu, lv, kernel, 10.0, 3.0, beta)
    dz, dmu, dlv = R.central_differences(z, prior, mu, lv, kernel, 10.0, 3.0, beta)
    errs = [np.abs(ref["dz"] - dz).max(), np.abs(ref["dmu"] - dmu).max(), np.abs(ref["dlogvar"] - dlv).max()]
    print(kernel, beta, "dz %.2e dmu %.2e dlogvar %.2e" % tuple(errs))
    assert max(errs) <= 1e-7
    if beta == 0.0:
        assert not ref["dmu"].any() and not ref["dlogvar"].any()


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_zz_weights_are_symmetric_with_a_zero_diagonal(kernel):
    z, prior, mu, lv = R.make_inputs(9, 6, 4, seed=4)
    ref = R.mmd(z, prior, mu, lv, kernel, 8.0, 3.0, 0.5)
    A = ref["Wt"][:, :9]
    assert ref["Wt"].shape == (9, 15) and np.array_equal(A, A.T) and not np.diag(A).any()
    assert (A[~np.eye(9, dtype=bool)] < 0).all() and (ref["Wt"][:, 9:] > 0).all()     # k' < 0 for both kernels
    assert np.array_equal(ref["rs"], ref["Wt"].sum(1))


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_translation_identity(kernel):
    """The statistic depends on z and the prior through differences only: shifting both by one vector changes nothing, so
    sum_i dMMD^2/dz_i = -sum_j dMMD^2/dp_j, the gradient with respect to a common shift of the prior."""
    z, prior, mu, lv = (a.astype(np.float64) for a in R.make_inputs(11, 8, 6, seed=5))
    lam, h = 3.0, 12.0
    ref = R.mmd(z, prior, mu, lv, kernel, h, lam, 0.0)
    # analytic gradient with respect to the prior draws: the roles of the two sets exchanged
    swapped = R.mmd(prior, z, mu, lv, kernel, h, lam, 0.0)
    total = ref["dz"].sum(0)
    shift = swapped["dz"].sum(0)
    assert np.abs(total + shift).max() <= 1e-12 * np.abs(total).max()
    # ... and the same by central differences on the common shift itself
    num = np.zeros(6)
    for l in range(6):
        e = np.zeros(6)
        e[l] = 1e-5
        num[l] = (R.loss_only(z, prior + e, mu, lv, kernel, h, lam, 0.0)
                  - R.loss_only(z, prior - e, mu, lv, kernel, h, lam, 0.0)) / 2e-5
    assert np.abs(total + num).max() <= 1e-7
    # a common shift of both sets leaves the value where it was
    moved = R.loss_only(z + 0.25, prior + 0.25, mu, lv, kernel, h, lam, 0.0)
    assert abs(moved - ref["loss"]) <= 1e-12 * abs(ref["loss"])


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_gram_form_cancels_in_fp32(kernel):
    """Why d^2 is taken as sum (a - b)^2 in fp64: with a column offset of 1000 standard deviations |a|^2 + |b|^2 - 2 a.b
    is the difference of numbers 10^6 times d^2, 2^-24 of them is several percent of a d^2, and what survives the
    averaging over the pairs is an error of the statistic hundreds of times the project's 1e-4 bar (asserted: more than
    100 times); the fp64 difference form is the yardstick, and the fp64 Gram form keeps it to the digits the offset
    leaves."""
    rng = np.random.default_rng(0)
    D = 4
    z = (rng.normal(size=(64, D)) * 0.0013 + 1.0).astype(np.float32)
    p = (rng.normal(size=(64, D)) * 0.001 + 1.0).astype(np.float32)
    h = 2.0 * D * 1e-6                                            # the bandwidth of this scale: 2 D sigma^2
    want = np.array(R.sums(z, p, kernel, h))
    mmd2 = want[0] + want[1] - 2 * want[2]
    assert abs(mmd2) >= 1e-2 * want.max()

    def gram(a, b, dtype):
        a, b = a.astype(dtype), b.astype(dtype)
        return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - dtype(2) * (a @ b.T)).astype(np.float64)

    def stat(dtype):
        k = [R.kernel_values(gram(a, b, dtype), kernel, h)[0] for a, b in ((z, z), (p, p), (z, p))]
        np.fill_diagonal(k[0], 0.0)
        np.fill_diagonal(k[1], 0.0)
        return k[0].sum() / (64 * 63) + k[1].sum() / (64 * 63) - 2 * k[2].sum() / 64 ** 2

    e32, e64 = abs(stat(np.float32) - mmd2), abs(stat(np.float64) - mmd2)
    print(kernel, "MMD^2 %.3e  fp32 Gram error %.3e  fp64 Gram error %.3e" % (mmd2, e32, e64))
    assert e64 <= 1e-6 * abs(mmd2) < 1e-2 * abs(mmd2) < e32


def test_torch_form_equals_numpy_form():
    z, prior, mu, lv = R.make_inputs(9, 7, 6, seed=5)
    for kernel in R.KERNELS:
        ref = R.mmd(z, prior, mu, lv, kernel, 12.0, 3.0, 0.5)
        tz, tp, tm, tl = (torch.from_numpy(a).double().requires_grad_(True) for a in (z, prior, mu, lv))
        loss = R.torch_hook(tz, tp, tm, tl, kernel, None, 3.0, 0.5)
        loss.backward()
        assert tp.grad is None
        assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"])
        for got, k in ((tz.grad, "dz"), (tm.grad, "dmu"), (tl.grad, "dlogvar")):
            assert np.abs(got.numpy() - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), k


def test_shard_algebra_of_the_restatement():
    """The mean over equal shards of (global statistic + shard KL) is the single-rank hook, in value and gradients."""
    z, prior, mu, lv = R.make_inputs(64, 64, 16, seed=6)
    one = R.mmd(z, prior, mu, lv, "imq", 32.0, 3.0, 0.5)
    parts = [R.mmd(z, prior, mu[8 * r:8 * r + 8], lv[8 * r:8 * r + 8], "imq", 32.0, 3.0, 0.5) for r in range(8)]
    assert abs(np.mean([p["loss"] for p in parts]) - one["loss"]) <= 1e-12 * abs(one["loss"])
    assert np.abs(np.mean([p["dz"] for p in parts], 0) - one["dz"]).max() <= 1e-12 * np.abs(one["dz"]).max()
    for k in ("dmu", "dlogvar"):
        got = np.concatenate([p[k] for p in parts]) / 8
        assert np.abs(got - one[k]).max() <= 1e-12 * np.abs(one[k]).max()


def test_stored_vectors():
    g = np.load(os.path.join(GOLDEN, "mmd.npz"))
    lam, beta = g["hp"]
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    for must in [(2, 2, 1), (2, 3, 3), (3, 2, 64), (35, 20, 10), (64, 64, 128), (33, 65, 130), (65, 64, 65), (512, 512, 128),
                 (16, 16, 300), (7, 9, 512)]:
        assert must in shapes
    full = 0
    for Bt, P, D in shapes:
        z, prior, mu, lv = R.make_inputs(Bt, P, D, int(g[f"{Bt}x{P}x{D}:imq:seed"]))
        assert z.dtype == prior.dtype == mu.dtype == lv.dtype == np.float32
        for kernel in R.KERNELS:
            p = f"{Bt}x{P}x{D}:{kernel}:"
            assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in (z, prior, mu, lv)])
            ref = R.mmd(z, prior, mu, lv, kernel, 2.0 * D, lam, beta)
            t = g[p + "terms"]
            assert abs(ref["loss"] - float(g[p + "loss"])) <= 1e-12 * abs(ref["loss"])
            assert np.abs(ref["terms"] - t).max() <= 1e-12 * np.abs(ref["terms"]).max()
            # the condition on the inputs that keeps a relative bound on MMD^2 meaningful
            assert abs(t[1]) >= 1e-2 * t[2:].max(), (p, t)
            assert float(g[p + "gmax"]) > 1e-6                                     # far from fp32 underflow
            if p + "dz" in g.files:
                full += 1
                for k in ("dz", "Wt"):
                    assert np.abs(ref[k] - g[p + k]).max() <= 1e-12 * np.abs(ref[k]).max(), (p, k)
    assert full >= 4


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
    from solvers.mmd import IntroMMDSolver, MMDSolver
    return MMDSolver, IntroMMDSolver


def test_solver_defaults_and_exports():
    import solvers
    from solvers import IntroSolver, VAESolver
    MMDSolver, IntroMMDSolver = _classes()
    assert solvers.MMDSolver is MMDSolver and solvers.IntroMMDSolver is IntroMMDSolver
    assert issubclass(MMDSolver, VAESolver) and issubclass(IntroMMDSolver, IntroSolver)
    for cls in _classes():
        for name, default in (("lambda_mmd", 10.0), ("mmd_kernel", "imq"), ("mmd_bandwidth", None)):
            p = inspect.signature(cls.__init__).parameters[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == default
        sig = inspect.signature(cls.compute_kl_loss)
        assert list(sig.parameters) == ["self", "z", "mu", "logvar", "reduce", "beta", "write"]
        s = _solver(cls)
        assert (s.lambda_mmd, s.mmd_kernel, s.mmd_bandwidth) == (10.0, "imq", None)
        s = _solver(cls, lambda_mmd=4, mmd_kernel="rbf", mmd_bandwidth=5)
        assert (s.lambda_mmd, s.mmd_kernel, s.mmd_bandwidth) == (4.0, "rbf", 5.0)
        assert isinstance(s.lambda_mmd, float) and isinstance(s.mmd_bandwidth, float)
        s.mmd_bandwidth = None
        assert s.mmd_bandwidth is None


def test_solver_validation_on_every_assignment():
    for cls in _classes():
        for bad in ("IMQ", "gauss", "", None, 1):
            with pytest.raises(ValueError, match="mmd_kernel"):
                _solver(cls, mmd_kernel=bad)
        for bad in (-1.0, float("nan"), float("inf"), "3", None, True):
            with pytest.raises(ValueError, match="lambda_mmd"):
                _solver(cls, lambda_mmd=bad)
        for bad in (0.0, -0.5, float("nan"), float("inf"), "3", False):
            with pytest.raises(ValueError, match="mmd_bandwidth"):
                _solver(cls, mmd_bandwidth=bad)
        s = _solver(cls, lambda_mmd=2.0, mmd_kernel="rbf", mmd_bandwidth=3.0)
        with pytest.raises(ValueError, match="mmd_kernel"):
            s.mmd_kernel = "RBF"
        with pytest.raises(ValueError, match="lambda_mmd"):
            s.lambda_mmd = -2.0
        with pytest.raises(ValueError, match="mmd_bandwidth"):
            s.mmd_bandwidth = 0
        assert (s.lambda_mmd, s.mmd_kernel, s.mmd_bandwidth) == (2.0, "rbf", 3.0)
        s.lambda_mmd = 0                                                          # zero switches the statistic off
        assert s.lambda_mmd == 0.0


def test_graph_key_holds_the_triple():
    from solvers import IntroSolver, VAESolver
    for cls, step in zip(_classes(), (VAESolver, IntroSolver)):
        s = _solver(cls, lambda_mmd=2.0)
        base = tuple(step._graph_key_extra(s))
        assert s._graph_key_extra() == base + (2.0, "imq", None)
        s.lambda_mmd *= 2
        assert s._graph_key_extra() == base + (4.0, "imq", None)
        s.mmd_kernel = "rbf"
        s.mmd_bandwidth = 7
        assert s._graph_key_extra() == base + (4.0, "rbf", 7.0)


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


def test_mean_needs_z_and_draws_the_prior_from_the_noise_source():
    import ops
    from hipvae import abi
    mu, lv = torch.zeros(4, 10), torch.zeros(4, 10)
    for cls in _classes():
        s = _solver(cls)
        with pytest.raises(ValueError, match="sampled latents"):
            s.compute_kl_loss(None, mu, lv)
        # the one draw of the call is taken from the queue, in the shape of z, before the kernels refuse the CPU tensors
        q = [torch.ones(4, 10), torch.ones(4, 10)]
        with ops.noise_queue(q):
            with pytest.raises(abi.HipExtensionError):
                s.compute_kl_loss(mu, mu, lv)
            assert len(ops._noise["queue"]) == 1


def test_cpu_tensors_and_bad_arguments_raise():
    import ops
    from hipvae import abi
    z, p, mu, lv = torch.zeros(4, 10), torch.zeros(6, 10), torch.zeros(4, 10), torch.zeros(4, 10)
    with pytest.raises(abi.HipExtensionError):
        ops.mmd_kl_loss(z, mu, lv, p, 1.0, 1.0)
    with pytest.raises(abi.HipExtensionError):
        ops.mmd_regularizer(z, p, 1.0, kernel="rbf", bandwidth=3.0)
    with pytest.raises(ValueError, match="kernel"):
        ops.mmd_kl_loss(z, mu, lv, p, 1.0, 1.0, kernel="gauss")
    with pytest.raises(ValueError, match="together"):
        ops.mmd_kl_loss(z, mu, lv, p, 1.0, 1.0, z_all=z)
    with pytest.raises(ValueError, match="together"):
        ops.mmd_kl_loss(z, mu, lv, p, 1.0, 1.0, prior_all=p)
    with pytest.raises(ValueError, match="share D"):
        ops.mmd_kl_loss(z, mu, lv, torch.zeros(6, 9), 1.0, 1.0)
    with pytest.raises(ValueError, match="share D"):
        ops.mmd_kl_loss(z, torch.zeros(4, 9), torch.zeros(4, 9), p, 1.0, 1.0)
    with pytest.raises(ValueError, match="share D"):
        ops.mmd_regularizer(z, torch.zeros(6, 11), 1.0)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_library_and_makefile():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    i32, f64, p, sz = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
    declared = {"itcv_mmd_kl_workspace": (sz, [i32, i32]),
                "itcv_mmd_kl_fwd": (i32, [p] * 8 + [i32] * 5 + [f64] * 3 + [p, sz, p]),
                "itcv_mmd_kl_bwd": (i32, [p] * 10 + [i32] * 4 + [f64] * 2 + [p])}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES and hasattr(lib, name), name
        fn = getattr(abi.lib._cdll, name)                 # the ctypes function behind the memoising wrapper
        assert (fn.restype, list(fn.argtypes)) == declared[name], name
    assert abi.lib.itcv_abi_version() == abi.ABI_VERSION
    makefile = open(os.path.join(abi.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmmd\.hip\b", makefile, re.M)
    assert os.path.exists(os.path.join(abi.CSRC, "mmd.hip"))
    # one fp64 partial per 32 x 32 tile of the pair matrix of [z ; prior], one fp64 row sum per strip and row of z
    ws = abi.lib.itcv_mmd_kl_workspace
    assert ws(64, 64) == (4 * 4 + 4 * 64) * 8
    assert ws(2, 2) == ws(2, 32) == (2 * 2 + 2 * 2) * 8
    assert ws(33, 32) == (3 * 3 + 3 * 33) * 8
    assert ws(4096, 4096) == (256 * 256 + 256 * 4096) * 8 <= 9 << 20
    assert ws(1, 8) == ws(8, 1) == ws(4097, 8) == ws(8, 4097) == 0


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
P = [0x10000 * (k + 1) for k in range(11)]
INF, NAN = float("inf"), float("nan")


def _fwd(z=P[0], pr=P[1], mu=P[2], lv=P[3], out=P[4], terms=P[5], Wt=P[6], rs=P[7], Bl=4, Bt=8, Pn=8, D=8, kern=2, h=16.0,
         lam=1.0, ckl=1.0, ws=P[10], nws=1 << 20):
    return ("itcv_mmd_kl_fwd", z, pr, mu, lv, out, terms, Wt, rs, Bl, Bt, Pn, D, kern, h, lam, ckl, ws, nws, None)


def _bwd(g=P[0], z=P[1], pr=P[2], mu=P[3], lv=P[4], Wt=P[5], rs=P[6], dz=P[7], dmu=P[8], dlv=P[9], Bl=4, Bt=8, Pn=8, D=8,
         lam=1.0, ckl=1.0):
    return ("itcv_mmd_kl_bwd", g, z, pr, mu, lv, Wt, rs, dz, dmu, dlv, Bl, Bt, Pn, D, lam, ckl, None)


@pytest.mark.parametrize("args, msg", [
    (_fwd(z=None), "NULL"), (_fwd(pr=None), "NULL"), (_fwd(mu=None), "NULL"), (_fwd(lv=None), "NULL"),
    (_fwd(out=None), "NULL"), (_fwd(terms=None), "NULL"), (_fwd(Wt=None), "NULL"), (_fwd(rs=None), "NULL"),
    (_fwd(ws=None), "workspace"), (_fwd(nws=8), "workspace"), (_fwd(nws=(2 * 2 + 2 * 8) * 8 - 1), "workspace"),
    (_fwd(Bt=1), "Bt = 1 rows"), (_fwd(Bt=0), "Bt = 0 rows"), (_fwd(Bt=4097), "Bt = 4097 rows"), (_fwd(Bt=-5), "Bt = -5"),
    (_fwd(Pn=1), "P = 1 prior rows"), (_fwd(Pn=0), "P = 0 prior rows"), (_fwd(Pn=4097), "P = 4097 prior rows"),
    (_fwd(Bl=0), "Bl = 0 local rows"), (_fwd(Bl=-1), "Bl = -1"), (_fwd(Bl=2 ** 24 + 1), "Bl = 16777217"),
    (_fwd(D=0), "D = 0 is outside 1..512"), (_fwd(D=513), "D = 513 is outside 1..512"), (_fwd(D=-3), "D = -3"),
    (_fwd(kern=0), "kernel 0"), (_fwd(kern=3), "kernel 3"),
    (_fwd(h=0.0), "bandwidth"), (_fwd(h=-1.0), "bandwidth"), (_fwd(h=NAN), "bandwidth"), (_fwd(h=INF), "bandwidth"),
    (_fwd(lam=-1e-30), "lambda_mmd"), (_fwd(lam=NAN), "lambda_mmd"), (_fwd(lam=INF), "lambda_mmd"),
    (_fwd(ckl=NAN), "coef_kl"), (_fwd(ckl=-INF), "coef_kl"),
    (_bwd(g=None), "NULL"), (_bwd(z=None), "NULL"), (_bwd(pr=None), "NULL"), (_bwd(mu=None), "NULL"),
    (_bwd(lv=None), "NULL"), (_bwd(Wt=None), "NULL"), (_bwd(rs=None), "NULL"), (_bwd(dz=None), "NULL"),
    (_bwd(dmu=None), "NULL"), (_bwd(dlv=None), "NULL"),
    (_bwd(Bt=1), "Bt = 1 rows"), (_bwd(Bt=4097), "Bt = 4097"), (_bwd(Pn=1), "P = 1 prior rows"), (_bwd(Pn=4097), "P = 4097"),
    (_bwd(Bl=0), "Bl = 0"), (_bwd(Bl=2 ** 24 + 1), "Bl = 16777217"), (_bwd(D=513), "D = 513"), (_bwd(D=0), "D = 0"),
    (_bwd(lam=-1.0), "lambda_mmd"), (_bwd(lam=NAN), "lambda_mmd"), (_bwd(ckl=NAN), "coef_kl"), (_bwd(ckl=INF), "coef_kl"),
])
def test_refusals_fire_before_any_launch(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(abi.HipExtensionError):
        abi.call(*args)
