"""CPU-only tests of the semi-supervised S2 family: the fp64 restatement of the label regulariser (tests/sup_ref.py)
against torch's own float64 autograd of an independent expression, the stored vectors (golden/sup.npz), the weight's three
schedules, the loader's label derivation, and everything ``ops.supervised_regularizer``, the solvers, the loader and the
new entry points refuse before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NET = dict(cdim=3, zdim=10, channels=(8, 16), image_size=16)
NEW = ("itcv_sup_workspace", "itcv_sup_fwd", "itcv_sup_bwd")
SHAPES = [(1, 1, 1), (2, 3, 3), (5, 10, 7), (64, 128, 5), (33, 65, 64)]
S2 = ("S2VAESolver", "S2TCSolver", "S2DIPSolver", "S2FactorSolver")


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("B, D, F", SHAPES)
def test_restatement_equals_torch_float64_autograd(B, D, F, kind):
    mu, y, sizes = R.make_inputs(B, D, F, seed=11)
    ref = R.sup(mu, y, kind, sizes, gamma=0.75, scale=1.25)
    tm = torch.from_numpy(mu).double().requires_grad_(True)
    loss = 0.75 * R.torch_sup(tm, torch.from_numpy(y).double(), kind, sizes, scale=1.25)
    loss.backward()
    e_loss = abs(float(loss.detach()) - ref["loss"])
    e_grad = np.abs(tm.grad.numpy() - ref["dmu"]).max()
    print(kind, (B, D, F), "loss", e_loss, "dmu", e_grad)
    assert e_loss <= 1e-12 * abs(ref["loss"])
    assert e_grad <= 1e-12 * np.abs(ref["dmu"]).max()
    if kind != "cov":
        assert not ref["dmu"][:, F:].any() and not tm.grad[:, F:].any()
    if kind == "cov" and D == F == 1:
        assert ref["loss"] == 0.0 and not ref["dmu"].any()


def test_restatement_edges():
    mu, y, sizes = R.make_big_inputs(5, 10, 7, seed=12)
    assert np.abs(mu).max() == 80.0 and mu[0, 0] == 80.0 and mu[4, 6] == -80.0
    ref = R.sup(mu, y, "xent", sizes)
    assert np.isfinite(ref["sup"]) and np.isfinite(ref["dmu"]).all()
    tm = torch.from_numpy(mu).double().requires_grad_(True)
    loss = R.torch_sup(tm, torch.from_numpy(y).double(), "xent", sizes)
    loss.backward()
    assert abs(float(loss.detach()) - ref["sup"]) <= 1e-12 * ref["sup"]
    assert np.abs(tm.grad.numpy() - ref["dmu"]).max() <= 1e-12
    zero = R.sup(mu, y, "xent", sizes, gamma=0.0)
    assert zero["loss"] == 0.0 and not zero["dmu"].any() and zero["sup"] == ref["sup"]
    # sums, not means: twice the batch is twice the term (xent, l2)
    for kind in ("xent", "l2"):
        one = R.sup(mu, y, kind, sizes)["sup"]
        two = R.sup(np.concatenate([mu, mu]), np.concatenate([y, y]), kind, sizes)["sup"]
        assert abs(two - 2 * one) <= 1e-12 * two


def test_stored_vectors():
    g = np.load(os.path.join(GOLDEN, "sup.npz"))
    gamma, scale = (float(v) for v in g["hp"])
    shapes = [tuple(int(v) for v in s) for s in g["shapes"]]
    for must in SHAPES:
        assert must in shapes
    full = 0
    cases = [("", s, R.make_inputs) for s in shapes] + [("big:", tuple(int(v) for v in s), R.make_big_inputs)
                                                        for s in g["big"]]
    for tag, (B, D, F), make in cases:
        for kind in R.KINDS:
            p = f"{tag}{B}x{D}x{F}:{kind}:"
            mu, y, sizes = make(B, D, F, int(g[p + "seed"]))
            assert mu.dtype == y.dtype == np.float32
            assert np.array_equal(g[p + "checksum"], [mu.astype(np.float64).sum(), y.astype(np.float64).sum()])
            ref = R.sup(mu, y, kind, sizes, gamma, scale)
            assert abs(ref["sup"] - float(g[p + "sup"])) <= 1e-12 * abs(ref["sup"])
            assert abs(ref["loss"] - float(g[p + "loss"])) <= 1e-12 * abs(ref["loss"])
            assert abs(np.abs(ref["dmu"]).max() - float(g[p + "gmax"])) <= 1e-12 * float(g[p + "gmax"])
            if p + "mu" in g.files:
                full += 1
                assert np.array_equal(g[p + "mu"], mu) and np.array_equal(g[p + "y"], y)
                assert np.abs(ref["dmu"] - g[p + "dmu"]).max() <= 1e-12 * max(np.abs(ref["dmu"]).max(), 1e-300), p
    assert full >= 20


# ---- the schedules -----------------------------------------------------------------------------------------------------
def _solver(name, **kw):
    import models
    import solvers
    m = models.SoftIntroVAE(arch="conv", **NET)

    class DS:
        def __len__(self):
            return 100

    args = [DS(), m, 4, torch.optim.Adam(m.encoder.parameters()), torch.optim.Adam(m.decoder.parameters()), "mse",
            0.5, 0.75]
    if name == "S2FactorSolver":
        disc = models.Discriminator(NET["zdim"], hidden=16, layers=2)
        kw.update(discriminator=disc, optimizer_disc=torch.optim.Adam(disc.parameters(), lr=1e-4, betas=(0.5, 0.9)))
    kw.setdefault("factor_sizes", (3, 4, 5))
    return getattr(solvers, name)(*args, torch.device("cpu"), False, None, **kw)


@pytest.mark.parametrize("T", [4, 100000])
def test_the_three_schedules(T):
    from solvers.semi import SUP_SCHEDULES, gamma_sup_at
    assert SUP_SCHEDULES == ("fixed", "anneal", "fine_tune")
    ts = (0, T // 2, T, T + 1, 2 * T)
    want = {"fixed": [3.0] * 5, "anneal": [0.0, 1.5, 3.0, 3.0, 3.0], "fine_tune": [0.0, 0.0, 0.0, 3.0, 3.0]}
    for schedule in SUP_SCHEDULES:
        s = _solver("S2VAESolver", gamma_sup=3.0, sup_schedule=schedule, sup_threshold=T)
        for t, w in zip(ts, want[schedule]):
            assert gamma_sup_at(schedule, 3.0, T, t) == s.gamma_sup_at(t) == R.gamma_sup(schedule, 3.0, T, t) == w, \
                (schedule, t)
    with pytest.raises(ValueError, match="sup_schedule"):
        gamma_sup_at("cosine", 1.0, T, 0)


# ---- the solvers' surface ------------------------------------------------------------------------------------------
def test_solver_classes_defaults_and_graph_key():
    import solvers
    from solvers.semi import SupervisedHook
    bases = dict(S2VAESolver=solvers.VAESolver, S2TCSolver=solvers.TCSovler, S2DIPSolver=solvers.DIPSolver,
                 S2FactorSolver=solvers.FactorSolver)
    for name in S2:
        cls = getattr(solvers, name)
        assert cls.__mro__[1] is SupervisedHook and cls.__mro__[2] is bases[name], name
        assert set(vars(cls)) <= {"__module__", "__doc__"}
        assert cls.train_step is solvers.VAESolver.train_step and cls._device_step is solvers.VAESolver._device_step
        s = _solver(name)
        assert (s.sup_kind, s.gamma_sup, s.sup_schedule, s.sup_threshold, s.sup_scale) == ("xent", 1.0, "fixed", 100000.0,
                                                                                          1.0)
        assert s.factor_sizes == (3, 4, 5) and s.steps_taken == 0
        assert s._gsup.dtype == torch.float64 and tuple(s._gsup.shape) == (1,)
        base = tuple(bases[name]._graph_key_extra(s))
        assert s._graph_key_extra() == base + ("xent", 1.0, (3, 4, 5), None, s._gsup.data_ptr())
        x = s._batch((torch.zeros(6, 3, 16, 16), torch.tensor([[1.0, 2.0, 3.0], [0.0, 0.0, 4.0]])))
        assert tuple(x.shape) == (6, 3, 16, 16) and s._labels.dtype == torch.float32
        assert s._labels.tolist() == [[1.0, 2.0, 3.0], [0.0, 0.0, 4.0]]
        key = s._graph_key_extra()
        assert key[-2] == (s._labels.data_ptr(), (2, 3))
        # the weight is not in the key: a moving gamma_sup(t) never re-captures; the kind and the scale are
        s.gamma_sup = 7.0
        s.steps_taken = 5
        assert s._graph_key_extra() == key
        s.sup_kind = "cov"
        assert s._graph_key_extra() != key
        s.sup_kind, s.sup_scale = "xent", 2.0
        assert s._graph_key_extra() != key


def test_solver_refusals():
    for name in S2:
        with pytest.raises(ValueError, match="factor_sizes"):
            _solver(name, factor_sizes=None)
        for bad in ((), (3, 0), (3, 2.5), "ab", (True, 2), tuple([2] * 65), 3):
            with pytest.raises(ValueError, match="factor_sizes"):
                _solver(name, factor_sizes=bad)
        with pytest.raises(ValueError, match="latent dimensions"):
            _solver(name, factor_sizes=tuple([2] * 11))
        with pytest.raises(ValueError, match="sup_kind"):
            _solver(name, sup_kind="embed")
        with pytest.raises(ValueError, match="sup_schedule"):
            _solver(name, sup_schedule="cosine")
        for attr in ("gamma_sup", "sup_threshold", "sup_scale"):
            for bad in (-1.0, float("nan"), "3", None, True):
                with pytest.raises(ValueError, match=attr):
                    _solver(name, **{attr: bad})
    s = _solver("S2VAESolver")
    x, y = torch.zeros(6, 3, 16, 16), torch.zeros(2, 3)
    for bad in (x, (x,), (x, y, y), (x, torch.zeros(2, 4)), (x, torch.zeros(2)), (x[0], y), (x, torch.zeros(6, 3)),
                (x, torch.zeros(0, 3)), (x, None)):
        with pytest.raises(ValueError, match=r"\(x \[B \+ B_l, C, H, W\], y \[B_l, 3\]\)"):
            s._batch(bad)


# ---- the op refuses before any device call ------------------------------------------------------------------------------
def test_op_value_errors_come_before_any_device_call():
    import ops
    from hipvae import abi
    assert tuple(ops.SUP_KINDS) == ("xent", "l2", "cov")
    mu, y = torch.zeros(4, 10), torch.zeros(4, 3)
    with pytest.raises(ValueError, match="kind"):
        ops.supervised_regularizer(mu, y, kind="embed")
    for bad in (torch.zeros(4), torch.zeros(5, 3), torch.zeros(4, 3, 1), torch.zeros(4, 0), None, [[0.0] * 3] * 4):
        with pytest.raises(ValueError, match=r"labels must be a \[B_l, F\]"):
            ops.supervised_regularizer(mu, bad, "l2")
    with pytest.raises(ValueError, match="F = 11, D = 10"):
        ops.supervised_regularizer(mu, torch.zeros(4, 11), "l2")
    with pytest.raises(ValueError, match="F = 65, D = 100"):
        ops.supervised_regularizer(torch.zeros(4, 100), torch.zeros(4, 65), "cov")
    with pytest.raises(ValueError, match="D = 513"):
        ops.supervised_regularizer(torch.zeros(4, 513), y, "cov")
    with pytest.raises(ValueError, match="needs factor_sizes"):
        ops.supervised_regularizer(mu, y, "xent")
    for bad in ((3, 4), (3, 4, 5, 6), (3, 0, 5), (3, 2.5, 5)):
        with pytest.raises(ValueError, match="factor_sizes must be 3 integers"):
            ops.supervised_regularizer(mu, y, "xent", factor_sizes=bad)
    with pytest.raises(ValueError, match="mu must be"):
        ops.supervised_regularizer(torch.zeros(10), y, "l2")
    for bad in (torch.zeros(2, dtype=torch.float64), torch.zeros(1)):
        with pytest.raises(ValueError, match=r"gamma must be a number or a \[1\] float64"):
            ops.supervised_regularizer(mu, y, "l2", gamma=bad)
    with pytest.raises(ValueError, match="gamma must be finite"):
        ops.supervised_regularizer(mu, y, "l2", gamma=float("nan"))
    with pytest.raises(ValueError, match="scale must be finite"):
        ops.supervised_regularizer(mu, y, "l2", scale=float("inf"))
    # a CPU tensor: the binding's one sentence, from abi.need_device
    for kind, sizes in (("xent", (3, 4, 5)), ("l2", None), ("cov", None)):
        with pytest.raises(abi.HipExtensionError) as e:
            ops.supervised_regularizer(mu, y, kind, factor_sizes=sizes)
        assert str(e.value) == "HIP kernels need device tensors (got a CPU tensor); there is no CPU path"


# ---- the loader -----------------------------------------------------------------------------------------------------
def test_label_derivation_round_trip():
    """index -> factors -> index on a synthetic table of 3 * 1 * 4 * 5 images, with torch ops on the CPU."""
    from hipvae.dataset import factor_bases, index_factors
    sizes = (3, 1, 4, 5)
    idx = torch.arange(60, dtype=torch.int64)
    f = index_factors(idx, sizes)
    assert f.dtype == torch.int64 and tuple(f.shape) == (60, 4)
    assert [int(f[:, c].max()) + 1 for c in range(4)] == list(sizes) and int(f.min()) == 0
    assert len({tuple(r) for r in f.tolist()}) == 60
    bases = torch.tensor(factor_bases(sizes))
    assert bases.tolist() == [20, 20, 5, 1]
    assert torch.equal((f * bases).sum(1), idx)
    # the order of the factor datasets: the last factor varies fastest
    assert f[:6].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 0, 3], [0, 0, 0, 4], [0, 0, 1, 0]]
    lat = (0, 2, 3)
    sub = index_factors(torch.tensor([59, 7, 23]), sizes, lat)
    assert sub.tolist() == [[2, 3, 4], [0, 1, 2], [1, 0, 3]]
    assert torch.equal((sub * bases[list(lat)]).sum(1), torch.tensor([59, 7, 23]))     # the size-1 factor carries nothing
    assert index_factors(torch.tensor([23]), sizes, (3, 0)).tolist() == [[3, 1]]


def _table(sizes=(3, 1, 4, 5), lat=(0, 2, 3), n=None):
    from hipvae.dataset import DeviceImageTable
    n = int(np.prod(sizes)) if n is None else n
    t = DeviceImageTable(torch.zeros((n, 1, 8, 8), dtype=torch.uint8))
    t.factor_sizes, t.latent_indices = sizes, lat
    return t


def test_loader_surface_and_refusals():
    from hipvae.dataset import DeviceImageTable, DeviceLabelledLoader
    plain = DeviceImageTable(torch.zeros((60, 1, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="carries no factor_sizes"):
        DeviceLabelledLoader(plain, 8)
    with pytest.raises(ValueError, match="carries no factor_sizes"):
        DeviceLabelledLoader(object(), 8)
    with pytest.raises(ValueError, match="the table holds 50"):
        DeviceLabelledLoader(_table(n=50), 8)
    t = _table()
    for kw, msg in ((dict(batch_size=0), "positive"), (dict(labelled_batch_size=0), "positive"),
                    (dict(num_labelled=0), "num_labelled"), (dict(num_labelled=61), "num_labelled"),
                    (dict(factors=(1,)), "factors"), (dict(factors=(0, 0)), "factors"), (dict(factors=()), "factors"),
                    (dict(factors=(0, 7)), "factors")):
        args = dict(batch_size=8, num_labelled=10)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            DeviceLabelledLoader(t, **args)
    ld = DeviceLabelledLoader(t, 8, num_labelled=10)
    assert ld.factor_sizes == (3, 4, 5) and ld.columns == (0, 2, 3) and ld.labelled_batch_size == 8 and len(ld) == 7
    ld = DeviceLabelledLoader(t, 8, labelled_batch_size=3, num_labelled=10, factors=(3, 0), drop_last=False)
    assert ld.factor_sizes == (5, 3) and ld.labelled_batch_size == 3 and len(ld) == 8 and ld.labelled_indices is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_library_and_makefile():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert abi.ABI_VERSION == 4 and abi.lib.itcv_abi_version() == 4
    makefile = open(os.path.join(abi.CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bsup\.hip\b", makefile, re.M)
    src = open(os.path.join(abi.CSRC, "sup.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace itcv")[1].lower()
    ws = abi.lib.itcv_sup_workspace
    # one fp64 partial per labelled row (xent, l2) or per 32 x 32 tile of C (cov)
    assert ws(64, 10, 5, 1) == ws(64, 10, 5, 2) == 64 * 8 and ws(1, 1, 1, 1) == 8
    assert ws(64, 10, 5, 3) == ws(4096, 32, 32, 3) == 8 and ws(7, 33, 33, 3) == 4 * 8 and ws(7, 512, 64, 3) == 32 * 8
    assert ws(0, 10, 5, 1) == ws(4, 513, 5, 1) == ws(4, 100, 65, 3) == ws(4, 5, 6, 2) == ws(4, 10, 5, 0) == ws(4, 10, 5, 4) == 0


# fake 16-byte aligned device addresses: every call below must fail in its host-side checks, before any launch
P = [0x10000 * (k + 1) for k in range(12)]
INF, NAN = float("inf"), float("nan")


def _fwd(mu=P[0], ldm=10, y=P[1], ldy=5, sizes=P[2], mins=1, gdev=None, gamma=1.0, scale=1.0, out=P[3], terms=P[4], Wt=P[5],
         keep=P[6], ws=P[7], nws=1 << 20, B=8, D=10, F=5, form=1):
    return ("itcv_sup_fwd", mu, ldm, y, ldy, sizes, mins, gdev, gamma, scale, out, terms, Wt, keep, ws, nws, B, D, F, form,
            None)


def _bwd(g=P[0], mu=P[1], ldm=10, y=P[2], ldy=5, sizes=P[3], mins=1, scale=1.0, Wt=P[4], keep=P[5], dmu=P[6], B=8, D=10, F=5,
         form=1):
    return ("itcv_sup_bwd", g, mu, ldm, y, ldy, sizes, mins, scale, Wt, keep, dmu, B, D, F, form, None)


@pytest.mark.parametrize("args, msg", [
    (_fwd(mu=None), "NULL"), (_fwd(y=None), "NULL"), (_fwd(out=None), "NULL"), (_fwd(terms=None), "NULL"),
    (_fwd(keep=None), "NULL"), (_fwd(sizes=None), "NULL"), (_fwd(Wt=None, form=3), "NULL"),
    (_fwd(ws=None), "workspace"), (_fwd(nws=56), "workspace"),
    (_fwd(B=0), "B_l = 0"), (_fwd(B=-2), "B_l = -2"), (_fwd(B=(1 << 24) + 1), "outside 1..2^24"),
    (_fwd(D=513, ldm=513), "D = 513 is outside 1..512"), (_fwd(D=0, F=0), "D = 0"),
    (_fwd(F=0), "F = 0 factors is outside 1..64"), (_fwd(F=65, D=100, ldm=100, ldy=65), "F = 65 factors is outside 1..64"),
    (_fwd(F=11, ldy=11), "F = 11 factors exceed the D = 10"),
    (_fwd(form=0), "form 0"), (_fwd(form=4), "form 4"),
    (_fwd(mins=0), "factor size >= 1 (got 0)"), (_fwd(mins=-3), "got -3"),
    (_fwd(gamma=NAN), "gamma"), (_fwd(gamma=INF), "gamma"), (_fwd(scale=NAN, form=2), "scale"),
    (_fwd(ldm=9), "row stride of 9 is below D = 10"), (_fwd(ldy=4), "row stride of 4 is below F = 5"),
    (_bwd(g=None), "NULL"), (_bwd(mu=None), "NULL"), (_bwd(y=None), "NULL"), (_bwd(keep=None), "NULL"),
    (_bwd(dmu=None), "NULL"), (_bwd(sizes=None), "NULL"), (_bwd(Wt=None, form=3), "NULL"),
    (_bwd(B=0), "B_l = 0"), (_bwd(D=513, ldm=513), "D = 513"), (_bwd(F=65, D=100, ldm=100, ldy=65), "F = 65"),
    (_bwd(F=11, ldy=11), "exceed"), (_bwd(form=7), "form 7"), (_bwd(mins=0), "factor size"),
    (_bwd(scale=INF, form=2), "scale"), (_bwd(ldm=3), "row stride of 3"), (_bwd(ldy=2), "row stride of 2"),
])
def test_refusals_fire_before_any_launch(args, msg):
    from hipvae import abi
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    err = abi.last_error()
    assert err.startswith(args[0]) and msg in err, err
    with pytest.raises(abi.HipExtensionError):
        abi.call(*args)


def test_forms_that_do_not_need_a_pointer_do_not_ask_for_it():
    """l2 and cov read no factor sizes and only cov writes W: with those pointers NULL the checks still reach the one
    deliberately bad argument behind them."""
    from hipvae import abi
    for args in (_fwd(sizes=None, mins=0, form=2, ldm=9), _fwd(sizes=None, Wt=None, mins=0, form=2, ldm=9),
                 _fwd(sizes=None, mins=0, form=3, ldm=9), _bwd(sizes=None, Wt=None, mins=0, form=2, ldm=9)):
        assert getattr(abi.lib, args[0])(*args[1:]) != 0
        assert "row stride of 9" in abi.last_error()
