"""CPU checks of the yardstick of the Ada-GVAE / Ada-ML-VAE latent op and of everything around the kernels that needs no
GPU: (1) the numpy restatement tests/ada_ref.py equals a torch-fp64 autograd transcription of the library's lines to
1e-12; (2) its analytic gradients equal central differences with the mask held fixed; (3) every deliberate defect
(ada_ref.DEFECTS) moves a quantity that tests/test_hip_ada.py compares above that test's bar; (4) the stored vectors are
those of the restatement; (5) the ABI table and the header agree on the two symbols and the library refuses bad arguments
before any launch; (6) ``pair_factors``; (7) the argument errors of the op, the solver and the loader."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ada_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4                      # the GPU test's bar
GPU_SHAPES = [(1, 1), (1, 2), (2, 3), (3, 64), (4, 63), (5, 65), (33, 10), (7, 128), (32, 128), (9, 129), (2, 511),
              (3, 512), (1025, 10)]
SMALL = [(1, 1), (1, 2), (2, 3), (3, 5), (4, 10)]


def rel(x, want):
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    return float(np.abs(x - want).max() / scale) if scale else float(np.abs(x).max())


def inputs(B, D, seed=None):
    mu, lv, eps, seed = R.make_inputs(B, D, 7000 + 31 * B + D if seed is None else seed)
    return mu, lv, eps, R.make_mask(B, D, seed), R.make_dz(B, D, seed)


# ---- 1. restatement == the library's lines in torch fp64 ------------------------------------------------------------------
@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("averaging", R.AVERAGINGS)
@pytest.mark.parametrize("B, D", SMALL + [(5, 65), (7, 128), (33, 10)])
def test_restatement_equals_torch_transcription(B, D, averaging, mask):
    mu, lv, eps, own, dz = inputs(B, D)
    own = own if mask == "external" else None
    beta, g = 0.75, -1.25
    ref = R.ada(mu, lv, eps, beta, averaging, own, dz, g)
    a, b = (torch.from_numpy(x).double().requires_grad_(True) for x in (mu, lv))
    z, loss, used, terms = R.torch_op(a, b, torch.from_numpy(eps).double(), beta, averaging,
                                      None if own is None else torch.from_numpy(own))
    ((torch.from_numpy(dz).double() * z).sum() + g * loss).backward()
    assert np.array_equal(used.numpy(), ref["own"])
    got = dict(z=z.detach().numpy(), loss=float(loss.detach()), terms=terms.numpy(), dmu=a.grad.numpy(), dlogvar=b.grad.numpy())
    for k, v in got.items():
        assert rel(v, ref[k]) <= 1e-12, (k, rel(v, ref[k]))


# ---- 2. analytic gradients == central differences ---------------------------------------------------------------------------
@pytest.mark.parametrize("mask", R.MASKS)
@pytest.mark.parametrize("averaging", R.AVERAGINGS)
@pytest.mark.parametrize("B, D", SMALL)
def test_gradients_equal_central_differences(B, D, averaging, mask):
    mu, lv, eps, own, dz = inputs(B, D)
    beta, g = 0.75, 1.5
    ref = R.ada(mu, lv, eps, beta, averaging, own if mask == "external" else None, dz, g)
    dmu, dlv = R.central_differences(mu, lv, eps, beta, averaging, ref["own"], dz, g)      # the mask held fixed
    assert rel(dmu, ref["dmu"]) <= 1e-7 and rel(dlv, ref["dlogvar"]) <= 1e-7, (rel(dmu, ref["dmu"]), rel(dlv, ref["dlogvar"]))
    # each path on its own: through z alone, through the KL alone
    for dz_k, g_k in ((dz, 0.0), (None, g)):
        part = R.ada(mu, lv, eps, beta, averaging, ref["own"], dz_k, g_k)
        cd = R.central_differences(mu, lv, eps, beta, averaging, ref["own"], np.zeros_like(mu) if dz_k is None else dz_k, g_k)
        assert rel(cd[0], part["dmu"]) <= 1e-7 and rel(cd[1], part["dlogvar"]) <= 1e-7


def test_degenerate_pairs_keep_every_dimension():
    """D = 1 and two equal rows: delta equals the threshold, every dimension is own and the op is the plain VAE's."""
    mu, lv, eps, _, _ = inputs(3, 1)
    assert R.ada(mu, lv, eps, 1.0, "gvae")["own"].all()
    mu, lv, eps, _, _ = inputs(4, 10)
    r = R.ada(mu, lv, eps, 1.0, "mlvae")
    assert r["own"][3].all() and not r["own"][:3].all()           # the last pair of make_inputs: two equal rows
    allown = R.ada(mu, lv, eps, 1.0, "gvae", own=np.ones((4, 10), np.uint8))
    z = mu.astype(np.float64) + eps.astype(np.float64) * np.exp(0.5 * lv.astype(np.float64))
    kl = (-0.5 * (1.0 + lv.astype(np.float64) - mu.astype(np.float64) ** 2 - np.exp(lv.astype(np.float64))).sum(1)).mean()
    assert rel(allown["z"], z) <= 1e-15 and abs(allown["loss"] - kl) <= 1e-14 * abs(kl) and allown["terms"][1] == 0.0


# ---- 3. the defects ----------------------------------------------------------------------------------------------------
def moved(good, bad):
    """The largest normwise move of a compared quantity; a changed mask counts as a move without bound."""
    if not np.array_equal(good["own"], bad["own"]):
        return np.inf
    out = [rel(bad[k], good[k]) for k in ("loss", "z", "dmu", "dlogvar")]
    out += [rel(bad["terms"][0], good["terms"][0]), rel(bad["terms"][1], good["terms"][1])]
    return max(out)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defects_are_visible(defect):
    """Over the GPU test's own cases: a defect moves a compared quantity above the bar wherever it can apply, and it can
    apply somewhere."""
    threshold_only = ("half_in_delta", "symmetric_delta", "mask_inverted", "threshold_at_mean")
    seen = 0
    for B, D in GPU_SHAPES[:-1] + [(65, 10)]:
        mu, lv, eps, own, dz = inputs(B, D)
        for averaging in R.AVERAGINGS:
            for mask in R.MASKS:
                if (defect in threshold_only and (mask == "external" or D == 1)) or \
                        (defect == "drop_tail" and (D <= 64 or D % 64 == 0)) or \
                        (defect == "mlvae_mean_unweighted" and averaging != "mlvae"):
                    continue
                ext = own if mask == "external" else None
                good = R.ada(mu, lv, eps, 0.75, averaging, ext, dz, 1.0)
                if defect not in threshold_only and good["own"].all():
                    continue                                   # nothing shared: the averages are not used
                if defect == "threshold_at_mean" and D == 2:
                    continue                                   # two values: their mean is the middle of their range
                bad = R.ada(mu, lv, eps, 0.75, averaging, ext, dz, 1.0, defect=defect)
                m = moved(good, bad)
                if defect in ("half_in_delta", "symmetric_delta", "threshold_at_mean") and m <= BAR:
                    continue                                   # another delta can give the same mask on a small case
                assert m > BAR, (defect, B, D, averaging, mask, m)
                seen += 1
    print(defect, "visible on", seen, "cases")
    assert seen >= 4, (defect, seen)


# ---- 4. the stored vectors ------------------------------------------------------------------------------------------------
def test_golden_is_the_restatement():
    g = np.load(os.path.join(GOLDEN, "ada.npz"))
    assert [tuple(s) for s in g["shapes"]] == GPU_SHAPES
    beta = float(g["hp"][0])
    assert set(g.files) == {"shapes", "hp"} | {f"{B}x{D}:{k}" for B, D in GPU_SHAPES for k in (
        ["seed", "checksum"] + [f"{a}:{m}:loss" for a in R.AVERAGINGS for m in R.MASKS])}      # nothing else is stored
    for B, D in GPU_SHAPES:
        p = f"{B}x{D}:"
        mu, lv, eps, seed = R.make_inputs(B, D, int(g[p + "seed"]))
        assert seed == int(g[p + "seed"]), "the stored seed is the one the generator used"
        assert R.margin_holds(mu, lv)
        assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in (mu, lv, eps)])
        for averaging in R.AVERAGINGS:
            for mask in R.MASKS:
                own = R.make_mask(B, D, seed) if mask == "external" else None
                want = float(g[p + f"{averaging}:{mask}:loss"])
                assert abs(R.ada(mu, lv, eps, beta, averaging, own)["loss"] - want) <= 1e-12 * abs(want)


def test_make_inputs_moves_to_a_seed_that_holds_the_margin(monkeypatch):
    calls = []
    real = R.margin_holds
    monkeypatch.setattr(R, "margin_holds", lambda mu, lv: (calls.append(1), len(calls) > 2 and real(mu, lv))[1])
    *_, seed = R.make_inputs(3, 5, 40)
    assert seed == 42 and len(calls) == 3


# ---- 5. the boundary ------------------------------------------------------------------------------------------------------
def test_abi_table_and_header_agree():
    from hipvae import abi
    text = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in ("itcv_ada_group_fwd", "itcv_ada_group_bwd"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/itcv_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = abi.SIGNATURES[name]
        assert res is abi.i32 and len(args) == len(params), (name, len(args), len(params))
        for a, prm in zip(args, params):
            want = abi.p if "*" in prm else {"size_t": abi.sz, "int": abi.i32, "double": abi.f64}[prm.split()[0]]
            assert a is want, (name, prm)
        assert hasattr(lib, name)
    assert abi.ABI_VERSION == 4 and lib.itcv_abi_version() == 4


def test_library_refuses_bad_arguments_before_any_launch():
    from hipvae import abi
    buf = (ctypes.c_double * 64)()
    q = ctypes.addressof(buf)           # never dereferenced: every call below is refused by the host-side checks

    def fwd(B, D, averaging=1, beta=1.0, ld=None, mu=q):
        ld = D if ld is None else ld
        return abi.lib.itcv_ada_group_fwd(mu, ld, q, ld, q, ld, None, q, q, q, q, q, B, D, averaging, beta, None)

    def bwd(B, D, averaging=1, beta=1.0, ld=None, own=q):
        ld = D if ld is None else ld
        return abi.lib.itcv_ada_group_bwd(q, ld, q, q, ld, q, ld, q, ld, own, q, q, B, D, averaging, beta, None)

    for call in (fwd, bwd):
        assert call(1, 0) != 0 and "outside 1..512" in abi.last_error()
        assert call(1, 513) != 0 and "outside 1..512" in abi.last_error()
        assert call(0, 8) != 0 and "pairs" in abi.last_error()
        assert call(4, 8, averaging=3) != 0 and "averaging" in abi.last_error()
        assert call(4, 8, beta=float("nan")) != 0 and "finite" in abi.last_error()
        assert call(4, 8, ld=7) != 0 and "row stride" in abi.last_error()
    assert fwd(4, 8, mu=None) != 0 and "NULL" in abi.last_error()
    assert bwd(4, 8, own=None) != 0 and "NULL" in abi.last_error()


# ---- 6. pair_factors ------------------------------------------------------------------------------------------------------
SIZES, LATENT = [3, 4, 2, 5, 6], [1, 3, 4]


@pytest.mark.parametrize("k", [1, 2, 3, -1])
def test_pair_factors(k):
    from hipvae.dataset import factor_bases, pair_factors
    from hipvae.disentangle import FactorSampler
    B = 4000
    gen = torch.Generator().manual_seed(11)
    first, second, changed = pair_factors(SIZES, LATENT, B, k, gen, "cpu")
    assert first.shape == second.shape == (B, 5) and first.dtype == second.dtype == torch.int64
    assert changed.shape == (B, 3) and changed.dtype == torch.bool
    count = changed.sum(1)
    if k == -1:
        assert count.min() == 1 and count.max() == 2                    # 1 .. num_latents - 1, both reached
        assert 0.4 < float((count == 1).float().mean()) < 0.6
    else:
        assert (count == k).all()                                       # exactly k columns are flagged
    sizes = torch.tensor(SIZES)
    for f in (first, second):
        assert (f >= 0).all() and (f < sizes).all()                     # every value inside its factor's range
        for j, s in enumerate(SIZES):
            assert sorted(f[:, j].unique().tolist()) == list(range(s))  # and every value reached
    differs = first != second
    full = torch.zeros(B, 5, dtype=torch.bool)
    full[:, LATENT] = changed
    assert not (differs & ~full).any()                                  # unflagged factors (observed ones included) equal
    assert (differs & full).any(0)[LATENT].all()                        # flagged ones do change ...
    assert (~differs & full).any()                                      # ... but a redrawn value may equal the old one
    if k != 3:
        freq = changed.float().mean(0)                                  # every latent factor is chosen equally often
        assert float(freq.max() - freq.min()) < 0.05
    # reproducible per seed, and another seed draws other pairs
    again = pair_factors(SIZES, LATENT, B, k, torch.Generator().manual_seed(11), "cpu")
    assert all(torch.equal(a, b) for a, b in zip((first, second, changed), again))
    other = pair_factors(SIZES, LATENT, B, k, torch.Generator().manual_seed(12), "cpu")
    assert not torch.equal(first, other[0])
    # the global streams are not touched when a generator is given
    state = torch.get_rng_state()
    pair_factors(SIZES, LATENT, 8, k, torch.Generator().manual_seed(1), "cpu")
    assert torch.equal(state, torch.get_rng_state())

    # indices: FactorSampler.indices_from_factors of a dataset whose factors all vary draws nothing and is the mixed radix
    class DS:
        factor_sizes, latent_indices = SIZES, list(range(5))
    fs = FactorSampler(DS(), "cpu", seed=0)
    bases = torch.tensor(factor_bases(SIZES))
    assert factor_bases(SIZES) == fs.factor_bases
    for f in (first, second):
        assert np.array_equal(((f * bases).sum(1)).numpy(), fs.indices_from_factors(f.numpy()))


def test_pair_factors_argument_errors():
    from hipvae.dataset import pair_factors
    for k in (0, 4, -2, 1.5, True):
        with pytest.raises(ValueError):
            pair_factors(SIZES, LATENT, 8, k, device="cpu")
    with pytest.raises(ValueError):
        pair_factors(SIZES, [1], 8, -1, device="cpu")              # k = -1 needs two latent factors
    with pytest.raises(ValueError):
        pair_factors(SIZES, [1, 1], 8, 1, device="cpu")
    with pytest.raises(ValueError):
        pair_factors(SIZES, [5], 8, 1, device="cpu")
    with pytest.raises(ValueError):
        pair_factors(SIZES, LATENT, 0, 1, device="cpu")


# ---- 7. argument errors of the op, the solver and the loader -----------------------------------------------------------------
def test_op_argument_errors():
    import ops
    from hipvae import abi
    mu = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="averaging"):
        ops.ada_group(mu, mu, 1.0, averaging="mean")
    with pytest.raises(ValueError, match="pairs"):
        ops.ada_group(torch.zeros(5, 6), torch.zeros(5, 6), 1.0)
    with pytest.raises(ValueError, match="512"):
        ops.ada_group(torch.zeros(4, 513), torch.zeros(4, 513), 1.0)
    with pytest.raises(ValueError, match="own"):
        ops.ada_group(mu, mu, 1.0, own=torch.ones(4, 6))            # [2B, D] where [B, D] is wanted
    with pytest.raises(ValueError, match="shape"):
        ops.ada_group(mu, torch.zeros(4, 5), 1.0)
    with pytest.raises(ValueError, match="eps"):
        ops.ada_group(mu, mu, 1.0, eps=torch.zeros(2, 6))
    state = torch.get_rng_state()
    with pytest.raises(abi.HipExtensionError):
        ops.ada_group(mu, mu, 1.0)
    with pytest.raises(abi.HipExtensionError):
        ops.ada_group(mu, mu, 1.0, own=torch.ones(2, 6), eps=torch.zeros(4, 6))
    assert torch.equal(state, torch.get_rng_state())                # refused before the draw


def test_solver_argument_errors():
    import models
    from solvers import AdaGVAESolver, VAESolver
    from solvers.ada import ADA_AVERAGINGS

    class DS:
        def __len__(self):
            return 100

    model = models.SoftIntroVAE(arch="conv", cdim=3, zdim=4, channels=(8, 16), image_size=16)
    opt = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in (model.encoder, model.decoder)]
    args = (DS(), model, 4, opt[0], opt[1], "mse", 1.0, 1.0, torch.device("cpu"), False, None)
    with pytest.raises(ValueError, match="averaging"):
        AdaGVAESolver(*args, averaging="mean")
    solver = AdaGVAESolver(*args, averaging="mlvae")
    assert isinstance(solver, VAESolver) and solver.averaging == "mlvae" and ADA_AVERAGINGS == ("gvae", "mlvae")
    with pytest.raises(ValueError, match="averaging"):
        solver.averaging = "argmax"
    assert solver.averaging == "mlvae"                              # a refused assignment changes nothing
    assert AdaGVAESolver(*args).averaging == "gvae"
    assert ("mlvae", None) == solver._graph_key_extra()[-2:]
    solver.averaging = "gvae"
    assert ("gvae", None) == solver._graph_key_extra()[-2:]
    for shape in ((5, 3, 16, 16), (3, 16, 16), (0, 3, 16, 16)):     # refused before anything is launched
        with pytest.raises(ValueError, match="pair"):
            solver.train_step(torch.zeros(*shape), 0)


def test_loader_argument_errors():
    from hipvae.dataset import DeviceImageTable, DevicePairLoader
    table = DeviceImageTable(torch.zeros(24, 1, 2, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="factor_sizes"):
        DevicePairLoader(table, 4)
    with pytest.raises(ValueError, match="factor_sizes"):
        DevicePairLoader(np.zeros((24, 2, 2), np.uint8), 4)
    table.factor_sizes, table.latent_indices = [2, 3, 5], [0, 1, 2]
    with pytest.raises(ValueError, match="index"):
        DevicePairLoader(table, 4)                                  # 30 images by the factors, 24 in the table
    table.factor_sizes = [2, 3, 4]
    for k in (0, 4, -2):
        with pytest.raises(ValueError, match="k must"):
            DevicePairLoader(table, 4, k=k)
    with pytest.raises(ValueError, match="batch_size"):
        DevicePairLoader(table, 0)
    with pytest.raises(ValueError, match="lives on"):
        DevicePairLoader(table, 4, device="cuda:0")
    state = torch.get_rng_state()
    assert len(DevicePairLoader(table, 4)) == 3 and len(DevicePairLoader(table, 4, k=-1, steps_per_epoch=7)) == 7
    assert len(DevicePairLoader(table, 5)) == 2
    assert torch.equal(state, torch.get_rng_state())
