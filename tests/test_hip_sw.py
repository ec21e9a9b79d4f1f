"""GPU tests of the sliced-Wasserstein KL hook (csrc/sw.hip, ops.sw_kl_loss / sliced_wasserstein, solvers/swae.py, the
scores of hipvae/quality.py) against the fp64 restatement tests/sw_ref.py.

Bounds, all normwise: the loss and each of the three terms relative to the fp64 value; per, G, Theta and each gradient
tensor as max |err| / max |value|.  The ceiling is the project's fp32 bar, 1e-4; a quantity whose fp64 value is exactly
zero (the KL gradients without a KL coefficient, dz without the distance, everything for equal sets) must come out
exactly zero.  Sorting is discontinuous, so every case asserts a condition on the REFERENCE's inputs first: the smallest
gap between adjacent sorted projections, of u and of v, is at least 1e-11 max |u|.  The kernels project in fp64 (error
~1e-13 relative), so under that condition the device's order is the restatement's and G is comparable element by
element.  Worst values measured on an MI355X over every case of test_kernel_against_restatement (printed by it):

    loss 7.2e-08, mean KL 8.6e-08, SW^2 5.5e-08, max SW_l^2 5.4e-08, per 2.5e-15, G 2.6e-15, Theta 2.0e-16, dz 5.2e-08,
    dmu 5.2e-08, dlogvar 7.6e-08
"""
import os

import numpy as np
import pytest
import torch

import sw_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
GAP = 1e-11
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
# (Bt, D, L).  The smallest; the sort network off powers of two (Bt in {31 .. 1025}); the staging edges of both kernels:
# the projection's 64 lanes over D and the backward's 16 rows x 64 columns over chunks of 32 directions (Bt in {15, 16,
# 17}, D in {63, 64, 65, 130, 512, 2048}, L = 33); L in {1, 2, 50, 257}, 257 above the grid cap of 256; the training
# shapes; Bt at and one above the rows whose keys sit in LDS (asserted equal to itcv_sw_lds_rows() below).
SHAPES = [(1, 1, 1), (2, 1, 1), (2, 3, 2), (3, 64, 5),
          (31, 5, 3), (32, 5, 3), (33, 5, 3), (63, 4, 3), (64, 4, 3), (65, 4, 3), (1023, 3, 3), (1024, 3, 3), (1025, 3, 3),
          (15, 63, 4), (16, 64, 4), (17, 65, 4), (9, 130, 4), (5, 512, 2), (3, 2048, 2),
          (20, 7, 1), (20, 7, 2), (12, 6, 257), (65, 130, 33),
          (64, 128, 50), (512, 128, 50),
          (4096, 8, 3), (4097, 8, 3)]
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a)).to(dev())       # a copy: the stored cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "sw.npz"))
    return {k: g[k] for k in g.files}


_CASES = {}


def reference(z, prior, t, mu, lv, lam, beta):
    """The restatement's values after the condition on its inputs that makes G comparable element by element."""
    assert R.min_gap(z, prior, t) >= GAP
    return R.sw(z, prior, t, mu, lv, lam, beta)


def case(golden, Bt, D, L):
    """The stored inputs of a shape and the restatement's values, computed once per shape and never modified."""
    key = (Bt, D, L)
    if key not in _CASES:
        p = f"{Bt}x{D}x{L}:"
        lam, beta = (float(v) for v in golden["hp"])
        z, prior, t, mu, lv = R.make_inputs(Bt, D, L, int(golden[p + "seed"]))
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in (z, prior, t, mu, lv)])
        ref = reference(z, prior, t, mu, lv, lam, beta)
        assert abs(ref["loss"] - float(golden[p + "loss"])) <= 1e-12 * abs(ref["loss"])
        for a in (z, prior, t, mu, lv, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
            a.setflags(write=False)
        _CASES[key] = dict(z=z, prior=prior, t=t, mu=mu, lv=lv, ref=ref, hp=(lam, beta))
    return _CASES[key]


def place(x, layout):
    """A device tensor holding the values of ``x``: dense, or the right part of a wider nan tensor that must not be read."""
    if layout == "dense":
        return G(x)
    wide = np.full((x.shape[0], x.shape[1] + 3), np.nan, dtype=np.float32)
    wide[:, 3:] = x
    t = G(wide)[:, 3:]
    assert t.stride() == (x.shape[1] + 3, 1)
    return t


def run(z, prior, t, mu, lv, lam, beta, layout="dense", g=1.0):
    """loss, terms, per, Theta, G and the three gradients of ops.sw_kl_loss on the device (per, Theta, G from the same
    forward entry)."""
    import ops
    from hipvae import functional as HF
    tz, tm, tl = (place(a, layout).detach().requires_grad_(True) for a in (z, mu, lv))
    tp, tt = (place(a, layout).detach().requires_grad_(True) for a in (prior, t))
    loss, terms = ops.sw_kl_loss(tz, tm, tl, tp, tt, beta, lam, with_terms=True)
    assert not terms.requires_grad and loss.shape == () and terms.shape == (3,)
    dz, dmu, dlv, dp, dt = torch.autograd.grad(loss * g if g != 1.0 else loss, (tz, tm, tl, tp, tt), allow_unused=True)
    assert dp is None and dt is None                     # the prior and the directions are constants
    assert dz.shape == tz.shape
    out2, terms2, per, Theta, Gd = HF.sw_kl_forward(tz.detach(), tp.detach(), tt.detach(), tm.detach(), tl.detach(), lam, beta)
    assert torch.equal(out2, loss.detach()) and torch.equal(terms2, terms)
    assert per.dtype == Theta.dtype == Gd.dtype == torch.float64
    assert per.shape == (t.shape[0],) and Theta.shape == t.shape and Gd.shape == (t.shape[0], z.shape[0])
    return dict(loss=loss.detach(), terms=terms, per=per, Theta=Theta, G=Gd, dz=dz, dmu=dmu, dlv=dlv)


def errors(got, ref):
    """Normwise errors of a run against the restatement; a quantity that is exactly zero there must be exactly zero."""
    def rel(x, want):
        x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
        scale = np.abs(want).max()
        if scale == 0.0:
            assert not x.any()
            return 0.0
        assert np.isfinite(x).all()
        return float(np.abs(x - want).max() / scale)

    t = N(got["terms"])
    e = dict(loss=rel(N(got["loss"]), ref["loss"]))
    for i, name in enumerate(("kl", "sw2", "sw2_max")):
        e[name] = rel(t[i], ref["terms"][i])
    for k, r in (("per", "per"), ("G", "G"), ("Theta", "Theta"), ("dz", "dz"), ("dmu", "dmu"), ("dlv", "dlogvar")):
        e[r] = rel(N(got[k]), ref[r])
    return e


def check(got, ref, tag):
    e = errors(got, ref)
    print(tag, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= BAR, (tag, k, v)
    return e


def same_bits(a, b, keys=None):
    for k in (a if keys is None else keys):
        assert torch.equal(a[k], b[k]), k


def same_order(got, ref):
    """The device ranked the rows as the restatement did: G agrees in every element to fp64 rounding, which it cannot
    when two rows of unequal projections (or of equal ones, in another order) were exchanged and v is not constant."""
    scale = np.abs(ref["G"]).max()
    assert np.abs(N(got["G"]) - ref["G"]).max() <= 1e-12 * max(scale, 1.0)


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
def test_the_lds_edge_is_where_the_cases_put_it():
    from hipvae import abi
    assert abi.lib.itcv_sw_lds_rows() == 4096 and (4096, 8, 3) in SHAPES and (4097, 8, 3) in SHAPES
    assert abi.lib.itcv_sw_workspace(4096, 3, 8) == 0 < abi.lib.itcv_sw_workspace(4097, 3, 8)


@pytest.mark.parametrize("Bt, D, L", SHAPES)
def test_kernel_against_restatement(golden, Bt, D, L):
    c = case(golden, Bt, D, L)
    lam, beta = c["hp"]
    dense = run(c["z"], c["prior"], c["t"], c["mu"], c["lv"], lam, beta)
    check(dense, c["ref"], f"[{Bt}x{D}x{L} dense]")
    same_order(dense, c["ref"])
    # the same bits from strided views (z and the prior read in place): the nan around them is not read
    same_bits(dense, run(c["z"], c["prior"], c["t"], c["mu"], c["lv"], lam, beta, layout="strided"))
    p = f"{Bt}x{D}x{L}:"
    if p + "dz" in golden:                # the stored expected values themselves
        for k in ("dz", "G", "per"):
            assert np.abs(N(dense[k]) - golden[p + k]).max() <= BAR * np.abs(golden[p + k]).max(), k
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


# ---- 2. exact cases: the stable order on the device -----------------------------------------------------------------------
def _exact(z, prior, t, mu, lv, lam=3.0, beta=0.5):
    """No gap condition here: ties are the point.  A tie is exact on the device too -- equal rows get equal bits -- so
    the order is decided by the row index on both sides."""
    ref = R.sw(z, prior, t, mu, lv, lam, beta)
    got = run(z, prior, t, mu, lv, lam, beta)
    same_order(got, ref)
    check(got, ref, "[exact]")
    return got, ref


def test_duplicated_rows(golden):
    c = case(golden, 33, 5, 3)
    z = c["z"].copy()
    z[5], z[17], z[32], z[0] = z[2], z[2], z[2], z[31]
    order = R.distance(z, c["prior"], c["t"])["order"]
    for l in range(3):                                   # the duplicates sit next to each other in row order
        pos = {int(r): k for k, r in enumerate(order[l])}
        assert pos[5] == pos[2] + 1 and pos[17] == pos[2] + 2 and pos[32] == pos[2] + 3 and pos[31] == pos[0] + 1
    got, ref = _exact(z, c["prior"], c["t"], c["mu"], c["lv"])
    assert len({float(v) for v in N(got["G"])[0, [2, 5, 17, 32]]}) == 4        # equal u, four different v
    # every row equal: the order is the identity for any direction, G[l][i] = u - sort(v)[i]
    same = np.repeat(c["z"][:1], 33, axis=0)
    got, ref = _exact(same, c["prior"], c["t"], c["mu"], c["lv"])
    assert np.all(np.diff(N(got["G"]), axis=1) <= 0)
    # +0 and -0 are one key: a column of zeros of either sign, one direction along it
    zero = np.zeros((6, 2), np.float32)
    zero[::2, 0] = -0.0
    zero[:, 1] = [3, 1, 2, 0, 5, 4]
    pr = np.stack([np.arange(6, dtype=np.float32), np.zeros(6, np.float32)], 1)
    _exact(zero, pr, np.array([[2.0, 0.0], [0.0, -1.0]], np.float32), zero, zero)


@pytest.mark.parametrize("Bt", [33, 64, 1025])
def test_sorted_and_reversed_inputs(Bt):
    rng = np.random.default_rng(Bt)
    col = np.sort(rng.normal(size=Bt)).astype(np.float32)
    pr = rng.normal(size=(Bt, 2)).astype(np.float32)
    t = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 3.0]], np.float32)       # ascending, descending and constant projections
    for z0 in (col, col[::-1].copy()):
        z = np.stack([z0, np.full(Bt, 0.25, np.float32)], 1)
        _exact(z, pr, t, z, pr)


def test_equal_sets_give_exact_zeros(golden):
    c = case(golden, 65, 4, 3)
    got, ref = _exact(c["z"], c["z"].copy(), c["t"], c["mu"], c["lv"], beta=0.0)
    assert float(got["loss"]) == 0.0 and not got["per"].any() and not got["G"].any() and not got["dz"].any()
    assert not got["terms"][1:].any()


def test_shift_identity(golden):
    c = case(golden, 65, 4, 3)
    shift = np.array([0.5, -0.25, 1.0, 0.125], np.float32)
    z = c["prior"] + shift                               # fp32: the restatement sees the same rounded rows
    got, ref = _exact(z, c["prior"], c["t"], c["mu"], c["lv"])
    want = ((R.directions(c["t"]) @ shift.astype(np.float64)) ** 2).mean()
    assert abs(float(got["terms"][1]) - want) <= 1e-6 * want                    # fp32 rows: (prior + c) - prior is c to 2^-24


# ---- 3. layouts and scaling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bt, D, L, Bl", [(33, 5, 3, 5), (65, 130, 33, 1), (17, 65, 4, 17)])
def test_local_rows_and_upstream_gradient(golden, Bt, D, L, Bl):
    """The KL of a rank's rows only (Bl need not be Bt) and an upstream gradient other than 1."""
    c = case(golden, Bt, D, L)
    mu, lv = c["mu"][:Bl], c["lv"][:Bl]
    ref = reference(c["z"], c["prior"], c["t"], mu, lv, 2.0, 1.5)
    check(run(c["z"], c["prior"], c["t"], mu, lv, 2.0, 1.5), ref, f"[{Bt}x{D}x{L} Bl {Bl}]")
    got = run(c["z"], c["prior"], c["t"], mu, lv, 2.0, 1.5, layout="strided", g=-0.375)
    ref = dict(ref, dz=-0.375 * ref["dz"], dmu=-0.375 * ref["dmu"], dlogvar=-0.375 * ref["dlogvar"])
    check(got, ref, f"[{Bt}x{D}x{L} Bl {Bl} g=-0.375 strided]")


def test_kl_and_distance_parts(golden):
    import ops
    c = case(golden, 33, 5, 3)
    beta, lam = 0.75, 3.0
    prior, t = G(c["prior"]), G(c["t"])

    def grads(fn, lv=None):
        z, mu = G(c["z"]).requires_grad_(True), G(c["mu"]).requires_grad_(True)
        lv = G(c["lv"] if lv is None else lv).requires_grad_(True)
        out = fn(z, mu, lv)
        return (out.detach(),) + torch.autograd.grad(out, (z, mu, lv), allow_unused=True)

    def close(x, y, tag):
        x, y = N(x), N(y)
        err = np.abs(x - y).max() / np.abs(y).max()
        print(tag, f"{err:.2e}")
        assert err <= BAR, (tag, err)

    whole = grads(lambda z, mu, lv: ops.sw_kl_loss(z, mu, lv, prior, t, beta, lam))
    reg = grads(lambda z, mu, lv: ops.sw_regularizer(z, prior, t, lam))
    kl = grads(lambda z, mu, lv: ops.kl_divergence(lv, mu, reduce="mean", scale=beta))
    assert reg[2] is None and reg[3] is None and kl[1] is None    # the regulariser reads z only, the KL never
    close(whole[0], reg[0] + kl[0], "loss = regulariser + beta KL")
    assert torch.equal(whole[1], reg[1])                         # dz does not depend on the KL at all
    close(whole[2], kl[2], "dmu")
    close(whole[3], kl[3], "dlogvar")
    plain = grads(lambda z, mu, lv: ops.sw_kl_loss(z, mu, lv, prior, t, beta, 0.0))
    close(plain[0], kl[0], "lambda = 0: beta KL")
    assert not plain[1].any()                                    # ... and no gradient reaches z, exactly
    close(plain[2], kl[2], "lambda = 0: its dmu")
    close(plain[3], kl[3], "lambda = 0: its dlogvar")
    # without a KL coefficient the KL's value does not reach the result, whatever it is
    lv_inf = c["lv"].copy()
    lv_inf[0, 0] = 100.0                  # exp overflows fp32: the KL is infinite
    r0 = grads(lambda z, mu, lv: ops.sw_kl_loss(z, mu, lv, prior, t, 0.0, lam))
    r1 = grads(lambda z, mu, lv: ops.sw_kl_loss(z, mu, lv, prior, t, 0.0, lam), lv=lv_inf)
    assert torch.isfinite(r1[0]) and torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    assert not r1[2].any() and not r1[3].any()
    assert torch.equal(r0[0], reg[0]) and torch.equal(r0[1], reg[1])
    # a direction of norm zero stays zero and contributes nothing
    t0 = c["t"].copy()
    t0[1] = 0.0
    ref = R.sw(c["z"], c["prior"], t0, c["mu"], c["lv"], lam, beta)
    got = run(c["z"], c["prior"], t0, c["mu"], c["lv"], lam, beta)
    check(got, ref, "[zero direction]")
    assert not got["Theta"][1].any() and not got["G"][1].any() and float(got["per"][1]) == 0.0


# ---- 4. bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bt, D, L", [(64, 128, 50), (65, 130, 33), (12, 6, 257), (1025, 3, 3)])
def test_bitwise_reproducible_and_independent_of_the_grid(golden, Bt, D, L):
    from hipvae import functional as HF
    c = case(golden, Bt, D, L)
    lam, beta = c["hp"]
    args = (c["z"], c["prior"], c["t"], c["mu"], c["lv"], lam, beta)
    a = run(*args)
    same_bits(a, run(*args))
    try:
        for blocks in (1, 2):
            with HF.option_scope("sw_max_blocks", blocks):
                same_bits(a, run(*args))
    finally:
        HF.set_option("sw_max_blocks", 0)
    # another split of the local rows (another Bl, mu / logvar taken from other rows): the distance keeps its bits
    Bl = max(Bt // 4, 1)
    s = run(c["z"], c["prior"], c["t"], c["mu"][Bt - Bl:], c["lv"][Bt - Bl:], lam, beta)
    same_bits(a, s, ("per", "G", "Theta", "dz"))
    assert torch.equal(a["terms"][1:], s["terms"][1:])


def test_workspace_path_gives_the_bits_of_the_lds_path(golden):
    from hipvae import abi
    from hipvae import functional as HF
    c = case(golden, 65, 130, 33)
    lam, beta = c["hp"]
    args = (c["z"], c["prior"], c["t"], c["mu"], c["lv"], lam, beta)
    a = run(*args)
    try:
        with HF.option_scope("sw_lds_rows", 1):
            assert abi.lib.itcv_sw_lds_rows() == 1 and abi.lib.itcv_sw_workspace(65, 33, 130) == 33 * 1312
            same_bits(a, run(*args))
            with HF.option_scope("sw_max_blocks", 2):
                assert abi.lib.itcv_sw_workspace(65, 33, 130) == 2 * 1312
                same_bits(a, run(*args))
    finally:
        HF.set_option("sw_lds_rows", 0)
        HF.set_option("sw_max_blocks", 0)
    assert abi.lib.itcv_sw_workspace(65, 33, 130) == 0


@pytest.mark.parametrize("Bt, D, L", [(65, 130, 33), (1025, 3, 3), (31, 5, 3)])
@pytest.mark.parametrize("rows", [1, 2, 16, 100])
def test_workspace_path_with_every_mix_of_staged_and_in_place_steps(golden, Bt, D, L, rows):
    """On the workspace path the steps of the sort that stay inside an aligned chunk (the largest power of two of rows that
    the LDS limit allows) run on the chunk staged in LDS, the others on the workspace in place.  ``sw_lds_rows`` moves the
    limit: 1 runs every step in place, 2 / 16 / 100 (chunks of 2 / 16 / 64 rows) mix both kinds, mirror steps and the
    steps behind them, with a last chunk that is not full.  Same bits as with the keys in LDS, and the restatement's
    order."""
    from hipvae import functional as HF
    c = case(golden, Bt, D, L)
    lam, beta = c["hp"]
    args = (c["z"], c["prior"], c["t"], c["mu"], c["lv"], lam, beta)
    a = run(*args)
    try:
        with HF.option_scope("sw_lds_rows", rows):
            b = run(*args)
    finally:
        HF.set_option("sw_lds_rows", 0)
    same_bits(a, b)
    same_order(b, c["ref"])


@pytest.mark.parametrize("Bt, D, L", [(65, 130, 33), (4097, 8, 3), (512, 128, 50)])
def test_forward_only_form_equals_the_hook_bit_for_bit(golden, Bt, D, L):
    import ops
    c = case(golden, Bt, D, L)
    full = run(c["z"], c["prior"], c["t"], c["mu"], c["lv"], 1.0, 0.0)
    for layout in ("dense", "strided"):
        sw2, per = ops.sliced_wasserstein(place(c["z"], layout), place(c["prior"], layout), G(c["t"]))
        assert sw2.shape == () and sw2.dtype == torch.float32 and per.dtype == torch.float64 and not sw2.requires_grad
        assert torch.equal(sw2, full["terms"][1]) and torch.equal(sw2, full["loss"]) and torch.equal(per, full["per"])


# ---- 5. scores ---------------------------------------------------------------------------------------------------------
def test_score_against_the_restatement_with_the_same_directions():
    from hipvae import quality as Q
    rng = np.random.default_rng(21)
    real = (rng.normal(size=(300, 12)) * 1.5 + 0.3).astype(np.float32)
    fake = rng.normal(size=(300, 12)).astype(np.float32)
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    got = Q.sliced_wasserstein_distance(G(real), G(fake), num_projections=40, seed=6)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev()), dev_state)
    t = Q.sliced_wasserstein_directions(40, 12, seed=6).numpy()
    assert R.min_gap(real, fake, t) >= GAP
    ref = R.distance(real, fake, t)
    assert sorted(got) == ["per", "sw2", "sw2_std", "swd"] and got["per"].dtype == torch.float64
    assert abs(got["sw2"] - ref["sw2"]) <= 1e-12 * ref["sw2"]
    assert abs(got["swd"] - np.sqrt(ref["sw2"])) <= 1e-12 * np.sqrt(ref["sw2"])
    assert np.abs(N(got["per"]) - ref["per"]).max() <= 1e-12 * ref["per"].max()
    se = ref["per"].std(ddof=1) / np.sqrt(40)
    assert abs(got["sw2_std"] - se) <= 1e-10 * se
    again = Q.sliced_wasserstein_distance(G(real), G(fake), num_projections=40, seed=6)
    assert torch.equal(again["per"], got["per"]) and again["sw2"] == got["sw2"] and again["sw2_std"] == got["sw2_std"]
    other = Q.sliced_wasserstein_distance(G(real), G(fake), num_projections=40, seed=7)
    assert other["sw2"] != got["sw2"]
    one = Q.sliced_wasserstein_distance(G(real), G(fake), num_projections=1, seed=6)
    assert one["sw2_std"] == 0.0 and one["per"].shape == (1,)
    assert Q.sliced_wasserstein_distance(G(real), G(real), num_projections=5)["swd"] == 0.0
    with pytest.raises(ValueError, match="non-finite"):
        bad = real.copy()
        bad[3, 3] = np.inf
        Q.sliced_wasserstein_distance(G(bad), G(fake), num_projections=5)


class _Images:
    """A dataset of 96 random images (no factors)."""

    def __init__(self):
        self.x = torch.rand(96, 3, 32, 32, generator=torch.Generator().manual_seed(9))

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i]


def test_compute_sliced_wasserstein_in_both_spaces():
    import models
    from hipvae import density
    from hipvae import quality as Q
    torch.manual_seed(0)
    model = models.SoftIntroVAE(arch="conv", **TINY).to(dev()).train()
    ds = _Images()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    cpu_state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev())
    kw = dict(num=96, num_projections=16, batch_size=40, seed=3)
    feat = Q.compute_sliced_wasserstein(ds, model, **kw)
    assert sorted(feat) == ["indices", "per", "sw2", "sw2_std", "swd"] and len(feat["indices"]) == 96
    assert np.isfinite(feat["swd"]) and feat["swd"] > 0 and feat["per"].shape == (16,)
    assert abs(feat["swd"] ** 2 - feat["sw2"]) <= 1e-12 * feat["sw2"]
    # ... it is the distance of the features that compute_sample_quality uses
    q = Q.compute_sample_quality(ds, model, num_real=96, batch_size=40, seed=3, scores=("kid",))
    by_hand = Q.sliced_wasserstein_distance(q["features"]["real"], q["features"]["fake"], 16, 3)
    assert by_hand["sw2"] == feat["sw2"] and torch.equal(by_hand["per"], feat["per"])
    lat = Q.compute_sliced_wasserstein(ds, model, space="latent", **kw)
    assert np.isfinite(lat["swd"]) and lat["swd"] > 0 and lat["sw2"] != feat["sw2"]
    assert Q.compute_sliced_wasserstein(ds, model, space="latent", **kw)["sw2"] == lat["sw2"]
    assert Q.compute_sliced_wasserstein(ds, model, space="latent", prior="normal", **kw)["sw2"] == lat["sw2"]
    # the priors: a fitted mixture, a given one, a VampPrior
    for space in ("feature", "latent"):
        a = Q.compute_sliced_wasserstein(ds, model, space=space, prior="gmm", gmm_params=dict(n_components=2), **kw)
        assert isinstance(a["gmm"], density.GaussianMixture) and a["gmm"].n_components == 2 and np.isfinite(a["swd"])
        b = Q.compute_sliced_wasserstein(ds, model, space=space, prior=a["gmm"], **kw)
        assert b["gmm"] is a["gmm"] and b["sw2"] == a["sw2"]
        gen = torch.Generator().manual_seed(1)
        vamp = density.VampPrior(torch.randn(5, 10, generator=gen).to(dev()), (torch.randn(5, 10, generator=gen) - 1.0).to(dev()))
        v = Q.compute_sliced_wasserstein(ds, model, space=space, prior=vamp, **kw)
        assert v["prior"] is vamp and "gmm" not in v and np.isfinite(v["swd"])
        assert v["sw2"] != (feat if space == "feature" else lat)["sw2"]
    # the model and the global generators are as they were
    assert model.training and all(torch.equal(v, model.state_dict()[k]) for k, v in before.items())
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev()), dev_state)


# ---- 6. training steps against the oracle ----------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


L_STEP = 7


def _oracle_trainer(name, state, lam, hp, draws):
    from oracle import latent_math as lm
    from oracle.network import Net
    from oracle.steps import Trainer

    class SwTrainer(Trainer):
        """The oracle's step with the torch restatement of the hook on every ``reduce="mean"`` call; the prior and the
        directions of those calls come from ``draws``, in call order.  The oracle is evaluated in fp64 (its network, the
        batch and the draws are widened), as in test_hip_mmd.py's step test."""

        def kl_loss(self, z, mu, logvar, reduce="mean", beta=None):
            beta = self.beta_kl if beta is None else beta
            if reduce == "mean":
                prior, t = draws.pop(0), draws.pop(0)
                out = R.torch_hook(z, prior, t, mu, logvar, lam, beta)
            else:
                out = beta * lm.kl(logvar, mu, reduce)
            self.trace.setdefault("kl", []).append(out.detach().reshape(-1).clone())
            return out

    state = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in state.items()}
    return SwTrainer(name, Net("conv", state=state, **TINY), dataset_size=1000,
                     beta_kl=hp[0], beta_rec=hp[1], beta_neg=hp[2], gamma_r=hp[3], clip=hp[4], lr=hp[5])


def _hip_solver(name, state, lam, hp, L=L_STEP):
    import models
    from solvers import IntroSWAESolver, SWAESolver
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    model = model.to(dev()).train()
    args = [_DS(), model, 8, torch.optim.Adam(model.encoder.parameters(), lr=hp[5]),
            torch.optim.Adam(model.decoder.parameters(), lr=hp[5]), "mse", hp[0], hp[1]]
    if name == "intro":
        args += [hp[2], hp[3]]
    cls = IntroSWAESolver if name == "intro" else SWAESolver
    solver = cls(*args, dev(), False, None, clip=hp[4], lambda_sw=lam, num_projections=L)
    assert solver.conv_math == "fp32"
    return solver, model


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


def _queue(name, draws, pri):
    """The recorded draws in the HIP solver's call order: the prior and then the directions of a ``reduce="mean"`` call
    are drawn inside that call.  VAE: eps, (prior, t).  Intro: noise, eps_real, (prior, t) of the real batch, eps_rec,
    eps_fake, eps_rec_D, eps_fake_D, (prior, t) of the reconstructions, (prior, t) of the fakes."""
    if name == "vae":
        return [draws[0], *pri[0:2]]
    return [draws[0], draws[1], *pri[0:2], draws[2], draws[3], draws[4], draws[5], *pri[2:4], *pri[4:6]]


def _draws(g, name):
    nd, npr = (6, 3) if name == "intro" else (1, 1)
    x = torch.rand(8, 3, 32, 32, generator=g)
    draws = [torch.randn(8, 10, generator=g) for _ in range(nd)]
    pri = [torch.randn((8, 10) if k % 2 == 0 else (L_STEP, 10), generator=g) for k in range(2 * npr)]
    return x, draws, pri


@pytest.mark.parametrize("name", ["vae", "intro"])
def test_two_steps_against_the_oracle(name):
    """Two training steps of the tiny model (B = 8, fp32 arithmetic on the device, recorded draws) against the CPU oracle
    in fp64 whose KL hook is the torch restatement.  Tolerances: those of test_hip_mmd.py's step test, which are
    test_hip_model.py's run_golden_steps for this model -- the returned dict to 1e-4 at step 0 and 3e-4 at step 1, every
    hook output to 3e-4 / 3e-3 of its scale."""
    import ops
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    lam = 2.0
    state = _init_state()
    ref_draws = []
    tr = _oracle_trainer(name, state, lam, hp, ref_draws)
    solver, _ = _hip_solver(name, state, lam, hp)
    kl_log, kl0 = [], solver.compute_kl_loss
    solver.compute_kl_loss = lambda *a, _f=kl0, **k: (kl_log.append(_f(*a, **k)), kl_log[-1])[1]
    g = torch.Generator().manual_seed(1)
    keys = ("loss_enc", "loss_dec", "loss_kl", "loss_rec", "L2")
    for s in range(2):
        x, draws, pri = _draws(g, name)
        kl_log.clear()
        with ops.noise_queue([t.clone() for t in _queue(name, draws, pri)]):
            got = solver.train_step(x, s)
            assert not ops._noise["queue"]                       # every recorded draw was taken
        ref_draws[:] = [t.double() for t in pri]
        ref = tr.step(x.double(), [t.double() for t in draws])
        assert not ref_draws
        first = got if s == 0 else first
        print(name, s, {k: (got[k], ref[k]) for k in keys})
        np.testing.assert_allclose([got[k] for k in keys], [ref[k] for k in keys], rtol=1e-4 if s == 0 else 3e-4)
        tol = 3e-4 if s == 0 else 3e-3
        assert len(kl_log) == len(tr.trace["kl"]) == (5 if name == "intro" else 1)
        for i, (t, want) in enumerate(zip(kl_log, tr.trace["kl"])):
            err = float((t.detach().reshape(-1).cpu() - want).abs().max())
            assert err < tol * float(want.abs().max()), (name, s, i, err)
    # the distance is live: the same first step without it reports another KL term
    plain, _ = _hip_solver(name, state, 0.0, hp)
    x, draws, pri = _draws(torch.Generator().manual_seed(1), name)
    with ops.noise_queue(_queue(name, draws, pri)):
        d0 = plain.train_step(x, 0)
    assert abs(d0["loss_kl"] - first["loss_kl"]) > 1e-2 * abs(first["loss_kl"]), (d0["loss_kl"], first["loss_kl"])


def test_writer_records_the_terms():
    import ops

    class Recorder:
        def __init__(self):
            self.log = {}

        def add_scalar(self, tag, value, global_step=None):
            self.log[tag] = float(value)

        def add_scalars(self, tag, values, global_step=None):
            self.log[tag] = {k: float(v) for k, v in values.items()}

    solver, _ = _hip_solver("vae", _init_state(), 2.0, [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4])
    solver.writer = Recorder()
    z, prior, t, mu, lv = R.make_inputs(8, 10, L_STEP, seed=2)
    with ops.noise_queue([torch.from_numpy(prior), torch.from_numpy(t)]):
        loss = solver.compute_kl_loss(G(z), G(mu), G(lv), write=True)
    ref = R.sw(z, prior, t, mu, lv, 2.0, 0.5)
    assert abs(float(loss) - ref["loss"]) <= BAR * abs(ref["loss"])
    log = solver.writer.log
    assert sorted(log["sw"]) == ["sw2", "sw2_max"]
    assert abs(log["kl_loss_unscaled"] - ref["terms"][0]) <= BAR * ref["terms"][0]
    assert abs(log["sw"]["sw2"] - ref["terms"][1]) <= BAR * ref["terms"][1]
    assert abs(log["sw"]["sw2_max"] - ref["terms"][2]) <= BAR * ref["terms"][2]


# ---- 7. graph capture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vae", "intro"])
def test_captured_steps_equal_eager_steps_and_changes_recapture(name):
    """With enable_graph() the trajectory is the eager one from the same state through the capture, bit for bit; after
    ``lambda_sw *= 2`` it still is, which it could not be if the step replayed the graph captured with the old value:
    the key re-captures.  A change of ``num_projections`` (another shape of the direction draw) re-captures too."""
    hp = [0.5, 0.75, 512.0, 1e-8, 100.0, 2e-4]
    state = _init_state()
    gen = torch.Generator().manual_seed(5)
    xs = [torch.rand(8, 3, 32, 32, generator=gen).to(dev()) for _ in range(2)]

    def trajectory(graph):
        solver, model = _hip_solver(name, state, 2.0, hp)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys = [], []
        for k in range(12):
            if k == 6:
                solver.lambda_sw *= 2
            if k == 9:
                solver.num_projections = 20
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8, 10, 11) else None)
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), keys

    (e, we, _), (gr, wg, keys) = trajectory(False), trajectory(True)

    def holds(key, pair):
        return key is not None and any(key[i:i + 2] == pair for i in range(len(key) - 1))

    assert holds(keys[3], (2.0, L_STEP)) and keys[3] == keys[4] == keys[5]
    assert holds(keys[7], (4.0, L_STEP)) and keys[7] == keys[8] != keys[5]
    assert holds(keys[10], (4.0, 20)) and keys[10] == keys[11] != keys[8]
    print(name, "largest difference of a reported value %.3e, of a weight %.3e" % (
        max(abs(x[k] - y[k]) / (abs(x[k]) + 1e-30) for x, y in zip(e, gr) for k in x), float((we - wg).abs().max())))
    for x, y in zip(e, gr):
        assert x == y, (x, y)                            # the captured step's reported values, bit for bit
    assert torch.equal(we, wg)
    # the doubled distance is visible in the eager trajectory itself (the check above is not vacuous)
    assert abs(e[6]["loss_kl"] - e[5]["loss_kl"]) > 1e-2 * abs(e[5]["loss_kl"])
