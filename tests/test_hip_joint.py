"""GPU tests of the JointVAE / AnnealedVAE latent op (csrc/joint.hip, ops.joint_latent) and its solvers (solvers/joint.py)
against the fp64 restatement tests/joint_ref.py.

Bounds: the loss and the four terms relative to the fp64 value; z (as a whole, and its discrete block y on its own), dmu and
dlogvar normwise, max |err| / max |value|.  The ceiling is the project's fp32 bar, 1e-4; a quantity that is exactly zero in
fp64 (the logvar gradient of the discrete block, the KL and the capacity of an empty block) must come out exactly zero.
The capacities of a case keep |KL - C| = KL / 2 (joint_ref.make_inputs), so no sign hangs on a last bit.  The kernels
compute in fp64 and round once to fp32, so they stay near 2^-24 = 6e-8.  Worst values measured on an MI355X over every case
of test_kernel_against_restatement (printed by it):

    loss 3.93e-08  kl_z 5.66e-08  kl_c 4.53e-08  cap_z 5.66e-08  cap_c 4.53e-08  z 4.12e-08  y 4.73e-08  dmu 5.30e-08
    dlogvar 4.20e-08
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import joint_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
TINY = dict(cdim=3, zdim=10, channels=(8, 16, 32), image_size=32)
SPEC = dict(cont=6, disc=(4,))
# one row, one column, purely discrete, the four-rows-per-block tail; zdim 63 / 64 / 65; a group across the 64-lane edge and
# the tail; the benchmark's width; one 511-wide group; 256 + 256; 256 groups of two; a grid larger than one trip (256 blocks
# of 4 rows)
CASES = [(1, 1, ()), (1, 0, (2,)), (2, 3, (2,)), (7, 6, (3,)), (33, 10, (10,)), (4, 61, (2,)), (3, 62, (2,)), (5, 60, (5,)),
         (9, 60, (3, 7, 59)), (32, 118, (10,)), (2, 0, (511,)), (3, 256, (256,)), (2, 0, (2,) * 256), (1025, 10, (3, 4))]
G_LOSS = -1.25
WORST = {}


def dev():
    return torch.device("cuda:0")


def G(a):
    return torch.from_numpy(np.array(a, order="C")).to(dev())      # a copy: the cases are read-only


def N(t):
    return t.detach().double().cpu().numpy()


def tag(B, nc, disc):
    """``<B>x<n_cont>+<K_1>.<K_2>...:``, four or more equal sizes as ``<K>*<G>``."""
    sizes = ".".join(map(str, disc)) if len(set(disc)) != 1 or len(disc) < 4 else f"{disc[0]}*{len(disc)}"
    return f"{B}x{nc}+{sizes}:"


def sign_tag(signs):
    return "+-"[signs[0] < 0] + "+-"[signs[1] < 0]


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "joint.npz"))
    return {k: g[k] for k in g.files}


_INPUTS, _REFS = {}, {}


def case(golden, B, nc, disc):
    """The stored inputs of a case, regenerated once and never modified."""
    key = (B, nc, disc)
    if key not in _INPUTS:
        p = tag(B, nc, disc)
        seed = int(golden[p + "seed"])
        mu, lv, eps, u, caps = R.make_inputs(B, nc, disc, seed)
        assert np.array_equal(golden[p + "checksum"], [a.astype(np.float64).sum() for a in (mu, lv, eps, u)])
        dz = R.make_dz(B, nc + sum(disc), seed)
        beta, gz, gc, tau = (float(v) for v in golden["hp"])
        for a in (mu, lv, eps, u, dz):
            a.setflags(write=False)
        _INPUTS[key] = dict(mu=mu, lv=lv, eps=eps, u=u, dz=dz, caps=caps, nc=nc, disc=disc, beta=beta, gz=gz, gc=gc, tau=tau)
    return _INPUTS[key]


def reference(golden, c, signs):
    """The restatement's values of a case under the capacities of ``signs``, computed once."""
    key = (c["mu"].shape[0], c["nc"], c["disc"], signs)
    if key not in _REFS:
        cap = c["caps"][signs]
        p = tag(*key[:3]) + sign_tag(signs)
        assert np.array_equal(golden[p + ":cap"], cap)
        ref = R.joint(c["mu"], c["lv"], c["eps"], c["u"], c["nc"], c["disc"], cap, c["gz"], c["gc"], c["beta"], c["tau"],
                      c["dz"], G_LOSS)
        want = float(golden[p + ":loss"])
        assert abs(ref["loss"] - want) <= 1e-12 * abs(want)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def strided(x):
    """The right part of a wider nan tensor."""
    wide = np.full((x.shape[0], x.shape[1] + 3), np.nan, dtype=np.float32)
    wide[:, 3:] = x
    return G(wide)[:, 3:]


def layouts(c, layout, lv=None):
    """(mu, logvar, eps, u) device tensors holding the case's values in the given layout."""
    mu, lv, eps, u = c["mu"], c["lv"] if lv is None else lv, c["eps"], c["u"]
    B, D = mu.shape
    if layout == "dense":
        return G(mu), G(lv), G(eps), G(u)
    if layout == "packed":            # the halves of one [B, 2D] tensor, inside nan rows that must not be read
        buf = np.full((B + 2, 2 * D), np.nan, dtype=np.float32)
        buf[1:-1, :D], buf[1:-1, D:] = mu, lv
        t = G(buf)[1:-1]
        a, b = t[:, :D], t[:, D:]
        assert b.data_ptr() == a.data_ptr() + 4 * D and (B == 1 or a.stride() == (2 * D, 1))
        return a, b, G(eps), G(u)
    if layout == "strided":
        out = tuple(strided(x) for x in (mu, lv, eps, u))
        assert B == 1 or out[0].stride() == (D + 3, 1)
        return out
    raise ValueError(layout)


def run(c, cap, layout="dense", dz=None, g=G_LOSS, lv=None, u=None):
    """z, loss, terms and both gradients of ops.joint_latent on the device; ``cap`` a pair or a device tensor, ``dz`` a
    device tensor or None (the case's, dense)."""
    import ops
    a, b, e, uu = layouts(c, layout, lv)
    uu = uu if u is None else G(u)
    a, b = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    cap = cap if isinstance(cap, torch.Tensor) else torch.tensor(cap, dtype=torch.float64, device=dev())
    z, loss, terms = ops.joint_latent(a, b, c["nc"], c["disc"], cap, c["gz"], c["gc"], beta=c["beta"], temperature=c["tau"],
                                      eps=e if c["nc"] else None, u=uu if c["disc"] else None, with_terms=True)
    assert z.shape == c["mu"].shape and loss.shape == () and terms.shape == (4,) and not terms.requires_grad
    assert z.requires_grad and loss.requires_grad and z.dtype == loss.dtype == terms.dtype == torch.float32
    dz = G(c["dz"]) if dz is None else dz
    dmu, dlv = torch.autograd.grad((z, loss), (a, b), grad_outputs=(dz, torch.tensor(g, device=dev())))
    return dict(z=z.detach(), loss=loss.detach(), terms=terms, dmu=dmu, dlv=dlv)


def errors(got, ref, nc):
    """Errors of a run against the restatement; a quantity that is exactly zero there must be exactly zero."""
    def rel(x, want):
        x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
        assert np.isfinite(x).all()
        scale = np.abs(want).max() if want.size else 0.0
        if scale == 0.0:
            assert not x.any()
            return 0.0
        return float(np.abs(x - want).max() / scale)

    t, z = N(got["terms"]), N(got["z"])
    assert not got["dlv"][:, nc:].any(), "the logvar gradient of the discrete block is not exactly zero"
    return dict(loss=rel(N(got["loss"]), ref["loss"]), kl_z=rel(t[0], ref["terms"][0]), kl_c=rel(t[1], ref["terms"][1]),
                cap_z=rel(t[2], ref["terms"][2]), cap_c=rel(t[3], ref["terms"][3]), z=rel(z, ref["z"]),
                y=rel(z[:, nc:], ref["z"][:, nc:]), dmu=rel(N(got["dmu"]), ref["dmu"]),
                dlogvar=rel(N(got["dlv"]), ref["dlogvar"]))


def check(got, ref, nc, label):
    e = errors(got, ref, nc)
    print(label, " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= BAR, (label, k, v)
    return e


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("signs", R.SIGNS, ids=sign_tag)
@pytest.mark.parametrize("B, nc, disc", CASES, ids=[tag(*c)[:-1] for c in CASES])
def test_kernel_against_restatement(golden, B, nc, disc, signs):
    c = case(golden, B, nc, disc)
    ref = reference(golden, c, signs)
    got = run(c, c["caps"][signs])
    check(got, ref, nc, f"[{tag(B, nc, disc)}{sign_tag(signs)}]")
    t = N(got["terms"])
    assert (np.sign(t[0] - t[2]), np.sign(t[1] - t[3])) == (signs[0] if nc else 0, signs[1] if disc else 0)
    assert np.allclose(N(got["z"])[:, nc:].sum(1), len(disc), rtol=0, atol=1e-5)        # every y_i is a distribution
    print("worst so far:", " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


def test_exact_zeros(golden):
    """What is exactly zero in fp64 is exactly zero: the KL and the capacity of an empty block (its sign is then 0, as
    torch.abs differentiates, and it adds nothing); with beta = 0 and no incoming gradient of z the loss and both
    gradients."""
    for B, nc, disc in ((2, 0, (511,)), (1, 1, ())):
        c = case(golden, B, nc, disc)
        got = run(c, c["caps"][(1, 1)])
        t = N(got["terms"])
        assert (t[0] == 0.0 and t[2] == 0.0) if nc == 0 else (t[1] == 0.0 and t[3] == 0.0)
    # beta = 0 and no incoming gradient of z: everything is exactly zero
    c = dict(case(golden, 33, 10, (10,)), beta=0.0)
    got = run(c, c["caps"][(1, -1)], dz=torch.zeros(33, 20, device=dev()))
    assert float(got["loss"]) == 0.0 and not got["dmu"].any() and not got["dlv"].any()


# ---- 2. layouts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, nc, disc", [(1, 0, (2,)), (7, 6, (3,)), (5, 60, (5,)), (9, 60, (3, 7, 59)), (3, 256, (256,))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_layouts(golden, B, nc, disc):
    """The packed pair (the halves of one [B, 2D] tensor between nan rows) and strided views, all read in place, give the
    bits of the dense tensors; so does a logvar whose discrete columns are nan -- they are never read -- and their
    gradient stays exactly zero."""
    c = case(golden, B, nc, disc)
    cap = c["caps"][(1, -1)]
    dense = run(c, cap)
    for layout in ("packed", "strided"):
        other = run(c, cap, layout=layout)
        for k in dense:
            assert torch.equal(dense[k], other[k]), (layout, k)
    lv = np.array(c["lv"])
    lv[:, nc:] = np.nan
    for layout in ("dense", "packed"):
        other = run(c, cap, layout=layout, lv=lv)
        for k in dense:
            assert torch.equal(dense[k], other[k]), ("nan logvar", layout, k)
        assert not other["dlv"][:, nc:].any() and torch.isfinite(other["dlv"]).all()


@pytest.mark.parametrize("B, nc, disc", [(5, 60, (5,)), (33, 10, (10,))], ids=lambda v: str(v).replace(" ", ""))
def test_non_contiguous_output_gradient(golden, B, nc, disc):
    """An incoming dz with a row stride (read in place), with a column stride (copied dense) and a broadcast one (what
    ``z.sum().backward()`` sends) give the bits of the dense dz."""
    import ops
    c = case(golden, B, nc, disc)
    cap = c["caps"][(-1, 1)]
    dense = run(c, cap)
    wide = strided(c["dz"])
    assert not wide.is_contiguous()
    tr = G(np.ascontiguousarray(c["dz"].T)).t()
    assert tr.shape == c["dz"].shape and tr.stride() == (1, B)
    for dz in (wide, tr):
        got = run(c, cap, dz=dz)
        for k in dense:
            assert torch.equal(dense[k], got[k]), k
    a, b = G(c["mu"]).requires_grad_(True), G(c["lv"]).requires_grad_(True)
    z, loss = ops.joint_latent(a, b, nc, disc, torch.tensor(cap, dtype=torch.float64, device=dev()), c["gz"], c["gc"],
                               beta=c["beta"], temperature=c["tau"], eps=G(c["eps"]), u=G(c["u"]))
    (z.sum() + G_LOSS * loss).backward()
    ones = run(c, cap, dz=torch.ones(B, nc + sum(disc), device=dev()))
    assert torch.equal(a.grad, ones["dmu"]) and torch.equal(b.grad, ones["dlv"])
    # one output unused: its gradient counts as zero
    D = nc + sum(disc)
    for use_z, want in ((False, run(c, cap, dz=torch.zeros(B, D, device=dev()))), (True, run(c, cap, g=0.0))):
        a.grad = b.grad = None
        z, loss = ops.joint_latent(a, b, nc, disc, torch.tensor(cap, dtype=torch.float64, device=dev()), c["gz"], c["gc"],
                                   beta=c["beta"], temperature=c["tau"], eps=G(c["eps"]), u=G(c["u"]))
        ((z * G(c["dz"])).sum() if use_z else G_LOSS * loss).backward()
        assert torch.equal(a.grad, want["dmu"]) and torch.equal(b.grad, want["dlv"]), use_z


# ---- 3. edge draws, the hard code, bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B, nc, disc", R.EDGE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_edge_draws(golden, B, nc, disc):
    """u exactly 0 (taken as 2^-25) and exactly 1 - 2^-24, the two ends of torch.rand's range: finite, and the
    restatement's values."""
    c = case(golden, B, nc, disc)
    u = R.edge_draws(c["u"], c["mu"], nc, disc)
    assert u.min() == 0.0 and u.max() == np.float32(1.0 - 2.0 ** -24)
    cap = c["caps"][(1, 1)]
    ref = R.joint(c["mu"], c["lv"], c["eps"], u, nc, disc, cap, c["gz"], c["gc"], c["beta"], c["tau"], c["dz"], G_LOSS)
    got = run(c, cap, u=u)
    for k in ("z", "dmu", "dlv", "loss"):
        assert torch.isfinite(got[k]).all(), k
    check(got, ref, nc, f"[{tag(B, nc, disc)} edge draws]")


def test_hard_code(golden):
    """``hard=True``: z_cont is mu bit for bit, every group the one-hot of the FIRST maximum of its logits (ties, made on
    purpose inside one group, across the 64-lane edge and over a whole group, take the lowest column); no gradient."""
    import ops
    for B, nc, disc in ((7, 6, (3,)), (9, 60, (3, 7, 59)), (2, 0, (511,)), (2, 0, (2,) * 256), (1, 1, ())):
        c = case(golden, B, nc, disc)
        mu = np.array(c["mu"])
        if disc:
            s, e = R.groups(nc, disc)[-1]
            mu[0, s:e] = mu[0, s:e].max()                    # a whole group tied: column s
            if B > 1:
                mu[1, e - 1] = mu[1, s + 1] = np.float32(mu[1, s:e].max() + 1.0)      # two equal maxima far apart: the first
        a = G(mu).requires_grad_(True)
        nan = torch.full_like(a, float("nan"))
        z = ops.joint_latent(a, nan, nc, disc, None, 0.0, 0.0, hard=True)
        assert isinstance(z, torch.Tensor) and not z.requires_grad and z.dtype == torch.float32
        want = R.hard(mu, nc, disc)
        assert torch.equal(z, G(want)), (B, nc, disc)
        assert torch.equal(z[:, :nc], a.detach()[:, :nc])
        if disc:
            s, e = R.groups(nc, disc)[-1]
            assert float(z[0, s]) == 1.0 and (B == 1 or float(z[1, s + 1]) == 1.0)
        # a packed view is read in place
        wide = G(np.concatenate([mu, np.full_like(mu, np.nan)], axis=1))
        D = mu.shape[1]
        assert torch.equal(ops.joint_latent(wide[:, :D], wide[:, D:], nc, disc, None, 0.0, 0.0, hard=True), z)


@pytest.mark.parametrize("B, nc, disc", [(33, 10, (10,)), (9, 60, (3, 7, 59)), (3, 256, (256,)), (1025, 10, (3, 4))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_bitwise_repeatable(golden, B, nc, disc):
    c = case(golden, B, nc, disc)
    a, b = run(c, c["caps"][(-1, -1)]), run(c, c["caps"][(-1, -1)])
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 4. the capacity is a run-time value; launches ---------------------------------------------------------------------
def test_capacity_is_read_when_the_kernel_runs(golden):
    """The op, forward and backward, captured in a graph with capacities BELOW the KLs and replayed after the capacity
    tensor was overwritten with capacities ABOVE them: both signs flip, and the replay equals an eager call with the new
    capacities bit for bit."""
    import ops
    c = case(golden, 33, 10, (10,))
    a, b = G(c["mu"]).requires_grad_(True), G(c["lv"]).requires_grad_(True)
    e, u, dz, gl = G(c["eps"]), G(c["u"]), G(c["dz"]), torch.tensor(G_LOSS, device=dev())
    cap = torch.tensor(c["caps"][(1, 1)], dtype=torch.float64, device=dev())

    def op():
        z, loss, terms = ops.joint_latent(a, b, 10, (10,), cap, c["gz"], c["gc"], beta=c["beta"], temperature=c["tau"], eps=e,
                                          u=u, with_terms=True)
        return (z, loss, terms) + torch.autograd.grad((z, loss), (a, b), grad_outputs=(dz, gl))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = [t.detach().clone() for t in op()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = op()
    graph.replay()
    for x, y in zip(first, held):
        assert torch.equal(x, y.detach())
    cap.copy_(torch.tensor(c["caps"][(-1, -1)], dtype=torch.float64))
    graph.replay()
    torch.cuda.synchronize()
    flipped = [t.detach().clone() for t in held]
    eager = run(c, c["caps"][(-1, -1)])
    for x, k in zip(flipped, ("z", "loss", "terms", "dmu", "dlv")):
        assert torch.equal(x, eager[k]), k
    assert torch.equal(flipped[0], first[0]) and not torch.equal(flipped[3], first[3])       # z does not see the capacity
    t0, t1 = N(first[2]), N(flipped[2])
    assert t0[0] > t0[2] and t0[1] > t0[3] and t1[0] < t1[2] and t1[1] < t1[3]
    check(dict(zip(("z", "loss", "terms", "dmu", "dlv"), flipped)), reference(golden, c, (-1, -1)), 10, "[replay]")


@contextlib.contextmanager
def recorded_calls(log):
    """The names of the library calls made through hipvae.functional.call inside the block."""
    from hipvae import functional

    def call(name, *args):
        log.append(name)
        return saved(name, *args)

    saved = functional.call
    functional.call = call
    try:
        yield log
    finally:
        functional.call = saved


def test_one_call_forward_one_backward(golden):
    """The op is ONE library call forward (two launches: include/itcv_hip.h) and ONE backward (one launch), with nothing
    else of the library around them; the hard code is one call."""
    import ops
    c = case(golden, 32, 118, (10,))
    run(c, c["caps"][(1, 1)])
    log = []
    with recorded_calls(log):
        run(c, c["caps"][(1, 1)])
        ops.joint_latent(G(c["mu"]), G(c["lv"]), 118, (10,), None, 0.0, 0.0, hard=True)
    assert log == ["itcv_joint_latent_fwd", "itcv_joint_latent_bwd", "itcv_joint_latent_fwd"], log


# ---- 5. the noise source and what is refused -----------------------------------------------------------------------------
def test_noise_source_and_refusals():
    """``eps=None`` / ``u=None`` take one draw each from the project's noise source, eps first, and none for an empty
    block; what the op cannot take is refused."""
    import ops
    from hipvae import abi
    mu, lv, eps, u, caps = R.make_inputs(4, 6, (4,), 5)
    cap = torch.tensor(caps[(1, 1)], dtype=torch.float64, device=dev())

    def op(m=mu, l=lv, nc=6, disc=(4,), cap=cap, gz=1.0, gc=2.0, **kw):
        return ops.joint_latent(G(m) if isinstance(m, np.ndarray) else m, G(l) if isinstance(l, np.ndarray) else l, nc, disc,
                                cap, gz, gc, **kw)

    with ops.noise_queue([torch.from_numpy(eps), torch.from_numpy(u), torch.zeros(1)]):
        z, loss = op()
        assert len(ops._noise["queue"]) == 1
    want, want_loss = op(eps=G(eps), u=G(u))
    assert torch.equal(z, want) and torch.equal(loss, want_loss)
    with ops.noise_queue([torch.from_numpy(u), torch.zeros(1)]):               # no continuous block: no eps draw
        z, _ = op(m=mu[:, 6:], l=lv[:, 6:], nc=0)
        assert len(ops._noise["queue"]) == 1
    assert torch.equal(z, op(m=mu[:, 6:], l=lv[:, 6:], nc=0, u=G(u))[0])
    with ops.noise_queue([torch.from_numpy(eps), torch.zeros(1)]):             # no discrete block: no u draw
        z, _ = op(m=mu[:, :6], l=lv[:, :6], disc=())
        assert len(ops._noise["queue"]) == 1
    assert torch.equal(z, op(m=mu[:, :6], l=lv[:, :6], disc=(), eps=G(eps))[0])
    torch.cuda.manual_seed(5)
    z1 = op()[0]
    torch.cuda.manual_seed(5)
    e5, u5 = torch.randn((4, 6), device=dev()), torch.rand((4, 4), device=dev())
    assert torch.equal(z1, op(eps=e5, u=u5)[0])                                 # device draws: randn, then rand
    wide = np.zeros((4, 513), np.float32)
    for kw in (dict(l=lv[:, :9]), dict(m=mu[0], l=lv[0]), dict(nc=5), dict(disc=(3,)), dict(nc=9, disc=(1,)),
               dict(m=wide, l=wide, nc=513, disc=()), dict(m=wide[:, :0], l=wide[:, :0], nc=0, disc=()),
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
               dict(gz=-1.0), dict(gc=-1.0), dict(gz=float("inf")), dict(gc=float("nan")),
               dict(eps=G(u)), dict(u=G(eps)),
               dict(cap=cap.cpu()), dict(cap=cap.float()), dict(cap=torch.zeros(3, dtype=torch.float64, device=dev())),
               dict(cap=(0.0, 0.0)), dict(cap=None)):
        with pytest.raises(ValueError):
            op(**kw)
    with pytest.raises(abi.HipExtensionError):
        op(m=torch.from_numpy(mu), l=torch.from_numpy(lv))
    with pytest.raises(abi.HipExtensionError):
        op(eps=torch.from_numpy(eps))
    with pytest.raises(abi.HipExtensionError):
        op(m=G(mu).double(), l=G(lv).double())


# ---- 6. the solvers ------------------------------------------------------------------------------------------------------
class _DS:
    def __len__(self):
        return 1000


HP = dict(beta_kl=0.5, beta_rec=0.75, clip=100.0, lr=2e-4)
ROWS = 8


def _init_state():
    import models
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.SoftIntroVAE(arch="conv", **TINY).state_dict().items()}


def _model(state):
    import models
    model = models.SoftIntroVAE(arch="conv", **TINY)
    model.load_state_dict(state)
    return model.to(dev()).train()


def _solver(state, cls=None, beta_kl=HP["beta_kl"], **kw):
    from solvers import JointVAESolver
    cls = JointVAESolver if cls is None else cls
    model = _model(state)
    solver = cls(_DS(), model, ROWS, torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                 torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), "mse", beta_kl, HP["beta_rec"], dev(),
                 False, None, clip=HP["clip"], **kw)
    assert solver.conv_math == "fp32"
    return solver, model


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(ROWS, 3, 32, 32, generator=g), torch.randn(ROWS, TINY["zdim"], generator=g), \
        torch.rand(ROWS, TINY["zdim"], generator=g)


def _params_close(model, other, lr, steps=1):
    """The bar of tests/test_hip_model.py's run_golden_steps (and of test_hip_ada.py's step tests): Adam's first updates
    are +-lr sign(g), so where |g| is at rounding level 2 lr of a weight can differ per step; the bulk is bounded tightly
    and every element by the Adam limit."""
    a, b = model.state_dict(), other.state_dict()
    diffs = torch.cat([(a[k] - b[k]).abs().reshape(-1) for k in a if a[k].dtype.is_floating_point and "running" not in k])
    assert float(diffs.max()) <= 2.05 * lr * steps, float(diffs.max())
    assert float((diffs > 0.25 * lr * steps).float().mean()) < 2e-3
    assert float(diffs.median()) < 0.02 * lr
    for k in a:
        if "running" in k:
            err = float((a[k] - b[k]).abs().max() / b[k].abs().max())
            assert err < 1e-3, (k, err)


JOINT_KW = dict(latent_spec=SPEC, cont_capacity=(0.0, 8.0, 2, 3.0), disc_capacity=(0.0, 2.0, 2, 2.0), temperature=0.67)


def test_two_train_steps_equal_the_assembled_steps():
    """Two consecutive ``train_step``s with queued draws (eps, then u) against the same steps assembled from
    ``model.encode``, the torch-fp64 transcription of the op, ``model.decode``, the existing loss ops, torch's clip and
    torch's Adam: the returned dicts to 1e-4 (the bar of the existing solver tests), the parameters within their Adam bar.
    The first step is held to the capacities (0, 0), the second to the advanced ones (4, 1)."""
    import ops
    from hipvae.functional import conv_math_scope
    state = _init_state()
    solver, model = _solver(state, **JOINT_KW)
    ref_model = _model(state)
    opts = [torch.optim.Adam(m.parameters(), lr=HP["lr"]) for m in (ref_model.encoder, ref_model.decoder)]
    nc, disc = SPEC["cont"], SPEC["disc"]
    for step, want_cap in enumerate(((0.0, 0.0), (4.0, 1.0))):
        x, eps, u = _batch(step + 1)
        eps, u = eps[:, :nc].contiguous(), u[:, :sum(disc)].contiguous()
        assert solver.capacity_at(step) == want_cap and solver.steps_taken == step
        with ops.noise_queue([eps.clone(), u.clone()]):
            got = solver.train_step(x, step)
        # the assembled step
        xd = x.to(dev())
        for o in opts:
            o.zero_grad()
        with conv_math_scope("fp32"):
            mu, logvar = ref_model.encode(xd)
            z64, cl64, terms = R.torch_op(mu.double(), logvar.double(), eps.to(dev()).double(), u.to(dev()).double(), nc,
                                          disc, want_cap, 3.0, 2.0, HP["beta_kl"], 0.67)
            loss_kl = cl64.float()
            rec = ref_model.decode(z64.float())
            loss_rec = ops.reconstruction_loss(xd, rec, "mse", "mean", scale=HP["beta_rec"])
            loss = solver.scale * (loss_rec + loss_kl)
            loss.backward()
        params = [p for p in ref_model.parameters() if p.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(params, HP["clip"])
        for o in opts:
            o.step()
        t = terms.tolist()
        loss, loss_kl, loss_rec = loss.detach(), loss_kl.detach(), loss_rec.detach()
        want = dict(loss_enc=float(loss), loss_dec=float(loss), loss_kl=float(loss_kl), loss_rec=float(loss_rec),
                    L2=float(norm), kl_cont=t[0], kl_disc=t[1], cap_cont=t[2], cap_disc=t[3])
        print(step, {k: (got[k], want[k]) for k in want})
        assert set(got) == set(want) and (got["cap_cont"], got["cap_disc"]) == want_cap
        # no sign of this step hangs on a last bit
        assert abs(t[0] - t[2]) >= 0.1 * max(t[0], t[2]) and abs(t[1] - t[3]) >= 0.1 * max(t[1], t[3])
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]), (step, k, got[k], want[k])
        _params_close(model, ref_model, HP["lr"], steps=step + 1)
    assert solver.steps_taken == 2


def test_annealed_step_at_capacity_zero_equals_the_vae_step():
    """``AnnealedVAESolver`` with ``c_max = 0`` and ``gamma = beta`` (beta_kl = 1) is ``VAESolver`` with ``beta_kl = beta``,
    since |KL - 0| = KL -- WITHIN THE BAR, not bit for bit: the op evaluates z and the KL sums in fp64 and rounds once,
    ``itcv_reparam_fwd`` / ``itcv_kl_loss_fwd`` work in fp32."""
    import ops
    from solvers import AnnealedVAESolver, VAESolver
    state = _init_state()
    x, eps, _ = _batch(2)
    ann, m_ann = _solver(state, cls=AnnealedVAESolver, beta_kl=1.0, gamma=HP["beta_kl"], c_max=0.0, iteration_threshold=10)
    vae, m_vae = _solver(state, cls=VAESolver)
    with ops.noise_queue([eps.clone()]):
        got = ann.train_step(x, 0)
    with ops.noise_queue([eps.clone()]):
        want = vae.train_step(x, 0)
    print({k: (got[k], want[k]) for k in want})
    assert (got.pop("kl_disc"), got.pop("cap_cont"), got.pop("cap_disc")) == (0.0, 0.0, 0.0)
    assert abs(HP["beta_kl"] * got.pop("kl_cont") - want["loss_kl"]) <= 1e-4 * want["loss_kl"] and set(got) == set(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-4 * abs(want[k]), (k, got[k], want[k])
    _params_close(m_ann, m_vae, HP["lr"])


def test_captured_steps_equal_eager_steps_and_temperature_recaptures():
    """With enable_graph() the trajectory follows the eager one from the same state through the capture (steps 3-5 are
    replays) WHILE THE CAPACITY RISES EVERY STEP: one graph serves them all, and every replay reports the capacity of its
    own step.  After a change of ``temperature`` the trajectory still follows, under another graph key: that re-captures."""
    state = _init_state()
    xs = [_batch(5)[0].to(dev()), _batch(6)[0].to(dev())]
    kw = dict(JOINT_KW, cont_capacity=(0.0, 4.0, 16, 3.0), disc_capacity=(0.0, 1.0, 16, 2.0))

    def trajectory(graph, switch=True):
        solver, model = _solver(state, **kw)
        if graph:
            solver.enable_graph()
        torch.cuda.manual_seed(1234)
        res, keys, counts = [], [], []
        for k in range(9):
            if k == 6 and switch:
                solver.temperature = 1.5
            res.append(solver.train_step(xs[k % 2], k))
            if graph:
                keys.append(solver._graph_key if solver._graph is not None and k in (3, 4, 5, 7, 8) else None)
                counts.append(len(solver._graphs))
        return res, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), keys, counts

    (e, we, _, _), (gr, wg, keys, counts) = trajectory(False), trajectory(True)
    assert keys[3] is not None and 0.67 in keys[3] and keys[3] == keys[4] == keys[5]
    assert keys[7] is not None and 1.5 in keys[7] and keys[7] == keys[8] != keys[5]
    assert counts == [0, 0, 0, 1, 1, 1, 1, 2, 2]          # exactly one capture serves steps 3-5; the temperature adds one
    for k, (x, y) in enumerate(zip(e, gr)):
        assert set(x) == set(y) and "kl_disc" in x
        assert (y["cap_cont"], y["cap_disc"]) == (4.0 * k / 16, 1.0 * k / 16) == (x["cap_cont"], x["cap_disc"])
        for name in x:
            assert abs(x[name] - y[name]) <= 1e-5 * abs(x[name]) + 1e-9, (k, name, x[name], y[name])
    assert float((we - wg).abs().max()) < 1e-6
    # the switch is visible in the eager trajectory itself: without it the last step reports other numbers
    never = trajectory(False, switch=False)[0]
    print("switched / not:", e[8], never[8])
    assert any(abs(e[8][k] - never[8][k]) > 1e-5 * abs(e[8][k]) + 1e-9 for k in ("loss_kl", "loss_rec", "kl_disc"))


def test_constructor_refuses_a_zdim_mismatch_and_images_use_the_hard_code():
    from solvers import JointVAESolver
    state = _init_state()
    with pytest.raises(ValueError, match="is not D = 10"):
        _solver(state, latent_spec=dict(cont=6, disc=(5,)))
    with pytest.raises(ValueError):
        _solver(state, latent_spec=dict(cont=9, disc=(1,)))

    class Writer:
        def __init__(self):
            self.images, self.records, self.scalars = [], {}, {}

        def add_images(self, name, grid, global_step=None):
            self.images.append((name, grid))

        def add_scalars(self, name, values, global_step=None):
            self.records[name] = values

        def add_scalar(self, name, value, global_step=None):
            self.scalars[name] = value

        def flush(self):
            pass

    solver, model = _solver(state, **JOINT_KW)
    assert isinstance(solver, JointVAESolver)
    solver.writer = Writer()
    seen = []
    decode = model.decode
    model.decode = lambda z: (seen.append(z.detach().clone()), decode(z))[1]
    torch.cuda.manual_seed(3)
    out = solver.train_step(_batch(3)[0], 0)
    w = solver.writer
    assert set(w.records["joint"]) == {"kl_cont", "kl_disc", "cap_cont", "cap_disc"}
    assert w.records["joint"]["kl_disc"] == out["kl_disc"] and w.records["joint"]["cap_cont"] == out["cap_cont"]
    assert abs(w.scalars["kl_loss_unscaled"] - (out["kl_cont"] + out["kl_disc"])) <= 1e-12
    assert len(w.images) == 1 and w.images[0][1].shape == (3 * ROWS, 3, 32, 32)
    # decode saw: the step's soft sample, the prior sample of the fakes, the hard code of the reconstruction row
    assert len(seen) == 3
    for z in seen[1:]:
        y = z[:, 6:]
        assert ((y == 0) | (y == 1)).all() and torch.equal(y.sum(1), torch.ones(ROWS, device=dev()))
    assert not ((seen[0][:, 6:] == 0) | (seen[0][:, 6:] == 1)).all()
