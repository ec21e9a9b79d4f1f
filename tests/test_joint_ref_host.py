"""CPU checks of the yardstick of the JointVAE / AnnealedVAE latent op and of everything around the kernels that needs no
GPU: (1) the analytic backward of tests/joint_ref.py equals torch autograd in fp64 to 1e-10 on every case of the GPU test
and both signs of both terms; (2) every deliberate defect (joint_ref.DEFECTS) moves a quantity that tests/test_hip_joint.py
compares above that test's bar; (3) the stored vectors are those of the restatement; (4) the ABI table and the header agree
on the two symbols and the library refuses bad arguments before any launch; (5) the capacity schedule, the prior sample,
the recorded uniform draws and the argument errors of the op and the solvers."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import joint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_bytecode = sys.dont_write_bytecode
sys.path.insert(0, GOLDEN)
sys.dont_write_bytecode = True            # no cache directory next to the stored vectors
import make_golden_joint as MG  # noqa: E402

sys.path.remove(GOLDEN)
sys.dont_write_bytecode = _bytecode
BAR = 1e-4                      # the GPU test's bar
GPU_CASES = [(1, 1, ()), (1, 0, (2,)), (2, 3, (2,)), (7, 6, (3,)), (33, 10, (10,)), (4, 61, (2,)), (3, 62, (2,)),
             (5, 60, (5,)), (9, 60, (3, 7, 59)), (32, 118, (10,)), (2, 0, (511,)), (3, 256, (256,)), (2, 0, (2,) * 256),
             (1025, 10, (3, 4))]
BETA, GZ, GC, TAU = 0.75, 3.0, 2.0, 0.67


def rel(x, want):
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max()
    return float(np.abs(x - want).max() / scale) if scale else float(np.abs(x).max())


def inputs(B, nc, disc):
    """The GPU test's own inputs where the case is one of its cases."""
    case = (B, nc, tuple(disc))
    seed = MG.seed_of(GPU_CASES.index(case)) if case in GPU_CASES else 9000 + 31 * B + nc + 7 * len(disc)
    return R.make_inputs(B, nc, disc, seed) + (R.make_dz(B, nc + sum(disc), seed),)


# ---- 1. the analytic backward == torch autograd in fp64 ------------------------------------------------------------------
@pytest.mark.parametrize("B, nc, disc", GPU_CASES + [(5, 3, (2, 5, 3))])
def test_restatement_equals_torch_autograd(B, nc, disc):
    mu, lv, eps, u, caps, dz = inputs(B, nc, disc)
    g = -1.25
    for signs, cap in caps.items():
        ref = R.joint(mu, lv, eps, u, nc, disc, cap, GZ, GC, BETA, TAU, dz, g)
        a, b = (torch.from_numpy(x).double().requires_grad_(True) for x in (mu, lv))
        z, loss, terms = R.torch_op(a, b, torch.from_numpy(eps).double(), torch.from_numpy(u).double(), nc, disc, cap, GZ,
                                    GC, BETA, TAU)
        ((torch.from_numpy(dz).double() * z).sum() + g * loss).backward()
        got = dict(z=z.detach().numpy(), loss=float(loss.detach()), terms=terms.numpy(), dmu=a.grad.numpy(),
                   dlogvar=np.zeros_like(ref["dlogvar"]) if b.grad is None else b.grad.numpy())    # None: never used
        for k, v in got.items():
            assert rel(v, ref[k]) <= 1e-10, (signs, k, rel(v, ref[k]))
        assert not ref["dlogvar"][:, nc:].any() and not got["dlogvar"][:, nc:].any()
        want = (signs[0] if nc else 0, signs[1] if disc else 0)
        assert (np.sign(ref["terms"][0] - cap[0]), np.sign(ref["terms"][1] - cap[1])) == want


def test_sign_zero_and_empty_blocks():
    """KL = C exactly gives the sign 0 (torch.abs's subgradient) and no capacity gradient; an empty block has KL = 0."""
    mu, lv, eps, u, caps, dz = inputs(5, 3, (2, 5, 3))
    base = R.joint(mu, lv, eps, u, 3, (2, 5, 3), (0.0, 0.0), GZ, GC, BETA, TAU)
    at = R.joint(mu, lv, eps, u, 3, (2, 5, 3), base["terms"][:2], GZ, GC, BETA, TAU, None, 2.0)
    assert at["loss"] == 0.0 and not at["dmu"].any() and not at["dlogvar"].any()
    only_c = R.joint(mu[:, :3], lv[:, :3], eps, None, 3, (), (1.0, 0.0), GZ, GC, BETA, TAU)
    assert only_c["terms"][1] == 0.0 and only_c["z"].shape == (5, 3)
    only_d = R.joint(mu[:, 3:], lv[:, 3:], None, u, 0, (2, 5, 3), (0.0, 1.0), GZ, GC, BETA, TAU, dz[:, 3:])
    assert only_d["terms"][0] == 0.0 and not only_d["dlogvar"].any()
    assert np.allclose(only_d["z"].reshape(5, -1)[:, :2].sum(1), 1.0)


def test_hard_code_takes_the_first_maximum():
    mu = np.array([[0.5, 1.0, 3.0, 3.0, -1.0, -1.0, -1.0], [-0.5, 2.0, 1.0, 0.0, 0.0, 2.0, 2.0]], np.float32)
    z = R.hard(mu, 1, (3, 3))
    assert np.array_equal(z, np.array([[0.5, 0, 1, 0, 1, 0, 0], [-0.5, 1, 0, 0, 0, 1, 0]], np.float32))


# ---- 2. the defects ----------------------------------------------------------------------------------------------------
def applies(defect, B, nc, disc, signs):
    D, nd = nc + sum(disc), sum(disc)
    straddles = any(s // 64 != (e - 1) // 64 for s, e in R.groups(nc, disc))
    return {"mean_over_BD": D > 1,
            "no_abs": (nc and signs[0] < 0) or (nd and signs[1] < 0),
            "capacity_per_group": len(disc) >= 2,
            "drop_tail": D > 64 and D % 64 != 0,
            "u_zero_kept": nd > 0 and B >= 2,       # one row: the largest draw sits in the same group and decides it
            "cut_at_64": straddles}.get(defect, nd > 0)


def moved(good, bad, nc):
    """The largest move of what the GPU test compares: the scalars relative, the tensors normwise -- z as a whole and its
    discrete block ``y`` on its own (its values are at most 1, the continuous ones are not)."""
    out = [rel(bad[k], good[k]) for k in ("loss", "z", "dmu", "dlogvar")]
    if good["z"].shape[1] > nc:
        out.append(rel(bad["z"][:, nc:], good["z"][:, nc:]))
    return max(out + [rel(bad["terms"][i], good["terms"][i]) for i in range(4)])


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defects_are_visible(defect):
    """Over the GPU test's own cases (its edge draws for ``u_zero_kept``): a defect moves a compared quantity above the
    bar wherever it can apply, and it can apply somewhere."""
    seen = 0
    assert set(R.EDGE_CASES) <= set(GPU_CASES)
    for B, nc, disc in list(R.EDGE_CASES) if defect == "u_zero_kept" else GPU_CASES[:-1] + [(65, 10, (3, 4))]:
        mu, lv, eps, u, caps, dz = inputs(B, nc, disc)
        if defect == "u_zero_kept":
            u = R.edge_draws(u, mu, nc, disc)
        for signs, cap in caps.items():
            if not applies(defect, B, nc, disc, signs):
                continue
            good = R.joint(mu, lv, eps, u, nc, disc, cap, GZ, GC, BETA, TAU, dz, -1.25)
            bad = R.joint(mu, lv, eps, u, nc, disc, cap, GZ, GC, BETA, TAU, dz, -1.25, defect=defect)
            m = moved(good, bad, nc)
            assert m > BAR, (defect, B, nc, disc, signs, m)
            seen += 1
    print(defect, "visible on", seen, "cases")
    assert seen >= 8, (defect, seen)


# ---- 3. the stored vectors ------------------------------------------------------------------------------------------------
def test_golden_is_the_restatement():
    g = np.load(os.path.join(GOLDEN, "joint.npz"))
    assert MG.CASES == GPU_CASES and (MG.BETA, MG.GAMMA_Z, MG.GAMMA_C, MG.TAU) == (BETA, GZ, GC, TAU)
    assert g["hp"].tolist() == [BETA, GZ, GC, TAU] and g["cases"].tolist() == [MG.tag(*c) for c in GPU_CASES]
    assert len(set(g["cases"].tolist())) == len(GPU_CASES)
    keys = ["seed", "checksum"] + [MG.sign_tag(*s) + k for s in R.SIGNS for k in (":cap", ":loss")]
    assert set(g.files) == {"hp", "cases"} | {MG.tag(*c) + k for c in GPU_CASES for k in keys}      # nothing else is stored
    for B, nc, disc in GPU_CASES:
        p = MG.tag(B, nc, disc)
        mu, lv, eps, u, caps = R.make_inputs(B, nc, disc, int(g[p + "seed"]))
        assert np.array_equal(g[p + "checksum"], [a.astype(np.float64).sum() for a in (mu, lv, eps, u)])
        assert mu.dtype == lv.dtype == eps.dtype == u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
        for signs, cap in caps.items():
            t = MG.sign_tag(*signs)
            assert np.array_equal(g[p + t + ":cap"], cap)
            want = float(g[p + t + ":loss"])
            assert abs(R.joint(mu, lv, eps, u, nc, disc, cap, GZ, GC, BETA, TAU)["loss"] - want) <= 1e-12 * abs(want)


# ---- 4. the boundary ------------------------------------------------------------------------------------------------------
NAMES = ("itcv_joint_latent_fwd", "itcv_joint_latent_bwd")


def test_abi_table_and_header_agree():
    from hipvae import abi
    text = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NAMES:
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

    def fwd(B, nc, nd, tau=0.67, gz=1.0, gc=1.0, beta=1.0, ld=None, lde=None, ldu=None, hard=0, mu=q, eps=q, u=q, seg=q,
            cap=q):
        ld = nc + nd if ld is None else ld
        return abi.lib.itcv_joint_latent_fwd(mu, ld, q, ld, eps, nc if lde is None else lde, u, nd if ldu is None else ldu,
                                             seg, cap, q, q, q, q, q, B, nc, nd, hard, tau, gz, gc, beta, None)

    def bwd(B, nc, nd, tau=0.67, gz=1.0, gc=1.0, beta=1.0, ld=None, lde=None, ldu=None, mu=q, eps=q, u=q, seg=q, cap=q):
        """``cap`` stands for the stored signs here: what the backward reads in the capacities' place."""
        ld = nc + nd if ld is None else ld
        return abi.lib.itcv_joint_latent_bwd(q, ld, q, cap, mu, ld, q, ld, eps, nc if lde is None else lde, u,
                                             nd if ldu is None else ldu, seg, q, q, B, nc, nd, tau, gz, gc, beta, None)

    for call in (fwd, bwd):
        assert call(1, 0, 0) != 0 and "outside 1..512" in abi.last_error()
        assert call(1, 500, 13) != 0 and "outside 1..512" in abi.last_error()
        assert call(1, -1, 4) != 0 and "negative" in abi.last_error()
        assert call(0, 4, 4) != 0 and "rows" in abi.last_error()
        for tau in (0.0, -1.0, float("inf"), float("nan")):
            assert call(4, 4, 4, tau=tau) != 0 and "temperature" in abi.last_error()
        for bad in (-1.0, float("inf"), float("nan")):
            assert call(4, 4, 4, gz=bad) != 0 and "gamma" in abi.last_error()
            assert call(4, 4, 4, gc=bad) != 0 and "gamma" in abi.last_error()
        assert call(4, 4, 4, beta=float("nan")) != 0 and "finite" in abi.last_error()
        assert call(4, 4, 4, ld=7) != 0 and "row stride" in abi.last_error()
        assert call(4, 4, 4, lde=3) != 0 and "n_cont" in abi.last_error()
        assert call(4, 4, 4, ldu=3) != 0 and "n_disc" in abi.last_error()
        for missing in ("mu", "eps", "u", "seg", "cap"):
            assert call(4, 4, 4, **{missing: None}) != 0 and "NULL" in abi.last_error(), missing
    # the hard code needs mu, seg and z alone, but still a shape the kernel can take
    assert fwd(4, 300, 300, hard=1, eps=None, u=None, cap=None) != 0 and "outside 1..512" in abi.last_error()
    assert fwd(4, 4, 4, hard=1, seg=None) != 0 and "NULL" in abi.last_error()
    assert fwd(4, 4, 4, hard=1, ld=7) != 0 and "row stride" in abi.last_error()


# ---- 5. the Python side ---------------------------------------------------------------------------------------------------
def test_capacity_schedule():
    import models
    from solvers import AnnealedVAESolver, JointVAESolver, VAESolver

    class DS:
        def __len__(self):
            return 100

    model = models.SoftIntroVAE(arch="conv", cdim=3, zdim=10, channels=(8, 16), image_size=16)
    opt = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in (model.encoder, model.decoder)]
    args = (DS(), model, 4, opt[0], opt[1], "mse", 1.0, 1.0, torch.device("cpu"), False, None)
    s = JointVAESolver(*args, latent_spec=dict(cont=6, disc=(4,)), cont_capacity=(1.0, 5.0, 100, 30.0),
                       disc_capacity=(0.0, 5.0, 50, 20.0), temperature=0.5)
    assert isinstance(s, VAESolver) and s.latent_spec == dict(cont=6, disc=(4,)) and s.temperature == 0.5
    assert (s.gamma_cont, s.gamma_disc, s.steps_taken) == (30.0, 20.0, 0)
    assert s._cap.shape == (2,) and s._cap.dtype == torch.float64
    for t in (0, 1, 10, 50, 99, 100, 1000):
        cz, cc = s.capacity_at(t)
        assert cz == R.capacity_at(t, 1.0, 5.0, 100) == min(5.0, 1.0 + 4.0 * t / 100)
        assert cc == R.capacity_at(t, 0.0, 5.0, 50, ceiling=math.log(4)) and cc <= math.log(4)
    assert s.capacity_at(1000) == (5.0, math.log(4))
    # the validated attributes, each a part of the graph key
    key = s._graph_key_extra()
    for name, bad, good in (("temperature", 0.0, 1.0), ("temperature", float("nan"), 0.8),("gamma_cont", -1.0, 2.0),
                            ("gamma_disc", float("inf"), 3.0),
                            ("latent_spec", dict(cont=6, disc=(3,)), dict(cont=4, disc=(3, 3))),
                            ("latent_spec", dict(cont=9, disc=(1,)), dict(cont=0, disc=(10,)))):
        before = getattr(s, name)
        with pytest.raises(ValueError):
            setattr(s, name, bad)
        assert getattr(s, name) == before                           # a refused assignment changes nothing
        setattr(s, name, good)
        assert s._graph_key_extra() != key
        key = s._graph_key_extra()
    assert s.capacity_at(10 ** 6) == (0.0, math.log(10))             # no continuous block: its capacity is 0
    with pytest.raises(ValueError, match="D = 10|is not D"):
        JointVAESolver(*args, latent_spec=dict(cont=6, disc=(5,)))
    for bad in ((0.0, 5.0, 0, 30.0), (0.0, 5.0, 100), (-1.0, 5.0, 100, 1.0), (0.0, 5.0, 100, -1.0)):
        with pytest.raises(ValueError):
            JointVAESolver(*args, latent_spec=dict(cont=6, disc=(4,)), cont_capacity=bad)
    a = AnnealedVAESolver(*args, gamma=7.0, c_max=25.0, iteration_threshold=1000)
    assert isinstance(a, JointVAESolver) and a.latent_spec == dict(cont=10, disc=()) and a.gamma == a.gamma_cont == 7.0
    assert [a.capacity_at(t) for t in (0, 500, 1000, 5000)] == [(0.0, 0.0), (12.5, 0.0), (25.0, 0.0), (25.0, 0.0)]
    d = AnnealedVAESolver(*args)
    assert (d.gamma, d.cont_capacity) == (1000.0, (0.0, 25.0, 100000.0)) and JointVAESolver(*args).latent_spec["disc"] == ()


def test_uniform_noise_and_prior_sample():
    import ops
    rec = torch.rand(3, 4)
    with ops.noise_queue([torch.zeros(3, 2), rec]):
        assert ops.noise((3, 2), "cpu").shape == (3, 2)
        assert torch.equal(ops.uniform_noise((3, 4), "cpu"), rec)
        with pytest.raises(RuntimeError, match="exhausted"):
            ops.uniform_noise((3, 4), "cpu")
    with ops.noise_queue([rec]), pytest.raises(AssertionError):
        ops.uniform_noise((3, 5), "cpu")
    ops.set_noise_mode("host")
    try:
        torch.manual_seed(3)
        a = ops.uniform_noise((5, 7), "cpu")
        torch.manual_seed(3)
        assert torch.equal(a, torch.rand(5, 7)) and 0.0 <= float(a.min()) and float(a.max()) < 1.0
    finally:
        ops.set_noise_mode("device")
    z = ops.joint_prior_sample(500, 3, (2, 5), "cpu")
    assert z.shape == (500, 10) and z.dtype == torch.float32
    for s, e in ((3, 5), (5, 10)):
        assert torch.equal(z[:, s:e].sum(1), torch.ones(500)) and ((z[:, s:e] == 0) | (z[:, s:e] == 1)).all()
        assert (z[:, s:e].sum(0) > 0).all()                          # every category is drawn
    assert 0.7 < float(z[:, :3].std()) < 1.3
    assert ops.joint_prior_sample(4, 0, (3,), "cpu").shape == (4, 3)
    assert ops.joint_prior_sample(4, 2, (), "cpu").shape == (4, 2)
    seg = ops.joint_segments((3, 2), "cpu")
    assert seg.dtype == torch.int32 and seg.tolist() == [[0, 3], [0, 3], [0, 3], [3, 5], [3, 5]]
    assert ops.joint_segments((3, 2), "cpu") is seg                 # built once per spec


def test_op_argument_errors():
    import ops
    from hipvae import abi
    from hipvae.functional import JOINT_MAX_D
    assert JOINT_MAX_D == 512
    mu, cap = torch.zeros(4, 6), torch.zeros(2, dtype=torch.float64)

    def op(m=mu, lv=mu, nc=2, disc=(4,), gz=1.0, gc=1.0, **kw):
        return ops.joint_latent(m, lv, nc, disc, cap, gz, gc, **kw)

    for kw in (dict(lv=torch.zeros(4, 5)), dict(m=torch.zeros(6), lv=torch.zeros(6)), dict(nc=3), dict(disc=(3,)),
               dict(nc=5, disc=(1,)), dict(nc=-1, disc=(7,)), dict(temperature=0.0), dict(temperature=float("inf")),
               dict(temperature=float("nan")), dict(gz=-1.0), dict(gc=float("nan")), dict(gz=float("inf")),
               dict(eps=torch.zeros(4, 6)), dict(u=torch.zeros(4, 2)), dict(nc=2, disc=(4,), hard=True, m=torch.zeros(4, 7)),
               dict(m=torch.zeros(4, 513), lv=torch.zeros(4, 513), nc=513, disc=()),
               dict(m=torch.zeros(4, 0), lv=torch.zeros(4, 0), nc=0, disc=())):
        with pytest.raises(ValueError):
            op(**kw)
    state = torch.get_rng_state()
    with pytest.raises(abi.HipExtensionError):
        op()                                                         # CPU tensors: refused before the draws
    with pytest.raises(abi.HipExtensionError):
        op(hard=True)
    assert torch.equal(state, torch.get_rng_state())
