#!/usr/bin/env python3
"""Golden vectors for the full beta-TC decomposition loss.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference).

Calls the unmodified reference's ``TCSovler._compute_kl_loss_full`` (solvers/tc.py:91-144) -- on a stub ``self`` whose
``dataset`` has length N -- and writes ``tc_full.npz``:
  * per latent case (tags a-c of ops.npz, d of ops_c4.npz: same seeds, inputs checked equal and not stored again) the
    loss and d/dz, d/dmu, d/dlogvar of ``reduce="mean"`` at beta = 512, 0.5 and 1 (``{tag}_b{beta}[_dz|_dmu|_dlogvar]``),
    and of a per-row-weighted ``reduce="none"`` case at beta = 512: sum_j w_j * loss_j (``{tag}_w*``, rows in
    ``{tag}_w_rows``);
  * the gradients of the large tags as every ``{tag}_stride``-th element of the flattened array (1 for a and b, 4 for c,
    16 for d), which keeps the file under 1 MB.
It also writes ``steps_tc_full.npz``: 2 steps of the TC and intro-TC solvers (conv arch, B=8) whose ``compute_kl_loss``
is overridden to call ``TCSovler._compute_kl_loss_full`` -- the reference's own extension point -- from the initial
weights, inputs and noise draws of steps_conv.npz (checked equal, not stored again).  Per solver it holds the returned
dicts and every 4th final weight (``weight_keys`` order) as the XOR of its fp32 bits with the initial one, in 4 byte
planes (``{name}:final_xor``), as steps_optim.npz does.

    python tests/golden/make_golden_tc_full.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (installs the stub modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CASES = {"a": ("ops.npz", (16, 10, 1000), 1), "b": ("ops.npz", (64, 128, 10000), 1),
         "c": ("ops.npz", (256, 64, 10000), 4), "d": ("ops_c4.npz", (512, 128, 10000), 16)}
BETAS = ((512.0, "512p0"), (0.5, "0p5"), (1.0, "1p0"))


class _Self:
    """What _compute_kl_loss_full reads of its solver when write=False: beta_kl and len(dataset)."""

    def __init__(self, n):
        self.dataset = MG._DS(n)
        self.beta_kl = 1.0


def gen_tc_full():
    MG.SingletonWriter().writer = None
    out = {}
    for tag, (src, (B, D, N), stride) in CASES.items():
        g = np.load(os.path.join(MG.HERE, src))
        z, mu, logvar, _ = MG.latent_inputs(B, D, seed=100 + B)
        assert np.array_equal(g[f"{tag}_BDN"], [B, D, N])
        for k, t in (("z", z), ("mu", mu), ("logvar", logvar)):
            assert np.array_equal(MG.npy(t), g[f"{tag}_{k}"]), (tag, k)
        out[f"{tag}_stride"] = np.int64(stride)
        me = _Self(N)
        for beta, bt in BETAS:
            zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, logvar))
            loss = MG.TCSovler._compute_kl_loss_full(me, zz, mm, ll, "mean", beta)
            loss.backward()
            p = f"{tag}_b{bt}"
            out[p] = MG.npy(loss)
            for k, t in (("dz", zz), ("dmu", mm), ("dlogvar", ll)):
                out[f"{p}_{k}"] = MG.npy(t.grad).reshape(-1)[::stride].copy()
        zz, mm, ll = (t.clone().requires_grad_(True) for t in (z, mu, logvar))
        w = torch.linspace(-1.0, 2.0, B)
        rows = MG.TCSovler._compute_kl_loss_full(me, zz, mm, ll, "none", 512.0)
        (w * rows).sum().backward()
        out[f"{tag}_w"], out[f"{tag}_w_rows"] = MG.npy(w), MG.npy(rows)
        for k, t in (("dz", zz), ("dmu", mm), ("dlogvar", ll)):
            out[f"{tag}_w_{k}"] = MG.npy(t.grad).reshape(-1)[::stride].copy()
    MG.save("tc_full.npz", **out)


def sample(a):
    """Every 4th element of a weight tensor: the stored subset of the final weights."""
    return np.ascontiguousarray(a.reshape(-1)[::4])


def gen_steps_tc_full(nsteps=2, B=8, N=1000):
    HP = MG.HP
    MG.SingletonWriter().writer = None
    MG.SingletonWriter().cur_iter = 0
    MG.SingletonWriter().test_iter = N // B
    out = {}
    conv = np.load(os.path.join(MG.HERE, "steps_conv.npz"))
    g = torch.Generator().manual_seed(21)                 # the inputs of make_golden.gen_steps
    xs = [torch.rand(B, 3, 32, 32, generator=g) for _ in range(nsteps)]
    out["hp"] = np.array([HP["beta_kl"], HP["beta_rec"], HP["beta_neg"], HP["gamma_r"], HP["clip"], HP["lr"], N],
                         dtype=np.float64)
    assert np.array_equal(out["hp"], conv["hp"])
    for s, x in enumerate(xs):
        assert np.array_equal(MG.npy(x), conv[f"x{s}"]), s

    def full(self, z, mu, logvar, reduce="mean", beta=None, write=False):
        return MG.TCSovler._compute_kl_loss_full(self, z, mu, logvar, reduce, beta, write)

    classes = {"tc": type("TCFull", (MG.TCSovler,), {"compute_kl_loss": full}),
               "intro_tc": type("IntroTCFull", (MG.IntroTCSovler,), {"compute_kl_loss": full})}
    for name, cls in classes.items():
        model = MG.build_model("conv")
        model.train()
        init = MG.state_arrays(model, "init:")
        assert all(np.array_equal(v, conv[k]) for k, v in init.items())
        keys = [k for k, v in model.state_dict().items() if v.is_floating_point() and "running" not in k]
        out["weight_keys"] = np.array(keys)
        kw = dict(dataset=MG._DS(N), model=model, batch_size=B,
                  optimizer_e=torch.optim.Adam(model.encoder.parameters(), lr=HP["lr"]),
                  optimizer_d=torch.optim.Adam(model.decoder.parameters(), lr=HP["lr"]), recon_loss_type="mse",
                  beta_kl=HP["beta_kl"], beta_rec=HP["beta_rec"], device=torch.device("cpu"), use_amp=False,
                  grad_scaler=None, writer=None, test_iter=1000, clip=HP["clip"])
        if name == "intro_tc":
            kw.update(beta_neg=HP["beta_neg"], gamma_r=HP["gamma_r"])
        solver = cls(**kw)
        torch.manual_seed(1234)
        for s, x in enumerate(xs):
            with MG.Recorder() as rec:
                d = solver.train_step(x, s)
            out[f"{name}:s{s}:dict"] = np.array([d["loss_enc"], d["loss_dec"], d["loss_kl"], d["loss_rec"], d["L2"]],
                                                dtype=np.float64)
            assert len(rec.draws) == len([k for k in conv.files if k.startswith(f"{name}:s{s}:draw")])
            for i, t in enumerate(rec.draws):
                assert np.array_equal(MG.npy(t), conv[f"{name}:s{s}:draw{i}"]), (name, s, i)
        sd = model.state_dict()
        xor = np.concatenate([sample(MG.npy(sd[k])).view(np.uint32)
                              ^ sample(conv["init:" + k.replace(".", "/")]).view(np.uint32) for k in keys])
        out[f"{name}:final_xor"] = np.ascontiguousarray(xor.view(np.uint8).reshape(-1, 4).T)
    MG.save("steps_tc_full.npz", **out)


if __name__ == "__main__":
    gen_tc_full()
    gen_steps_tc_full()
