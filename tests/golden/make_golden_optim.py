#!/usr/bin/env python3
"""Golden vectors for the fused optimiser updates.  RUNS ONLY IN THE BUILD CONTAINER (needs the reference).

Drives the unmodified reference's intro-TC solver (solvers/intro_tc.py, solvers/intro.py:56-196) with torch's own
optimisers -- one configuration per family the HIP path fuses (the reference picks its optimiser from the run config,
train.py:140-144) -- on the conv architecture at the golden shape (B=8), 2 steps, and writes ``steps_optim.npz``.
Helpers come from make_golden.py, which this file does not change.

The run starts from the initial weights, inputs and noise draws of steps_conv.npz's intro-TC run (make_golden.gen_steps:
same seeds), checked equal here and not stored again.  Per configuration the file holds the returned dicts, the names
of the parameters left without a gradient (checked unchanged here), and the final weights of every 4th element of each
weight tensor (``weight_keys`` order), stored losslessly as the XOR of their fp32 bit patterns with the initial ones,
split into 4 byte planes (``{name}:final_xor``, uint8 [4, n]) so that they compress.

    python tests/golden/make_golden_optim.py
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden as MG  # noqa: E402  (installs the stub modules and puts the reference on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

# name -> (torch.optim class name, kwargs); lr is HP["lr"] unless given.  RMSprop's first steps move a weight by up to
# lr / sqrt(1 - alpha) = 10 lr: it runs at lr / 10, the per-step move of the Adam fixtures.
CONFIGS = {
    "sgd": ("SGD", dict(momentum=0.9, nesterov=True, weight_decay=1e-4)),
    "adamw": ("AdamW", dict(weight_decay=1e-2, amsgrad=True)),
    "adagrad": ("Adagrad", dict(lr_decay=1e-3, weight_decay=1e-4, initial_accumulator_value=0.1)),
    "rmsprop": ("RMSprop", dict(lr=MG.HP["lr"] / 10, momentum=0.9, centered=True, weight_decay=1e-4)),
}


def gen_steps_optim(nsteps=2, B=8, N=1000):
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
    for name, (cls, kw) in CONFIGS.items():
        model = MG.build_model("conv")
        model.train()
        init = MG.state_arrays(model, "init:")
        assert all(np.array_equal(v, conv[k]) for k, v in init.items()) and len(init) == len(
            [k for k in conv.files if k.startswith("init:")])
        keys = [k for k, v in model.state_dict().items() if v.is_floating_point() and "running" not in k]
        out["weight_keys"] = np.array(keys)
        opt = getattr(torch.optim, cls)
        kw = dict(dict(lr=HP["lr"]), **kw)
        out[f"{name}:lr"] = np.float64(kw["lr"])
        opt_e = opt(model.encoder.parameters(), **kw)
        opt_d = opt(model.decoder.parameters(), **kw)
        solver = MG.IntroTCSovler(dataset=MG._DS(N), model=model, batch_size=B, optimizer_e=opt_e, optimizer_d=opt_d,
                                  recon_loss_type="mse", beta_kl=HP["beta_kl"], beta_rec=HP["beta_rec"],
                                  beta_neg=HP["beta_neg"], gamma_r=HP["gamma_r"], device=torch.device("cpu"),
                                  use_amp=False, grad_scaler=None, writer=None, test_iter=1000, clip=HP["clip"])
        torch.manual_seed(1234)
        for s, x in enumerate(xs):
            with MG.Recorder() as rec:
                d = solver.train_step(x, s)
            p = f"{name}:s{s}:"
            out[p + "dict"] = np.array([d["loss_enc"], d["loss_dec"], d["loss_kl"], d["loss_rec"], d["L2"]],
                                       dtype=np.float64)
            assert len(rec.draws) == len([k for k in conv.files if k.startswith(f"intro_tc:s{s}:draw")])
            for i, t in enumerate(rec.draws):
                assert np.array_equal(MG.npy(t), conv[f"intro_tc:s{s}:draw{i}"]), (name, s, i)
        # parameters the reference's backward never reaches keep grad None (the fused path must leave them alone)
        free = [k for k, p in model.named_parameters() if p.grad is None]
        out[f"{name}:no_grad"] = np.array(free)
        sd = model.state_dict()
        for k in free:
            assert np.array_equal(MG.npy(sd[k]), conv["init:" + k.replace(".", "/")]), k
        xor = np.concatenate([sample(MG.npy(sd[k])).view(np.uint32)
                              ^ sample(conv["init:" + k.replace(".", "/")]).view(np.uint32) for k in keys])
        out[f"{name}:final_xor"] = np.ascontiguousarray(xor.view(np.uint8).reshape(-1, 4).T)
    MG.save("steps_optim.npz", **out)


def sample(a):
    """Every 4th element of a weight tensor: the stored subset of the final weights."""
    return np.ascontiguousarray(a.reshape(-1)[::4])


if __name__ == "__main__":
    gen_steps_optim()
