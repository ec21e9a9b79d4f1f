"""Case table, inputs and references of the optimiser kernel tests (no GPU): one case per launchable instance of
``csrc/optim.hip`` (12 ``adamx_kernel``, 12 of the 16 ``sgd_kernel``, 4 ``adagrad_kernel``, 16 ``rmsprop_kernel``) plus
``adam_dev_kernel`` and ``adam_kernel`` of ``csrc/loss_optim.hip``, the sizes and ``live`` masks that reach each grid
trip and edge, inputs that take both sides of every branch, and the real ``torch.optim`` class on the CPU in fp64
(the reference) or fp32 (the yardstick).  ``tests/test_optim_cases_host.py`` holds the table to its promises;
``tests/test_hip_optim_kernels.py`` runs it on the device."""
import collections

import numpy as np
import torch

# ITCV_OPT_* of include/itcv_hip.h (pinned against the header by tests/test_optim_host.py)
MAXIMIZE, NESTEROV, AMSGRAD, DECOUPLED_WD, CENTERED = 0x1, 0x2, 0x4, 0x8, 0x10

# the grid cap of optim_grid / stream_grid: 2048 blocks of 256 threads, one float4 (optim.hip) or one float
# (the plain-Adam kernels) per thread and trip
BLOCK = 256
MAX_BLOCKS = 2048
GRID = MAX_BLOCKS * BLOCK

SIZES4 = (4, 4 * BLOCK + 4, 4100, 4 * GRID, 4 * GRID + 4, 4 * (GRID + 77))
SIZES1 = (1, 3, 4 * BLOCK + 3, GRID, GRID + 1, GRID + 77)
SMALL = slice(0, 3)                     # the sizes every case runs at
TRIPS = slice(3, 6)                     # exactly one trip, one thread on the second, 77 on the second

Case = collections.namedtuple("Case", "name entry kind cls kw flags hp states")
Ref = collections.namedtuple("Ref", "arrays ratio")

ENTRY = {"adamx": "itcv_adamx_step_dev", "sgd": "itcv_sgd_step_dev", "adagrad": "itcv_adagrad_step_dev",
         "rmsprop": "itcv_rmsprop_step_dev", "adam_dev": "itcv_adam_step_dev", "adam": "itcv_adam_step"}


def spec_of(cls, kw):
    """(kind, flags, hyper-parameters in the entry point's order) of ``torch.optim.<cls>(**kw)``: what
    ``hipvae.flat.fused_update`` has to return for it (restated here from the entry points' signatures)."""
    flags = MAXIMIZE if kw.get("maximize") else 0
    wd = float(kw.get("weight_decay", 1e-2 if cls == "AdamW" else 0.0))
    if cls in ("Adam", "AdamW"):
        b = kw.get("betas", (0.9, 0.999))
        flags |= AMSGRAD if kw.get("amsgrad") else 0
        flags |= DECOUPLED_WD if cls == "AdamW" or kw.get("decoupled_weight_decay") else 0
        return "adamx", flags, (float(kw["lr"]), float(b[0]), float(b[1]), float(kw.get("eps", 1e-8)), wd)
    if cls == "SGD":
        flags |= NESTEROV if kw.get("nesterov") else 0
        return "sgd", flags, (float(kw["lr"]), float(kw.get("momentum", 0.0)), float(kw.get("dampening", 0.0)), wd)
    if cls == "Adagrad":
        return "adagrad", flags, (float(kw["lr"]), float(kw.get("lr_decay", 0.0)), wd, float(kw.get("eps", 1e-10)))
    assert cls == "RMSprop", cls
    flags |= CENTERED if kw.get("centered") else 0
    return "rmsprop", flags, (float(kw["lr"]), float(kw.get("alpha", 0.99)), float(kw.get("eps", 1e-8)), wd,
                              float(kw.get("momentum", 0.0)))


def states_of(kind, flags, hp):
    """torch's state keys of a case, in the order the entry point takes the buffers."""
    if kind in ("adamx", "adam_dev", "adam"):
        return ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if flags & AMSGRAD else ())
    if kind == "sgd":
        return ("momentum_buffer",) if hp[1] != 0 else ()
    if kind == "adagrad":
        return ("sum",)
    return ("square_avg",) + (("momentum_buffer",) if hp[4] > 0 else ()) + (("grad_avg",) if flags & CENTERED else ())


def _f32(x):
    return float(np.float32(x))


def _case(cls, kind=None, **kw):
    k, flags, hp = spec_of(cls, kw)
    kind = kind or k
    if kind in ("adam_dev", "adam"):
        hp = hp[:4]
    bits = [cls.lower()] + [f"{a}{v}".replace("True", "") for a, v in kw.items() if a != "lr" and kind == k]
    name = "-".join([kind] + bits).replace("(", "").replace(")", "").replace(", ", "_").replace("_weight_decay", "")
    return Case(name, ENTRY[kind], kind, cls, kw, flags, hp, states_of(kind, flags, hp))


def _table():
    cases = []
    # adamx_kernel<WD, AMSGRAD, MAXIMIZE>: beta1 on both sides of lerp_t's |1 - beta1| < 0.5 branch and on it
    beta1 = (0.9, 0.5, 0.3, 0.0)
    lrs = (1e-2, 3e-2, 1e-1)
    i = 0
    for wd in (0, 1, 2):
        for ams in (False, True):
            for mx in (False, True):
                kw = dict(lr=lrs[i % 3], betas=(beta1[i % 4], (0.999, 0.99, 0.9)[i % 3]))
                cls = "Adam"
                if wd == 1:
                    kw["weight_decay"] = 1e-2
                elif wd == 2 and i % 2 == 0:
                    cls, kw["weight_decay"] = "AdamW", 5e-2
                elif wd == 2:
                    kw["weight_decay"], kw["decoupled_weight_decay"] = 1e-1, True
                if ams:
                    kw["amsgrad"] = True
                if mx:
                    kw["maximize"] = True
                if i % 5 == 3:
                    kw["eps"] = 1e-6
                cases.append(_case(cls, **kw))
                i += 1
    # sgd_kernel<MOMENTUM, NESTEROV, WD, MAXIMIZE>: the four <false, true, *, *> are refused on the host
    i = 0
    for mom in (False, True):
        for nes in ((False, True) if mom else (False,)):
            for wd in (False, True):
                for mx in (False, True):
                    kw = dict(lr=lrs[i % 3])
                    if mom:
                        kw["momentum"] = (0.9, 0.5)[i % 2]
                    if nes:
                        kw["nesterov"] = True
                    elif mom and i % 2 == 1:
                        kw["dampening"] = 0.3
                    if wd:
                        kw["weight_decay"] = (1e-2, 1e-1)[i % 2]
                    if mx:
                        kw["maximize"] = True
                    cases.append(_case("SGD", **kw))
                    i += 1
    # adagrad_kernel<WD, MAXIMIZE>
    i = 0
    for wd in (False, True):
        for mx in (False, True):
            kw = dict(lr=(1e-1, 5e-2)[i % 2], lr_decay=(0.0, 1e-2)[(i + wd) % 2],
                      initial_accumulator_value=(0.0, 0.1)[i % 2])
            if wd:
                kw["weight_decay"] = 1e-2
            if mx:
                kw["maximize"] = True
            if i == 2:
                kw["eps"] = 1e-8
            cases.append(_case("Adagrad", **kw))
            i += 1
    # rmsprop_kernel<WD, MAXIMIZE, CENTERED, MOMENTUM>: 1 - alpha on both sides of lerp_t's branch and on it
    i = 0
    for wd in (False, True):
        for mx in (False, True):
            for cen in (False, True):
                for mom in (False, True):
                    kw = dict(lr=lrs[i % 3], alpha=(0.99, 0.5, 0.3)[(i // 2) % 3] if cen else (0.99, 0.9)[i % 2])
                    if wd:
                        kw["weight_decay"] = 1e-2
                    if mx:
                        kw["maximize"] = True
                    if cen:
                        kw["centered"] = True
                    if mom:
                        kw["momentum"] = (0.9, 0.5)[(i // 4) % 2]
                    cases.append(_case("RMSprop", **kw))
                    i += 1
    # the plain kernels of loss_optim.hip (adamx<0, false, false> is the first case of the table).  Their entry points
    # take lr, the betas and eps as C floats, so the update they make is torch's at the fp32-rounded values: a kernel
    # handed float(0.999) runs Adam at beta2 = 0.99900001287, whose 1 - beta2 is 1.3e-5 off 0.001.
    cases.append(_case("Adam", kind="adam_dev", lr=_f32(5e-2), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8)))
    cases.append(_case("Adam", kind="adam", lr=_f32(3e-2), betas=(0.5, _f32(0.99)), eps=_f32(1e-8)))
    return tuple(cases)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "case names collide"

# the case of each family with the most state buffers (grid trips, masks, FlatGroup, replay)
FAMILY = {
    "adamx": _case("AdamW", lr=1e-2, betas=(0.9, 0.999), weight_decay=5e-2, amsgrad=True, maximize=True),
    "sgd": _case("SGD", lr=3e-2, momentum=0.9, nesterov=True, weight_decay=1e-2, maximize=True),
    "adagrad": _case("Adagrad", lr=1e-1, lr_decay=1e-2, initial_accumulator_value=0.1, weight_decay=1e-2,
                     maximize=True),
    "rmsprop": _case("RMSprop", lr=1e-2, alpha=0.3, weight_decay=1e-2, maximize=True, centered=True, momentum=0.9),
}
PLAIN = {c.kind: c for c in CASES[-2:]}


def instance_of(case):
    """The kernel template arguments a case launches, mirrored from the dispatch of the entry points in optim.hip."""
    f, hp = case.flags, case.hp
    if case.kind in ("adam_dev", "adam"):
        return (case.kind,)
    if case.kind == "adamx":
        wd = 0 if hp[4] == 0.0 else (2 if f & DECOUPLED_WD else 1)
        return "adamx", wd, bool(f & AMSGRAD), bool(f & MAXIMIZE)
    if case.kind == "sgd":
        mom = hp[1] != 0.0
        return "sgd", mom, bool(f & NESTEROV) and mom, hp[3] != 0.0, bool(f & MAXIMIZE)
    if case.kind == "adagrad":
        return "adagrad", hp[2] != 0.0, bool(f & MAXIMIZE)
    return "rmsprop", hp[3] != 0.0, bool(f & MAXIMIZE), bool(f & CENTERED), hp[4] > 0.0


def launchable_instances():
    """Every instance the entry points can launch: 44 of optim.hip and the two plain kernels."""
    tf = (False, True)
    out = [("adamx", wd, a, m) for wd in (0, 1, 2) for a in tf for m in tf]
    out += [("sgd", mo, ne, wd, m) for mo in tf for ne in tf for wd in tf for m in tf if mo or not ne]
    out += [("adagrad", wd, m) for wd in tf for m in tf]
    out += [("rmsprop", wd, m, c, mo) for wd in tf for m in tf for c in tf for mo in tf]
    return out + [("adam_dev",), ("adam",)]


def sizes(case):
    return SIZES1 if case.kind in ("adam_dev", "adam") else SIZES4


# ---- live masks, one byte per float4 ---------------------------------------------------------------------------------
def _dead(n4, lo, hi):
    live = np.ones(n4, np.uint8)
    live[lo:hi] = 0
    return live


def _alternate(n4):
    live = np.ones(n4, np.uint8)
    live[1::2] = 0
    return live


MASKS = {
    "first": lambda n4: _dead(n4, 0, 1),
    "last": lambda n4: _dead(n4, n4 - 1, n4),
    "alternate": _alternate,
    "block_edge": lambda n4: _dead(n4, BLOCK - 3, BLOCK + 2),
    "trip_edge": lambda n4: _dead(n4, GRID - 2, GRID + 3),
    "all": lambda n4: np.zeros(n4, np.uint8),
}


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _rng(seed, k):
    return np.random.default_rng([seed, k])


def inputs(case, n, step, seed=0):
    """fp32 arrays ``p``, ``g`` and the state of ``case`` after ``step`` earlier steps (all zero at step 0, Adagrad's
    ``sum`` at its initial value), each drawn from a stream of its own so that a longer array starts with the shorter
    one.  p ~ N(0, 1) with exact zeros; g ~ 0.01 N(0, 1) with every 7th element 0 and every 11th times 5000 (an
    outlier the moments have not seen, so that one step moves it by about lr)."""
    i = np.arange(n)
    p = _rng(seed, 0).standard_normal(n)
    p[i % 13 == 2] = 0.0
    g = 0.01 * _rng(seed, 1).standard_normal(n)
    g[i % 11 == 1] *= 5000.0
    g[i % 7 == 3] = 0.0
    a = {"p": p, "g": g}
    z = _rng(seed, 2).standard_normal(n)                        # first-moment direction
    c = 0.5 + _rng(seed, 3).random(n)                          # second-moment spread, 0.5 .. 1.5
    kw = case.kw
    if case.kind in ("adamx", "adam_dev", "adam"):
        b1, b2 = case.hp[1], case.hp[2]
        a["exp_avg"] = (1 - b1 ** step) * 0.01 * z
        a["exp_avg_sq"] = (1 - b2 ** step) * 1e-4 * c
        if "max_exp_avg_sq" in case.states:
            a["max_exp_avg_sq"] = a["exp_avg_sq"] * np.where(_rng(seed, 4).random(n) < 0.5, 0.5, 1.5)
    elif case.kind == "sgd":
        if case.states and step > 0:
            mom, damp = case.hp[1], case.hp[2]
            a["momentum_buffer"] = (1 - damp) * (1 - mom ** step) / (1 - mom) * 0.003 * z
    elif case.kind == "adagrad":
        a["sum"] = kw.get("initial_accumulator_value", 0.0) + step * 1e-4 * c
    else:
        alpha, mom = case.hp[1], case.hp[4]
        w = 1 - alpha ** step
        ga = w * 0.01 * z if "grad_avg" in case.states else 0.0
        a["square_avg"] = ga * ga + w * 1e-4 * c                # centred: square_avg - grad_avg^2 > 0 by construction
        if "grad_avg" in case.states:
            a["grad_avg"] = ga
        if "momentum_buffer" in case.states:
            a["momentum_buffer"] = 0.3 * (1 - mom ** step) / (1 - mom) * z
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in a.items()}


# ---- the reference: the real torch.optim class on the CPU -----------------------------------------------------------------
def reference(case, arrays, step, dtype=torch.float64, **override):
    """One ``opt.step()`` of ``torch.optim.<case.cls>(**case.kw)`` (single-tensor form) on one parameter holding
    ``arrays["p"]`` with gradient ``arrays["g"]`` and the state of ``arrays`` loaded at ``step`` through
    ``load_state_dict``.  Returns ``Ref(arrays, ratio)``: fp64 copies of ``p``, ``dp = p_new - p_old`` and every state
    tensor after the step, and max |dp| / max |p_old|.  ``override``: keyword arguments replacing the case's."""
    def T(a):
        return torch.tensor(a, dtype=dtype)                     # a copy: the step updates its tensors in place

    p = torch.nn.Parameter(T(arrays["p"]))
    opt = getattr(torch.optim, case.cls)([p], **{**case.kw, **override}, foreach=False)
    names = [k for k in case.states if k in arrays]
    st = {k: T(arrays[k]) for k in names}
    if case.cls != "SGD":
        st["step"] = torch.tensor(float(step))
    if st:
        sd = opt.state_dict()
        sd["state"] = {0: st}
        opt.load_state_dict(sd)
    p.grad = T(arrays["g"])
    p_old = p.detach().double().clone()
    opt.step()
    state = opt.state[p]
    if case.cls != "SGD":
        assert float(state["step"]) == step + 1, (float(state["step"]), step)
    out = {"p": p.detach().double(), "dp": p.detach().double() - p_old}
    for k in case.states:
        out[k] = state[k].detach().double()
    ratio = float(out["dp"].abs().max()) / float(p_old.abs().max())
    return Ref({k: v.numpy() for k, v in out.items()}, ratio)


def figure(got, ref):
    """max |got - ref| / max |ref| (0 / 0 is 0: an all-zero reference has to be met exactly)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))


FLOOR = 2.0 ** -22


def bar(e32):
    return max(4 * e32, FLOOR)


# ---- the raw call --------------------------------------------------------------------------------------------------------
def call_args(case, ptrs, live, n, step, stream):
    """Argument list of ``abi.call(case.entry, ...)``.  ``ptrs``: {array name: device address} (absent state: NULL);
    ``step``: the address of ``step_dev``, for ``itcv_adam_step`` the host step count (1-based)."""
    s = [ptrs.get(k) for k in {"adamx": ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), "sgd": ("momentum_buffer",),
                               "adagrad": ("sum",), "rmsprop": ("square_avg", "momentum_buffer", "grad_avg"),
                               "adam_dev": ("exp_avg", "exp_avg_sq"), "adam": ("exp_avg", "exp_avg_sq")}[case.kind]]
    if case.kind in ("adam_dev", "adam"):
        assert live is None
        return [case.entry, ptrs["p"], ptrs["g"], *s, n, *case.hp, step, stream]
    return [case.entry, ptrs["p"], ptrs["g"], *s, live, n, *case.hp, case.flags, step, stream]
