"""Flat parameter / gradient / optimiser-state buffers for one half of the model (encoder or decoder).

Parameters are re-pointed (``p.data``) into one contiguous fp32 buffer and their ``.grad`` into
a second one, so that the global gradient norm, the clip scaling, the Adam update and the
data-parallel all-reduce are each ONE kernel / ONE collective per half instead of one per
tensor (20 M parameters in ~100 tensors at the 64x64 configuration).  The nn.Parameter objects
themselves are untouched, so optimizers and state_dicts that reference them stay valid.
"""
import weakref

import torch

from . import abi
from .abi import call, lib, ptr, stream
from .functional import bump_weight_epoch, register_pack_group

F32 = torch.float32


class FlatGroup:
    def __init__(self, params, inherit=None, grad_free=()):
        """``inherit``: the group these parameters lived in before they were moved (``model.to()``, ``.float()``,
        ``load_state_dict(assign=True)`` ... after the first step): its optimiser state and step count carry over, so
        losing ownership never silently restarts the optimiser.  ``grad_free``: parameters torch never gives a gradient
        (models.grad_free_parameters); the fused updates other than plain Adam leave them untouched."""
        self.params = [p for p in params]
        assert self.params, "empty parameter group"
        dev = self.params[0].device
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.numel = total
        self.flat_p = torch.zeros(total, dtype=F32, device=dev)
        self.flat_g = torch.zeros(total, dtype=F32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=F32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=F32, device=dev)
        # optimiser state slots by torch's state key (Adam's two moments are the buffers above); the others are
        # allocated when an optimiser that keeps them is bound
        self.slots = {"exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq}
        self._family = None                                # state layout of the bound optimiser (see _state_names)
        self.step = 0                                      # host mirror (not advanced by graph replays)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)   # authoritative step count
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                n = p.numel()
                self.flat_p[o:o + n].copy_(p.data.reshape(-1))
                p.data = self.flat_p[o:o + n].view(p.shape)
        self._ws = torch.empty(lib.itcv_sumsq_workspace(total), dtype=torch.uint8, device=dev)
        # one byte per 4 elements, 0 over a grad-free parameter (every tensor starts on a 4-element boundary)
        free = {id(p) for p in grad_free}
        self.live = None
        if any(id(p) in free for p in self.params):
            live = torch.ones(total // 4, dtype=torch.uint8)
            for p, o in zip(self.params, self.offsets):
                if id(p) in free:
                    live[o // 4:(o + p.numel() + 3) // 4] = 0
            self.live = live.to(dev)
        self._opt, self._parent, self._names = None, inherit, None
        register_pack_group(self.params)       # their packed conv operands are refreshed by one launch per direction
        self.attach_grads()
        if inherit is not None:
            self._inherit(inherit)

    def _inherit(self, old):
        where = {id(p): (o, p.numel()) for p, o in zip(old.params, old.offsets)}
        self._family = old._family
        for name in old.slots:
            self._slot(name)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                src = where.get(id(p))
                if src is not None and src[1] == p.numel():
                    n = p.numel()
                    for name, buf in old.slots.items():
                        self.slots[name][o:o + n].copy_(buf[src[0]:src[0] + n])
                    # the (possibly stale) gradients too: the clip norm runs over them (solvers/intro.py:113-115)
                    self.flat_g[o:o + n].copy_(old.flat_g[src[0]:src[0] + n])
            self.step_dev.copy_(old.step_dev)
        self.step = old.step

    def _slot(self, name):
        buf = self.slots.get(name)
        if buf is None:
            buf = self.slots[name] = torch.zeros(self.numel, dtype=F32, device=self.flat_p.device)
        return buf

    # ---- torch.optim state mirror: optimizer.state_dict() / load_state_dict() keep working ------------------------
    def bind_optimizer(self, opt, spec=None):
        """Expose the state slots of ``spec``'s update (``fused_update(opt)``; None: plain Adam) as views inside
        ``opt.state`` under torch's own keys so ``opt.state_dict()`` saves them, and adopt whatever state ``opt`` already
        holds or later loads (``load_state_dict``).  The step count lives on the device (graph replays advance it); it
        is copied into the state's ``step`` entries right before a ``state_dict()`` call."""
        family, names, _ = _state_names(spec)
        if self._opt is opt and self._names == names:
            return
        if self._family is not None and self._family != family:
            # another optimiser class takes over the group: its state starts from torch's initial one
            for buf in self.slots.values():
                buf.zero_()
            self.step_dev.zero_()
            self.step = 0
        self._family, self._names = family, names
        for name in names:
            self._slot(name)
        new_opt, self._opt = self._opt is not opt, opt
        prev = getattr(opt, "_itcv_group", None)
        prev = prev() if prev is not None else None
        opt._itcv_group = weakref.ref(self)
        # state mirrored by the group these parameters came from was carried over by _inherit (with the device-side
        # step count, which the mirror's ``step`` entries lag behind): only re-point the views then
        self._adopt(opt, copy=not (prev is not None and prev is self._parent))
        if new_opt and hasattr(opt, "register_state_dict_pre_hook"):
            opt.register_state_dict_pre_hook(lambda o: self._refresh_steps(o) if self._current(o) else None)
            opt.register_load_state_dict_post_hook(lambda o: self._adopt(o) if self._current(o) else None)

    def _current(self, opt):
        ref = getattr(opt, "_itcv_group", None)
        return ref is not None and ref() is self

    def _mine(self, t, buf, o, n):
        return t is not None and t.data_ptr() == buf.data_ptr() + 4 * o and t.numel() == n and t.device == buf.device

    def _adopt(self, opt, copy=True):
        names, has_step = self._names, self._family != "sgd"
        step = None
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                n = p.numel()
                st = opt.state.get(p)
                if copy and st:
                    got = False
                    for name in names:
                        t = st.get(name)
                        if torch.is_tensor(t) and not self._mine(t, self.slots[name], o, n):
                            self.slots[name][o:o + n].copy_(t.reshape(-1))
                            got = True
                    if got:
                        # SGD keeps no count: a momentum buffer means its first step is behind it
                        k = int(st["step"]) if has_step and "step" in st else 1
                        step = k if step is None else max(step, k)
                if not names:
                    continue
                st = opt.state[p]
                for name in names:
                    st[name] = self.slots[name][o:o + n].view(p.shape)
                if has_step:
                    st.setdefault("step", torch.tensor(0.0))
            if step is not None:
                self.step = step
                self.step_dev.fill_(step)
        self._refresh_steps(opt)

    def _refresh_steps(self, opt):
        if opt is not self._opt or self._family == "sgd":
            return
        step = float(int(self.step_dev.item()))
        for p in self.params:
            st = opt.state.get(p)
            if st is not None:
                st["step"] = torch.tensor(step)

    def owns(self, params):
        ps = list(params)
        return len(ps) == len(self.params) and all(a is b for a, b in zip(ps, self.params)) and all(
            p.data_ptr() == self.flat_p.data_ptr() + 4 * o for p, o in zip(self.params, self.offsets))

    def attach_grads(self):
        for p, o in zip(self.params, self.offsets):
            want = self.flat_g.data_ptr() + 4 * o
            if p.grad is None or p.grad.data_ptr() != want:
                p.grad = self.flat_g[o:o + p.numel()].view(p.shape)

    def zero_grad(self):
        call("itcv_fill", ptr(self.flat_g), self.numel, 0.0, stream())
        self.attach_grads()

    def sumsq_into(self, out_f64_slot):
        call("itcv_sumsq", ptr(self.flat_g), self.numel, ptr(out_f64_slot), ptr(self._ws), self._ws.numel(), stream())

    def scale_grads(self, coef_dev):
        call("itcv_scale_by_dev", ptr(self.flat_g), self.numel, ptr(coef_dev), stream())

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8):
        self.step += 1
        call("itcv_adam_step_dev", ptr(self.flat_p), ptr(self.flat_g), ptr(self.exp_avg), ptr(self.exp_avg_sq),
             self.numel, float(lr), float(betas[0]), float(betas[1]), float(eps), ptr(self.step_dev), stream())
        bump_weight_epoch(self.params)   # these parameters changed behind torch's back: drop their packed copies

    def fused_step(self, spec):
        """One update of ``spec = fused_update(opt)`` over the whole group (the state slots bound by
        ``bind_optimizer``): plain Adam is ``adam_step``, every other kind one launch of its own kernel."""
        kind, flags, hp = spec
        if kind == "adam":
            self.adam_step(*hp)
            return
        self.step += 1
        s, live = self.slots, ptr(self.live)
        head = (ptr(self.flat_p), ptr(self.flat_g))
        if kind == "adamx":
            call("itcv_adamx_step_dev", *head, ptr(s["exp_avg"]), ptr(s["exp_avg_sq"]), ptr(s.get("max_exp_avg_sq")),
                 live, self.numel, *hp, flags, ptr(self.step_dev), stream())
        elif kind == "sgd":
            call("itcv_sgd_step_dev", *head, ptr(s.get("momentum_buffer")), live, self.numel, *hp, flags,
                 ptr(self.step_dev), stream())
        elif kind == "adagrad":
            call("itcv_adagrad_step_dev", *head, ptr(s["sum"]), live, self.numel, *hp, flags, ptr(self.step_dev),
                 stream())
        elif kind == "rmsprop":
            call("itcv_rmsprop_step_dev", *head, ptr(s["square_avg"]), ptr(s.get("momentum_buffer")),
                 ptr(s.get("grad_avg")), live, self.numel, *hp, flags, ptr(self.step_dev), stream())
        else:
            raise ValueError(f"unknown fused update {kind!r}")
        bump_weight_epoch(self.params)


def clip_grad_norm(groups, clip):
    """torch.nn.utils.clip_grad_norm_ over the union of ``groups`` (solvers/intro.py:113-115): returns the
    total norm as a 1-element device tensor; no host synchronisation."""
    dev = groups[0].flat_g.device
    sumsq = torch.empty(len(groups), dtype=torch.float64, device=dev)
    for i, g in enumerate(groups):
        g.sumsq_into(sumsq[i:i + 1])
    out = torch.empty(2, dtype=F32, device=dev)          # [norm, coef]
    call("itcv_clip_coef", ptr(sumsq), len(groups), float(clip), ptr(out[0:1]), ptr(out[1:2]), stream())
    for g in groups:
        g.scale_grads(out[1:2])
    return out[0:1]


_NUMBER = (float, int)


def _scalar(v):
    return v.__class__ in _NUMBER or (isinstance(v, (float, int)) and not isinstance(v, bool))


def fused_update(opt):
    """The fused update that reproduces ``opt.step()``, as a hashable ``(kind, flags, hyper-parameters)`` spec, or None
    when there is none (the caller then falls back to ``opt.step()``).  Covered: exactly (not subclasses of)
    torch.optim.Adam / AdamW / SGD / Adagrad / RMSprop with one param group of Python-number hyper-parameters, neither
    ``capturable`` nor ``differentiable``.  Adam without weight decay, amsgrad or maximize is ``"adam"`` (the plain
    kernel, ``FlatGroup.adam_step``); flags are the ITCV_OPT_* bits of include/itcv_hip.h.  Called on every step of a
    captured run (it is part of the graph key), so it stays cheap."""
    t = type(opt)
    keys = _HP_KEYS.get(t)
    if keys is None or len(opt.param_groups) != 1:
        return None
    g = opt.param_groups[0]
    if g.get("capturable", False) or g.get("differentiable", False):
        return None
    for k in keys:
        if not _scalar(g[k]):
            return None
    flags = _MAXIMIZE if g.get("maximize", False) else 0
    lr = g["lr"]
    if t is _ADAM or t is _ADAMW:
        betas = g["betas"]
        if len(betas) != 2 or not (_scalar(betas[0]) and _scalar(betas[1])):
            return None
        wd, ams = g["weight_decay"], bool(g.get("amsgrad", False))
        if wd == 0 and not ams and not flags:
            return "adam", 0, (lr, tuple(betas), g["eps"])
        flags |= (_AMSGRAD if ams else 0)
        flags |= _DECOUPLED_WD if t is _ADAMW or g.get("decoupled_weight_decay", False) else 0
        return "adamx", flags, (float(lr), float(betas[0]), float(betas[1]), float(g["eps"]), float(wd))
    if t is torch.optim.SGD:
        flags |= _NESTEROV if g.get("nesterov", False) else 0
        return "sgd", flags, (float(lr), float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"]))
    if t is torch.optim.Adagrad:
        return "adagrad", flags, (float(lr), float(g["lr_decay"]), float(g["weight_decay"]), float(g["eps"]))
    flags |= _CENTERED if g.get("centered", False) else 0
    return "rmsprop", flags, (float(lr), float(g["alpha"]), float(g["eps"]), float(g["weight_decay"]),
                              float(g["momentum"]))


_ADAM, _ADAMW = torch.optim.Adam, torch.optim.AdamW
_MAXIMIZE, _NESTEROV, _AMSGRAD, _DECOUPLED_WD, _CENTERED = (abi.OPT_MAXIMIZE, abi.OPT_NESTEROV, abi.OPT_AMSGRAD,
                                                            abi.OPT_DECOUPLED_WD, abi.OPT_CENTERED)
_HP_KEYS = {
    torch.optim.Adam: ("lr", "eps", "weight_decay"),
    torch.optim.AdamW: ("lr", "eps", "weight_decay"),
    torch.optim.SGD: ("lr", "momentum", "dampening", "weight_decay"),
    torch.optim.Adagrad: ("lr", "lr_decay", "weight_decay", "eps"),
    torch.optim.RMSprop: ("lr", "alpha", "eps", "weight_decay", "momentum"),
}


def _state_names(spec):
    """(family, torch state keys held in flat slots, spec) of a ``fused_update`` spec (None: plain Adam)."""
    if spec is None or spec[0] == "adam":
        return "adam", ("exp_avg", "exp_avg_sq"), spec
    kind, flags, hp = spec
    if kind == "adamx":
        return "adam", ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if flags & abi.OPT_AMSGRAD else ()), spec
    if kind == "sgd":
        return "sgd", ("momentum_buffer",) if hp[1] != 0 else (), spec
    if kind == "adagrad":
        return "adagrad", ("sum",), spec
    return "rmsprop", (("square_avg",) + (("momentum_buffer",) if hp[4] > 0 else ())
                       + (("grad_avg",) if flags & abi.OPT_CENTERED else ())), spec
