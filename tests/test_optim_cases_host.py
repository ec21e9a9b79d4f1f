"""CPU-only checks of tests/optim_cases.py: the table reaches every launchable optimiser kernel instance, its cases are
what ``fused_update`` makes of the same torch optimiser, its inputs meet the conditions the device test relies on, its
sizes and masks hold every grid edge, and its fp64 reference with the device test's bar sees each of eight arithmetic
mistakes."""
import collections

import numpy as np
import pytest
import torch

import optim_cases as oc

STEPS = (0, 1, 999)
O = torch.optim


def test_table_reaches_every_launchable_instance():
    want = oc.launchable_instances()
    assert len(want) == 46 and len(set(want)) == 46
    assert collections.Counter(w[0] for w in want) == dict(adamx=12, sgd=12, adagrad=4, rmsprop=16, adam_dev=1, adam=1)
    got = [oc.instance_of(c) for c in oc.CASES]
    assert len(oc.CASES) == 46
    assert sorted(got) == sorted(want), sorted(set(want) - set(got))
    assert oc.instance_of(oc.CASES[0]) == ("adamx", 0, False, False)
    # the family cases are the instance with every flag set
    assert oc.instance_of(oc.FAMILY["adamx"]) == ("adamx", 2, True, True)
    assert oc.instance_of(oc.FAMILY["sgd"]) == ("sgd", True, True, True, True)
    assert oc.instance_of(oc.FAMILY["adagrad"]) == ("adagrad", True, True)
    assert oc.instance_of(oc.FAMILY["rmsprop"]) == ("rmsprop", True, True, True, True)
    assert [c.entry for c in oc.CASES[-2:]] == ["itcv_adam_step_dev", "itcv_adam_step"]


def test_hyper_parameters_are_spread():
    adam = [c for c in oc.CASES if c.kind == "adamx"]
    assert {c.hp[1] for c in adam} == {0.9, 0.5, 0.3, 0.0}
    assert {c.cls for c in adam if c.flags & oc.DECOUPLED_WD} == {"Adam", "AdamW"}
    cen = [c for c in oc.CASES if c.kind == "rmsprop" and c.flags & oc.CENTERED]
    assert {c.hp[1] for c in cen} == {0.99, 0.5, 0.3}
    sgd = [c for c in oc.CASES if c.kind == "sgd"]
    assert {c.hp[2] for c in sgd} == {0.0, 0.3}
    ada = [c for c in oc.CASES if c.kind == "adagrad"]
    assert {(c.hp[1], c.kw["initial_accumulator_value"]) for c in ada} == {(0.0, 0.0), (0.0, 0.1), (1e-2, 0.0),
                                                                          (1e-2, 0.1)}
    assert all(1e-2 <= c.kw["lr"] <= 1e-1 for c in list(oc.CASES) + list(oc.FAMILY.values()))


@pytest.mark.parametrize("case", list(oc.CASES) + list(oc.FAMILY.values()), ids=lambda c: c.name)
def test_fused_update_gives_the_case(case):
    from hipvae import abi
    from hipvae.flat import _state_names, fused_update
    assert (oc.MAXIMIZE, oc.NESTEROV, oc.AMSGRAD, oc.DECOUPLED_WD, oc.CENTERED) == (
        abi.OPT_MAXIMIZE, abi.OPT_NESTEROV, abi.OPT_AMSGRAD, abi.OPT_DECOUPLED_WD, abi.OPT_CENTERED)
    opt = getattr(O, case.cls)([torch.nn.Parameter(torch.zeros(4))], **case.kw)
    spec = fused_update(opt)
    if oc.instance_of(case) == ("adamx", 0, False, False) or case.kind in ("adam_dev", "adam"):
        # plain Adam goes to the plain kernel: the adamx instance is reached through the raw entry point only
        b, eps = case.kw.get("betas", (0.9, 0.999)), case.kw.get("eps", 1e-8)
        assert spec == ("adam", 0, (case.kw["lr"], b, eps))
        assert case.hp[:4] == (case.kw["lr"], b[0], b[1], eps)
        if case.kind != "adamx":                                   # what a C float argument holds
            assert all(float(np.float32(v)) == v for v in case.hp)
    else:
        assert spec == (case.kind, case.flags, case.hp)
    assert set(_state_names(spec)[1]) == set(case.states)


# fake 16-byte aligned device addresses: the calls fail in the host-side checks, before any launch
A, B, C, STEP = 0x10000, 0x20000, 0x30000, 0x50000


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("maximize", [0, oc.MAXIMIZE])
def test_nesterov_without_momentum_is_refused(wd, maximize):
    from hipvae import abi
    args = ("itcv_sgd_step_dev", A, B, C, None, 8, 0.1, 0.0, 0.0, wd, oc.NESTEROV | maximize, STEP, None)
    assert getattr(abi.lib, args[0])(*args[1:]) != 0
    assert "nesterov" in abi.last_error()
    with pytest.raises(abi.HipExtensionError):
        abi.call(*args)


def test_sizes_and_masks_hold_every_edge():
    grid = 2048 * 256
    assert oc.GRID == grid and oc.BLOCK == 256
    s4 = [n // 4 for n in oc.SIZES4]
    assert all(n % 4 == 0 for n in oc.SIZES4)
    assert s4[0] == 1 and s4[1] == 256 + 1 and s4[2] == 4 * 256 + 1      # 1, 2 and 5 blocks, the last with one thread
    assert s4[3] == grid and s4[4] == grid + 1 and s4[5] == grid + 77
    s1 = list(oc.SIZES1)
    assert s1[0] == 1 and s1[1] == 3 and s1[2] == 4 * 256 + 3
    assert s1[3:] == [grid, grid + 1, grid + 77]
    assert list(oc.SIZES4[oc.SMALL]) == [4, 1028, 4100] and [n // 4 for n in oc.SIZES4[oc.TRIPS]] == s4[3:]
    assert list(oc.SIZES1[oc.TRIPS]) == s1[3:]
    n4 = s4[5]
    m = {k: f(n4) for k, f in oc.MASKS.items()}
    assert set(m) == {"first", "last", "alternate", "block_edge", "trip_edge", "all"}
    assert all(v.dtype == np.uint8 and v.shape == (n4,) and set(np.unique(v)) <= {0, 1} for v in m.values())
    assert m["first"][0] == 0 and m["first"][1:].all()
    assert m["last"][-1] == 0 and m["last"][:-1].all()
    assert not m["alternate"][1::2].any() and m["alternate"][0::2].all()
    for name, edge in (("block_edge", 256), ("trip_edge", grid)):
        dead = np.flatnonzero(m[name] == 0)
        assert dead[0] < edge - 1 and dead[-1] > edge and (np.diff(dead) == 1).all() and len(dead) < 16, name
        assert m[name][dead[0] - 1] == 1 and m[name][dead[-1] + 1] == 1
    assert not m["all"].any()


def _denominators(case, ref):
    """The arrays whose square root (plus eps) divides the update."""
    r = ref.arrays
    if case.kind in ("adamx", "adam_dev", "adam"):
        return r["max_exp_avg_sq" if "max_exp_avg_sq" in case.states else "exp_avg_sq"], case.hp[3]
    if case.kind == "adagrad":
        return r["sum"], case.hp[3]
    if case.kind == "rmsprop":
        sq = r["square_avg"]
        return (sq - r["grad_avg"] ** 2 if "grad_avg" in case.states else sq), case.hp[2]
    return None, None


@pytest.mark.parametrize("case", list(oc.CASES) + list(oc.FAMILY.values()), ids=lambda c: c.name)
def test_inputs_meet_their_conditions(case):
    for n in oc.sizes(case)[oc.SMALL]:
        for step in STEPS:
            a = oc.inputs(case, n, step, seed=3)
            assert set(a) == {"p", "g"} | (set(case.states) if step or case.kind != "sgd" else set()), (n, step)
            assert all(v.dtype == np.float32 and v.shape == (n,) and np.isfinite(v).all() for v in a.values())
            i = np.arange(n)
            assert (a["g"][i % 7 == 3] == 0).all() and (a["p"][i % 13 == 2] == 0).all()
            if n >= 12:
                big = np.abs(a["g"][(i % 11 == 1) & (i % 7 != 3)])
                assert np.median(big) > 1000 * np.median(np.abs(a["g"][(i % 11 != 1)]))
            if n > 4:                                                   # a longer array starts with the shorter one
                b = oc.inputs(case, 4, step, seed=3)
                assert all(np.array_equal(a[k][:4], b[k]) for k in a)
            if "max_exp_avg_sq" in case.states and step and n >= 1028:
                above = float((a["max_exp_avg_sq"] > a["exp_avg_sq"]).mean())
                assert 0.4 < above < 0.6, above
            ref, r32 = oc.reference(case, a, step), oc.reference(case, a, step, torch.float32)
            for k, v in list(ref.arrays.items()) + list(r32.arrays.items()):
                assert np.isfinite(v).all(), (n, step, k)
            assert set(ref.arrays) == {"p", "dp"} | set(case.states)
            assert ref.ratio >= 1e-3, (n, step, ref.ratio)
            den, eps = _denominators(case, ref)
            if den is not None:
                assert eps > 0 and (den >= 0).all()
                if "grad_avg" in case.states:                              # the centred margin
                    assert (den >= 1e-3 * ref.arrays["square_avg"]).all(), (n, step)
                    d32 = r32.arrays["square_avg"] - r32.arrays["grad_avg"] ** 2
                    assert (d32 >= 0).all()
            if "max_exp_avg_sq" in case.states and step and n >= 1028:
                # both sides of fmaxf are taken
                kept = float((ref.arrays["max_exp_avg_sq"] > ref.arrays["exp_avg_sq"]).mean())
                assert 0.1 < kept < 0.9, kept


# ---- the reference moves under mistakes --------------------------------------------------------------------------------
def _lerp(s, e, w):
    return s + w * (e - s)


def np_step(case, a, step, mistake=None):
    """One step of the case's family restated in numpy (fp64), with one arithmetic ``mistake`` at most."""
    f, hp = case.flags, case.hp
    a = {k: v.astype(np.float64) for k, v in a.items()}
    p, g = a["p"].copy(), a["g"]
    if f & oc.MAXIMIZE and mistake != "maximize_ignored":
        g = -g
    t = step + 1
    out = {}
    if case.kind in ("adamx", "adam_dev", "adam"):
        lr, b1, b2, eps = hp[:4]
        wd = hp[4] if case.kind == "adamx" else 0.0
        g0 = g
        if wd and f & oc.DECOUPLED_WD:
            p = p * (1 - lr * wd)
        elif wd:
            g = g + wd * p
        m = _lerp(a["exp_avg"], g0 if mistake == "l2_after_moment" else g, 1 - b1)
        v = b2 * a["exp_avg_sq"] + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** t, 1 - (b1 if mistake == "bc2_from_beta1" else b2) ** t
        den = v
        if f & oc.AMSGRAD:
            out["max_exp_avg_sq"] = np.maximum(a["max_exp_avg_sq"], v)
            den = v if mistake == "amsgrad_max_dropped" else out["max_exp_avg_sq"]
        p = p - (lr / bc1) * m / (np.sqrt(den) / np.sqrt(bc2) + eps)
        out.update(exp_avg=m, exp_avg_sq=v)
    elif case.kind == "sgd":
        lr, mom, damp, wd = hp
        if wd:
            g = g + wd * p
        if mom:
            if step == 0 and mistake != "first_step_skipped":
                buf = g.copy()
            else:
                buf = mom * a.get("momentum_buffer", np.zeros_like(g)) + (1 - damp) * g
            out["momentum_buffer"] = buf
            if f & oc.NESTEROV:
                g = (buf if mistake == "nesterov_buf_for_g" else g) + mom * buf
            else:
                g = buf
        p = p - lr * g
    elif case.kind == "adagrad":
        lr, lr_decay, wd, eps = hp
        if wd:
            g = g + wd * p
        clr = lr / (1 + ((t if mistake == "clr_without_step_minus_1" else t - 1)) * lr_decay)
        out["sum"] = a["sum"] + g * g
        p = p - clr * g / (np.sqrt(out["sum"]) + eps)
    else:
        lr, alpha, eps, wd, mom = hp
        if wd:
            g = g + wd * p
        sq = alpha * a["square_avg"] + (1 - alpha) * g * g
        out["square_avg"] = sq
        if f & oc.CENTERED:
            ga = _lerp(a["grad_avg"], g, 1 - alpha)
            out["grad_avg"] = ga
            avg = np.sqrt(sq + ga * ga if mistake == "centred_plus" else sq - ga * ga)
        else:
            avg = np.sqrt(sq)
        avg = avg + eps
        if mom > 0:
            out["momentum_buffer"] = mom * a["momentum_buffer"] + g / avg
            p = p - lr * out["momentum_buffer"]
        else:
            p = p - lr * g / avg
    out["p"], out["dp"] = p, p - a["p"]
    return out


@pytest.mark.parametrize("case", list(oc.CASES) + list(oc.FAMILY.values()), ids=lambda c: c.name)
def test_numpy_restatement_equals_torch_fp64(case):
    for step in STEPS:
        a = oc.inputs(case, 4100, step, seed=5)
        ref, got = oc.reference(case, a, step).arrays, np_step(case, a, step)
        assert set(got) == set(ref)
        for k in ref:
            assert oc.figure(got[k], ref[k]) < 1e-12, (step, k, oc.figure(got[k], ref[k]))


MISTAKES = {
    "maximize_ignored": lambda c: c.flags & oc.MAXIMIZE,
    "l2_after_moment": lambda c: oc.instance_of(c)[:2] == ("adamx", 1),
    "bc2_from_beta1": lambda c: c.kind in ("adamx", "adam_dev", "adam"),
    "amsgrad_max_dropped": lambda c: c.flags & oc.AMSGRAD,
    "first_step_skipped": lambda c: c.kind == "sgd" and c.hp[1] != 0,
    "nesterov_buf_for_g": lambda c: c.flags & oc.NESTEROV,
    "clr_without_step_minus_1": lambda c: c.kind == "adagrad",
    "centred_plus": lambda c: c.flags & oc.CENTERED,
}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_reference_moves_under_mistake(mistake):
    """The mistaken step is further from the fp64 reference than the device test's bar, max(4 e32, 2^-22), on some array
    of some case (on ``p`` or ``dp`` wherever the mistake touches the update)."""
    red = []
    for case in oc.CASES:
        if not MISTAKES[mistake](case):
            continue
        for step in STEPS:
            a = oc.inputs(case, 4100, step, seed=5)
            ref, r32 = oc.reference(case, a, step).arrays, oc.reference(case, a, step, torch.float32).arrays
            bad = np_step(case, a, step, mistake)
            over = [k for k in ref if oc.figure(bad[k], ref[k]) > oc.bar(oc.figure(r32[k], ref[k]))]
            if over:
                red.append((case.name, step, over))
    print(mistake, len(red), red[:3])
    assert red, mistake
    assert any("p" in over and "dp" in over for _, _, over in red), red
