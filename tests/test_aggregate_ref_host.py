"""CPU-only checks of tests/aggregate_ref.py, the fp64 restatement that tests/test_hip_aggregate.py holds the streaming
aggregate-posterior kernel to, and of the new entry point's argument checks (which need no GPU):
the decomposition telescopes, uniform weights equal ``logw=None``, the generated inputs have the properties the GPU
tests rely on (a dominant component at the very end of the stream, spread rows, a floor that fires on some elements and
not on most), and every deliberate defect moves a checked array by more than 10 * TOL wherever it can apply."""
import ctypes
import math

import pytest
import torch

import aggregate_ref as R

SHAPES = [s for s in R.SHAPES + R.NARROW if s != R.LONG]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for shape in SHAPES:
        z, rows, mu, lv, lw = R.make_inputs(*shape)
        out[shape] = tuple(t.double() if t.is_floating_point() else t for t in (z, rows, mu, lv, lw))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=R.sid)
def test_decomposition_telescopes(cases, shape):
    z, rows, mu, lv, lw = cases[shape]
    for w in (None, lw):
        ps = R.per_sample(z, rows, mu, lv, w)
        total, direct = ps["mi"] + ps["tc"] + ps["dwkl"], ps["logqcx"] - ps["logpz"]
        scale = max(float(ps[k].abs().max()) for k in ("logqcx", "logpz", "logqz")) + float(ps["lse"].abs().sum(1).max())
        assert float((total - direct).abs().max()) <= 1e-14 * scale
        got = R.decomposition(z, rows, mu, lv, w)
        assert got["kl"] == got["mi"] + got["tc"] + got["dwkl"]
        assert abs(got["kl"] - float(direct.mean())) <= 1e-13 * scale
        assert got["marginal_entropies"].shape == got["dimwise_kl"].shape == (shape[2],)
        assert abs(got["dimwise_kl"].sum() - got["dwkl"]) <= 1e-12 * scale


@pytest.mark.parametrize("shape", SHAPES, ids=R.sid)
def test_no_weights_are_uniform_weights(cases, shape):
    z, _, mu, lv, _ = cases[shape]
    N = shape[1]
    a = R.log_density(z, mu, lv, None)
    b = R.log_density(z, mu, lv, torch.full((N,), -math.log(N), dtype=torch.float64))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and the chunking over rows changes nothing
    c = R.log_density(z, mu, lv, None, chunk_elems=1)
    assert R.rel_err(c[0], a[0]) <= 1e-15 and R.rel_err(c[1], a[1]) <= 1e-15


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 4 and s not in R.NARROW], ids=R.sid)
def test_preconditions(cases, shape):
    z, rows, mu, lv, _ = cases[shape]
    S, N, _ = shape
    near = R.near_count(S, N)
    share, floored = R.joint_shares(z, mu, lv)
    top = share.max(1)
    print(R.sid(shape), "near rows", top.values[:near].tolist(), "least concentrated row", float(top.values[near:].min()),
          "floored share", floored)
    assert near == 4 and rows[:near].tolist() == [N - 1 - j for j in range(near)]
    assert bool((top.values[:near] > 0.99).all()) and top.indices[:near].tolist() == rows[:near].tolist()
    assert float(top.values[near:].min()) < 0.5
    assert 0.0 < floored < 0.9


def applies(defect, shape, cases):
    """Where a defect cannot change anything, and why: drop_tail needs a component left after the tail is dropped (N = 1
    and N = 5 lose everything); clamp_outside needs a row whose LEADING joint term it changes -- the row that was moved
    by +30 (every component is below the floor in three dimensions), or a D at which sum_l lp of the nearest component
    is itself below -50; an element floored under one far component alone weighs e^-50 against the others either way;
    stale_max needs a second tile of 64 components."""
    z, _, mu, lv, _ = cases[shape]
    if defect == "drop_tail":
        return shape[1] - (shape[1] % R.TILE or 1) >= 1
    if defect == "clamp_outside":
        d = z.unsqueeze(1) - mu.unsqueeze(0)
        raw = -0.5 * (d * d * torch.exp(-lv.unsqueeze(0)) + lv.unsqueeze(0) + math.log(2 * math.pi))
        good, bad = raw.clamp(min=-50.0).sum(2).max(1).values, raw.sum(2).clamp(min=-50.0).max(1).values
        return float((good - bad).abs().max()) > 0.01
    if defect == "stale_max":
        return shape[1] > R.TILE
    return shape[1] > 1              # no_weight: one component has the weight 1 either way


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("shape", SHAPES, ids=R.sid)
def test_defects_are_visible(cases, shape, defect):
    z, _, mu, lv, lw = cases[shape]
    if not applies(defect, shape, cases):
        assert shape in ((1, 1, 1), (3, 5, 10)), "only the two smallest shapes may be out of a defect's reach"
        return
    w = lw if defect == "no_weight" else None
    good, bad = R.log_density(z, mu, lv, w), R.log_density(z, mu, lv, w, defect)
    moved = max(R.rel_err(bad[0], good[0]), R.rel_err(bad[1], good[1]))
    print(R.sid(shape), defect, "moves logqz / lse by", moved)
    assert moved > 10 * R.TOL


def test_the_entry_point_refuses_bad_arguments_without_a_gpu():
    from hipvae import abi
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)            # non-null; never dereferenced: every call below is refused before a launch
    ok = dict(S=4, N=8, D=3)

    def run(S=4, N=8, D=3, splits=0, z=a, mu=a, lv=a, lw=None, q=a, e=a, ws=a, nws=1 << 30):
        return abi.lib.itcv_aggregate_logdensity(z, mu, lv, lw, q, e, S, N, D, splits, ws, nws, None)

    assert run(D=513) != 0 and "latent size" in abi.last_error()
    assert run(D=0) != 0 and "latent size" in abi.last_error()
    assert run(S=0) != 0 and "at least one" in abi.last_error()
    assert run(N=0) != 0 and "at least one" in abi.last_error()
    for name in ("z", "mu", "lv", "q", "e"):
        assert run(**{name: None}) != 0 and "requirement failed" in abi.last_error(), name
    assert run(ws=None) != 0 and "workspace" in abi.last_error()
    need = abi.lib.itcv_aggregate_workspace(ok["S"], ok["N"], ok["D"], 2)
    assert need == 2 * 4 * 2 * (3 + 1) * 4
    assert run(splits=2, nws=need - 1) != 0 and "workspace" in abi.last_error()
    # the workspace is 2 * S * slices * (D + 1) floats with slices <= min(N, 1024): nothing grows with S * N
    ws = abi.lib.itcv_aggregate_workspace
    assert ws(100, 1000, 10, 3) == 2 * 100 * 3 * 11 * 4
    assert ws(100, 2, 10, 3) == 2 * 100 * 2 * 11 * 4                       # no more slices than components
    assert ws(100, 10, 10, 4) == 2 * 100 * 4 * 11 * 4 and ws(100, 9, 10, 4) == 2 * 100 * 3 * 11 * 4    # none empty
    assert ws(0, 5, 10, 1) == 0 and ws(5, 0, 10, 1) == 0 and ws(5, 5, 513, 1) == 0
    for S, N, D in ((1, 1, 1), (10000, 737280, 10), (256, 737280, 10), (1 << 20, 1 << 30, 512)):
        assert 0 < ws(S, N, D, 0) <= 2 * S * 1024 * (D + 1) * 4
        assert ws(S, N, D, 1 << 20) <= 2 * S * min(N, 1024) * (D + 1) * 4
    assert ws(10000, 737280, 10, 0) == ws(10000, 2 * 737280, 10, 0)        # the slice count follows the row tiles, not N
