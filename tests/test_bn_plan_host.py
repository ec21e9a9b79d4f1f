"""CPU-only: which launches a BatchNorm training call gets (``bn_plan()`` of norm_act.hip, read through
``itcv_bn_plan_query``), pinned as literals for every BatchNorm layer of the c2 / c3 / c5 configurations, for the
transitions between the six paths, and for every case of tests/test_hip_bn.py.  A change to ``bn_splits`` or ``bn_plan``
that moves a shape onto other kernels fails here before a GPU is involved."""
import pytest

from test_hip_bn import CASES, plan

SF, OB, SC, FB, PG, TS = "SlicedFold", "OneBlock", "SlicedCombine", "Fallback", "PerGroup", "TileStats"

# (B per BatchNorm group, C, H, W) -> (path, slices): the same for the plain forward, the pooled forward and the backward
LAYERS = {
    "c2": [((64, 64, 64, 64), (SF, 16)), ((64, 128, 32, 32), (SF, 8)), ((64, 256, 16, 16), (OB, 1)),
           ((64, 512, 8, 8), (OB, 1)), ((64, 512, 4, 4), (OB, 1))],
    "c3": [((128, 64, 128, 128), (SF, 16)), ((128, 128, 64, 64), (SF, 8)), ((128, 256, 32, 32), (SF, 4)),
           ((128, 512, 16, 16), (OB, 1)), ((128, 512, 8, 8), (OB, 1)), ((128, 512, 4, 4), (OB, 1))],
    "c5": [((32, 64, 256, 256), (SF, 16)), ((32, 128, 128, 128), (SF, 8)), ((32, 256, 64, 64), (SF, 4)),
           ((32, 512, 32, 32), (OB, 1)), ((32, 512, 16, 16), (OB, 1)), ((32, 512, 8, 8), (OB, 1)),
           ((32, 512, 4, 4), (OB, 1))],
}


def q(*a, **k):
    from hipvae import abi
    return abi.bn_plan_query(*a, **k)


@pytest.mark.parametrize("cfg", sorted(LAYERS))
def test_production_layers(cfg):
    for shape, want in LAYERS[cfg]:
        for groups in (1, 2, 3):
            for ns in (2, 4):
                assert q(False, *shape, groups=groups, ns=ns) == want, (shape, groups, ns, "forward")
                assert q(False, *shape, pool=1, groups=groups, ns=ns) == want, (shape, groups, ns, "pooled forward")
                assert q(True, *shape, groups=groups, ns=ns) == want, (shape, groups, ns, "backward")
                assert q(True, *shape, pool=1, groups=groups, ns=ns) == want, (shape, groups, ns, "pooled backward")


def test_path_constants_follow_the_header():
    import os
    import re
    from hipvae import abi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "itcv_hip.h")).read()
    vals = dict(re.findall(r"#define ITCV_BN_PATH_([A-Z_]+) (\d+)", text))
    assert [vals[k] for k in ("ONE_BLOCK", "SLICED_FOLD", "SLICED_COMBINE", "FALLBACK", "PER_GROUP", "TILE_STATS")] == list("012345")
    assert abi.BN_PATHS == (OB, SF, SC, FB, PG, TS)


def test_transitions():
    from hipvae import abi
    # 64 threads per (image, 8 channels) plane: the apply launch folds the slices itself; below, a combine launch
    assert q(False, 16, 128, 16, 16) == (SF, 4)                      # per_plane = 256 / 4 = 64
    assert q(False, 16, 128, 16, 16, pool=1) == (SC, 4)              # pooled: 64 / 2 = 32
    assert q(True, 16, 128, 16, 16, pool=1) == (SF, 4)               # the backward's planes are those of dx: 64 again
    assert q(False, 6, 24, 12, 20) == (SC, 2) and q(True, 6, 24, 12, 20, up2=1) == (SC, 2)       # 240 / 4 = 60
    assert q(False, 6, 24, 16, 16) == (SF, 2)                        # 256 / 4 = 64
    assert q(False, 64, 128, 8, 8) == (SC, 4) and q(True, 64, 128, 8, 8, groups=2, ns=4) == (SC, 4)
    # C >= 256 with at most 65536 values a channel: one block per channel
    assert q(False, 64, 256, 32, 32) == (OB, 1) and q(False, 65, 256, 32, 32) == (SF, 4)
    assert q(False, 64, 248, 32, 32) == (SF, 5) and q(True, 64, 248, 16, 16) == (SF, 5)
    assert q(False, 3, 40, 6, 12) == (OB, 1) and q(False, 5, 16, 10, 12) == (OB, 1)             # at most 1024 values: one slice
    # no planes: the plain apply kernels, sliced or not
    assert q(False, 64, 64, 64, 64, planes=False) == (FB, 16) and q(True, 64, 512, 8, 8, planes=False, ns=0) == (FB, 1)
    assert q(False, 16, 32, 16, 16, planes=False) == (FB, 4) and q(False, 4, 6, 8, 8, planes=False) == (FB, 1)
    # shapes the planes kernels do not take
    assert q(False, 16, 12, 8, 8) == (FB, 1) and q(True, 16, 36, 16, 16) == (FB, 4)            # C % 8
    assert q(False, 3, 8, 4, 6) == (FB, 1) and q(True, 20, 8, 10, 6) == (FB, 2)                # W % 4
    assert q(False, 4, 16, 6, 8, pool=1) == (OB, 1) and q(False, 4, 16, 5, 8, pool=1) == (FB, 1)   # pooled planes: H % 2
    assert q(True, 4, 16, 5, 8, pool=1) == (OB, 1)                   # (the backward's planes are not pooled)
    assert q(False, 4, 16, 8, 8, ns=5) == (FB, 1)                    # no such plane format
    assert q(False, 3, 8, 4, 6, groups=2) == (PG, 1)                 # groups without planes go one by one
    # groups > 1 and a workspace that does not hold every group's partial sums (backward, fp16: and maxima)
    one = abi.lib.itcv_bn_workspace(16, 64, 32 * 32)
    assert q(False, 16, 64, 32, 32, groups=2, ws_bytes=one) == (PG, 16) and q(True, 16, 64, 32, 32, groups=2, ws_bytes=one) == (PG, 16)
    assert q(False, 16, 64, 32, 32, groups=2, ws_bytes=2 * one) == (SF, 16) and q(False, 16, 64, 32, 32, groups=1, ws_bytes=0) == (SF, 16)
    fwd_need = 2 * 16 * 2 * 64 * 8                                    # [G][slices][2][C] doubles
    assert q(False, 16, 64, 32, 32, groups=2, ws_bytes=fwd_need) == (SF, 16)
    assert q(False, 16, 64, 32, 32, groups=2, ws_bytes=fwd_need - 1) == (PG, 16)
    assert q(True, 16, 64, 32, 32, groups=2, ns=2, ws_bytes=fwd_need) == (SF, 16)
    assert q(True, 16, 64, 32, 32, groups=2, ns=4, ws_bytes=fwd_need) == (PG, 16)             # + [2][G * slices * C] floats
    assert q(True, 16, 64, 32, 32, groups=2, ns=4, ws_bytes=fwd_need * 3 // 2) == (SF, 16)
    assert q(False, 64, 512, 4, 4, groups=3, ws_bytes=0) == (OB, 1)  # one block per channel needs no workspace
    # statistics from the conv epilogue
    assert q(False, 4, 128, 32, 32, tile_stats=True) == (TS, 4) and q(False, 4, 128, 32, 32, groups=2, tile_stats=True) == (PG, 4)
    assert q(False, 4, 128, 32, 32, planes=False, tile_stats=True) == (TS, 4)
    # arguments
    assert abi.lib.itcv_bn_plan_query(0, 0, 8, 4, 4, 0, 0, 1, 1, 2, 0, 0, None, None) != 0
    assert "itcv_bn_plan_query" in abi.last_error()
    assert abi.lib.itcv_bn_plan_query(0, 4, 8, 4, 4, 0, 0, 1, 1, 2, 0, 0, None, None) == 0


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_gpu_cases_take_their_declared_path(c):
    for ns in (c.ns or (0,)):
        assert plan(c, False, ns) == c.fwd and plan(c, True, ns) == c.bwd, ns


def test_gpu_cases_cover_every_path_format_and_mode():
    paths = {p[0] for c in CASES for p in (c.fwd, c.bwd)}
    assert paths == {SF, OB, SC, FB, PG}                             # TileStats: test_hip_bn.test_bn_tile_stats_vs_fp64
    planes_cases = [c for c in CASES if c.planes]
    assert {n for c in planes_cases for n in c.ns} == {2, 3, 4}
    assert {(c.pool, c.up2) for c in planes_cases} == {(0, 0), (1, 0), (0, 1)}
    assert {c.G for c in planes_cases} == {1, 2, 3}
    assert any(c.skip for c in planes_cases) and any(c.acc for c in planes_cases)
    assert any(c.shape[3] & (c.shape[3] - 1) for c in planes_cases)  # a width that is no power of two
