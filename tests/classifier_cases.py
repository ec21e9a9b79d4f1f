"""Case tables of the softmax-regression kernels (csrc/logreg.hip) and of the boosted-tree kernels (csrc/gbt.hip), with
the inputs and the numpy fp64 references they are compared against.  Importable without a GPU:
test_classifier_cases_host.py proves on the CPU that the tables reach every kernel instance, grid trip and tail they
claim, test_hip_classifier_kernels.py runs them on the device.

The references are the restatements of test_classify_host.py and test_gbt_host.py, imported, never copied.  Inputs and
references are built once per process (``functools.lru_cache``) and must not be modified by a test.

The library has no query function for its planning rules, so the few lines below restate them from logreg.hip / gbt.hip
(``lr_lds``, ``lr_mt``, ``lr_blocks``, ``proba_blocks``, ``stat_slices``, ``auc_plan``, ``gbt_chunks``, ``hist_tf``,
``split_scan_steps``); the host test pins them with literals.

Tolerances of the softmax regression (``lr_bounds``).  tests/test_hip_classify.py derives (D + 2) ulp of A per logit,
A = max_i,c (sum_d |x_id| |W_dc| + |b_c|), and allows 512 ulp = 4 (D + 2) at D + 2 <= 130; here D reaches 512, so the
factor is max(512, 4 (D + 2)) with the same multipliers:
  |f - ref| <= U ulp max(1, A, f)      |grad - ref| <= U ulp max(1, max|x|) max(1, A)      |P - ref| <= U ulp max(1, A).
That derivation says "the means over the rows do not grow it", which ignores the length of the sums.  Where a block
takes more than one trip (the two second-trip cases) the longest chain of additions behind one gradient element is
  16 MT          one per row of a tile: 4 MT MFMA steps (v_mfma_f64_16x16x4) of 4 products each,
  x trips        tiles of one block, ceil(tiles / blocks),
  + (trips - 1)  the ``*q + acc[i]`` of every trip after the first,
  + blocks       lr_fold_grad_kernel's ascending fold of the per-block partials (fold_strided: one addition per term).
Every partial sum is at most n max|x| (|P - Y| <= 1) and the result is scaled by 1 / n, so each addition contributes at
most one ulp of max|x|: ``lr_grad_additions`` ulp of max(1, max|x|) are allowed on top.  That is 32 * 2 + 1 + 1024 = 1089
at mt2-second-trip and 16 * 2 + 1 + 1024 = 1057 at mt1-second-trip.  The value's chain: a wave adds the losses of its
4 MT rows of every tile, the four waves are combined with 3 additions, lr_fold_value_kernel folds the blocks:
4 MT trips + 3 + blocks additions (1043 and 1035), each of at most one ulp of the largest row loss, which is at most
2 A + log(segmax) (logsumexp <= A + log S, -z_y <= A)."""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

from test_classify_host import offsets, ref_colstats, ref_pair_counts, ref_prepare, ref_proba, ref_valgrad_all
from test_gbt_host import NODES, ONE_Q, ref_bin, ref_cuts, ref_hist, ref_leaf, ref_split, ref_walk

ULP = 2.220446049250313e-16


def cdiv(a, b):
    return -(-a // b)


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


# ---- mirrors of the host's planning rules (logreg.hip) ---------------------------------------------------------------
LR_MAX_K, LR_MAX_BLOCKS, LR_PART_BUDGET, LR_LDS_TWO_TILES = 16, 1024, 256 << 20, 96 * 1024
LR_LDS_LIMIT = 160 * 1024                    # LDS of a CDNA4 compute unit


def lr_lds(mt, D, segmax):
    """Dynamic LDS of lr_softmax_kernel<mt, *>: xs[16 mt][D | 1], zs[16 mt][segmax | 1], fs and cs [4][16]."""
    return (16 * mt * ((D | 1) + (segmax | 1)) + 4 * LR_MAX_K) * 8 + 4 * LR_MAX_K * 4


def lr_mt(D, segmax):
    return 2 if lr_lds(2, D, segmax) <= LR_LDS_TWO_TILES else 1


def lr_blocks(N, D, csum, mt):
    """(blocks, row tiles) of itcv_logreg_valgrad: one partial gradient per block within 256 MiB, 1024 blocks at most."""
    nb = min(max(LR_PART_BUDGET // ((D + 1) * csum * 8), 1), LR_MAX_BLOCKS)
    nt = cdiv(N, 16 * mt)
    return min(nt, nb), nt


def proba_blocks(N, mt):
    """(blocks, row tiles) of itcv_logreg_proba: no partials, so four times the block cap."""
    nt = cdiv(N, 16 * mt)
    return min(nt, 4 * LR_MAX_BLOCKS), nt


def stat_slices(N):
    """(slices, rows per slice) of itcv_logreg_colstats: 256 rows, doubled until at most 1024 slices remain."""
    rows = 256
    while cdiv(N, rows) > 1024:
        rows *= 2
    return cdiv(N, rows), rows


def auc_plan(N, K):
    """(js, jrows) of itcv_logreg_auc: slices of whole 16-row LDS tiles, enough blocks to fill the device, 64 at most."""
    ni = cdiv(N, 256)
    js = min(max(cdiv(2048, ni * K), 1), 64)
    jrows = cdiv(cdiv(N, js), 16) * 16
    return cdiv(N, jrows), jrows


def auc_lds(segmax):
    return 16 * segmax * 8 + 16 * 4


# ---- mirrors of the host's planning rules (gbt.hip) ------------------------------------------------------------------
def gbt_slot_bytes(D, max_depth, max_bin):
    """One class slot of the histogram table: the nodes of the deepest level x D x max_bin x (G, H) int64."""
    return (1 << (max_depth - 1)) * D * max_bin * 16


def gbt_chunks(tab_bytes, D, max_depth, max_bin, csum):
    """The (c0, nc) class chunks of itcv_gbt_round under a table of ``tab_bytes``."""
    chunk = min(tab_bytes // gbt_slot_bytes(D, max_depth, max_bin), csum)
    assert chunk >= 1
    return [(c0, min(chunk, csum - c0)) for c0 in range(0, csum, chunk)]


def hist_tf(level, D, B):
    """Features per block of gbt_hist_kernel: what fits 64 KiB of LDS, 32 at most, one at least."""
    tf = min(max((64 * 1024) // ((1 << level) * B * 16), 1), 32)
    return min(tf, D)


def split_scan_steps(nbins):
    """64-bin steps of gbt_split_kernel's scan over a feature: ``for (b0 = 0; b0 < nbins - 1; b0 += 64)``."""
    return cdiv(max(nbins - 1, 0), 64)


# ---- softmax regression: the cases -----------------------------------------------------------------------------------
# std: x is standardised (mean, scale handed to the kernel); ld: row stride of x (0: dense).  Wherever a problem has
# S >= 3 classes its class S // 2 is invalid and rows 0..2 (at least) are labelled with it.
LrCase = namedtuple("LrCase", "id N D sizes std ld")
LR_CASES = [
    LrCase("mt2-largest-lds", 70, 377, (3,), 1, 0),                  # 98048 B, last tile 6 rows
    LrCase("mt1-smallest", 70, 379, (3, 2), 0, 384),                 # first one-tile shape, two problems share xs
    LrCase("mt1-wide-classes", 37, 257, (129, 3), 1, 261),           # 9 column tiles, last of one column, two lane strides
    LrCase("mt2-wide-classes", 37, 251, (129,), 0, 0),               # the same on the two-tile instance
    LrCase("mt1-top-of-range", 19, 512, (256,), 1, 0),               # 99328 B, four lane strides
    LrCase("mt2-second-trip", 32805, 3, (2, 3), 1, 4),               # 1026 tiles on 1024 blocks, last tile 5 rows
    LrCase("mt1-second-trip", 16389, 379, (3,), 0, 0),               # 1025 tiles on 1024 blocks, last tile 5 rows
    LrCase("k16-single-class", 50, 5, (1,) * 3 + (2,) * 13, 0, 8),   # K = 16, problems of one class
    LrCase("argmax-ties", 64, 4, (130,), 0, 0),                      # equal logits in different lane strides and lanes
    LrCase("column-tiles-16-17-65", 37, 5, (16, 17, 65), 1, 0),      # a full tile, tile + 1 column, lane stride + 1 column
]
LR_BY_ID = {c.id: c for c in LR_CASES}
# argmax-ties: the classes of a group share one column of theta, so their logits are equal bit for bit.  Group A wins
# where x . (wA - wB) > 0, group B elsewhere; the invalid class 65 carries group A's column too and must be skipped.
TIE_GROUP_A, TIE_GROUP_B, TIE_INVALID = (69, 5, 70, 129), (64, 128, 1), 65
PROBA_CASE = LrCase("proba-above-block-cap", 131107, 2, (2,), 1, 0)  # 4098 tiles on 4096 blocks
COLSTATS_CASES = [("doubled-rows", 262401, 2, 0), ("second-column-tile-of-one", 300, 65, 70)]   # id, N, D, ld
AUC_CASES = [("largest-lds-tile", 300, (256, 2)), ("short-last-slice", 1100, (3,))]               # id, N, sizes


def lr_invalid(sizes):
    """cvalid[csum]: class S // 2 of every problem with S >= 3 takes no part."""
    off = offsets(sizes)
    cvalid = np.ones(off[-1], dtype=bool)
    for k, s in enumerate(sizes):
        if s >= 3:
            cvalid[off[k] + s // 2] = False
    return cvalid


@functools.lru_cache(maxsize=None)
def lr_inputs(cid):
    """dict(wide fp32 [N, ld or D], x = wide[:, :D], y int32 [N, K], cvalid, stats or None, thetas [zero, random])."""
    c = LR_BY_ID[cid] if cid in LR_BY_ID else PROBA_CASE
    assert c.id == cid
    rs = np.random.RandomState(seed_of(cid))
    K, off = len(c.sizes), offsets(c.sizes)
    y = np.stack([rs.randint(s, size=c.N) for s in c.sizes], 1).astype(np.int32)
    for k, s in enumerate(c.sizes):
        if s >= 3:
            y[:min(3, c.N), k] = s // 2
    wide = (1.5 * rs.randn(c.N, c.ld or c.D) + 0.7).astype(np.float32)
    wide[:, 0] += 2.0 * y[:, -1] / c.sizes[-1]                                          # something to learn
    x = wide[:, :c.D]
    theta = 0.5 * rs.randn(c.D + 1, off[-1])
    if cid == "argmax-ties":
        theta *= 0.2
        wa, wb = 0.5 * rs.randn(c.D + 1), 0.5 * rs.randn(c.D + 1)
        wa[-1], wb[-1] = 30.0, 30.0                                         # far above every other class
        theta[:, list(TIE_GROUP_A) + [TIE_INVALID]] = wa[:, None]
        theta[:, list(TIE_GROUP_B)] = wb[:, None]
    stats = ref_colstats(x) if c.std else None
    return dict(case=c, wide=wide, x=x, y=y, cvalid=lr_invalid(c.sizes), stats=stats,
                thetas=[np.zeros((c.D + 1, off[-1])), theta])


def lr_grad_additions(N, D, sizes):
    """(gradient chain, value chain, trips): additions on the longest path (module docstring)."""
    mt = lr_mt(D, max(sizes))
    nb, nt = lr_blocks(N, D, sum(sizes), mt)
    trips = cdiv(nt, nb)
    return 16 * mt * trips + (trips - 1) + nb, 4 * mt * trips + 3 + nb, trips


def lr_bounds(c, X, theta, rf):
    """(A, bound on f, bound on the gradient, bound on the probabilities) of the module docstring."""
    A = max(1.0, float((np.abs(X) @ np.abs(theta[:-1]) + np.abs(theta[-1])).max()))
    xmax = max(1.0, float(np.abs(X).max()))
    u = max(512, 4 * (c.D + 2)) * ULP
    bf, bg = u * max(A, float(np.max(rf))), u * xmax * A
    ng, nf, trips = lr_grad_additions(c.N, c.D, c.sizes)
    if trips > 1:
        bg += ng * ULP * xmax
        bf += nf * ULP * (2.0 * A + math.log(max(c.sizes)))
    return A, bf, bg, u * A


@functools.lru_cache(maxsize=None)
def lr_reference(cid):
    """Per theta: dict(f, g, P [N, csum], pred [N, K], A, bf, bg, bp).  X is the prepared fp64 matrix."""
    inp = lr_inputs(cid)
    c, y, cvalid = inp["case"], inp["y"], inp["cvalid"]
    X = ref_prepare(inp["x"], inp["stats"])
    off = offsets(c.sizes)
    out = []
    for theta in inp["thetas"]:
        P, pred = np.zeros((c.N, off[-1])), np.zeros((c.N, len(c.sizes)), dtype=np.int64)
        for k in range(len(c.sizes)):
            sl = slice(off[k], off[k + 1])
            P[:, sl], pred[:, k] = ref_proba(theta[:, sl], X, y[:, k], cvalid[sl])
        if cid == PROBA_CASE.id:
            rf, rg = np.zeros(len(c.sizes)), None
        else:
            rf, rg = ref_valgrad_all(theta, X, y, list(c.sizes), cvalid)
        if not theta.any():                                                 # every logit ties: the first valid class
            pred = np.stack([np.full(c.N, np.flatnonzero(cvalid[off[k]:off[k + 1]])[0]) for k in range(len(c.sizes))], 1)
        elif cid == "argmax-ties":                                          # stated directly, not through BLAS
            wa, wb = theta[:, TIE_GROUP_A[0]], theta[:, TIE_GROUP_B[0]]
            za, zb = X @ wa[:-1] + wa[-1], X @ wb[:-1] + wb[-1]
            assert (za != zb).all() and (np.delete(X @ theta[:-1] + theta[-1], TIE_GROUP_A + TIE_GROUP_B + (TIE_INVALID,),
                                                   axis=1).max(1) < np.minimum(za, zb)).all()
            pred = np.where(za > zb, min(TIE_GROUP_A), min(TIE_GROUP_B))[:, None]
        A, bf, bg, bp = lr_bounds(c, X, theta, rf)
        out.append(dict(f=rf, g=rg, P=P, pred=pred, A=A, bf=bf, bg=bg, bp=bp))
    return out


@functools.lru_cache(maxsize=None)
def colstats_inputs(cid):
    _, N, D, ld = next(c for c in COLSTATS_CASES if c[0] == cid)
    rs = np.random.RandomState(seed_of(cid))
    wide = (rs.randn(N, ld or D) * 2.0 + 3.0).astype(np.float32)
    wide[:, 1] = np.float32(1.25)                                           # a constant column: scale 1
    return wide, wide[:, :D], ref_colstats(wide[:, :D])


@functools.lru_cache(maxsize=None)
def auc_inputs(cid):
    """(P [N, csum] with heavy ties, y [N, K] with labels of the invalid class and labels out of range, cvalid, and per
    problem the reference (count2, pos, neg) over the rows whose label is in range)."""
    _, N, sizes = next(c for c in AUC_CASES if c[0] == cid)
    rs = np.random.RandomState(seed_of(cid))
    off = offsets(sizes)
    P = rs.randint(0, 8, size=(N, off[-1])) / 8.0                           # eight distinct scores: most pairs tie
    y = np.stack([rs.randint(s, size=N) for s in sizes], 1).astype(np.int32)
    cvalid = lr_invalid(sizes)
    y[:4, 0] = sizes[0] // 2 if sizes[0] >= 3 else y[:4, 0]                 # rows of the invalid class
    y[5, 0], y[6, 0], y[7, -1] = sizes[0], -1, sizes[-1] + 3                # out of range: flag 1, the rows count nowhere
    want = []
    for k, s in enumerate(sizes):
        ok = (y[:, k] >= 0) & (y[:, k] < s)
        want.append(ref_pair_counts(P[ok, off[k]:off[k + 1]], y[ok, k], cvalid[off[k]:off[k + 1]]))
    return P, y, cvalid, want


# ---- boosted trees: growing one tree a stage at a time ----------------------------------------------------------------
GROW_CHUNKS = ((0, 2), (2, 3), (5, 1))           # (c0, nc): six class slots, the middle chunk holds the invalid class 3
GROW_CVALID = np.array([1, 1, 1, 0, 1, 1], dtype=bool)
GROW_DEPTH, GROW_B, GROW_LAM, GROW_ETA = 6, 256, 1.0, 0.3
GROW_NBINS = {"six-features": [1, 2, 65, 66, 129, 256], "one-feature-three-rows": [3]}
GROW_SHAPES = {"six-features": (1500, 6), "one-feature-three-rows": (3, 1)}
LEAF_CLASS, LEAF_NODE = 1, 2                     # six-features: this node exists from level 1 on and never splits


def _level_values(rs, N, k, groups=None):
    """N values out of k levels, every level on at least N // k rows (so every level is hit by a quantile candidate),
    in random row order; with ``groups`` (0 / 1 per row) the lower half of the levels goes to group 0."""
    if groups is None:
        return rs.permutation(np.arange(N) % k).astype(np.float32)
    out = np.zeros(N, dtype=np.float32)
    lo = k // 2
    for g, (first, n) in enumerate(((0, lo), (lo, k - lo))):
        rows = np.flatnonzero(groups == g)
        out[rows] = first + rs.permutation(np.arange(len(rows)) % n)
    return out


@functools.lru_cache(maxsize=None)
def grow_inputs(name):
    """dict(x fp32 [N, D], cuts, nbins, bins uint8 [D, N], gq, hq int64 [6, N]).

    six-features: feature 0 is constant, 1 binary, 2 / 3 / 4 have 65 / 66 / 129 levels, 5 is continuous (256 bins).
    Feature 4's levels 0..63 lie on the rows with feature 1 == 0 and 64..128 on the others: its cut at bin 63 makes the
    partition of feature 1's only cut, with bit-equal sums and gain, and the smaller key (feature 1, another wave) must
    win.  Class 1's gradient follows feature 1, and its rows with feature 1 == 1 carry a hessian sum of 1.5 units in
    all: the root's split is admissible, no split of node 2 is (min_child_weight = 1 on both sides)."""
    N, D = GROW_SHAPES[name]
    rs = np.random.RandomState(seed_of(name))
    if name == "one-feature-three-rows":
        x = np.array([[0.5], [-1.0], [2.0]], dtype=np.float32)
        gq = rs.randint(-ONE_Q, ONE_Q + 1, size=(6, N)).astype(np.int64)
        hq = np.full((6, N), ONE_Q, dtype=np.int64)
    else:
        x = np.zeros((N, D), dtype=np.float32)
        x[:, 0] = np.float32(-2.5)
        f1 = rs.permutation(np.arange(N) % 2)
        x[:, 1] = f1
        x[:, 2], x[:, 3] = _level_values(rs, N, 65), _level_values(rs, N, 66)
        x[:, 4] = _level_values(rs, N, 129, groups=f1)
        x[:, 5] = rs.randn(N).astype(np.float32)
        t2, t3, t4, t5 = x[:, 2] > 32, x[:, 3] > 40, x[:, 4] > 30, x[:, 5] > 0.3
        sign = np.stack([np.where(t5 ^ t3, 1, -1), 2 * f1 - 1, np.where(t3 ^ t2 ^ (x[:, 5] < -0.5), 1, -1),
                         np.ones(N, dtype=int), np.where(t2 ^ t4, 1, -1), np.where(t5 ^ t4 ^ t2, 1, -1)])
        gq = (sign * (ONE_Q // 2) + rs.randint(-ONE_Q // 2, ONE_Q // 2 + 1, size=(6, N))).astype(np.int64)
        hq = (ONE_Q // 4 + rs.randint(0, ONE_Q // 8, size=(6, N))).astype(np.int64)
        gq[LEAF_CLASS] = (2 * f1 - 1) * (ONE_Q // 2) + rs.randint(-1000, 1001, size=N)
        right = np.flatnonzero(f1 == 1)
        hq[LEAF_CLASS, right] = (3 * ONE_Q // 2) // len(right)
    cuts, nbins = ref_cuts(x, GROW_B)
    return dict(x=x, cuts=cuts, nbins=nbins, bins=ref_bin(x, cuts), gq=gq, hq=hq)


def np_advance(bins, tfeat, tbin, node, level, cvalid):
    """The numpy advance: rows in a split node of the level move to its children; everything else stays."""
    out = node.copy()
    base, nn = (1 << level) - 1, 1 << level
    for c in np.flatnonzero(cvalid):
        nid = node[c].astype(np.int64)
        f = tfeat[c][np.minimum(nid, NODES - 1)]
        move = (nid >= base) & (nid < base + nn) & (f >= 0)
        right = bins[np.where(move, f, 0), np.arange(node.shape[1])] > tbin[c][np.minimum(nid, NODES - 1)]
        out[c] = np.where(move, 2 * nid + 1 + right, nid).astype(node.dtype)
    return out


@functools.lru_cache(maxsize=None)
def grow_reference(name):
    """One snapshot per level: dict(tabs {class: [2^level, D, B, 2]}, tfeat, tbin, tvalue, tgain [6, 127], nsum
    [6, 127, 2], node [6, N] after the level's advance, ties {class: root tie seen}) by ref_hist / ref_split / ref_leaf."""
    inp = grow_inputs(name)
    bins, nbins, gq, hq = inp["bins"], inp["nbins"], inp["gq"], inp["hq"]
    N = bins.shape[1]
    tfeat, tbin = np.full((6, NODES), -1, dtype=np.int32), np.zeros((6, NODES), dtype=np.int32)
    tvalue, tgain = np.zeros((6, NODES)), np.zeros((6, NODES))
    nsum, node = np.zeros((6, NODES, 2), dtype=np.int64), np.zeros((6, N), dtype=np.uint8)
    levels = []
    for level in range(GROW_DEPTH):
        base, tabs = (1 << level) - 1, {}
        for c in np.flatnonzero(GROW_CVALID):
            tabs[c] = ref_hist(bins, gq[c], hq[c], node[c], level, GROW_B)
            if level == 0:
                nsum[c, 0] = gq[c].sum(), hq[c].sum()
                tvalue[c, 0] = ref_leaf(*nsum[c, 0], GROW_LAM, GROW_ETA)
            for j in range(1 << level):
                nid = base + j
                if level and tfeat[c, (nid - 1) // 2] < 0:
                    continue                                                # the parent is a leaf
                GP, HP = (int(v) for v in nsum[c, nid])
                got = ref_split(tabs[c][j], nbins, GP, HP, GROW_LAM)
                if got is None:
                    continue
                d, b, gain, GL, HL, _ = got
                tfeat[c, nid], tbin[c, nid], tgain[c, nid] = d, b, gain
                nsum[c, 2 * nid + 1], nsum[c, 2 * nid + 2] = (GL, HL), (GP - GL, HP - HL)
                tvalue[c, 2 * nid + 1] = ref_leaf(GL, HL, GROW_LAM, GROW_ETA)
                tvalue[c, 2 * nid + 2] = ref_leaf(GP - GL, HP - HL, GROW_LAM, GROW_ETA)
        node = np_advance(bins, tfeat, tbin, node, level, GROW_CVALID)
        levels.append(dict(tabs=tabs, tfeat=tfeat.copy(), tbin=tbin.copy(), tvalue=tvalue.copy(), tgain=tgain.copy(),
                           nsum=nsum.copy(), node=node.copy()))
    return levels


def grown_tree():
    """(bins, final node ids, (tfeat, tbin, tvalue, tgain)) of six-features after all six levels."""
    last = grow_reference("six-features")[-1]
    return grow_inputs("six-features")["bins"], last["node"], (last["tfeat"], last["tbin"], last["tvalue"], last["tgain"])


# ---- boosted trees: the other stages ----------------------------------------------------------------------------------
MARGIN_ROWS = (1, 257)
PREDICT_ROWS = (1, 63, 64, 65, 257)
PREDICT_SIZES = (3, 4, 2)                        # the last problem has no valid class
PREDICT_CVALID = np.array([1, 1, 1, 0, 1, 1, 1, 0, 0], dtype=bool)
IMPORTANCE = dict(rounds=3, sizes=(3, 2), D=300, unused=7)
CUTS_CASES = ((2, 130), (257, 130))              # (N, D) at max_bin = 256
GRAD_CASE = dict(N=65, sizes=(256, 2))
ROUND_SLOTS = (1, 2, 4)                          # class slots of the table in the chunked fits (csum = 11)


@functools.lru_cache(maxsize=None)
def margin_inputs(N):
    """(other bins uint8 [6, N], F0 [6, N]) and per max_depth in (6, 2) the leaves ref_walk reaches."""
    _, _, (tfeat, tbin, _, _) = grown_tree()
    nbins = grow_inputs("six-features")["nbins"]
    rs = np.random.RandomState(1000 + N)
    bins = np.stack([rs.randint(nb, size=N) for nb in nbins]).astype(np.uint8)
    F0 = rs.randn(6, N)
    walks = {md: np.stack([ref_walk(bins, tfeat[c], tbin[c], md) for c in range(6)]) for md in (6, 2)}
    return bins, F0, walks


@functools.lru_cache(maxsize=None)
def predict_inputs(N):
    """(F [9, N] out of three values so that maxima tie, y [N, 3] with labels out of range, pred [N, 3], correct [3])."""
    rs = np.random.RandomState(2000 + N)
    off = offsets(PREDICT_SIZES)
    F = rs.randint(0, 3, size=(off[-1], N)).astype(np.float64) - 1.0
    y = np.stack([rs.randint(s, size=N) for s in PREDICT_SIZES], 1).astype(np.int32)
    y[0, 1] = PREDICT_SIZES[1]                                               # out of range: flag 1, a miss
    y[N // 2, 2] = -1                                                        # equals the "no valid class" answer: a miss
    pred = np.full((N, len(PREDICT_SIZES)), -1, dtype=np.int32)
    for k, s in enumerate(PREDICT_SIZES):
        V = np.flatnonzero(PREDICT_CVALID[off[k]:off[k + 1]])
        if len(V):
            pred[:, k] = V[np.argmax(F[off[k] + V], axis=0)]                 # the first maximum
    return F, y, pred, ((pred == y) & (pred >= 0)).sum(0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def importance_inputs():
    """Hand-made tree arrays [3, 5, 127]: problem 0 splits on a few features up to 299 (never on ``unused``), problem 1
    never splits."""
    rs = np.random.RandomState(77)
    r, sizes, D = IMPORTANCE["rounds"], IMPORTANCE["sizes"], IMPORTANCE["D"]
    used = np.array([0, 3, 255, 256, 257, 299, 64, 63])
    tfeat = np.full((r, sum(sizes), NODES), -1, dtype=np.int32)
    tgain = np.zeros((r, sum(sizes), NODES))
    mask = rs.rand(r, sizes[0], NODES) < 0.4
    tfeat[:, :sizes[0]][mask] = used[rs.randint(len(used), size=int(mask.sum()))]
    tgain[:, :sizes[0]][mask] = np.exp(rs.randn(int(mask.sum())) * 3.0)
    assert not (tfeat == IMPORTANCE["unused"]).any() and (tfeat[:, sizes[0]:] == -1).all()
    return tfeat, tgain


@functools.lru_cache(maxsize=None)
def cuts_inputs(N, D):
    """(x fp32 [N, D], other rows [40, D] whose values include the cuts themselves, -0.0 and 0.0)."""
    rs = np.random.RandomState(3000 + N)
    x = rs.randn(N, D).astype(np.float32)
    x[:, 100] = np.float32(4.0)                                              # constant, in the second block of 64
    x[:, 70] = np.where(np.arange(N) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    x[:, 71] = np.where(np.arange(N) % 2 == 0, np.float32(-1.0), np.float32(0.0))    # the cut is +0.0 ...
    other = np.concatenate([x[rs.randint(N, size=20)], rs.randn(20, D).astype(np.float32) * 2.0])
    other[::2, 71] = np.float32(-0.0)                                        # ... and -0.0 lies on it: bin 1
    other[1::2, 70] = np.float32(-0.0)
    return x, other


@functools.lru_cache(maxsize=None)
def grad_inputs():
    """(F [258, 65], y [65, 2], cvalid): random margins, and rows whose margins differ by 40 (the two-class problem: the
    sum is 1 + e^-40 = 1, p is exactly 1 and h lies on its floor) and by 800 (e^-800 = 0: p exactly 0 and 1)."""
    rs = np.random.RandomState(88)
    N, sizes = GRAD_CASE["N"], GRAD_CASE["sizes"]
    F = rs.randn(sum(sizes), N) * 3.0
    y = np.stack([rs.randint(s, size=N) for s in sizes], 1).astype(np.int32)
    cvalid = lr_invalid(sizes)
    y[:3, 0] = sizes[0] // 2
    F[256, 10:20], F[257, 10:20] = 40.0, 0.0
    F[256, 20:30], F[257, 20:30] = -400.0, 400.0
    F[:256, 30:40] = 0.0
    F[y[30:40, 0], np.arange(30, 40)] = 800.0                                # the label's class dominates: g = 0 exactly
    F[:256, 40:50] = -5.0
    F[(y[40:50, 0] + 1) % 256, np.arange(40, 50)] = 795.0                    # another class dominates
    return F, y, cvalid
