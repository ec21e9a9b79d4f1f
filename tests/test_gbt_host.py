"""CPU-only checks of the device-side DCI score: a plain-loop numpy fp64 restatement of the boosted-tree rule of
include/itcv_hip.h -- written here, shared with tests/test_hip_gbt.py -- and of the closed-form completeness /
disentanglement formulas, which are held to what was recorded from the unmodified reference (golden/dci.npz, part (a))
to 1e-12.  The restatement itself must rank the informative columns of the synthetic fixture (part (b)) first and be
reproducible, and the fixture must satisfy the stability condition under which a device run (whose ``exp`` may differ
from numpy's in the last bit) builds the SAME trees: no g * 2^24 or h * 2^24 within 1e-6 of a half-integer, and at every
split node the largest gain not bit-equal to the best below best * (1 - 1e-9).  The new entry points are declared, bound
and exported alike and refuse what lies outside their range before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("itcv_gbt_workspace", "itcv_gbt_cuts", "itcv_gbt_bin", "itcv_gbt_grad", "itcv_gbt_hist", "itcv_gbt_split",
       "itcv_gbt_advance", "itcv_gbt_margins", "itcv_gbt_predict", "itcv_gbt_importance", "itcv_gbt_round")
NODES = 127
Q = 2.0 ** 24
ONE_Q = 1 << 24
MIN_GAIN = 1e-6
RUNS = (dict(rounds=5, max_depth=3, max_bin=256), dict(rounds=3, max_depth=6, max_bin=32))   # the end-to-end cases


# ---- the rule, restated in numpy fp64 (include/itcv_hip.h) -----------------------------------------------------------
def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def ref_present(y, sizes):
    """cvalid[csum]: the class occurs in column k of y."""
    return np.concatenate([np.bincount(y[:, k][(y[:, k] >= 0) & (y[:, k] < s)], minlength=s) > 0
                           for k, s in enumerate(sizes)])


def ref_cuts(x_train, max_bin):
    """(list of D fp32 cut arrays, nbins[D]): candidates s[(j * N) // B], the distinct values above s[0]."""
    x_train = np.asarray(x_train, dtype=np.float32)
    N, D = x_train.shape
    cuts = []
    for d in range(D):
        s = np.sort(x_train[:, d])
        keep, last = [], s[0]
        for j in range(1, max_bin):
            v = s[(j * N) // max_bin]
            if v > s[0] and v != last:
                keep.append(v)
                last = v
        cuts.append(np.array(keep, dtype=np.float32))
    return cuts, np.array([len(c) + 1 for c in cuts], dtype=np.int32)


def ref_bin(x, cuts):
    """bins[D][N] uint8: bin(x) = #{cuts <= x}."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros((x.shape[1], x.shape[0]), dtype=np.uint8)
    for d, c in enumerate(cuts):
        out[d] = (c[None, :] <= x[:, d][:, None]).sum(1)
    return out


def ref_grad(F, y, sizes, cvalid):
    """(g, h, gq, hq), each [csum][N]: fp64 softmax over the valid classes (max-subtracted, the sum in class order),
    g = p - [y == c], h = max((2 p)(1 - p), 1e-16), quantised with llrint; 0 for invalid classes and invalid rows."""
    off = offsets(sizes)
    csum, N = F.shape
    g, h = np.zeros((csum, N)), np.zeros((csum, N))
    for k, s in enumerate(sizes):
        V = [c for c in range(s) if cvalid[off[k] + c]]
        if not V:
            continue
        Fv = F[off[k] + np.array(V)]
        m = Fv.max(0)
        e = np.exp(Fv - m)
        tot = np.zeros(N)
        for i in range(len(V)):
            tot = tot + e[i]
        lab = y[:, k]
        ok = (lab >= 0) & (lab < s)
        rowvalid = ok & cvalid[off[k] + np.where(ok, lab, 0)].astype(bool)
        for i, c in enumerate(V):
            p = e[i] / tot
            gi = p - (lab == c)
            hi = np.maximum((2.0 * p) * (1.0 - p), 1e-16)
            g[off[k] + c] = np.where(rowvalid, gi, 0.0)
            h[off[k] + c] = np.where(rowvalid, hi, 0.0)
    return g, h, np.rint(g * Q).astype(np.int64), np.rint(h * Q).astype(np.int64)


def ref_hist(bins, gq, hq, node, level, B):
    """tab[2^level][D][B][2] int64 of ONE class slot: integer sums over the rows whose node id lies in the level."""
    D, N = bins.shape
    nn, base = 1 << level, (1 << level) - 1
    tab = np.zeros((nn, D, B, 2), dtype=np.int64)
    nid = node.astype(np.int64) - base
    rows = np.nonzero((nid >= 0) & (nid < nn))[0]
    for d in range(D):
        np.add.at(tab[:, d, :, 0], (nid[rows], bins[d, rows]), gq[rows])
        np.add.at(tab[:, d, :, 1], (nid[rows], bins[d, rows]), hq[rows])
    return tab


def ref_score(Gq, Hq, lam):
    G, H = np.asarray(Gq).astype(np.float64) * (1.0 / Q), np.asarray(Hq).astype(np.float64) * (1.0 / Q)
    return (G * G) / (H + lam)


def ref_leaf(Gq, Hq, lam, eta):
    G, H = np.float64(Gq) * (1.0 / Q), np.float64(Hq) * (1.0 / Q)
    return ((-G) / (H + lam)) * eta


def ref_split(tab, nbins, GP, HP, lam):
    """Best split of one node from its table [D][B][2]: ``None`` (a leaf) or (feat, bin, gain, GLq, HLq, runner-up), the
    runner-up being the largest admissible gain that is not bit-equal to the best (-inf without one)."""
    D, B = tab.shape[:2]
    GL, HL = np.cumsum(tab[:, :, 0], axis=1), np.cumsum(tab[:, :, 1], axis=1)
    HR = HP - HL
    cand = np.arange(B)[None, :] <= (np.asarray(nbins)[:, None] - 2)
    ok = cand & (HL >= ONE_Q) & (HR >= ONE_Q)
    gain = 0.5 * ((ref_score(GL, HL, lam) + ref_score(GP - GL, HR, lam)) - ref_score(GP, HP, lam))
    gain = np.where(ok, gain, -np.inf)
    i = int(np.argmax(gain))                               # the first maximum in (d, b) order: the tie rule
    d, b = divmod(i, B)
    best = gain[d, b]
    if not (best > MIN_GAIN):
        return None
    rest = gain[gain != best]
    return d, b, float(best), int(GL[d, b]), int(HL[d, b]), float(rest.max()) if rest.size else -np.inf


def ref_walk(bins, tfeat, tbin, max_depth):
    """Leaf of every column of bins[D][N] in one tree."""
    N = bins.shape[1]
    nid = np.zeros(N, dtype=np.int64)
    for _ in range(max_depth):
        f = tfeat[nid]
        go = f >= 0
        right = bins[np.where(go, f, 0), np.arange(N)] > tbin[nid]
        nid = np.where(go, 2 * nid + 1 + right, nid)
    return nid


def ref_fit(x_train, y_train, x_test, y_test, sizes, rounds=100, max_depth=6, max_bin=256, eta=0.3, lam=1.0, cvalid=None):
    """The whole rule.  Returns a dict: cuts, nbins, bins, bins_test, tfeat / tbin / tvalue / tgain
    [rounds][csum][127], F / F_test [csum][N], pred / pred_test [N][K], correct / correct_test [K], importance [K][D],
    and the two stability figures ``half_gap`` (smallest distance of g * 2^24, h * 2^24 from a half-integer) and
    ``gain_gap`` (smallest (best - runner-up) / best over the split nodes)."""
    sizes = [int(s) for s in sizes]
    off, K = offsets(sizes), len(sizes)
    csum = int(off[-1])
    y_train, y_test = np.asarray(y_train).astype(np.int64), np.asarray(y_test).astype(np.int64)
    cvalid = ref_present(y_train, sizes) if cvalid is None else np.asarray(cvalid).astype(bool)
    cuts, nbins = ref_cuts(x_train, max_bin)
    bins, bins_t = ref_bin(x_train, cuts), ref_bin(x_test, cuts)
    D, N = bins.shape
    F, Ft = np.zeros((csum, N)), np.zeros((csum, bins_t.shape[1]))
    tfeat = np.full((rounds, csum, NODES), -1, dtype=np.int32)
    tbin = np.zeros((rounds, csum, NODES), dtype=np.int32)
    tvalue, tgain = np.zeros((rounds, csum, NODES)), np.zeros((rounds, csum, NODES))
    half_gap, gain_gap = np.inf, np.inf
    for r in range(rounds):
        g, h, gq, hq = ref_grad(F, y_train, sizes, cvalid)
        for v in (g, h):
            t = v[cvalid] * Q
            half_gap = min(half_gap, float(np.abs(t - np.floor(t) - 0.5).min()))
        for c in range(csum):
            if not cvalid[c]:
                continue
            node = np.zeros(N, dtype=np.int64)
            sums = {0: (int(gq[c].sum()), int(hq[c].sum()))}
            tvalue[r, c, 0] = ref_leaf(*sums[0], lam, eta)
            for level in range(max_depth):
                for nid in range((1 << level) - 1, (2 << level) - 1):
                    if nid not in sums:
                        continue
                    rows = np.nonzero(node == nid)[0]
                    tab = np.zeros((D * max_bin, 2), dtype=np.int64)
                    flat = (np.arange(D)[:, None] * max_bin + bins[:, rows]).ravel()
                    np.add.at(tab[:, 0], flat, np.tile(gq[c, rows], D))
                    np.add.at(tab[:, 1], flat, np.tile(hq[c, rows], D))
                    GP, HP = sums[nid]
                    got = ref_split(tab.reshape(D, max_bin, 2), nbins, GP, HP, lam)
                    if got is None:
                        continue
                    d, b, gain, GL, HL, second = got
                    gain_gap = min(gain_gap, (gain - second) / gain)
                    tfeat[r, c, nid], tbin[r, c, nid], tgain[r, c, nid] = d, b, gain
                    sums[2 * nid + 1], sums[2 * nid + 2] = (GL, HL), (GP - GL, HP - HL)
                    tvalue[r, c, 2 * nid + 1] = ref_leaf(GL, HL, lam, eta)
                    tvalue[r, c, 2 * nid + 2] = ref_leaf(GP - GL, HP - HL, lam, eta)
                    node[rows] = 2 * nid + 1 + (bins[d, rows] > b)
            F[c] += tvalue[r, c][node]
            Ft[c] += tvalue[r, c][ref_walk(bins_t, tfeat[r, c], tbin[r, c], max_depth)]
    out = dict(cuts=cuts, nbins=nbins, bins=bins, bins_test=bins_t, tfeat=tfeat, tbin=tbin, tvalue=tvalue, tgain=tgain,
               F=F, F_test=Ft, cvalid=cvalid, half_gap=half_gap, gain_gap=gain_gap)
    for tag, M, y in (("", F, y_train), ("_test", Ft, y_test)):
        pred = np.full((M.shape[1], K), -1, dtype=np.int32)
        for k, s in enumerate(sizes):
            V = np.array([c for c in range(s) if cvalid[off[k] + c]], dtype=int)
            if len(V):
                pred[:, k] = V[np.argmax(M[off[k] + V], axis=0)]      # the first maximum
        out["pred" + tag] = pred
        out["correct" + tag] = (pred == y).sum(0).astype(np.int64)
    out["importance"] = ref_importance(tfeat, tgain, sizes, D)
    return out


def ref_importance(tfeat, tgain, sizes, D):
    """imp[K][D]: total gain / number of splits per feature, summed in the order round, class, node, then normalised."""
    off = offsets(sizes)
    imp = np.zeros((len(sizes), D))
    for k in range(len(sizes)):
        tot, cnt = np.zeros(D), np.zeros(D, dtype=np.int64)
        f, gn = tfeat[:, off[k]:off[k + 1]].ravel(), tgain[:, off[k]:off[k + 1]].ravel()
        for i in np.nonzero(f >= 0)[0]:
            tot[f[i]] += gn[i]
            cnt[f[i]] += 1
        raw = np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)
        s = 0.0
        for d in range(D):
            s += raw[d]
        imp[k] = raw / s if s > 0 else 0.0
    return imp


def ref_entropy(x, base, axis=0, eps=1e-9):
    """ops.entropy (ops.py:125-133)."""
    p = (x + eps) / np.sum(x + eps, axis=axis, keepdims=True)
    return -np.sum(p * np.log(p + eps), axis=axis) / np.log(base + eps)


def ref_disentanglement(P):
    """evaluation/utils.py:220-229 on P[K][D] as fit_info_clf returns it."""
    Dd = 1.0 - ref_entropy(P, P.shape[0])
    if np.sum(P) == 0:
        P = np.ones_like(P)
    return float(np.sum(np.sum(P, axis=0) / P.sum() * Dd))


def ref_completeness(P):
    """evaluation/utils.py:232-241."""
    C = 1.0 - ref_entropy(P.T, P.shape[1])
    if np.sum(P) == 0:
        P = np.ones_like(P)
    return float(np.sum(np.sum(P, axis=1) / P.sum() * C))


def ref_dci(fit, n_test):
    """(informativeness, completeness, disentanglement) of a ``ref_fit`` result."""
    return (float(np.mean(fit["correct_test"] / n_test)), ref_completeness(fit["importance"]),
            ref_disentanglement(fit["importance"]))


def load_fixture():
    g = np.load(os.path.join(GOLDEN, "dci.npz"))
    return {k: g[k] for k in g.files}


_FITS = {}


def fixture_fit(i):
    """``ref_fit`` of fixture (b) under RUNS[i], computed once per process and shared (never modified)."""
    if i not in _FITS:
        g = load_fixture()
        _FITS[i] = ref_fit(g["x_train"], g["y_train"], g["x_test"], g["y_test"], g["sizes"], **RUNS[i])
    return _FITS[i]


# ---- the closed-form half against the reference ------------------------------------------------------------------------
def test_formulas_reproduce_the_reference():
    g = load_fixture()
    n = int(g["n_matrices"])
    assert n >= 5
    kinds = set()
    for i in range(n):
        P = g[f"P{i}"]
        assert abs(ref_completeness(P) - float(g["completeness"][i])) <= 1e-12
        assert abs(ref_disentanglement(P) - float(g["disentanglement"][i])) <= 1e-12
        kinds |= {"zero"} if not P.any() else set()
        kinds |= {"onehot"} if ((P == 0) | (P == 1)).all() and (P.sum(1) == 1).all() else set()
        kinds |= {"zero_row"} if P.any() and not P.all(1).all() and (P.sum(1) == 0).any() else set()
    assert kinds == {"zero", "onehot", "zero_row"}


# ---- conditions on the restatement and on the fixture -------------------------------------------------------------------
def test_fixture_shape():
    g = load_fixture()
    sizes = [int(s) for s in g["sizes"]]
    assert sizes == [2, 5, 4] and g["x_train"].dtype == np.float32 and g["x_train"].shape[1] == g["x_test"].shape[1]
    cv = ref_present(g["y_train"], sizes)
    assert cv.sum() == sum(sizes) - 1 and not cv[-1]                       # the last class never occurs in training
    assert (g["y_test"][:, 2] == 3).any()                                   # ... but does in the test labels


@pytest.mark.parametrize("i", range(len(RUNS)))
def test_fixture_is_stable_and_informative_columns_rank_first(i):
    g, fit = load_fixture(), fixture_fit(i)
    print("half_gap", fit["half_gap"], "gain_gap", fit["gain_gap"])
    assert fit["half_gap"] > 1e-6
    assert fit["gain_gap"] > 1e-9                                           # runner-up < best * (1 - 1e-9) at every split
    imp, D = fit["importance"], g["x_train"].shape[1]
    for k, cols in enumerate(g["informative"]):
        cols = [int(c) for c in cols if c >= 0]
        rest = [d for d in range(D) if d not in cols]
        assert imp[k, cols].min() > imp[k, rest].max(), (k, imp[k])
        assert abs(imp[k].sum() - 1.0) <= 1e-12
    n = g["x_train"].shape[0]
    assert (fit["correct"] / n > 0.6).all() and (fit["tfeat"] >= 0).any()
    dci = ref_dci(fit, g["x_test"].shape[0])
    assert all(0.0 <= v <= 1.0 for v in dci)


def test_restatement_is_reproducible():
    g = load_fixture()
    a = fixture_fit(0)
    b = ref_fit(g["x_train"], g["y_train"], g["x_test"], g["y_test"], g["sizes"], **RUNS[0])
    for key in ("tfeat", "tbin", "tvalue", "tgain", "F", "F_test", "importance", "pred", "pred_test", "bins"):
        assert np.array_equal(a[key], b[key]), key


def test_pieces_of_the_restatement():
    cuts, nbins = ref_cuts(np.array([[1.0], [1.0], [2.0], [3.0], [3.0], [3.0], [5.0], [9.0]], dtype=np.float32), 4)
    assert np.array_equal(cuts[0], [2.0, 3.0, 5.0]) and nbins[0] == 4     # s[2], s[4], s[6]
    cuts, nbins = ref_cuts(np.full((10, 1), 7.0, dtype=np.float32), 256)
    assert len(cuts[0]) == 0 and nbins[0] == 1                             # a constant column has one bin
    assert np.array_equal(ref_bin(np.array([[0.5], [2.0], [2.5], [100.0]]), [np.array([2.0, 3.0], dtype=np.float32)])[0],
                          [0, 1, 1, 2])
    # an empty bin between two occupied ones: equal prefix sums, bit-equal gains, the lower bin wins
    tab = np.zeros((1, 4, 2), dtype=np.int64)
    tab[0, 0], tab[0, 2] = (-3 * ONE_Q, 2 * ONE_Q), (3 * ONE_Q, 2 * ONE_Q)
    assert ref_split(tab, [4], 0, 4 * ONE_Q, 1.0)[:2] == (0, 0)
    # min_child_weight: a left child below 1 is not admissible
    tab[0, 0] = (-3 * ONE_Q, ONE_Q - 1)
    assert ref_split(tab, [4], 0, 3 * ONE_Q - 1, 1.0) is None
    z = np.zeros((3, 4))
    assert ref_completeness(z) == ref_completeness(np.ones((3, 4))) and abs(ref_completeness(z)) <= 1e-6


# ---- boundary ------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library():
    from hipvae import abi
    header = open(os.path.join(ROOT, "include", "itcv_hip.h")).read()
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in abi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert abi.ABI_VERSION == 4 == lib.itcv_abi_version()
    assert re.search(r"#define ITCV_GBT_TREE_NODES %d\b" % NODES, header)


A = [0x10000 * i for i in range(1, 24)]     # fake device addresses: every call fails before a launch


def _round(N=100, D=8, max_bin=256, sizes=(3, 4), K=None, max_depth=6):
    from hipvae import abi
    K = len(sizes) if K is None else K
    cs = (ctypes.c_int * max(len(sizes), 1))(*sizes)
    return abi.lib.itcv_gbt_round(A[0], N, D, max_bin, A[1], A[2], K, cs, A[3], A[4], A[5], 10, A[6], max_depth, 1.0, 0.3,
                                  A[7], A[8], A[9], A[10], A[11], 1 << 30, A[12], A[13], A[14], A[15], A[16], None)


@pytest.mark.parametrize("kw, msg", [
    (dict(D=513), "D = 513"), (dict(max_depth=7), "max_depth = 7"), (dict(sizes=(3, 257)), "csize 257"),
    (dict(sizes=(2,) * 17), "K = 17"), (dict(N=1), "N = 1"), (dict(max_bin=257), "max_bin = 257"),
    (dict(max_bin=1), "max_bin = 1"), (dict(D=0), "D = 0"), (dict(max_depth=0), "max_depth = 0"),
    (dict(sizes=(0, 3)), "csize 0")])
def test_range_checks_fail_before_any_launch(kw, msg):
    from hipvae import abi
    assert _round(**kw) != 0
    assert abi.last_error().startswith("itcv_gbt_round") and msg in abi.last_error(), abi.last_error()


def test_argument_checks_and_the_table_budget():
    from hipvae import abi
    lib = abi.lib
    cs = (ctypes.c_int * 2)(3, 4)
    assert lib.itcv_gbt_cuts(A[0], 1, 8, 256, A[1], A[2], None) != 0 and "N = 1" in abi.last_error()
    assert lib.itcv_gbt_bin(A[0], 4, 10, 8, 256, A[1], A[2], A[3], A[4], None) != 0        # row stride below D
    assert lib.itcv_gbt_bin(A[0], 513, 10, 513, 256, A[1], A[2], A[3], A[4], None) != 0 and "D = 513" in abi.last_error()
    assert lib.itcv_gbt_hist(A[0], 10, 8, 256, A[1], A[2], A[3], A[4], 0, 1, 6, A[5], 1 << 30, None) != 0
    assert "level = 6" in abi.last_error()
    assert lib.itcv_gbt_hist(A[0], 10, 8, 256, A[1], A[2], A[3], A[4], 0, 1, 5, A[5], 1024, None) != 0   # table too small
    assert "table" in abi.last_error()
    assert lib.itcv_gbt_grad(A[0], A[1], 10, 17, cs, A[2], A[3], A[4], None, None, A[5], None) != 0
    assert lib.itcv_gbt_predict(A[0], A[1], 10, 0, cs, A[2], A[3], A[4], A[5], None) != 0
    assert lib.itcv_gbt_importance(A[0], A[1], 0, 2, cs, 8, A[2], None) != 0 and "rounds = 0" in abi.last_error()
    assert lib.itcv_gbt_margins(A[0], 10, 7, A[1], None, A[2], A[3], A[4], 7, A[5], None) != 0
    per = 32 * 128 * 256 * 16                                                          # one class slot at depth 6
    assert lib.itcv_gbt_workspace(10000, 128, 5, 113, 6, 256) == (512 << 20) // per * per   # 32 slots: the 512 MiB budget
    assert lib.itcv_gbt_workspace(600, 8, 3, 11, 3, 256) == 11 * 4 * 8 * 256 * 16           # everything fits
    assert lib.itcv_gbt_workspace(2, 512, 1, 1, 6, 256) == 32 * 512 * 256 * 16
    assert lib.itcv_gbt_workspace(1, 8, 3, 11, 3, 256) == 0 and lib.itcv_gbt_workspace(600, 8, 3, 11, 7, 256) == 0
    import torch
    from hipvae import gbt
    with pytest.raises(abi.HipExtensionError):                                         # no CPU path
        gbt.fit_boosted_trees(torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int32), torch.zeros(4, 3),
                              torch.zeros(4, 1, dtype=torch.int32), [2], rounds=1)
