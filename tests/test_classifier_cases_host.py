"""CPU-only proof that the tables of tests/classifier_cases.py reach what they claim: the mirrors of the planning rules
of csrc/logreg.hip and csrc/gbt.hip are pinned against literals worked out by hand from the source, every case is placed
on the kernel instance, grid trip, tail or branch it is there for, and every numpy restatement the device tests compare
against runs on every case in a few seconds."""
import time

import numpy as np

import classifier_cases as C
from test_gbt_host import NODES, ONE_Q, RUNS, load_fixture


# ---- the mirrors against literals --------------------------------------------------------------------------------------
def test_lr_mirrors_against_literals():
    assert C.lr_mt(377, 3) == 2 and C.lr_lds(2, 377, 3) == 98048 <= 98304
    assert C.lr_mt(379, 3) == 1 and C.lr_lds(2, 379, 3) == 98560
    assert C.lr_mt(251, 129) == 2 and C.lr_lds(2, 251, 129) == 98048
    assert C.lr_mt(257, 129) == 1
    assert C.lr_mt(512, 256) == 1 and C.lr_lds(1, 512, 256) == 99328 <= C.LR_LDS_LIMIT
    assert C.lr_mt(10, 40) == 2 and C.lr_mt(128, 3) == 2                  # what tests/test_hip_classify.py runs: two tiles only
    assert C.lr_blocks(32805, 3, 5, 2) == (1024, 1026)
    assert C.lr_blocks(16389, 379, 3, 1) == (1024, 1025)
    assert C.lr_blocks(1030, 128, 3, 2) == (33, 33)
    assert C.lr_blocks(1 << 20, 512, 4096, 1) == (15, 65536)              # the 256 MiB budget: 16416 KiB a partial
    assert C.proba_blocks(131107, 2) == (4096, 4098) and C.proba_blocks(1030, 2) == (33, 33)
    assert C.stat_slices(262144) == (1024, 256) and C.stat_slices(262145) == (513, 512) and C.stat_slices(262401) == (513, 512)
    assert C.stat_slices(300) == (2, 256) and C.stat_slices(1 << 30) == (1024, 1 << 20)
    assert C.auc_plan(300, 2) == (19, 16) and C.auc_plan(1100, 1) == (35, 32) and C.auc_plan(777, 7) == (49, 16)
    assert C.auc_plan(1 << 20, 16) == (1, 1 << 20)
    assert C.auc_lds(256) == 32832


def test_gbt_mirrors_against_literals():
    assert C.gbt_slot_bytes(8, 3, 256) == 128 << 10 and C.gbt_slot_bytes(128, 6, 256) == 16 << 20
    assert C.gbt_chunks(512 << 20, 128, 6, 256, 113) == [(0, 32), (32, 32), (64, 32), (96, 17)]
    assert C.gbt_chunks(11 * (128 << 10), 8, 3, 256, 11) == [(0, 11)]
    assert C.gbt_chunks(4 * (128 << 10) + 5, 8, 3, 256, 11) == [(0, 4), (4, 4), (8, 3)]
    assert [C.hist_tf(lv, 130, 256) for lv in range(6)] == [16, 8, 4, 2, 1, 1]
    assert C.hist_tf(0, 130, 16) == 32 and C.hist_tf(0, 3, 256) == 3 and C.hist_tf(2, 3, 64) == 3
    assert [C.split_scan_steps(n) for n in (1, 2, 65, 66, 129, 130, 256)] == [0, 1, 1, 2, 2, 3, 4]


# ---- softmax regression --------------------------------------------------------------------------------------------------
def test_lr_table_reaches_every_instance_trip_and_tail():
    ids = [c.id for c in C.LR_CASES]
    assert len(set(ids)) == len(ids)
    placed = {c.id: (C.lr_mt(c.D, max(c.sizes)),) + C.lr_blocks(c.N, c.D, sum(c.sizes), C.lr_mt(c.D, max(c.sizes)))
              for c in C.LR_CASES}
    for c in C.LR_CASES:                                                   # the id names the instance
        mt = placed[c.id][0]
        assert ("mt1" in c.id) <= (mt == 1) and ("mt2" in c.id) <= (mt == 2), c.id
        assert C.lr_lds(mt, c.D, max(c.sizes)) <= C.LR_LDS_LIMIT and 1 <= len(c.sizes) <= 16
    # both MT instances; every case runs valgrad (GRAD) and proba (!GRAD), so both GRAD values of each
    assert {placed[i][0] for i in ids} == {1, 2}
    assert C.lr_lds(2, 377, 3) == 98048 and placed["mt2-largest-lds"][0] == 2 and 70 % 32 == 6
    assert placed["mt1-smallest"] == (1, 5, 5) and placed["mt1-top-of-range"][0] == 1
    # it > 0 on each MT with a partial last tile
    for cid, mt, tiles, tail in (("mt2-second-trip", 2, 1026, 5), ("mt1-second-trip", 1, 1025, 5)):
        c = C.LR_BY_ID[cid]
        assert placed[cid] == (mt, 1024, tiles) and c.N - (tiles - 1) * 16 * mt == tail
        assert C.lr_grad_additions(c.N, c.D, c.sizes) == ((1089, 1043, 2) if mt == 2 else (1057, 1035, 2))
    # the largest workspace: 1024 partial gradients of mt1-second-trip, about 9 MB
    assert 1024 * 380 * 3 * 8 == 9338880
    # class counts: column tiles of 16, lane strides of 64
    S = {s for c in C.LR_CASES for s in c.sizes}
    assert {1, 2, 16, 17, 65, 129, 256} <= S and 130 in S and max(len(c.sizes) for c in C.LR_CASES) == 16
    assert C.cdiv(129, 16) == 9 and 129 - 8 * 16 == 1 and C.cdiv(256, 64) == 4
    # standardised and raw, dense and strided, on each instance
    combos = {(placed[c.id][0], c.std, bool(c.ld)) for c in C.LR_CASES}
    assert {(1, 0, True), (1, 1, True), (1, 1, False), (1, 0, False), (2, 1, False), (2, 0, False), (2, 1, True),
            (2, 0, True)} <= combos
    assert all(c.ld == 0 or c.ld > c.D for c in C.LR_CASES)
    # invalid classes wherever S >= 3, with rows labelled by them
    for c in C.LR_CASES:
        inp = C.lr_inputs(c.id)
        off = C.offsets(c.sizes)
        for k, s in enumerate(c.sizes):
            bad = np.flatnonzero(~inp["cvalid"][off[k]:off[k + 1]])
            assert (len(bad) == 1 and (inp["y"][:, k] == bad[0]).sum() >= 3) if s >= 3 else len(bad) == 0, (c.id, k)
    # the tie groups sit in different lane strides (c // 64) and lanes (c % 64); the winners are the smallest of each
    for grp in (C.TIE_GROUP_A, C.TIE_GROUP_B):
        assert len({g // 64 for g in grp}) == 3 and len({g % 64 for g in grp}) >= 2 and grp[0] != min(grp)
    assert C.TIE_INVALID == 130 // 2 and C.TIE_INVALID % 64 < min(C.TIE_GROUP_A) % 64   # the skipped class would win its lane
    pred = C.lr_reference("argmax-ties")[1]["pred"][:, 0]
    assert set(pred.tolist()) == {min(C.TIE_GROUP_A), min(C.TIE_GROUP_B)}
    # proba above its cap, colstats with doubled rows and a second column tile, the AUC tiles
    p = C.PROBA_CASE
    assert C.proba_blocks(p.N, C.lr_mt(p.D, max(p.sizes))) == (4096, 4098)
    assert C.stat_slices(C.COLSTATS_CASES[0][1]) == (513, 512) and C.COLSTATS_CASES[1][2] == 65
    assert max(C.AUC_CASES[0][2]) == 256 and C.auc_plan(300, 2) == (19, 16) and 300 - 18 * 16 == 12
    assert C.auc_plan(1100, 1) == (35, 32) and 1100 - 34 * 32 == 12       # two tiles a slice, the last slice one of 12 rows
    for cid, _, sizes in C.AUC_CASES:
        P, y, cvalid, _ = C.auc_inputs(cid)
        assert len(np.unique(P)) == 8 and not cvalid.all()
        assert ((y[:, 0] < 0) | (y[:, 0] >= sizes[0])).sum() >= 2


# ---- boosted trees -------------------------------------------------------------------------------------------------------
def test_gbt_tables_reach_every_level_chunk_and_branch():
    for name, nbins in C.GROW_NBINS.items():
        assert C.grow_inputs(name)["nbins"].tolist() == nbins
    assert sorted({C.split_scan_steps(n) for n in C.GROW_NBINS["six-features"]}) == [0, 1, 2, 4]
    assert [C.split_scan_steps(n) for n in C.GROW_NBINS["six-features"]] == [0, 1, 1, 2, 2, 4]
    # the chunks: c0 > 0, more than one class slot in a block row, the invalid class inside a chunk
    assert C.GROW_CHUNKS == ((0, 2), (2, 3), (5, 1)) and not C.GROW_CVALID[3] and 2 < 3 < 2 + 3
    assert sum(nc for _, nc in C.GROW_CHUNKS) == 6 and C.GROW_DEPTH == 6
    levels = C.grow_reference("six-features")
    last = levels[-1]
    for lv in range(6):                                                    # every level splits, beyond the first chunk too
        sl = slice((1 << lv) - 1, (2 << lv) - 1)
        assert (last["tfeat"][:2, sl] >= 0).any() and (last["tfeat"][2:, sl] >= 0).any(), lv
        assert [C.hist_tf(lv, 6, 256) for lv in range(6)] == [6, 6, 4, 2, 1, 1]
    assert set(last["tfeat"].ravel().tolist()) == {-1, 1, 2, 3, 4, 5}      # the constant feature never splits
    # the duplicate partition: feature 4's cut at bin 63 has the sums of feature 1's cut at bin 0; the smaller key wins
    tab = levels[0]["tabs"][C.LEAF_CLASS][0]
    assert np.array_equal(tab[1, :1].sum(0), tab[4, :64].sum(0))
    assert (last["tfeat"][C.LEAF_CLASS, 0], last["tbin"][C.LEAF_CLASS, 0]) == (1, 0)
    # a leaf known from level 1 on: admissible as a child (H >= 1), never splittable (H < 2); nothing below it
    H = int(last["nsum"][C.LEAF_CLASS, C.LEAF_NODE, 1])
    assert ONE_Q <= H < 2 * ONE_Q and last["tfeat"][C.LEAF_CLASS, C.LEAF_NODE] == -1
    below = [5, 6, 11, 12, 13, 14]
    for key in ("tfeat", "tbin", "tvalue", "tgain", "nsum"):
        init = -1 if key == "tfeat" else 0
        assert (last[key][C.LEAF_CLASS, below] == init).all() and (last[key][3] == init).all(), key
    assert all((lv["node"][C.LEAF_CLASS] == C.LEAF_NODE).sum() == 750 for lv in levels)
    assert all((lv["node"][3] == 0).all() for lv in levels)
    # leaves at other levels too: a node whose parent split and which does not, at every level from 1 to 5
    for lv in range(1, 6):
        nodes = np.arange((1 << lv) - 1, (2 << lv) - 1)
        exists = last["tfeat"][:, (nodes - 1) // 2] >= 0
        assert (exists & (last["tfeat"][:, nodes] < 0)).any() and (~exists[C.GROW_CVALID]).any() == (lv > 1), lv
    assert last["node"].max() <= NODES - 1 and last["node"].max() >= 63    # rows reach the deepest level
    small = C.grow_reference("one-feature-three-rows")[-1]
    assert (small["tfeat"][C.GROW_CVALID, 0] == 0).all() and (small["tfeat"][3] == -1).all()
    # class chunks of a round: 11 classes in 11, 6 and 3 chunks, the last one short
    g = load_fixture()
    csum, D = int(sum(g["sizes"])), g["x_train"].shape[1]
    assert (csum, D) == (11, 8)
    for run in RUNS:
        per = C.gbt_slot_bytes(D, run["max_depth"], run["max_bin"])
        counts = [len(C.gbt_chunks(s * per, D, run["max_depth"], run["max_bin"], csum)) for s in C.ROUND_SLOTS]
        assert counts == [11, 6, 3]
        assert C.gbt_chunks(2 * per, D, run["max_depth"], run["max_bin"], csum)[-1] == (10, 1)
        assert C.gbt_chunks(4 * per + 8, D, run["max_depth"], run["max_bin"], csum)[-1] == (8, 3)
    # the other stages
    assert C.PREDICT_ROWS == (1, 63, 64, 65, 257) and not C.PREDICT_CVALID[7:].any() and C.MARGIN_ROWS == (1, 257)
    for N in C.PREDICT_ROWS:
        F, y, pred, correct = C.predict_inputs(N)
        assert (pred[:, 2] == -1).all() and correct[2] == 0 and (y[:, 2] == -1).any() and y[0, 1] == 4
        top = F[:3].max(0)
        assert N < 63 or ((F[:3] == top).sum(0) > 1).any()                 # maxima that tie
    tfeat, tgain = C.importance_inputs()
    assert C.IMPORTANCE["D"] > 256 and tfeat.max() == 299 and tfeat.shape == (3, 5, NODES) and (tgain[tfeat < 0] == 0).all()
    assert all(D == 130 for _, D in C.CUTS_CASES) and [N for N, _ in C.CUTS_CASES] == [2, 257]
    F, y, cvalid = C.grad_inputs()
    assert F.shape == (258, 65) and not cvalid[128] and (y[:3, 0] == 128).all()


# ---- every restatement on every case, in a few seconds --------------------------------------------------------------------
def test_every_reference_runs_quickly():
    from test_classify_host import ref_colstats
    from test_gbt_host import ref_bin, ref_cuts, ref_grad, ref_importance
    t0 = time.perf_counter()
    for c in C.LR_CASES + [C.PROBA_CASE]:
        for ref in C.lr_reference(c.id):
            assert np.isfinite(ref["P"]).all() and np.isfinite(ref["f"]).all() and ref["bf"] > 0 and ref["bg"] > 0
            assert ref["g"] is None or not ref["g"][:, ~C.lr_inputs(c.id)["cvalid"]].any()
    for cid, _, _, _ in C.COLSTATS_CASES:
        _, x, (m, s) = C.colstats_inputs(cid)
        assert s[1] == 1.0 and m[1] == 1.25 and np.array_equal(ref_colstats(x)[0], m)
    for cid, _, _ in C.AUC_CASES:
        for c2, pos, neg in C.auc_inputs(cid)[3]:
            assert (c2 <= 2 * pos * neg).all() and c2.any()
    for name in C.GROW_SHAPES:
        assert len(C.grow_reference(name)) == 6
    for N in C.MARGIN_ROWS:
        walks = C.margin_inputs(N)[2]
        assert walks[6].shape == (6, N) and walks[2].max() <= 6
    assert (C.margin_inputs(257)[2][6] != C.margin_inputs(257)[2][2]).any()   # max_depth = 2 stops the walk early
    for N, D in C.CUTS_CASES:
        x, other = C.cuts_inputs(N, D)
        cuts, nbins = ref_cuts(x, 256)
        assert nbins[100] == 1 and nbins[70] == 1 and nbins[71] == 2 and nbins.max() <= min(N, 256)
        assert (ref_bin(other, cuts)[71, ::2] == 1).all() and (ref_bin(other, cuts)[70] == 0).all()
    F, y, cvalid = C.grad_inputs()
    g, h, gq, hq = ref_grad(F, y, list(C.GRAD_CASE["sizes"]), cvalid)
    floor = h == 1e-16
    assert floor[256:, 10:30].all() and (hq[floor] == 0).all() and floor[:256, 30:50][cvalid[:256]].sum() >= 2000
    assert (g[256:, 20:30] == np.where(y[20:30, 1] == np.array([[0], [1]]), -1.0, 0.0) + np.array([[0.0], [1.0]])).all()
    imp = ref_importance(*C.importance_inputs(), list(C.IMPORTANCE["sizes"]), C.IMPORTANCE["D"])
    assert abs(imp[0].sum() - 1.0) <= 1e-12 and imp[0, C.IMPORTANCE["unused"]] == 0 and not imp[1].any()
    took = time.perf_counter() - t0
    print("every reference on every case: %.2f s" % took)
    assert took < 30.0
