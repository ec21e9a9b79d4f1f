"""GPU tests of the softmax-regression kernels (csrc/logreg.hip) and the boosted-tree kernels (csrc/gbt.hip) on every
path the tables of tests/classifier_cases.py reach (test_classifier_cases_host.py proves on the CPU which): both tile
heights of lr_softmax_kernel with and without the gradient, the second grid trip, up to 256 classes, the AUC kernel's
largest tile; gbt_split_kernel at every level inside class chunks, gbt_advance / gbt_margins / gbt_predict /
gbt_importance on their own, and itcv_gbt_round with more than one class chunk.  The references are the numpy fp64
restatements of test_classify_host.py and test_gbt_host.py.

In the library's names: the mt1-* cases launch lr_softmax_kernel<1, true> (valgrad) and lr_softmax_kernel<1, false>
(proba); the *-second-trip cases take the ``it > 0`` branch; test_grow_a_tree_stage_by_stage calls itcv_gbt_split at
levels 1..5 with c0 > 0 and itcv_gbt_advance on its own; test_margins_by_node_id_and_by_walking calls itcv_gbt_margins
on its own; test_round_in_class_chunks_equals_the_whole_table runs itcv_gbt_round with 11, 6 and 3 chunks.

Bounds.  Integers (predictions, pair counts, bins, node ids, tables, split feature / bin, node sums, accuracy counts)
and leaf values are compared EXACTLY; margins after one leaf value was added are one correctly rounded fp64 addition:
exact.  Gains: 1e-15 relative, as in tests/test_hip_gbt.py.  Importances: exact, both sides being correctly rounded
fp64 sums in the order round, class, node.  Gradients of the trees: g, h within 1e-14, gq, hq within one unit.  Value,
gradient and probabilities of the softmax regression: the bounds derived in the docstring of classifier_cases.py
(``lr_bounds``), which include the counted additions of the two second-trip cases.  Nothing is taken from what the
kernels give; every test prints worst error / allowance.

Measured on the MI355X, worst error / allowance over both thetas (value; gradient; probabilities):
  mt2-largest-lds        1.8e-15 / 4.6e-11;  5.6e-16 / 1.9e-10;  5.3e-15 / 4.6e-11
  mt1-smallest           1.8e-15 / 7.7e-11;  5.0e-16 / 5.2e-10;  3.3e-15 / 7.7e-11
  mt1-wide-classes       2.8e-14 / 3.3e-11;  4.6e-16 / 8.4e-11;  3.8e-15 / 2.4e-11
  mt2-wide-classes       8.9e-16 / 1.1e-12;  1.1e-16 / 2.7e-10;  2.2e-16 / 4.0e-11
  mt1-top-of-range       2.3e-13 / 4.8e-10;  2.0e-15 / 3.0e-10;  1.1e-14 / 8.9e-11
  mt2-second-trip        1.4e-14 / 8.3e-13;  1.0e-15 / 3.7e-12;  2.2e-16 / 6.1e-13     (the largest ratio: 0.017, theta = 0)
  mt1-second-trip        7.1e-15 / 1.9e-10;  8.9e-16 / 6.8e-10;  2.2e-16 / 8.3e-11
  k16-single-class       4.4e-16 / 1.4e-12;  3.3e-16 / 6.8e-12;  2.2e-16 / 1.4e-12
  argmax-ties            3.6e-15 / 4.6e-12;  1.1e-16 / 2.8e-11;  1.1e-16 / 4.6e-12
  column-tiles-16-17-65  8.9e-16 / 4.7e-13;  5.6e-17 / 1.7e-12;  2.2e-16 / 6.7e-13
  proba-above-block-cap  probabilities 2.2e-16 / 5.1e-13
  column statistics      mean 0, scale 4.0e-15 (doubled rows) and 6.3e-16 (D = 65), of 1e-13
  tree gains             0 of 1e-15 relative at all 67 + 7 splits; importances: equal bits
  tree gradients         g, h 1.1e-16 of 1e-14; gq, hq 0 of 1 unit
Everything compared exactly was equal.  With ``*q + acc[i]`` replaced by ``acc[i]`` in a scratch build the gradient of
the two second-trip cases is off by 3e-4 and 8e-4; with the butterfly's tie rule or gbt_predict's ``v > m`` reversed, or
the split kernel's parent lookup made chunk-relative, the tie, predict and grow tests fail.
"""
import numpy as np
import pytest
import torch

import classifier_cases as C
from test_classify_host import offsets
from test_gbt_host import NODES, RUNS, fixture_fit, load_fixture, ref_bin, ref_cuts, ref_grad, ref_importance

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def G(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev())


def flags():
    from hipvae import functional as HF
    return HF.disent_flags(dev())


def strided(wide, D):
    """The device view wide[:, :D] with wide's row stride."""
    xd = G(wide)[:, :D]
    assert xd.stride() == (wide.shape[1], 1)
    return xd


# ---- softmax regression ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.LR_CASES])
def test_value_gradient_probabilities(cid):
    from hipvae import functional as HF
    inp, refs = C.lr_inputs(cid), C.lr_reference(cid)
    c, cvalid = inp["case"], inp["cvalid"]
    f = flags()
    stats = None if inp["stats"] is None else tuple(G(s) for s in inp["stats"])
    prob = HF.LogregProblem(strided(inp["wide"], c.D), G(inp["y"]), list(c.sizes), G(cvalid.astype(np.int32)), f, stats=stats)
    for theta, ref in zip(inp["thetas"], refs):
        fv, g = prob.valgrad(G(theta))
        f2, g2 = prob.valgrad(G(theta))
        assert torch.equal(fv, f2) and torch.equal(g, g2)                   # bitwise
        g = g.cpu().numpy()
        ef, eg = np.abs(fv.cpu().numpy() - ref["f"]).max(), np.abs(g - ref["g"]).max()
        P, pred = prob.proba(G(theta))
        ep = np.abs(P.cpu().numpy() - ref["P"]).max()
        print(cid, "A %.1f" % ref["A"], "f %.3g / %.3g = %.3f" % (ef, ref["bf"], ef / ref["bf"]),
              "grad %.3g / %.3g = %.3f" % (eg, ref["bg"], eg / ref["bg"]), "P %.3g / %.3g = %.3f" % (ep, ref["bp"], ep / ref["bp"]))
        assert ef <= ref["bf"] and eg <= ref["bg"] and ep <= ref["bp"]
        assert not g[:, ~cvalid].any()                                      # exactly 0 at invalid classes
        assert not P.cpu().numpy()[:, ~cvalid].any()
        assert np.array_equal(pred.cpu().numpy(), ref["pred"])
        off = offsets(c.sizes)
        for k, s in enumerate(c.sizes):                                     # rows of an invalid class: no probabilities at all
            if s >= 3:
                assert not P[:3, off[k]:off[k + 1]].any()
    assert f.tolist() == [0, 0]


def test_proba_above_its_block_cap():
    from hipvae import functional as HF
    cid = C.PROBA_CASE.id
    inp, refs = C.lr_inputs(cid), C.lr_reference(cid)
    c = inp["case"]
    f = flags()
    prob = HF.LogregProblem(G(inp["x"]), G(inp["y"]), list(c.sizes), G(inp["cvalid"].astype(np.int32)), f,
                            stats=tuple(G(s) for s in inp["stats"]))
    for theta, ref in zip(inp["thetas"], refs):
        P, pred = prob.proba(G(theta))
        ep = np.abs(P.cpu().numpy() - ref["P"]).max()
        print(cid, "P %.3g / %.3g = %.3f" % (ep, ref["bp"], ep / ref["bp"]))
        assert ep <= ref["bp"] and np.array_equal(pred.cpu().numpy(), ref["pred"])
    assert f.tolist() == [0, 0]


@pytest.mark.parametrize("cid", [c[0] for c in C.COLSTATS_CASES])
def test_column_statistics(cid):
    from hipvae import functional as HF
    wide, x, (m, s) = C.colstats_inputs(cid)
    xd, f = strided(wide, x.shape[1]), flags()
    mean, scale = HF.logreg_colstats(xd, f)
    em = (np.abs(mean.cpu().numpy() - m) / np.abs(x).max(0)).max()
    es = (np.abs(scale.cpu().numpy() - s) / s).max()
    print(cid, "mean %.3g / 1e-13" % em, "scale %.3g / 1e-13" % es)
    assert em <= 1e-13 and es <= 1e-13 and f.tolist() == [0, 0]
    assert scale[1].item() == 1.0 and mean[1].item() == 1.25               # the constant column
    m2, s2 = HF.logreg_colstats(xd, f)
    assert torch.equal(mean, m2) and torch.equal(scale, s2)


@pytest.mark.parametrize("cid", [c[0] for c in C.AUC_CASES])
def test_pair_counts_exact(cid):
    from hipvae import functional as HF
    sizes = next(c[2] for c in C.AUC_CASES if c[0] == cid)
    P, y, cvalid, want = C.auc_inputs(cid)
    f = flags()
    c2, pos, neg = HF.logreg_auc(G(P), G(y), list(sizes), G(cvalid.astype(np.int32)), f)
    c2b = HF.logreg_auc(G(P), G(y), list(sizes), G(cvalid.astype(np.int32)), f)[0]
    assert torch.equal(c2, c2b) and f.tolist() == [0, 1]                    # labels out of range: the flag, counts exact
    off = offsets(sizes)
    for k in range(len(sizes)):
        sl = slice(off[k], off[k + 1])
        r2, rp, rn = want[k]
        assert c2[sl].tolist() == r2.tolist() and pos[sl].tolist() == rp.tolist() and neg[sl].tolist() == rn.tolist()
        assert not c2[sl].cpu().numpy()[~cvalid[sl]].any() and not pos[sl].cpu().numpy()[~cvalid[sl]].any()


# ---- boosted trees: one tree, a stage at a time ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.GROW_SHAPES))
def test_grow_a_tree_stage_by_stage(name):
    """hist -> split per class chunk, then advance, for each level; after every call everything is compared."""
    from hipvae import functional as HF
    inp, levels = C.grow_inputs(name), C.grow_reference(name)
    N, D = C.GROW_SHAPES[name]
    f = flags()
    cuts, nbins = HF.gbt_cuts(G(inp["x"]), C.GROW_B)
    bins = HF.gbt_bin(G(inp["x"]), cuts, nbins, C.GROW_B, f)
    assert np.array_equal(nbins.cpu().numpy(), inp["nbins"]) and np.array_equal(bins.cpu().numpy(), inp["bins"])
    gq, hq, cvalid = G(inp["gq"]), G(inp["hq"]), G(C.GROW_CVALID.astype(np.int32))
    trees = tuple(t[0] for t in HF.gbt_tree_arrays(1, 6, dev()))
    nsum = torch.zeros((6, NODES, 2), dtype=torch.int64, device=dev())
    node = torch.zeros((6, N), dtype=torch.uint8, device=dev())
    worst = 0.0
    for level, want in enumerate(levels):
        prev = levels[level - 1] if level else None
        for c0, nc in C.GROW_CHUNKS:
            tab = HF.gbt_hist(bins, gq, hq, node, cvalid, level, C.GROW_B, c0=c0, nc=nc)
            assert tab.shape == (nc, 1 << level, D, C.GROW_B, 2)
            for j in range(nc):
                if C.GROW_CVALID[c0 + j]:
                    assert np.array_equal(tab[j].cpu().numpy(), want["tabs"][c0 + j]), (level, c0 + j)
                else:
                    assert not tab[j].any()
            HF.gbt_split(tab, nbins, cvalid, level, trees, nsum, lam=C.GROW_LAM, eta=C.GROW_ETA, c0=c0)
            done = slice(0, c0 + nc)                                        # these classes hold the level, the others the last
            for key, got in zip(("tfeat", "tbin", "tvalue", "nsum"), (trees[0], trees[1], trees[2], nsum)):
                got = got.cpu().numpy()
                assert np.array_equal(got[done], want[key][done]), (level, c0, key)
                if prev is not None:
                    assert np.array_equal(got[c0 + nc:], prev[key][c0 + nc:]), (level, c0, key)
            tg = trees[3].cpu().numpy()[done]
            err = np.abs(tg - want["tgain"][done])
            assert (err <= 1e-15 * np.abs(want["tgain"][done])).all(), (level, c0)
            worst = max(worst, float((err / np.maximum(np.abs(want["tgain"][done]), 1e-300)).max()))
        HF.gbt_advance(bins, cvalid, trees[0], trees[1], level, node)
        assert np.array_equal(node.cpu().numpy(), want["node"]), level
    last = levels[-1]
    print(name, "splits", int((last["tfeat"] >= 0).sum()), "worst gain error %.3g / 1e-15" % worst)
    tfeat = trees[0].cpu().numpy()
    assert (tfeat[3] == -1).all() and not nsum[3].any() and not trees[2][3].any() and not node[3].any()   # as initialised
    if name == "six-features":
        below = [5, 6, 11, 12, 13, 14]                                      # under the leaf: nothing written anywhere
        assert (tfeat[C.LEAF_CLASS, below] == -1).all() and not nsum[C.LEAF_CLASS, below].any()
        assert not any(t[C.LEAF_CLASS, below].any() for t in trees[1:])
        assert int((node[C.LEAF_CLASS] == C.LEAF_NODE).sum()) == 750       # its rows stopped at level 1
    assert f.tolist() == [0, 0]


def test_margins_by_node_id_and_by_walking():
    from hipvae import functional as HF
    bins, node, tr = C.grown_tree()
    tfeat, tbin, tvalue, tgain = tr
    trees = (G(tfeat), G(tbin), G(tvalue), G(tgain))
    cvalid = G(C.GROW_CVALID.astype(np.int32))
    rs = np.random.RandomState(5)
    for N in (bins.shape[1],) + C.MARGIN_ROWS:                              # training rows: both forms, bit for bit
        b, nd, F0 = bins[:, :N], node[:, :N], rs.randn(6, N)
        by_id = HF.gbt_margins(G(b), cvalid, G(nd), trees, 6, G(F0))
        walked = HF.gbt_margins(G(b), cvalid, None, trees, 6, G(F0))
        want = F0 + np.where(C.GROW_CVALID[:, None], np.take_along_axis(tvalue, nd.astype(np.int64), 1), 0.0)
        assert torch.equal(by_id, walked) and np.array_equal(by_id.cpu().numpy(), want), N
        assert np.array_equal(by_id[3].cpu().numpy(), F0[3])               # the invalid class is untouched
    for N in C.MARGIN_ROWS:                                                 # other rows: the walk, also cut short
        b, F0, walks = C.margin_inputs(N)
        for md in (6, 2):
            got = HF.gbt_margins(G(b), cvalid, None, trees, md, G(F0)).cpu().numpy()
            want = F0 + np.where(C.GROW_CVALID[:, None], np.take_along_axis(tvalue, walks[md], 1), 0.0)
            assert np.array_equal(got, want), (N, md)
    assert (C.margin_inputs(257)[2][6] != C.margin_inputs(257)[2][2]).any()


@pytest.mark.parametrize("N", C.PREDICT_ROWS)
def test_predict_ties_no_valid_class_and_labels_out_of_range(N):
    from hipvae import functional as HF
    F, y, want, correct = C.predict_inputs(N)
    f = flags()
    pred, cnt = HF.gbt_predict(G(F), G(y), list(C.PREDICT_SIZES), G(C.PREDICT_CVALID.astype(np.int32)), f)
    assert np.array_equal(pred.cpu().numpy(), want) and cnt.tolist() == correct.tolist()
    assert (pred[:, 2] == -1).all() and cnt[2].item() == 0 and f.tolist() == [0, 1]
    y2, f2 = np.clip(y, 0, None), flags()                                   # the same without them: no flag
    y2[0, 1] = 0
    pred2, cnt2 = HF.gbt_predict(G(F), G(y2), list(C.PREDICT_SIZES), G(C.PREDICT_CVALID.astype(np.int32)), f2)
    assert torch.equal(pred2, pred) and cnt2.tolist() == ((want == y2) & (want >= 0)).sum(0).tolist() and f2.tolist() == [0, 0]


def test_importance_exact():
    from hipvae import functional as HF
    tfeat, tgain = C.importance_inputs()
    sizes, D = list(C.IMPORTANCE["sizes"]), C.IMPORTANCE["D"]
    want = ref_importance(tfeat, tgain, sizes, D)
    got = HF.gbt_importance(G(tfeat), G(tgain), sizes, D).cpu().numpy()
    print("importance: max |got - ref|", np.abs(got - want).max(), "(exact required)")
    assert np.array_equal(got, want)
    assert got[0, C.IMPORTANCE["unused"]] == 0.0 and not got[1].any() and got[0, 299] > 0 and got[0, 257] > 0


@pytest.mark.parametrize("N, D", C.CUTS_CASES)
def test_cuts_and_bins_second_block(N, D):
    from hipvae import functional as HF
    x, other = C.cuts_inputs(N, D)
    cuts, nbins = ref_cuts(x, 256)
    f = flags()
    dc, dn = HF.gbt_cuts(G(x), 256)
    assert np.array_equal(dn.cpu().numpy(), nbins) and nbins[100] == 1 and nbins[70] == 1 and nbins[71] == 2
    for d in range(D):
        assert np.array_equal(dc[d, :nbins[d] - 1].cpu().numpy(), cuts[d]), d
    assert np.array_equal(HF.gbt_bin(G(x), dc, dn, 256, f).cpu().numpy(), ref_bin(x, cuts))
    got = HF.gbt_bin(G(other), dc, dn, 256, f).cpu().numpy()
    assert np.array_equal(got, ref_bin(other, cuts)) and (got[71, ::2] == 1).all() and f.tolist() == [0, 0]


def test_gradients_saturated():
    from hipvae import functional as HF
    F, y, cvalid = C.grad_inputs()
    sizes = list(C.GRAD_CASE["sizes"])
    g, h, gq, hq = ref_grad(F, y, sizes, cvalid)
    f = flags()
    dgq, dhq, dg, dh = (t.cpu().numpy() for t in HF.gbt_grad(G(F), G(y), sizes, G(cvalid.astype(np.int32)), f, with_fp64=True))
    eg, eh = np.abs(dg - g).max(), np.abs(dh - h).max()
    print("g %.3g / 1e-14" % eg, "h %.3g / 1e-14" % eh, "gq", np.abs(dgq - gq).max(), "/ 1", "hq", np.abs(dhq - hq).max(), "/ 1")
    assert eg <= 1e-14 and eh <= 1e-14 and np.abs(dgq - gq).max() <= 1 and np.abs(dhq - hq).max() <= 1
    floor = h == 1e-16
    assert floor.sum() >= 2000 and (dh[floor] == 1e-16).all() and (dhq[floor] == 0).all()
    assert (dg[256:, 20:30] == g[256:, 20:30]).all() and set(np.unique(dg[256:, 20:30])) <= {-1.0, 0.0, 1.0}
    assert not dgq[128].any() and not dhq[128].any() and not dgq[:256, :3].any() and f.tolist() == [0, 0]


# ---- class chunks of a round ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(RUNS)))
def test_round_in_class_chunks_equals_the_whole_table(i):
    from hipvae import abi
    from hipvae import gbt
    g, want = load_fixture(), fixture_fit(i)
    sizes = [int(s) for s in g["sizes"]]
    args = (G(g["x_train"]), G(g["y_train"]), G(g["x_test"]), G(g["y_test"]), sizes)
    per = C.gbt_slot_bytes(g["x_train"].shape[1], RUNS[i]["max_depth"], RUNS[i]["max_bin"])
    whole = gbt.fit_boosted_trees(*args, **RUNS[i])
    assert whole.train_correct == want["correct"].tolist() and whole.test_correct == want["correct_test"].tolist()
    for slots in C.ROUND_SLOTS:
        got = gbt.fit_boosted_trees(*args, table_bytes=slots * per + 8, **RUNS[i])   # rounded down to whole slots
        for a, b in zip(got.trees + (got.importance, got.margins, got.test_margins),
                        whole.trees + (whole.importance, whole.margins, whole.test_margins)):
            assert torch.equal(a, b), slots
        tfeat, tbin, tvalue, tgain = (t.cpu().numpy() for t in got.trees)
        assert np.array_equal(tfeat, want["tfeat"]) and np.array_equal(tbin, want["tbin"])
        assert np.array_equal(tvalue, want["tvalue"])
        assert (np.abs(tgain - want["tgain"]) <= 1e-15 * np.abs(want["tgain"])).all()
        assert np.abs(got.importance.cpu().numpy() - want["importance"]).max() <= 1e-12
        assert got.train_correct == want["correct"].tolist() and got.test_correct == want["correct_test"].tolist()
        assert np.abs(got.margins.cpu().numpy() - want["F"]).max() <= 1e-12
    with pytest.raises(abi.HipExtensionError, match="below one class slot"):   # refused by the host, before any launch
        gbt.fit_boosted_trees(*args, table_bytes=per - 1, **RUNS[i])
