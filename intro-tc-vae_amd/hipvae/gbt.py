"""Histogram gradient-boosted trees on the device (csrc/gbt.hip): the classifier of the DCI score.

The rule is fixed in include/itcv_hip.h: xgboost's documented ``hist`` algorithm and defaults with every gradient sum an
integer sum, so a fit is bitwise reproducible.  A fit is a fixed launch sequence -- cuts and bins once, then per round
``itcv_gbt_round`` (gradients; histogram + split per level and class chunk; advance; margins) -- and reads nothing back
until the end: ``fit_boosted_trees`` makes ONE host read-back that carries the accuracy counts, the number of valid
classes per problem and the two error flags."""
from collections import namedtuple

import torch

from . import abi
from . import functional as HF
from .abi import call, lib, ptr, stream

__all__ = ["BoostedTrees", "fit_device", "read_back", "fit_boosted_trees"]

BoostedTrees = namedtuple("BoostedTrees", "importance train_accuracy test_accuracy train_correct test_correct trees "
                                          "cuts nbins margins test_margins pred test_pred cvalid")


def _present(y, sizes):
    off, out = 0, torch.zeros((sum(sizes),), dtype=torch.int32, device=y.device)
    for k, s in enumerate(sizes):
        col = y[:, k].long()
        ok = (col >= 0) & (col < s)
        out[off:off + s] = (torch.bincount(col[ok], minlength=s) > 0).to(torch.int32)
        off += s
    return out


def fit_device(x_train, y_train, x_test, y_test, class_sizes, rounds=100, max_depth=6, max_bin=256, eta=0.3, lam=1.0,
               cvalid=None, flags=None, table_bytes=None):
    """The fit without any read-back: a dict of device tensors (``importance [K, D]`` fp64, ``correct`` /
    ``correct_test [K]`` int64, ``nvalid [K]``, ``flags [2]``, the tree arrays, margins and predictions).
    ``table_bytes`` bounds the histogram table (default: what ``itcv_gbt_workspace`` asks for); it is rounded down to
    whole class slots, the classes are taken in chunks of that many, and less than one slot is refused."""
    sizes, csizes = HF._lr_sizes(class_sizes)
    K, csum = len(sizes), sum(sizes)
    rounds, max_depth, max_bin = int(rounds), int(max_depth), int(max_bin)
    if rounds < 1:
        raise ValueError(f"gbt: rounds = {rounds} is below 1")
    x = HF._disent_mu(x_train)
    xt = HF._disent_mu(x_test)
    dev = x.device
    N, D = x.shape
    Nt = xt.shape[0]
    y = HF._disent_factors(y_train, sizes, N, dev)[0]
    yt = HF._disent_factors(y_test, sizes, Nt, dev)[0]
    flags = HF.disent_flags(dev) if flags is None else flags
    nws = lib.itcv_gbt_workspace(N, D, K, csum, max_depth, max_bin)
    if not nws:                                           # outside the supported range: let the library say what
        call("itcv_gbt_round", None, N, D, max_bin, None, None, K, csizes, None, None, None, Nt, None, max_depth,
             float(lam), float(eta), None, None, None, None, None, 0, None, None, None, None, None, None)
        raise abi.HipExtensionError("gbt: the problem lies outside the supported range")
    if table_bytes is not None:
        per = (1 << (max_depth - 1)) * D * max_bin * 16   # one class slot: deepest level's nodes x D x max_bin x (G, H)
        if int(table_bytes) < per:
            raise abi.HipExtensionError(f"gbt: table_bytes = {int(table_bytes)} is below one class slot ({per} bytes)")
        nws = min(nws, int(table_bytes) // per * per)
    cvalid = _present(y, sizes) if cvalid is None else cvalid.to(device=dev, dtype=torch.int32).contiguous()
    if cvalid.numel() != csum:
        raise abi.HipExtensionError(f"gbt: the class mask needs {csum} entries (got {cvalid.numel()})")
    cuts, nbins = HF.gbt_cuts(x, max_bin)
    bins, bins_t = HF.gbt_bin(x, cuts, nbins, max_bin, flags), HF.gbt_bin(xt, cuts, nbins, max_bin, flags)
    F = torch.zeros((csum, N), dtype=HF.F64, device=dev)
    Ft = torch.zeros((csum, Nt), dtype=HF.F64, device=dev)
    gq, hq = (torch.empty((csum, N), dtype=HF.I64, device=dev) for _ in range(2))
    node = torch.empty((csum, N), dtype=HF.U8, device=dev)
    nsum = torch.zeros((csum, HF.GBT_NODES, 2), dtype=HF.I64, device=dev)
    tab = torch.empty((nws // 8,), dtype=HF.I64, device=dev)
    trees = HF.gbt_tree_arrays(rounds, csum, dev)
    st = stream()
    for r in range(rounds):
        call("itcv_gbt_round", ptr(bins), N, D, max_bin, ptr(nbins), ptr(y), K, csizes, ptr(cvalid), ptr(F), ptr(bins_t),
             Nt, ptr(Ft), max_depth, float(lam), float(eta), ptr(gq), ptr(hq), ptr(node), ptr(nsum), ptr(tab), nws,
             ptr(trees[0][r]), ptr(trees[1][r]), ptr(trees[2][r]), ptr(trees[3][r]), ptr(flags), st)
    pred, correct = HF.gbt_predict(F, y, sizes, cvalid, flags)
    pred_t, correct_t = HF.gbt_predict(Ft, yt, sizes, cvalid, flags)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    nvalid = torch.stack([cvalid[a:b].ne(0).sum() for a, b in zip(off[:-1], off[1:])])
    return dict(importance=HF.gbt_importance(trees[0], trees[3], sizes, D), correct=correct, correct_test=correct_t,
                nvalid=nvalid, flags=flags, trees=trees, cuts=cuts, nbins=nbins, margins=F, test_margins=Ft, pred=pred,
                test_pred=pred_t, cvalid=cvalid, N=N, Nt=Nt, K=K)


def read_back(fit, extra=()):
    """The one host read-back of a fit: raises on the flags and on a problem with fewer than two valid classes; returns
    (train counts, test counts, the fp64 scalars of ``extra``)."""
    K = fit["K"]
    parts = [fit["correct"].to(HF.F64), fit["correct_test"].to(HF.F64), fit["nvalid"].to(HF.F64), fit["flags"].to(HF.F64)]
    if extra:
        parts.append(torch.stack(list(extra)))
    packed = torch.cat(parts).tolist()
    f0, f1 = packed[3 * K:3 * K + 2]
    if f0:
        raise ValueError("gbt: the representations contain non-finite values")
    if f1:
        raise ValueError("gbt: a label lies outside [0, class_size)")
    for k, nv in enumerate(packed[2 * K:3 * K]):
        if nv < 2:
            raise ValueError(f"gbt: problem {k} needs samples of at least 2 classes, but the data contains {int(nv)}")
    return [int(v) for v in packed[:K]], [int(v) for v in packed[K:2 * K]], packed[3 * K + 2:]


def fit_boosted_trees(x_train, y_train, x_test, y_test, class_sizes, rounds=100, max_depth=6, max_bin=256, eta=0.3,
                      lam=1.0, cvalid=None, table_bytes=None):
    """Fit the K boosted-tree classifiers of (x_train[N, D], y_train[N, K]) jointly and evaluate them on both sets.
    Returns a ``BoostedTrees``: ``importance [K, D]`` (fp64, on the device), per-problem train / test accuracy (integer
    counts divided by the number of rows), the counts, and the tree arrays / cuts / margins / predictions as device
    tensors.  Non-finite representations, labels outside their range and a problem with fewer than two valid classes
    raise ``ValueError``.  ``table_bytes``: see ``fit_device``."""
    fit = fit_device(x_train, y_train, x_test, y_test, class_sizes, rounds, max_depth, max_bin, eta, lam, cvalid,
                     table_bytes=table_bytes)
    tr, te, _ = read_back(fit)
    return BoostedTrees(fit["importance"], [c / fit["N"] for c in tr], [c / fit["Nt"] for c in te], tr, te, fit["trees"],
                        fit["cuts"], fit["nbins"], fit["margins"], fit["test_margins"], fit["pred"], fit["test_pred"],
                        fit["cvalid"])
