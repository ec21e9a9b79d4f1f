#!/usr/bin/env python3
"""Golden vectors for the device-side Unsupervised Disentanglement Ranking.  Needs numpy, scipy and sklearn; no GPU.

Writes ``udr.npz``:

* ``mu0, mu1, mu2`` and ``logvar0, logvar1, logvar2`` ``[600, 10]`` fp32: three synthetic "models" of five shared
  non-Gaussian sources.  Columns 0-4 are informative (``logvar`` about -3): model 0 a signed permutation of the sources
  plus small mixing, model 1 heavier mixing, model 2 mixing so strong that the correlation matrix of its informative
  columns has a condition number of about 100.  Column 1 is quantised to multiples of 0.25 (many ties).  Column 5 is exactly
  CONSTANT (0.3; ``logvar`` about 0, so its KL of about 0.045 keeps it in the mask: an informative-by-KL latent with an
  all-zero row).  Columns 6-9 are inactive: ``mu = 0.01 randn``, ``logvar`` about 0, KL < 0.01.  Every model has its
  columns shuffled by its own permutation (``perm0`` .. ``perm2`` map the positions above to columns).
* the library values, evaluated once here for every ordered pair (i, j), i != j, stacked in the order (0, 1), (0, 2),
  (1, 0), (1, 2), (2, 0), (2, 1) (``pairs``): ``lib_spearman [6, 10, 10]`` = ``|scipy.stats.spearmanr(a, b)|``'s cross
  block with the nan of a constant column replaced by 0; ``lib_lasso [6, 10, 10]`` = ``transpose(abs(Lasso(alpha = 0.1,
  tol = 1e-14, max_iter = 100000).fit(StandardScaler(a), StandardScaler(b)).coef_))``; ``lib_kl [3, 10]``; and the UDR of
  both forms by disentanglement_lib's arithmetic (``relative_strength_disentanglement`` with ``nan_to_num`` / ``nanmean``,
  ``np.median``): ``lib_pairwise_spearman / lib_pairwise_lasso [3, 3]`` and ``lib_scores_spearman / lib_scores_lasso
  [3]``.

The seed is the first for which the conditions the GPU bounds rest on hold (tests/test_udr_host.py asserts them again).
The file holds data only.

    python tests/golden/make_golden_udr.py
"""
import os
import sys
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy.stats  # noqa: E402
from sklearn.linear_model import Lasso  # noqa: E402
from sklearn.preprocessing import StandardScaler  # noqa: E402
import udr_ref as R  # noqa: E402

N, D = 600, 10
PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]


def mixing(rs, kind):
    if kind == 0:
        P = np.eye(5)[rs.permutation(5)] * rs.choice([-1.0, 1.0], size=5)
        return P + 0.08 * rs.randn(5, 5)
    if kind == 1:
        return np.eye(5)[rs.permutation(5)] + 0.45 * rs.randn(5, 5)
    U, _ = np.linalg.qr(rs.randn(5, 5))
    V, _ = np.linalg.qr(rs.randn(5, 5))
    return (U * np.array([1.0, 0.8, 0.55, 0.3, 0.1])) @ V.T


def make(seed):
    rs = np.random.RandomState(seed)
    src = np.stack([rs.uniform(-1.7, 1.7, N), rs.laplace(0, 0.7, N), rs.randn(N), rs.uniform(-1, 1, N) ** 3 * 2.0,
                    rs.beta(2, 5, N) * 4 - 1.2], 1)
    out = {}
    for m in range(3):
        mu, lv = np.empty((N, D)), np.empty((N, D))
        mu[:, :5] = src @ mixing(rs, m) + 0.05 * rs.randn(N, 5)
        mu[:, 1] = np.round(mu[:, 1] * 4) / 4
        lv[:, :5] = -3.0 + 0.2 * rs.randn(N, 5)
        mu[:, 5] = 0.3
        mu[:, 6:] = 0.01 * rs.randn(N, 4)
        lv[:, 5:] = 0.02 * rs.randn(N, 5)
        perm = rs.permutation(D)
        out[f"mu{m}"] = np.ascontiguousarray(mu[:, np.argsort(perm)]).astype(np.float32)
        out[f"logvar{m}"] = np.ascontiguousarray(lv[:, np.argsort(perm)]).astype(np.float32)
        out[f"perm{m}"] = perm.astype(np.int32)
    return out


def conditions(g):
    """(smallest eigenvalue of a live G, largest condition number, smallest margin of a zero, smallest nonzero |w|, most
    sweeps) over the six ordered pairs."""
    lam, cond, margin, small, most = np.inf, 0.0, np.inf, np.inf, 0
    for i, j in PAIRS:
        _, w, sweeps, conv, G, cs = R.ref_lasso(g[f"mu{i}"], g[f"mu{j}"], details=True)
        assert conv.all()
        live = np.diag(G) != 0
        ev = np.linalg.eigvalsh(G[live][:, live])
        lam, cond, most = min(lam, ev[0]), max(cond, ev[-1] / ev[0]), max(most, int(sweeps.max()))
        grad = G @ w - cs
        zero = (w == 0) & live[:, None]
        margin = min(margin, (0.1 - np.abs(grad[zero])).min())
        if (w != 0).any():
            small = min(small, np.abs(w[w != 0]).min())
    return lam, cond, margin, small, most


def lib_relative_strength(c):
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = np.nanmean(np.nan_to_num(np.power(np.ndarray.max(c, axis=0), 2) / np.sum(c, axis=0), 0))
        sy = np.nanmean(np.nan_to_num(np.power(np.ndarray.max(c, axis=1), 2) / np.sum(c, axis=1), 0))
    return (sx + sy) / 2


def library(g):
    mus = [g[f"mu{m}"].astype(np.float64) for m in range(3)]
    lvs = [g[f"logvar{m}"].astype(np.float64) for m in range(3)]
    kl = np.stack([np.mean(0.5 * (np.square(m) + np.exp(lv) - lv - 1), axis=0) for m, lv in zip(mus, lvs)])
    masks = kl > 0.01
    sp, la = [], []
    for i, j in PAIRS:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rho = scipy.stats.spearmanr(mus[i], mus[j])[0]
        sp.append(np.nan_to_num(np.abs(rho[:D, D:]), nan=0.0))
        a, b = StandardScaler().fit_transform(mus[i]), StandardScaler().fit_transform(mus[j])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # the all-zero target of a constant column: "gap 0, tolerance 0"
            model = Lasso(alpha=0.1, tol=1e-14, max_iter=100000).fit(a, b)
        la.append(np.transpose(np.absolute(model.coef_)))
    rec = dict(pairs=np.array(PAIRS, dtype=np.int32), lib_spearman=np.stack(sp), lib_lasso=np.stack(la), lib_kl=kl)
    for name, mats in (("spearman", sp), ("lasso", la)):
        pw = np.full((3, 3), np.nan)
        for (i, j), c in zip(PAIRS, mats):
            pw[i, j] = lib_relative_strength(c[masks[i]][:, masks[j]])
        rec[f"lib_pairwise_{name}"] = pw
        rec[f"lib_scores_{name}"] = np.array([np.median([pw[j, i] for j in range(3) if j != i]) for i in range(3)])
    return rec


def main():
    for seed in range(100):
        g = make(seed)
        lam, cond, margin, small, most = conditions(g)
        print(f"seed {seed}: lambda_min {lam:.4f} cond {cond:.1f} zero margin {margin:.2e} smallest |w| {small:.2e} "
              f"sweeps <= {most}")
        if lam >= 0.005 and 60.0 <= cond <= 200.0 and margin >= 1e-5 and small >= 1e-5:
            break
    else:
        raise SystemExit("no seed meets the conditions")
    g.update(library(g))
    path = os.path.join(HERE, "udr.npz")
    np.savez_compressed(path, **g)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("kl masks", (g["lib_kl"] > 0.01).astype(int))
    print("scores spearman", g["lib_scores_spearman"], "lasso", g["lib_scores_lasso"])


if __name__ == "__main__":
    main()
