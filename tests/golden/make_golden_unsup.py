#!/usr/bin/env python3
"""Golden vectors for the device-side unsupervised scores and IRS.  Needs numpy and scipy; no GPU.

Writes ``unsup_scores.npz``:

* ``mu [600, 10]`` fp32: columns 0-3 carry factors 0-3 plus noise, 4-7 are fixed mixtures of other columns plus noise
  (correlated columns), column 8 is CONSTANT, column 9 mixes factor 1 and noise.  ``active = [0..7, 9]``: the unsupervised
  scores are taken on these nine columns (a constant column has no positive-definite covariance), IRS on all ten.
* ``factors [600, 4]`` int32 with ``sizes = (3, 5, 4, 7)``.
* From the numpy restatement (tests/unsup_ref.py): ``mean``, ``cov``, ``tc``, ``w``, ``w_norm``, ``eig`` (ascending),
  ``mi_matrix``, ``mi_score`` of the active columns; ``irs_*`` of all columns.
* The literal library formulas, evaluated once here: ``lib_cov = np.cov``, ``lib_tc`` from ``np.linalg.slogdet``,
  ``lib_w`` / ``lib_w_norm`` from ``scipy.linalg.sqrtm(C * diag(C)[:, None])``, ``lib_irs_*`` from
  disentanglement_lib's ``scalable_disentanglement_score`` arithmetic with ``np.percentile`` and ``np.average``.

The seed is the first for which cond(S) <= 100 and every row of the IRS matrix keeps its two largest entries 1e-3 apart.
The file holds data only.

    python tests/golden/make_golden_unsup.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy.linalg  # noqa: E402
import unsup_ref as R  # noqa: E402

SIZES = (3, 5, 4, 7)
ACTIVE = [0, 1, 2, 3, 4, 5, 6, 7, 9]


def make(seed):
    rs = np.random.RandomState(seed)
    N = 600
    f = np.stack([rs.randint(s, size=N) for s in SIZES], 1).astype(np.int32)
    z = np.empty((N, 10))
    for k in range(4):
        z[:, k] = (f[:, k] - (SIZES[k] - 1) / 2.0) * (1.6 / SIZES[k]) + 0.35 * rs.randn(N)
    z[:, 4] = 0.4 * z[:, 0] - 0.3 * z[:, 2] + 0.6 * rs.randn(N)
    z[:, 5] = 0.3 * z[:, 1] + 0.3 * z[:, 3] + 0.6 * rs.randn(N)
    z[:, 6] = 0.7 * rs.randn(N) + 0.3 * z[:, 4]
    z[:, 7] = 0.9 * rs.randn(N) - 0.2 * z[:, 5]
    z[:, 8] = 0.25
    z[:, 9] = 0.2 * (f[:, 1] - 2.0) + 0.6 * rs.randn(N)
    return z.astype(np.float32), f


def lib_irs(mu, f, q=0.99):
    """disentanglement_lib/evaluation/metrics/irs.py on the dimensions with var > 0, as its compute_irs does."""
    lat = mu.astype(np.float64)
    keep = lat.var(axis=0) > 0.0
    lat = lat[:, keep]
    maxdev = np.max(np.abs(lat - lat.mean(axis=0)), axis=0)
    cum = np.zeros([lat.shape[1], f.shape[1]])
    for i in range(f.shape[1]):
        uniq = np.unique(f[:, i], axis=0)
        for k in range(uniq.shape[0]):
            match = f[:, i] == uniq[k]
            e_loc = np.mean(lat[match, :], axis=0)
            diffs = np.abs(lat[match, :] - e_loc)
            cum[:, i] += np.percentile(diffs, q=q * 100, axis=0)
        cum[:, i] /= uniq.shape[0]
    M = 1.0 - cum / maxdev[:, np.newaxis]
    scores = M.max(axis=1)
    return dict(keep=keep, matrix=M, avg=np.average(scores, weights=maxdev), parents=M.argmax(axis=1), maxdev=maxdev)


def conditions(mu, f):
    _, C = R.ref_cov(mu[:, ACTIVE])
    cond = np.linalg.cond(R.ref_scaled(C))
    irs = R.ref_irs(mu, f, SIZES)
    top = np.sort(irs["IRS_matrix"][irs["active"]], axis=1)
    gap = (top[:, -1] - top[:, -2]).min()
    return cond, gap


def main():
    for seed in range(100):
        mu, f = make(seed)
        cond, gap = conditions(mu, f)
        if cond <= 100.0 and gap >= 1e-3:
            break
    else:
        raise SystemExit("no seed meets the conditions")
    print("seed", seed, "cond(S)", cond, "smallest gap of the two largest IRS entries", gap)
    x = mu[:, ACTIVE]
    mean, C = R.ref_cov(x)
    g = R.ref_gauss(C)
    assert g["fail_dim"] < 0 and g["converged"]
    mi, mis = R.ref_mi_matrix(x)
    irs = R.ref_irs(mu, f, SIZES)
    # the literal library formulas
    lc = np.cov(x.astype(np.float64).T)
    lib_tc = 0.5 * (np.sum(np.log(np.diag(lc))) - np.linalg.slogdet(lc)[1])
    sq = scipy.linalg.sqrtm(lc * np.expand_dims(np.diag(lc), axis=1))
    lib_w = 2 * np.trace(lc) - 2 * np.trace(sq)
    li = lib_irs(mu, f)
    print("tc", g["tc"], "lib", lib_tc, "w", g["w"], "lib", float(np.real(lib_w)), "sweeps", g["sweeps"])
    print("irs", irs["avg_score"], "lib", li["avg"], "mi score", mis)
    np.savez_compressed(
        os.path.join(HERE, "unsup_scores.npz"), seed=np.int64(seed), mu=mu, factors=f, sizes=np.asarray(SIZES, np.int64),
        active=np.asarray(ACTIVE, np.int64), mean=mean, cov=C, tc=g["tc"], w=g["w"], w_norm=g["w_norm"],
        eig=np.sort(g["eig"]), mi_matrix=mi, mi_score=mis, irs_avg=irs["avg_score"], irs_matrix=irs["IRS_matrix"],
        irs_cum=irs["cum"], irs_maxdev=irs["max_deviations"], irs_parents=irs["parents"], irs_scores=irs["scores"],
        irs_active=irs["active"], lib_cov=lc, lib_tc=lib_tc, lib_w=float(np.real(lib_w)),
        lib_w_norm=float(np.real(lib_w)) / np.trace(lc), lib_irs_matrix=li["matrix"], lib_irs_avg=li["avg"],
        lib_irs_parents=li["parents"], lib_irs_keep=li["keep"], lib_irs_maxdev=li["maxdev"])


if __name__ == "__main__":
    main()
