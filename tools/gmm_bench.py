#!/usr/bin/env python3
"""Time of the Gaussian-mixture entry points (hipvae.density.fit_gmm / gmm_log_prob / gmm_sample, csrc/gmm.hip) at N = 10000
rows of D = 128 with K = 10 components, next to a chunked fp64 torch restatement of the same quantities on the same GPU:
``linalg.cholesky`` + ``linalg.solve_triangular`` + ``logsumexp`` for the E-step, ``matmul`` for the M-step, ``bmm`` for the
sampler.  Both fits start from the same parameters (the device k-means initialisation, which is timed on its own) and run
the same fixed number of EM iterations (``tol = 0``), each with one host read-back.

A host clock around whole calls, each of which ends in a host read-back or a device synchronise, after warm-up calls of the
same shape; the median and the range of the repeats.  The two sides are timed alternately.  ``--json PATH`` also writes the
records."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hipvae import density as Dn  # noqa: E402
from hipvae import functional as HF  # noqa: E402

dev = torch.device("cuda:0")
CHUNK = 4096
ITERS = 10
REG = 1e-6


def inputs(N, D, K, seed=1):
    rs = np.random.RandomState(seed)
    parts = []
    for k in range(K):
        mix = np.eye(D) + 0.3 * rs.randn(D, D) / np.sqrt(D)
        parts.append(3.0 * rs.randn(D) / np.sqrt(D) + rs.randn(N // K + (k < N % K), D) @ mix)
    x = np.concatenate(parts, 0)[rs.permutation(N)]
    return torch.from_numpy(x.astype(np.float32)).to(dev)


# ---- the torch restatement ---------------------------------------------------------------------------------------------------
def t_logp(x, w, means, chol):
    """lp [N, K] fp64, chunked over rows."""
    D = x.shape[1]
    logdet = 2.0 * chol.diagonal(dim1=1, dim2=2).log().sum(1)
    out = []
    for a in range(0, len(x), CHUNK):
        d = x[a:a + CHUNK].double()[None] - means[:, None]                       # [K, n, D]
        y = torch.linalg.solve_triangular(chol, d.transpose(1, 2), upper=False)    # [K, D, n]
        out.append((w.log()[:, None] - 0.5 * (D * math.log(2 * math.pi) + logdet[:, None] + (y * y).sum(1))).T)
    return torch.cat(out)


def t_log_prob(x, w, means, chol):
    return torch.logsumexp(t_logp(x, w, means, chol), 1)


def t_fit(x, init, iters):
    w, means, cov = init
    xd = x.double()
    N, D = xd.shape
    bound = None
    for _ in range(iters):
        lp = t_logp(x, w, means, torch.linalg.cholesky(cov))
        lse = torch.logsumexp(lp, 1)
        resp = (lp - lse[:, None]).exp()
        nk = resp.sum(0) + 10 * torch.finfo(torch.float64).eps
        w, means = nk / nk.sum(), resp.T @ xd / nk[:, None]
        covs = []
        for k in range(len(nk)):
            d = xd - means[k]
            covs.append((resp[:, k:k + 1] * d).T @ d / nk[k])
        cov = torch.stack(covs) + REG * torch.eye(D, dtype=torch.float64, device=dev)
        bound = lse.mean().item()                                                  # the read-back of the iteration
    return w, means, cov, bound


def t_sample(means, chol, comp, eps):
    return (means[comp] + torch.bmm(chol[comp], eps.double()[:, :, None])[:, :, 0]).float()


# ---- timing ------------------------------------------------------------------------------------------------------------------
def wall_pair(ours, theirs, warm, reps):
    """((median, min, max) ms of ``ours``, the same of ``theirs``), timed alternately; both end in a device synchronise."""
    for _ in range(warm):
        ours()
        theirs()
    ts = ([], [])
    for _ in range(reps):
        for which, once in enumerate((ours, theirs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            ts[which].append((time.perf_counter() - t0) * 1e3)
    return tuple((float(np.median(t)), min(t), max(t)) for t in ts)


def run(N, D, K, warm, reps):
    x = inputs(N, D, K)
    w0, m0, c0 = Dn.kmeans_init(x, K, 10, 0, REG)[:3]
    init = (w0, m0, c0)
    print(f"N {N} x D {D}, K {K}, {ITERS} EM iterations: {warm} warm-up calls, median (min .. max) of {reps}, ms, "
          "device | torch fp64")
    gmm = Dn.fit_gmm(x, K, max_iter=ITERS, tol=0.0, reg_covar=REG, init=init)
    tw, tm, tc, tb = t_fit(x, init, ITERS)
    gen = torch.Generator().manual_seed(0)
    comp = torch.multinomial(gmm.weights.cpu(), N, replacement=True, generator=gen).to(dev)
    eps = torch.randn((N, D), generator=gen).to(dev)
    comp32, flags = comp.to(torch.int32), HF.disent_flags(dev)
    lp_d, lp_t = Dn.gmm_log_prob(gmm, x), t_log_prob(x, gmm.weights, gmm.means, gmm.chol)
    agree = dict(bound_device=gmm.lower_bound, bound_torch=tb,
                 weights_rel=float((gmm.weights / tw - 1).abs().max()),
                 cov_rel=float((gmm.covariances - tc).abs().max() / tc.abs().max()),
                 log_prob_rel=float(((lp_d - lp_t) / lp_t).abs().max()),
                 sample_abs=float((Dn.gmm_sample(gmm, N, 0) - t_sample(gmm.means, gmm.chol, comp, eps)).abs().max()))
    print("  agreement:", json.dumps(agree))
    ours = dict(fit=lambda: Dn.fit_gmm(x, K, max_iter=ITERS, tol=0.0, reg_covar=REG, init=init),
                log_prob=lambda: Dn.gmm_log_prob(gmm, x),
                sample=lambda: HF.gmm_sample(gmm.means, gmm.chol, comp32, eps, flags))
    theirs = dict(fit=lambda: t_fit(x, init, ITERS), log_prob=lambda: t_log_prob(x, gmm.weights, gmm.means, gmm.chol),
                  sample=lambda: t_sample(gmm.means, gmm.chol, comp, eps))
    rec = dict(N=N, D=D, K=K, iters=ITERS, warm=warm, reps=reps, agreement=agree, times={})
    for name in ours:
        o, t = wall_pair(ours[name], theirs[name], warm, reps)
        rec["times"][name] = dict(device_ms=o, torch_ms=t, ratio=t[0] / o[0])
        print(f"  {name:9s} {o[0]:10.3f} ({o[1]:.3f} .. {o[2]:.3f}) | {t[0]:10.3f} ({t[1]:.3f} .. {t[2]:.3f})   "
              f"torch / device {t[0] / o[0]:.2f}x")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Dn.kmeans_init(x, K, 10, 0, REG)
    torch.cuda.synchronize()
    rec["kmeans_init_ms"] = (time.perf_counter() - t0) * 1e3
    print(f"  k-means initialisation (10 Lloyd iterations, device only, one call): {rec['kmeans_init_ms']:.3f} ms")
    o, _ = wall_pair(lambda: Dn.gmm_sample(gmm, N, 0), lambda: None, 1, reps)
    rec["gmm_sample_call_ms"] = o
    print(f"  gmm_sample, the whole call (the draws on the host and their copy included; 'sample' above is the kernel on "
          f"device operands): {o[0]:.3f} ({o[1]:.3f} .. {o[2]:.3f}) ms")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gmm_bench: no GPU; nothing is measured without one")
    recs = [run(10000, 128, 10, warm=2, reps=10)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
