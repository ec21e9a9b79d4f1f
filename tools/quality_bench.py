#!/usr/bin/env python3
"""Time of the four sample-quality entry points (hipvae.quality.knn_radius / prdc / kernel_distance / frechet_distance,
csrc/quality.hip) at N = M = 10000 feature rows of D = 128 and at N = M = 50000 rows of D = 512, next to a chunked fp64
torch restatement of the same quantities on the same GPU: ``cdist`` + ``kthvalue`` for the radii and the counts,
``matmul`` for the kernel sums, ``cov`` + ``linalg.cholesky`` + ``linalg.eigvalsh`` for the Frechet distance.

A host clock around whole calls, each of which ends in its host read-back (a device synchronise), after warm-up calls of
the same shape; the median and the range of the repeats.  The two sides are timed alternately.  Also what the all-pairs
pass achieves: 3 N M D fp64 operations (a subtraction, a multiplication, an addition per pair and column) over the time
of one radius call.  ``--small`` runs the first shape alone; ``--json PATH`` also writes the records."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hipvae import functional as HF  # noqa: E402
from hipvae import quality as Q  # noqa: E402

dev = torch.device("cuda:0")
K = 5
CHUNK = 2048                      # rows of one torch chunk: 2048 x 50000 doubles = 0.8 GB


def inputs(N, M, D, seed=1):
    rs = np.random.RandomState(seed)
    mix = np.eye(D) + 0.3 * rs.randn(D, D) / np.sqrt(D)              # correlated columns, well-conditioned covariances
    real = rs.randn(N, D) @ mix
    fake = (1.1 * rs.randn(M, D) + 0.1) @ mix
    return torch.from_numpy(real.astype(np.float32)).to(dev), torch.from_numpy(fake.astype(np.float32)).to(dev)


# ---- the torch restatement ---------------------------------------------------------------------------------------------------
def t_radii(x, k=K):
    x = x.double()
    return torch.cat([torch.cdist(x[a:a + CHUNK], x).kthvalue(k + 1, dim=1).values for a in range(0, len(x), CHUNK)]) ** 2


def t_knn(x):
    return t_radii(x).sum().item()


def t_prdc(real, fake, k=K):
    rr, rf = t_radii(real, k).sqrt(), t_radii(fake, k).sqrt()
    real, fake = real.double(), fake.double()
    hits = torch.zeros(len(fake), dtype=torch.int64, device=dev)
    covered, inside = [], []
    for a in range(0, len(real), CHUNK):
        d = torch.cdist(real[a:a + CHUNK], fake)
        hits += (d < rr[a:a + CHUNK, None]).sum(0)
        covered.append((d < rf[None, :]).any(1))
        inside.append(d.min(1).values < rr[a:a + CHUNK])
    c = torch.stack([(hits > 0).sum(), torch.cat(covered).sum(), hits.sum(), torch.cat(inside).sum()]).tolist()
    N, M = len(real), len(fake)
    return dict(precision=c[0] / M, recall=c[1] / N, density=c[2] / (k * M), coverage=c[3] / N)


def _t_ksum(a, b, skip_diag):
    D = a.shape[1]
    s = torch.zeros((), dtype=torch.float64, device=dev)
    for r in range(0, len(a), CHUNK):
        kap = (a[r:r + CHUNK] @ b.T / D + 1.0) ** 3
        if skip_diag:
            kap.diagonal(offset=r).zero_()
        s += kap.sum()
    return s


def t_kid(real, fake):
    x, y = real.double(), fake.double()
    N, M = len(x), len(y)
    return (_t_ksum(x, x, True) / (N * (N - 1.0)) + _t_ksum(y, y, True) / (M * (M - 1.0))
            - 2.0 * _t_ksum(x, y, False) / (N * M)).item()


def t_frechet(real, fake):
    x, y = real.double(), fake.double()
    m1, m2, c1, c2 = x.mean(0), y.mean(0), torch.cov(x.T), torch.cov(y.T)
    L = torch.linalg.cholesky(c1)
    eig = torch.linalg.eigvalsh(L.T @ c2 @ L)
    return (((m1 - m2) ** 2).sum() + c1.trace() + c2.trace() - 2.0 * eig.clamp(min=0).sqrt().sum()).item()


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
            ts[which].append((time.perf_counter() - t0) * 1e3)
    return tuple((float(np.median(t)), min(t), max(t)) for t in ts)


def events(once, warm=2, reps=5):
    """ms per call from HIP events around ``reps`` calls."""
    for _ in range(warm):
        once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(N, M, D, warm, reps):
    real, fake = inputs(N, M, D)
    print(f"N {N} x M {M} x D {D}, k {K}: {warm} warm-up calls, median (min .. max) of {reps}, ms, device | torch fp64")
    ours = dict(knn_radius=lambda: Q.knn_radius(real, K), prdc=lambda: Q.prdc(real, fake, K),
                kernel_distance=lambda: Q.kernel_distance(real, fake), frechet_distance=lambda: Q.frechet_distance(real, fake))
    theirs = dict(knn_radius=lambda: t_knn(real), prdc=lambda: t_prdc(real, fake), kernel_distance=lambda: t_kid(real, fake),
                  frechet_distance=lambda: t_frechet(real, fake))
    # agreement first: what is timed computes the same thing
    a, b = ours["prdc"](), theirs["prdc"]()
    kid, fd = ours["kernel_distance"]()["kid"], ours["frechet_distance"]()["frechet"]
    r2 = ours["knn_radius"]()
    agree = dict(prdc_device=a, prdc_torch=b, radius_rel=float((r2 / t_radii(real) - 1).abs().max()),
                 kid_device=kid, kid_torch=theirs["kernel_distance"](), frechet_device=fd,
                 frechet_torch=theirs["frechet_distance"]())
    print("  agreement:", json.dumps(agree))
    rec = dict(N=N, M=M, D=D, k=K, warm=warm, reps=reps, agreement=agree, times={})
    for name in ours:
        o, t = wall_pair(ours[name], theirs[name], warm, reps)
        rec["times"][name] = dict(device_ms=o, torch_ms=t, ratio=t[0] / o[0])
        print(f"  {name:17s} {o[0]:10.3f} ({o[1]:.3f} .. {o[2]:.3f}) | {t[0]:10.3f} ({t[1]:.3f} .. {t[2]:.3f})   "
              f"torch / device {t[0] / o[0]:.2f}x")
    # the parts of the Frechet call: one covariance, and the one-block Cholesky / product / Jacobi launch
    flags = HF.disent_flags(dev)
    (m1, c1), (m2, c2) = HF.unsup_cov(real, flags), HF.unsup_cov(fake, flags)
    t_cov = events(lambda: HF.unsup_cov(real, flags), 1, min(reps, 5))
    t_fr = events(lambda: HF.frechet(m1, c1, m2, c2), 1, min(reps, 5))
    sweeps = int(HF.frechet(m1, c1, m2, c2)[2][3])
    rec["frechet_parts"] = dict(cov_ms=t_cov, kernel_ms=t_fr, sweeps=sweeps)
    print(f"  frechet parts: one covariance {t_cov:.3f} ms, the Cholesky / product / Jacobi launch {t_fr:.3f} ms "
          f"({sweeps} sweeps)")
    ops = 3.0 * N * N * D
    rate = ops / (rec["times"]["knn_radius"]["device_ms"][0] * 1e-3)
    rec["pairs_fp64_ops_per_s"] = rate
    print(f"  all-pairs pass: 3 N N D = {ops:.3e} fp64 operations in the radius call: {rate / 1e12:.2f} T operations / s "
          "(whole call, launches and read-back included)")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="the first shape alone")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench: no GPU; nothing is measured without one")
    recs = [run(10000, 10000, 128, warm=2, reps=10)]
    if not args.small:
        recs.append(run(50000, 50000, 512, warm=1, reps=3))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
