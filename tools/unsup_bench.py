#!/usr/bin/env python3
"""Time of the device-side unsupervised scores and IRS (hipvae.disentangle.unsupervised_scores / irs_score_matrix,
csrc/unsup_scores.hip) at N = 10000 representations of D = 128 latents and K = 7 factors of 3, 6, 40, 32, 32, 10 and 256
values, next to the numpy fp64 restatement of the same rules on the host (tests/unsup_ref.py).

Device: a host clock around whole calls, each of which ends in its host read-back (a device synchronise), after two
warm-up calls; the median and the range of 10 calls.  Host: one call each (seconds long).  Also the time of the parts
(covariance alone, the Cholesky / Jacobi launch alone) from HIP events, and the largest differences between the two."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import unsup_ref as R  # noqa: E402
from hipvae import disentangle as DS  # noqa: E402
from hipvae import functional as HF  # noqa: E402

dev = torch.device("cuda:0")
N, D, SIZES = 10000, 128, (3, 6, 40, 32, 32, 10, 256)


def inputs(seed=1):
    rs = np.random.RandomState(seed)
    f = np.stack([rs.randint(s, size=N) for s in SIZES], 1).astype(np.int32)
    z = rs.randn(N, D)
    for k, s in enumerate(SIZES):
        z[:, k] += 2.0 * f[:, k] / s
    x = z + 0.3 * (z @ (rs.randn(D, D) / np.sqrt(D)))                  # correlated columns, a well-conditioned covariance
    return x.astype(np.float32), f


def wall(once, warm=2, reps=10):
    """(median, min, max) ms of ``once``, which must end in a device synchronise."""
    for _ in range(warm):
        once()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        once()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def events(once, warm=2, reps=10):
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


def main():
    x, f = inputs()
    xd, fd = torch.from_numpy(x).to(dev), torch.from_numpy(f).to(dev)
    got_u, got_i = DS.unsupervised_scores(xd), DS.irs_score_matrix(xd, fd, SIZES)
    t_u, t_i = wall(lambda: DS.unsupervised_scores(xd)), wall(lambda: DS.irs_score_matrix(xd, fd, SIZES))
    flags = HF.disent_flags(dev)
    _, cov = HF.unsup_cov(xd, flags)
    t_cov, t_gauss = events(lambda: HF.unsup_cov(xd, flags)), events(lambda: HF.unsup_gauss(cov))
    sweeps = int(HF.unsup_gauss(cov)[2][3])

    t0 = time.perf_counter()
    _, C = R.ref_cov(x)
    g = R.ref_gauss(C)
    t_hg = time.perf_counter() - t0
    t0 = time.perf_counter()
    mi, mis = R.ref_mi_matrix(x)
    t_hm = time.perf_counter() - t0
    t0 = time.perf_counter()
    irs = R.ref_irs(x, f, SIZES)
    t_hi = time.perf_counter() - t0

    print(f"N {N} x D {D}, K {len(SIZES)} factors of {SIZES} values")
    print(f"unsupervised_scores (device, with its read-back): median {t_u[0]:8.3f} ms (min {t_u[1]:.3f}, max {t_u[2]:.3f}); "
          f"of that the covariance {t_cov:.3f} ms and the Cholesky / Jacobi launch {t_gauss:.3f} ms ({sweeps} sweeps)")
    print(f"  numpy restatement on the host: covariance + Cholesky + Jacobi {t_hg:.2f} s, mutual information {t_hm:.2f} s; "
          f"{(t_hg + t_hm) * 1e3 / t_u[0]:.0f}x")
    print(f"  |tc - ref| {abs(got_u['gaussian_total_correlation'] - g['tc']):.1e}, |w - ref| / tr C "
          f"{abs(got_u['gaussian_wasserstein_correlation'] - g['w']) / g['trace']:.1e}, |mi score - ref| "
          f"{abs(got_u['mutual_info_score'] - mis):.1e}")
    print(f"irs_score_matrix (device, with its read-back): median {t_i[0]:8.3f} ms (min {t_i[1]:.3f}, max {t_i[2]:.3f})")
    print(f"  numpy restatement on the host {t_hi:.2f} s; {t_hi * 1e3 / t_i[0]:.0f}x")
    act = irs["active"]
    print(f"  |IRS - ref| {abs(got_i['avg_score'] - irs['avg_score']):.1e}, largest |M - ref| "
          f"{np.abs(got_i['IRS_matrix'].cpu().numpy() - irs['IRS_matrix'][act]).max():.1e}")


if __name__ == "__main__":
    main()
