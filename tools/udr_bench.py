#!/usr/bin/env python3
"""Time of the device-side Unsupervised Disentanglement Ranking (hipvae.disentangle.udr_scores, csrc/udr.hip) in both forms
at M = 5 models, N = 10000 representations and D = 128 latents, next to the numpy fp64 restatement of the same rules on the
host (tests/udr_ref.py).

Device: a host clock around whole calls, each of which ends in its one host read-back (a device synchronise), after two
warm-up calls; the median and the range of 10 calls.  Also the time of the parts from HIP events: the rank launch, one
covariance, one Lasso call.  Host: one call of the restatement per form (all M (M - 1) = 20 ordered pairs; seconds long),
and the largest differences between the two."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "intro-tc-vae_amd"))
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import udr_ref as R  # noqa: E402
from hipvae import disentangle as DS  # noqa: E402
from hipvae import functional as HF  # noqa: E402

dev = torch.device("cuda:0")
M, N, D = 5, 10000, 128


def inputs(seed=1):
    """Every model: a signed permutation of 96 shared sources plus mixing of 0.3 / sqrt(96) per entry and noise (96
    informative latents, logvar -3), and 32 inactive latents (mu = 0.01 randn, logvar 0)."""
    rs = np.random.RandomState(seed)
    src = rs.randn(N, 96)
    mus, lvs = [], []
    for _ in range(M):
        A = np.eye(96)[rs.permutation(96)] * rs.choice([-1.0, 1.0], size=96) + 0.3 * rs.randn(96, 96) / np.sqrt(96)
        mu = np.concatenate([src @ A + 0.1 * rs.randn(N, 96), 0.01 * rs.randn(N, 32)], 1)
        lv = np.concatenate([-3.0 + 0.1 * rs.randn(N, 96), 0.01 * rs.randn(N, 32)], 1)
        perm = rs.permutation(D)
        mus.append(np.ascontiguousarray(mu[:, perm]).astype(np.float32))
        lvs.append(np.ascontiguousarray(lv[:, perm]).astype(np.float32))
    return mus, lvs


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
    mus, lvs = inputs()
    md, ld = [torch.from_numpy(m).to(dev) for m in mus], [torch.from_numpy(lv).to(dev) for lv in lvs]
    got = {form: DS.udr_scores(md, ld, correlation=form) for form in ("lasso", "spearman")}
    t = {form: wall(lambda form=form: DS.udr_scores(md, ld, correlation=form)) for form in ("lasso", "spearman")}
    flags = HF.disent_flags(dev)
    both = torch.cat([md[0], md[1]], 1)
    _, cov = HF.unsup_cov(both, flags)
    t_rank = events(lambda: HF.udr_ranks(md[0], flags))
    t_cov = events(lambda: HF.unsup_cov(both, flags))
    t_lasso = events(lambda: HF.udr_lasso(cov, D, D))
    sweeps = int(HF.udr_lasso(cov, D, D)[1][2])

    th, want = {}, {}
    for form in ("lasso", "spearman"):
        t0 = time.perf_counter()
        want[form] = R.ref_udr(mus, lvs, form)
        th[form] = time.perf_counter() - t0

    print(f"M {M} models, N {N} x D {D}; kept by the KL mask: {[int(m.sum()) for m in got['lasso']['kl_masks']]}")
    for form in ("lasso", "spearman"):
        a, g, w = t[form], got[form], want[form]
        raw = max(np.abs(g["raw_correlations"][k].cpu().numpy() - w["raw"][k]).max() for k in w["raw"])
        print(f"udr_scores {form:8s} (device, with its read-back): median {a[0]:8.3f} ms (min {a[1]:.3f}, max {a[2]:.3f}); "
              f"scores {[round(v, 4) for v in g['model_scores']]}")
        print(f"  numpy restatement on the host: {th[form]:.2f} s; {th[form] * 1e3 / a[0]:.0f}x; largest |matrix - ref| "
              f"{raw:.1e}, largest |score - ref| "
              f"{np.abs(np.array(g['model_scores']) - np.array(w['model_scores'])).max():.1e}")
    print(f"parts (HIP events): itcv_udr_ranks [N, D] {t_rank:.3f} ms; itcv_unsup_cov [N, 2 D] {t_cov:.3f} ms; "
          f"itcv_udr_lasso Da = Db = {D} {t_lasso:.3f} ms ({sweeps} sweeps at most)")


if __name__ == "__main__":
    main()
