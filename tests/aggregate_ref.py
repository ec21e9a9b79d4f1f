"""fp64 restatement of the dataset-scale aggregate-posterior kernel (csrc/aggregate.hip) and of the decomposition built on
it (hipvae/aggregate.py), for tests/test_hip_aggregate.py and tests/test_aggregate_ref_host.py: torch on the CPU,
chunked over the sample rows, and oracle/latent_math.py for the densities.

``z`` [S, D] are samples, ``(mu, logvar)`` [N, D] the mixture components, ``logw`` [N] their log weights (None: -log N),
``rows`` [S] the component each sample was drawn from.  Everything is dtype-generic.

``defect`` names one deliberate mistake of a kernel (DEFECTS below): the host tests use them to show that the checked
quantities move far beyond the tolerance when the kernel makes that mistake."""
import math

import torch

from oracle import latent_math as lm

# the tolerance on rel_err (max |got - ref| / max |ref|, per array): the ceiling tests/latent_ref.py documents
TOL = 1e-4
TILE = 64            # components per tile of the defects that depend on a tiling

DEFECTS = ("drop_tail",        # the last N mod 64 components are left out (1 when N mod 64 is 0)
           "no_weight",        # logw is ignored (every component weighs 1 / N)
           "clamp_outside",    # the -50 floor is applied to sum_l lp instead of per element
           "stale_max")        # the running sum is not rescaled when a later tile of 64 raises the maximum

#         (S, N, D)
SHAPES = ((1, 1, 1), (3, 5, 10), (9, 1000, 10), (33, 4099, 32), (9, 2051, 33), (9, 1500, 64), (9, 777, 65),
          (5, 300, 130), (5, 200, 512), (2, 300001, 10))
# the narrow lane groups of csrc/aggregate.hip that the shapes above do not reach (2, 4 and 8 lanes per component).  In two
# or three dimensions a tight component cannot hold 0.99 of a row's mass, so the preconditions on the near rows are not
# asked of these; the references, the defects and the tolerance are.
NARROW = ((9, 131, 2), (9, 131, 3), (9, 131, 7))
LONG = (2, 300001, 10)           # a long stream: checked for accumulation accuracy only


def sid(shape):
    return "x".join(map(str, shape))


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def near_count(S, N):
    return min(4, N // 2, S)


def make_inputs(S, N, D, seed=None):
    """fp32 ``(z [S, D], rows int64 [S], mu [N, D], logvar [N, D], logw [N])``: means (0.7 / sqrt D) randn, log variances
    -0.3 + 0.2 randn; the last ``near = min(4, N // 2, S)`` components have logvar -6 and the sample rows 0..near-1 are
    drawn from them in reverse order (their dominant component sits at the very end of the stream);
    logvar[1::5, ::7] = -12; the other rows are drawn from random components; the last row is moved +30 in three
    dimensions where S > near + 1 (the -50 floor fires far from its edge).  ``logw`` = log_softmax(randn(N)), for the
    tests that want non-uniform weights.  ``seed`` None: 1000 + D."""
    g = torch.Generator().manual_seed(1000 + D if seed is None else seed)
    mu = (0.7 / math.sqrt(D)) * torch.randn(N, D, generator=g)
    logvar = -0.3 + 0.2 * torch.randn(N, D, generator=g)
    near = near_count(S, N)
    if near:
        logvar[N - near:] = -6.0
    logvar[1::5, ::7] = -12.0
    rows = torch.randint(N, (S,), generator=g)
    for j in range(near):
        rows[j] = N - 1 - j
    z = mu[rows] + torch.randn(S, D, generator=g) * torch.exp(0.5 * logvar[rows])
    if S > near + 1:
        z[S - 1, :3] += 30.0
    logw = torch.log_softmax(torch.randn(N, generator=g), 0)
    return z, rows, mu, logvar, logw


def _lse_stale(v):
    """logsumexp over dim 1 of v [s, N, ...] by tiles of TILE with the stale_max defect: when a tile raises the running
    maximum, the sum accumulated so far is kept as it is instead of being rescaled."""
    m = torch.full_like(v[:, 0], -math.inf)
    s = torch.zeros_like(v[:, 0])
    for a in range(0, v.shape[1], TILE):
        t = v[:, a:a + TILE]
        m_new = torch.maximum(m, t.max(1).values)
        s = s + torch.exp(t - m_new.unsqueeze(1)).sum(1)
        m = m_new
    return m + torch.log(s)


def log_density(z, mu, logvar, logw=None, defect=None, chunk_elems=1 << 22):
    """``(logqz [S], lse [S, D])``: logsumexp_i(logw_i + sum_l lp[j, i, l]) and logsumexp_i(logw_i + lp[j, i, l]) with
    lp = clamp(log N(z_jl; mu_il, exp(logvar_il)), min=-50) (ops.py:24-29), in the dtype of the inputs."""
    S, D = z.shape
    N = mu.shape[0]
    lw = torch.full((N,), -math.log(N), dtype=z.dtype) if (logw is None or defect == "no_weight") else logw.to(z.dtype)
    if defect == "drop_tail":
        keep = N - (N % TILE or 1)
        mu, logvar, lw = mu[:keep], logvar[:keep], lw[:keep]
    step = max(1, chunk_elems // (mu.shape[0] * D))
    reduce = _lse_stale if defect == "stale_max" else (lambda v: torch.logsumexp(v, 1))
    logqz, lse = [], []
    for a in range(0, S, step):
        zc = z[a:a + step].unsqueeze(1)
        if defect == "clamp_outside":
            d = zc - mu.unsqueeze(0)
            lp = -0.5 * (d * d * torch.exp(-logvar.unsqueeze(0)) + logvar.unsqueeze(0) + lm.LOG_2PI)
            joint = lp.sum(2).clamp(min=lm.LOGP_FLOOR)
        else:
            lp = lm.log_density_plain(zc, mu.unsqueeze(0), logvar.unsqueeze(0))
            joint = lp.sum(2)
        logqz.append(reduce(lw.unsqueeze(0) + joint))
        lse.append(reduce(lw.view(1, -1, 1) + lp))
    return torch.cat(logqz), torch.cat(lse)


def joint_shares(z, mu, logvar, logw=None):
    """softmax_i(logw_i + sum_l lp[j, i, l]) [S, N] and the share of elements on which the floor fires, in fp64."""
    z, mu, logvar = z.double(), mu.double(), logvar.double()
    N = mu.shape[0]
    lw = torch.full((N,), -math.log(N), dtype=z.dtype) if logw is None else logw.double()
    d = z.unsqueeze(1) - mu.unsqueeze(0)
    raw = -0.5 * (d * d * torch.exp(-logvar.unsqueeze(0)) + logvar.unsqueeze(0) + lm.LOG_2PI)
    floored = float((raw < lm.LOGP_FLOOR).double().mean())
    return torch.softmax(lw + raw.clamp(min=lm.LOGP_FLOOR).sum(2), 1), floored


def per_sample(z, rows, mu, logvar, logw=None, defect=None):
    """The per-sample terms: dict of logqcx, logpz, logqz [S], lse [S, D], mi, tc, dwkl [S]."""
    logqz, lse = log_density(z, mu, logvar, logw, defect)
    logqcx = lm.log_density_plain(z, mu[rows], logvar[rows]).sum(1)
    zeros = torch.zeros_like(z)
    logpz = lm.log_density_plain(z, zeros, zeros).sum(1)
    prodm = lse.sum(1)
    return dict(logqcx=logqcx, logpz=logpz, logqz=logqz, lse=lse, mi=logqcx - logqz, tc=logqz - prodm,
                dwkl=prodm - logpz)


def decomposition(z, rows, mu, logvar, logw=None, defect=None):
    """What hipvae.aggregate.elbo_decomposition returns, from fp64 arithmetic on the given (fp32-valued) inputs, plus the
    per-sample terms under ``"per_sample"``."""
    z, mu, logvar = z.double(), mu.double(), logvar.double()
    ps = per_sample(z, rows, mu, logvar, None if logw is None else logw.double(), defect)
    zeros = torch.zeros_like(z)
    mi, tc, dwkl = float(ps["mi"].mean()), float(ps["tc"].mean()), float(ps["dwkl"].mean())
    return dict(mi=mi, tc=tc, dwkl=dwkl, kl=mi + tc + dwkl, kl_analytic=float(lm.kl_rows(logvar[rows], mu[rows]).mean()),
                joint_entropy=float(-ps["logqz"].mean()), marginal_entropies=(-ps["lse"].mean(0)).numpy(),
                dimwise_kl=(ps["lse"] - lm.log_density_plain(z, zeros, zeros)).mean(0).numpy(), per_sample=ps)
