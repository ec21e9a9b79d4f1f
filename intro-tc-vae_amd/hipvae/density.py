"""Ex-post latent density on the device: a full-covariance Gaussian mixture fitted to the encoder's latents (Ghosh et al.
2020, "From Variational to Deterministic Autoencoders", section 4; the second stage of Dai & Wipf 2019).

The sample-quality scores decode z ~ N(0, I), so they measure the decoder AND how far the aggregate posterior q(z) has
drifted from that prior.  Fitting a mixture to the latents of the training images separates the two: sample from the
mixture instead (``gmm_sample``; ``compute_sample_quality(prior="gmm")``), and read the prior mismatch directly as the gap
between the mixture's and the prior's held-out log-density (``compute_latent_density``).

The EM iteration is sklearn's ``GaussianMixture(covariance_type="full")``: E-step, M-step, ``|delta lower_bound| < tol``.
All arithmetic is fp64 in the kernels of csrc/gmm.hip (rules: include/itcv_hip.h); sklearn is not needed.  Out of scope:
other covariance types, ``n_init > 1``, Bayesian mixtures, gradients, data-parallel fitting."""
from dataclasses import dataclass, field
from math import log, pi

import numpy as np
import torch

from . import functional as HF
from .inference import device_of, eval_mode
from .quality import raise_on_nonfinite, real_features

MAX_COMPONENTS, MAX_DIM = 64, 512


@dataclass(eq=False)
class GaussianMixture:
    """A fitted mixture: fp64 device tensors ``weights [K]``, ``means [K, D]``, ``covariances [K, D, D]``, ``chol`` (the
    lower Cholesky factors), ``prec_chol`` (their inverses), ``log_det [K]``; ``lower_bound`` (the mean log-likelihood of
    the last E-step), ``n_iter``, ``converged`` and ``history`` (the mean log-likelihood of every iteration)."""
    weights: torch.Tensor
    means: torch.Tensor
    covariances: torch.Tensor
    chol: torch.Tensor
    prec_chol: torch.Tensor
    log_det: torch.Tensor
    lower_bound: float = float("-inf")
    n_iter: int = 0
    converged: bool = False
    history: list = field(default_factory=list)

    @property
    def n_components(self):
        return self.means.shape[0]

    @property
    def dim(self):
        return self.means.shape[1]


def _raise_on_pivot(info):
    for k, v in enumerate(info):
        if v:
            raise ValueError(f"fit_gmm: the covariance of component {k} is not positive definite (the Cholesky pivot of "
                             f"dimension {int(v) - 1} is not positive: a collapsed component or linearly dependent "
                             "columns); a larger reg_covar or a smaller n_components helps")


def _check_rows(x, K, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what}: x must be a [N, D] tensor")
    N, D = x.shape
    if not 1 <= K <= MAX_COMPONENTS:
        raise ValueError(f"{what}: n_components = {K} is outside 1..{MAX_COMPONENTS}")
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"{what}: D = {D} is outside 1..{MAX_DIM}")
    if N < K:
        raise ValueError(f"{what}: N = {N} rows are fewer than n_components = {K}")
    return N, D


def kmeans_init(x, n_components, kmeans_iters=10, seed=0, reg_covar=1e-6):
    """``(weights, means, covariances, centres, resp, flags)``: Lloyd's iteration through the hard E-step (identity factors, equal
    weights) from the seed rows ``np.random.RandomState(seed).choice(N, K, replace=False)``, exactly ``kmeans_iters``
    times (an empty cluster keeps its centre), then one M-step from the one-hot assignment ``resp`` to the final
    ``centres``.  ``kmeans_iters = 0`` is ``init="random"``.  Nothing is read back."""
    K = int(n_components)
    N, D = _check_rows(x, K, "fit_gmm")
    dev = x.device
    flags = HF.disent_flags(dev)
    seeds = np.random.RandomState(seed).choice(N, K, replace=False).astype(np.int64)
    centres = x.detach().index_select(0, torch.from_numpy(seeds).to(dev)).to(torch.float64).contiguous()
    ones, zeros = torch.ones((K,), dtype=torch.float64, device=dev), torch.zeros((K,), dtype=torch.float64, device=dev)
    eye = torch.eye(D, dtype=torch.float64, device=dev).expand(K, D, D).contiguous()
    for _ in range(int(kmeans_iters)):
        resp = HF.gmm_estep(x, ones, centres, eye, zeros, flags, hard=True)[1]
        nk, _, mean, _ = HF.gmm_mstep(x, resp, flags, with_cov=False)
        centres = torch.where((nk > 0.5)[:, None], mean, centres)
    resp = HF.gmm_estep(x, ones, centres, eye, zeros, flags, hard=True)[1]
    _, w, mean, cov = HF.gmm_mstep(x, resp, flags, reg=reg_covar)
    return w, mean, cov, centres, resp, flags


def fit_gmm(x, n_components=10, max_iter=100, tol=1e-3, reg_covar=1e-6, init="kmeans", kmeans_iters=10, seed=0):
    """Fit a ``GaussianMixture`` with full covariances to the fp32 device rows ``x [N, D]`` (a view with a row stride is read
    in place) by EM, as ``sklearn.mixture.GaussianMixture(covariance_type="full")``: every iteration is an E-step under the
    current parameters and an M-step from its responsibilities (``reg_covar`` added to the diagonals); it has converged when
    the mean log-likelihood of the E-step changes by less than ``tol``.  One read-back per iteration.

    ``init``: ``"kmeans"`` (``kmeans_init``), ``"random"`` (the seed rows as the centres: ``kmeans_iters = 0``) or a
    ``(weights [K], means [K, D], covariances [K, D, D])`` triple.  Limits: 1 <= K <= 64, 1 <= D <= 512, K <= N <= 2^24.
    A covariance that is not positive definite and non-finite rows raise ``ValueError``."""
    if int(max_iter) < 1:
        raise ValueError(f"fit_gmm: max_iter must be positive (got {max_iter})")
    if not reg_covar >= 0.0:
        raise ValueError(f"fit_gmm: reg_covar must be >= 0 (got {reg_covar!r})")
    if isinstance(init, str):
        if init not in ("kmeans", "random"):
            raise ValueError(f'fit_gmm: init must be "kmeans", "random" or a (weights, means, covariances) triple (got '
                             f"{init!r})")
        K = int(n_components)
        N, D = _check_rows(x, K, "fit_gmm")
        w, mean, cov, _, _, flags = kmeans_init(x, K, kmeans_iters if init == "kmeans" else 0, seed, reg_covar)
    else:
        w, mean, cov = (torch.as_tensor(t, dtype=torch.float64).to(x.device).contiguous() for t in init)
        K = mean.shape[0] if mean.dim() == 2 else 0
        N, D = _check_rows(x, K, "fit_gmm")
        if tuple(w.shape) != (K,) or tuple(mean.shape) != (K, D) or tuple(cov.shape) != (K, D, D):
            raise ValueError(f"fit_gmm: init must be (weights [K], means [K, {D}], covariances [K, {D}, {D}]) (got "
                             f"{tuple(w.shape)}, {tuple(mean.shape)}, {tuple(cov.shape)})")
        flags = HF.disent_flags(x.device)
    chol, linv, logdet, info = HF.gmm_factor(cov)
    got = torch.cat([flags[:1].to(torch.float64), info.to(torch.float64)]).tolist()
    raise_on_nonfinite(got[0])
    _raise_on_pivot(got[1:])
    history, prev, converged = [], float("-inf"), False
    for _ in range(int(max_iter)):
        _, resp, _, total = HF.gmm_estep(x, w, mean, linv, logdet, flags)
        _, w, mean, cov = HF.gmm_mstep(x, resp, flags, reg=reg_covar)
        chol, linv, logdet, info = HF.gmm_factor(cov)
        got = torch.cat([total, flags[:1].to(torch.float64), info.to(torch.float64)]).tolist()    # the one read-back
        raise_on_nonfinite(got[1])
        _raise_on_pivot(got[2:])
        bound = got[0] / N
        history.append(bound)
        if abs(bound - prev) < tol:
            converged = True
            break
        prev = bound
    return GaussianMixture(w, mean, cov, chol, linv, logdet, history[-1], len(history), converged, history)


def _estep(gmm, x):
    flags = HF.disent_flags(x.device)
    out = HF.gmm_estep(x, gmm.weights, gmm.means, gmm.prec_chol, gmm.log_det, flags)
    raise_on_nonfinite(flags.tolist()[0])
    return out


def gmm_log_prob(gmm, x):
    """fp64 ``[N]`` on the device: ``log p(x_n)`` of the fp32 device rows ``x [N, D]`` under the mixture."""
    return _estep(gmm, x)[2]


def gmm_responsibilities(gmm, x):
    """fp64 ``[N, K]`` on the device: the posterior probability of every component for every row of ``x [N, D]``."""
    return _estep(gmm, x)[1]


def gmm_sample(gmm, num, seed=0):
    """fp32 ``[num, D]`` on the device: ``z = means[c] + chol[c] eps`` with the components ``c`` from ``torch.multinomial`` on
    the read-back weights and ``eps`` from ``randn``, both from one private CPU ``torch.Generator`` seeded by ``seed``, the
    components first: torch's global generators are untouched and two calls with one seed give the same bits."""
    num = int(num)
    if num < 1:
        raise ValueError(f"gmm_sample: num must be positive (got {num})")
    gen = torch.Generator().manual_seed(int(seed))
    comp = torch.multinomial(gmm.weights.cpu(), num, replacement=True, generator=gen).to(torch.int32)
    eps = torch.randn((num, gmm.dim), generator=gen)
    dev = gmm.means.device
    flags = HF.disent_flags(dev)
    return HF.gmm_sample(gmm.means, gmm.chol, comp.to(dev), eps.to(dev), flags)


def prior_log_prob(z):
    """fp64 ``[N]``: ``log N(z_n; 0, I)`` of the rows ``z [N, D]``."""
    z = z.to(torch.float64)
    return -0.5 * (z.shape[1] * log(2.0 * pi) + (z * z).sum(1))


# ---- the learned prior of a VampSolver -------------------------------------------------------------------------------------
VAMP_CHUNK = 4096       # rows of one vamp_log_prob launch (the limit of csrc/vamp.hip), fewer when K is large


@dataclass(eq=False)
class VampPrior:
    """A VampPrior frozen for scoring: the encoder's outputs on the K pseudo-inputs, fp32 device tensors ``means`` and
    ``logvars`` [K, D].  The density is the uniform mixture (1 / K) sum_k N(z; means_k, diag exp(logvars_k))."""
    means: torch.Tensor
    logvars: torch.Tensor

    @property
    def n_components(self):
        return self.means.shape[0]

    @property
    def dim(self):
        return self.means.shape[1]


def vamp_prior(model, pseudo_inputs, batch_size=64):
    """The ``VampPrior`` of ``model`` and ``pseudo_inputs`` (a ``models.PseudoInputs``, or a [K, C, H, W] tensor): the
    encoder's (mu, logvar) of the pseudo-inputs in chunks of ``batch_size``.  The model runs in eval mode under
    ``no_grad``; its training flag is put back and its BatchNorm buffers are not written."""
    bs = int(batch_size)
    if bs < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    device = device_of(model)
    with eval_mode(model):
        u = (pseudo_inputs() if callable(pseudo_inputs) else pseudo_inputs).detach().to(device)
        if u.dim() != 4 or not u.shape[0]:
            raise ValueError(f"vamp_prior: the pseudo-inputs must be [K, C, H, W] (got {tuple(u.shape)})")
        parts = [model.encode(u[a:a + bs])[:2] for a in range(0, u.shape[0], bs)]
    return VampPrior(torch.cat([p[0] for p in parts], 0).to(torch.float32).contiguous(),
                     torch.cat([p[1] for p in parts], 0).to(torch.float32).contiguous())


def vamp_log_prob(prior, x):
    """fp64 ``[N]`` on the device: ``log p(x_n)`` of the fp32 device rows ``x [N, D]`` under the ``VampPrior``, in chunks
    of at most 4096 rows (fewer when K is large: a launch takes N K <= 2^22 pairs).  Non-finite values raise
    ``ValueError``.  One read-back."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != prior.dim:
        raise ValueError(f"vamp_log_prob: x must be a [N, {prior.dim}] tensor")
    rows = max(1, min(VAMP_CHUNK, HF.VAMP_MAX_PAIRS // prior.n_components))
    x = x.detach().to(torch.float32)
    out = torch.cat([HF.vamp_log_prob(x[a:a + rows], prior.means, prior.logvars) for a in range(0, x.shape[0], rows)])
    raise_on_nonfinite(not bool(torch.isfinite(out).all()))
    return out


def vamp_sample(prior, num, seed=0):
    """fp32 ``[num, D]`` on the device: ``z = means[c] + exp(logvars[c] / 2) eps`` with the components ``c`` from
    ``torch.randint`` and ``eps`` from ``randn``, both from one private CPU ``torch.Generator`` seeded by ``seed``, the
    components first: torch's global generators are untouched and two calls with one seed give the same bits."""
    num = int(num)
    if num < 1:
        raise ValueError(f"vamp_sample: num must be positive (got {num})")
    gen = torch.Generator().manual_seed(int(seed))
    comp = torch.randint(prior.n_components, (num,), generator=gen)
    eps = torch.randn((num, prior.dim), generator=gen)
    dev = prior.means.device
    comp = comp.to(dev)
    return prior.means.index_select(0, comp) + torch.exp(0.5 * prior.logvars.index_select(0, comp)) * eps.to(dev)


def compute_latent_density(source, model, num_fit=10000, num_eval=None, latent="mean", batch_size=64, seed=0, prior=None,
                           **fit_kw):
    """Fit a mixture to the latents of ``num_fit`` images of ``source`` (a ``DeviceImageTable`` or a dataset; no factors are
    needed) and score it on ``num_eval`` OTHER images (None: as many again, or what is left): a dict with ``gmm``,
    ``loglik_fit`` and ``loglik_heldout`` (the mean log-density of the fitted and of the held-out latents under the mixture),
    ``loglik_prior`` (the held-out mean of log N(z; 0, I)), ``gap = loglik_heldout - loglik_prior`` (nats per image: what
    the prior loses against the ex-post density), ``n_iter``, ``converged``, plus ``latents = dict(fit, heldout)`` (fp32
    device tensors) and ``indices = dict(fit, heldout)``.

    The two index sets are the sorted halves of one ``RandomState(seed).choice(len(source), num_fit + num_eval,
    replace=False)``.  ``latent``: ``"mean"`` (the encoder mean) or ``"sample"`` (mean + std * eps, eps from a private CPU
    generator seeded by ``seed``).  The latents come through ``real_features``: eval mode, no gradients, the BatchNorm
    buffers are not written.  ``fit_kw`` goes to ``fit_gmm`` (``seed`` too unless given there).  ``prior``: a ``VampPrior``
    replaces N(0, I) in ``loglik_prior`` and ``gap`` (the model's own learned prior); the result then carries ``prior``."""
    if prior is not None and not isinstance(prior, VampPrior):
        raise ValueError(f"compute_latent_density: prior must be None or a VampPrior (got {type(prior).__name__})")
    if latent not in ("mean", "sample"):
        raise ValueError(f'compute_latent_density: latent must be "mean" or "sample" (got {latent!r})')
    n = len(source)
    if n < 2:
        raise ValueError("compute_latent_density: at least two images are needed (one to fit, one held out)")
    nf = min(int(num_fit), n - 1)
    ne = min(nf if num_eval is None else int(num_eval), n - nf)
    if nf < 1 or ne < 1:
        raise ValueError(f"compute_latent_density: num_fit and num_eval must be positive (got {num_fit}, {num_eval})")
    drawn = np.random.RandomState(seed).choice(n, nf + ne, replace=False).astype(np.int64)
    idx = dict(fit=np.sort(drawn[:nf]), heldout=np.sort(drawn[nf:]))
    if latent == "mean":
        feature = "encoder"
    else:
        gen = torch.Generator().manual_seed(int(seed))
        device = device_of(model)

        def feature(images):
            mu, logvar = model.encode(images)[:2]
            return mu + torch.exp(0.5 * logvar) * torch.randn(mu.shape, generator=gen).to(device)

    z = {k: real_features(source, model, v, batch_size, feature) for k, v in idx.items()}
    fit_kw.setdefault("seed", seed)
    gmm = fit_gmm(z["fit"], **fit_kw)
    got = torch.stack([gmm_log_prob(gmm, z["fit"]).mean(), gmm_log_prob(gmm, z["heldout"]).mean(),
                       (prior_log_prob(z["heldout"]) if prior is None else vamp_log_prob(prior, z["heldout"])).mean()
                       ]).tolist()
    out = dict(gmm=gmm, loglik_fit=got[0], loglik_heldout=got[1], loglik_prior=got[2], gap=got[1] - got[2],
               n_iter=gmm.n_iter, converged=gmm.converged, latents=z, indices=idx)
    if prior is not None:
        out["prior"] = prior
    return out
