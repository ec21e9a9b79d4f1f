"""Sample quality on the device: how good, and how varied, are the images a model generates?  Five families of scores of
generated ("fake") against real feature rows, from the kernels of csrc/quality.hip (rules: include/itcv_hip.h):

* ``frechet_distance``: the Frechet distance of the two Gaussians fitted to the features (Heusel et al. 2017);
* ``kernel_distance``: the unbiased MMD^2 under the cubic polynomial kernel (KID, Binkowski et al. 2018);
* ``prdc``: precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020), the `prdc`
  package's definitions over k-th-neighbour radii;
* ``sliced_wasserstein_distance``: the sliced-Wasserstein distance over random directions (Deshpande et al. 2018), from
  the kernels of csrc/sw.hip; ``compute_sliced_wasserstein`` over the same features, or between encoder samples and
  the prior.

The features are pluggable.  The default is the model's own encoder mean, so the records are ``frechet`` and ``kid`` over
THAT feature map: they rank models that share an encoder architecture and are NOT comparable with a published FID, which
is defined over Inception features.  A callable ``feature(images) -> [B, D]`` replaces the encoder.

Pixel space, for reconstructions rather than samples: ``reconstruction_quality`` gives PSNR, SSIM (Wang et al. 2004) and
MS-SSIM (Wang et al. 2003) per image from the kernels of csrc/ssim.hip, ``compute_reconstruction_quality`` their means
over a dataset."""
import numpy as np
import torch
import torch.nn.functional as F

from . import functional as HF
from .inference import device_of, draw_indices, eval_mode, images

FRECHET_MAX_DIM = 512
SCORES = ("frechet", "kid", "prdc")


def raise_on_nonfinite(flag):
    if flag:
        raise ValueError("quality: the features contain non-finite values")


def knn_radius(x, k, splits=0):
    """fp64 ``[N]`` on the device: the squared distance from every row of ``x [N, D]`` to its k-th nearest neighbour among
    the other rows (the (k + 1)-th smallest of the row's distances, its own 0 included: ``prdc``'s
    ``get_kth_value(dist, k + 1)``, squared).  One read-back (the non-finite flag)."""
    flags = HF.disent_flags(x.device)
    r2 = HF.knn_radius(x, k, flags, splits)
    raise_on_nonfinite(flags.tolist()[0])
    return r2


def prdc_counts(real, fake, nearest_k=5, splits=0):
    """The integers the four scores are made of, as device tensors: ``dict(r2_real [N], r2_fake [M], fake_hits [M],
    real_covered [N], real_min [N])`` and the ``counts`` [5] int64 = (fakes with a hit, reals covered, hits, reals whose
    nearest fake is inside their radius, the non-finite flag).  Nothing is read back."""
    flags = HF.disent_flags(real.device)
    r2r, r2f = HF.knn_radius(real, nearest_k, flags, splits), HF.knn_radius(fake, nearest_k, flags, splits)
    hits, covered, rmin = HF.prdc_counts(real, fake, r2r, r2f, flags, splits)
    i64 = torch.int64
    counts = torch.stack([(hits > 0).sum(), covered.sum(dtype=i64), hits.sum(dtype=i64), (rmin < r2r).sum(),
                          flags[0].to(i64)])
    return dict(r2_real=r2r, r2_fake=r2f, fake_hits=hits, real_covered=covered, real_min=rmin, counts=counts)


def prdc(real, fake, nearest_k=5):
    """``dict(precision, recall, density, coverage)`` of ``fake [M, D]`` against ``real [N, D]``: exact fractions of
    integer counts (every comparison strict, as in ``prdc``).  One read-back."""
    nearest_k = int(nearest_k)
    c = prdc_counts(real, fake, nearest_k)["counts"].tolist()           # the one read-back
    raise_on_nonfinite(c[4])
    N, M = real.shape[0], fake.shape[0]
    return dict(precision=c[0] / M, recall=c[1] / N, density=c[2] / (nearest_k * M), coverage=c[3] / N)


_FRECHET_KEYS = ("frechet", "mean_term", "trace_real", "trace_fake", "trace_sqrt")


def _frechet_once(m1, c1, m2, c2, eps):
    res, eig, info = HF.frechet(m1, c1, m2, c2, eps)
    return torch.cat([res, info.to(torch.float64)]).tolist(), eig


def frechet_distance(real, fake, eps=0.0):
    """``dict(frechet, mean_term, trace_real, trace_fake, trace_sqrt, eigenvalues)`` of the Gaussians fitted to ``real
    [N, D]`` and ``fake [M, D]``: |m1 - m2|^2 + tr C1 + tr C2 - 2 tr sqrt(C1 C2), with C + eps I for both covariances.
    The Cholesky factor of the first covariance is needed; when its pivot fails the roles are exchanged (the trace is
    symmetric, and a singular second covariance is fine).  Both failing raises ``ValueError``."""
    D = real.shape[1] if real.dim() == 2 else 0
    if D > FRECHET_MAX_DIM:
        raise ValueError(f"frechet_distance: D = {D} features are above the limit of {FRECHET_MAX_DIM}")
    if not eps >= 0.0:
        raise ValueError(f"frechet_distance: eps must be >= 0 (got {eps!r})")
    flags = HF.disent_flags(real.device)
    (m1, c1), (m2, c2) = HF.unsup_cov(real, flags), HF.unsup_cov(fake, flags)
    out, eig = _frechet_once(m1, c1, m2, c2, eps)
    raise_on_nonfinite(flags.tolist()[0])
    swapped = False
    if out[5]:
        first = int(out[6])
        out, eig = _frechet_once(m2, c2, m1, c1, eps)
        swapped = True
        if out[5]:
            raise ValueError(f"frechet_distance: neither covariance is positive definite (the Cholesky pivot of dimension "
                             f"{first} of the real features and of dimension {int(out[6])} of the fake ones is not "
                             "positive: constant or linearly dependent columns); eps > 0 regularises both")
    if out[7]:
        raise RuntimeError("frechet_distance: the Jacobi iteration did not converge in 60 sweeps")
    if swapped:
        out[2], out[3] = out[3], out[2]
    got = dict(zip(_FRECHET_KEYS, out[:5]))
    got["eigenvalues"] = eig
    return got


def kernel_distance(real, fake, degree=3, gamma=None, coef0=1.0, subset_size=None, num_subsets=100, seed=0):
    """``dict(kid, kid_std)``: the unbiased MMD^2 of ``real [N, D]`` and ``fake [M, D]`` under (gamma a.b + coef0)^degree
    (gamma None: 1 / D).  ``subset_size`` None: the estimator over the full samples, ``kid_std`` 0.0.  Otherwise the mean and
    the (ddof = 0) standard deviation over ``num_subsets`` pairs of subsets of that size, drawn without replacement by a
    private ``np.random.RandomState(seed)`` (reals first, then fakes, per subset) and gathered by ``index_select``."""
    g = 0.0 if gamma is None else float(gamma)
    flags = HF.disent_flags(real.device)
    if subset_size is None:
        res = [HF.poly_mmd(real, fake, flags, degree, g, coef0)[3]]
    else:
        m = int(subset_size)
        if not 2 <= m <= min(real.shape[0], fake.shape[0]) or int(num_subsets) < 1:
            raise ValueError(f"kernel_distance: subset_size must lie in 2..min(N, M) and num_subsets be positive (got "
                             f"{subset_size!r}, {num_subsets!r})")
        rs = np.random.RandomState(seed)
        res = []
        for _ in range(int(num_subsets)):
            ir = torch.from_numpy(rs.choice(real.shape[0], m, replace=False).astype(np.int64)).to(real.device)
            jf = torch.from_numpy(rs.choice(fake.shape[0], m, replace=False).astype(np.int64)).to(real.device)
            res.append(HF.poly_mmd(real.index_select(0, ir), fake.index_select(0, jf), flags, degree, g, coef0)[3])
    vals = torch.stack(res)
    out = torch.cat([vals.mean().reshape(1), vals.std(unbiased=False).reshape(1) if len(res) > 1 else vals.new_zeros(1),
                     flags[:1].to(torch.float64)]).tolist()
    raise_on_nonfinite(out[2])
    return dict(kid=out[0], kid_std=out[1])


# ---- features ------------------------------------------------------------------------------------------------------------
def _feature_fn(model, feature):
    if callable(feature):
        return feature
    if feature != "encoder":
        raise ValueError(f'feature must be "encoder" or a callable images -> [B, D] (got {feature!r})')
    return lambda images: model.encode(images)[0]


def _collect(model, batches, feature):
    """The rows ``feature(images)`` of every batch in one fp32 [N, D] device tensor, under ``inference.eval_mode``."""
    fn = _feature_fn(model, feature)
    rows = []
    with eval_mode(model):
        for batch in batches():
            f = fn(batch)
            if not isinstance(f, torch.Tensor) or f.dim() != 2 or not f.is_floating_point():
                raise ValueError("feature(images) must return a floating-point [B, D] tensor")
            rows.append(f.detach().to(torch.float32))
    return torch.cat(rows, 0).contiguous()


def real_features(source, model, indices, batch_size=64, feature="encoder"):
    """fp32 ``[N, D]`` on the device: the features of the images of ``source`` (a ``DeviceImageTable`` or a dataset) at
    ``indices``, batch by batch.  The model runs in eval mode under ``no_grad``; its training flag is put back and its
    BatchNorm buffers are not written."""
    indices = np.asarray(indices, dtype=np.int64)
    if indices.ndim != 1 or not len(indices):
        raise ValueError("real_features: indices must be a non-empty 1-D integer array")
    device, bs = device_of(model), int(batch_size)
    if bs < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    return _collect(model, lambda: (images(source, indices[a:a + bs], device) for a in range(0, len(indices), bs)), feature)


def generated_features(model, num, batch_size=64, seed=0, feature="encoder", prior=None):
    """fp32 ``[num, D]`` on the device: the features of ``model.decode(z)``, z ~ N(0, I) from a private CPU
    ``torch.Generator`` seeded by ``seed``, one draw per batch in a fixed order: torch's global generators are untouched
    and two calls with one seed give the same bits.  Same contract for the model as ``real_features``.  ``prior``: a
    ``hipvae.density.GaussianMixture`` whose ``gmm_sample(prior, num, seed)`` replaces the normal draws, or a
    ``hipvae.density.VampPrior`` (``vamp_sample``)."""
    num, bs = int(num), int(batch_size)
    if num < 1 or bs < 1:
        raise ValueError(f"num and batch_size must be positive (got {num}, {batch_size})")
    device = device_of(model)
    zdim = model.zdim
    if prior is None:
        gen = torch.Generator().manual_seed(int(seed))

        def batches():
            for a in range(0, num, bs):
                z = torch.randn((min(bs, num - a), zdim), generator=gen).to(device)
                yield model.decode(z)
    else:
        from . import density
        if isinstance(prior, density.VampPrior) and prior.dim == zdim:
            zs = density.vamp_sample(prior, num, seed)
        elif not isinstance(prior, density.GaussianMixture) or prior.dim != zdim:
            raise ValueError(f"generated_features: prior must be None or a GaussianMixture over the model's {zdim} latent "
                             "dimensions")
        else:
            zs = density.gmm_sample(prior, num, seed)

        def batches():
            for a in range(0, num, bs):
                yield model.decode(zs[a:a + bs])

    return _collect(model, batches, feature)


def compute_sample_quality(source, model, num_real=10000, num_fake=None, feature="encoder", nearest_k=5, batch_size=64,
                           seed=0, scores=SCORES, eps=0.0, indices=None, kid_subset_size=None, prior="normal",
                           gmm_params=None):
    """The sample-quality scores of ``model`` on ``source`` (a ``DeviceImageTable`` or a dataset; no factors are needed): a
    flat dict with ``frechet`` ("frechet" in ``scores``), ``kid`` and ``kid_std`` ("kid") and ``precision``, ``recall``,
    ``density``, ``coverage`` ("prdc"), plus ``features = dict(real, fake)`` (fp32 device tensors) and the ``indices`` used.

    Real images: ``indices``, or ``inference.draw_indices(len(source), num_real, seed)``: a sorted draw without replacement,
    or all of them when ``num_real >= len(source)``.  Fakes: ``num_fake`` (None: as many as real images) decoded prior
    samples, ``generated_features(model, num_fake, batch_size, seed, feature)``.  The default feature is the model's own encoder
    mean, so the numbers compare models of one architecture and are not a published FID / KID.  The Frechet distance
    needs D <= 512; ``eps`` regularises its covariances.

    ``prior``: ``"normal"``, or ``"gmm"``: the fakes are decoded from an ex-post density instead (hipvae.density), a Gaussian
    mixture fitted to the real images' latents ``model.encode(x)[0]`` (whatever ``feature`` is) by ``fit_gmm(latents,
    **gmm_params)`` (``seed`` unless given there) and sampled by ``gmm_sample(gmm, num_fake, seed)``; a ``GaussianMixture``
    instance is used as given.  The result then carries ``gmm`` too.  The scores of the two priors differ by what the
    drift of the aggregate posterior from N(0, I) costs.  A ``hipvae.density.VampPrior`` instance -- the learned prior of a
    ``VampSolver`` -- is sampled by ``vamp_sample(prior, num_fake, seed)``; the result then carries ``prior``."""
    unknown = [s for s in scores if s not in SCORES]
    if unknown:
        raise ValueError(f"compute_sample_quality: unknown score(s) {unknown} (known: {', '.join(map(repr, SCORES))})")
    gmm = vamp = None
    if not isinstance(prior, str):
        from . import density
        if isinstance(prior, density.VampPrior):
            vamp = prior
        else:
            gmm = prior
    elif prior not in ("normal", "gmm"):
        raise ValueError(f'compute_sample_quality: prior must be "normal", "gmm" or a GaussianMixture (got {prior!r})')
    if indices is None:
        indices = draw_indices(len(source), num_real, seed)
    indices = np.asarray(indices, dtype=np.int64)
    real = real_features(source, model, indices, batch_size, feature)
    if isinstance(prior, str) and prior == "gmm":
        from . import density
        latents = real if feature == "encoder" else real_features(source, model, indices, batch_size)
        gmm = density.fit_gmm(latents, **{"seed": seed, **(gmm_params or {})})
    fake = generated_features(model, len(indices) if num_fake is None else num_fake, batch_size, seed, feature,
                              gmm if vamp is None else vamp)
    out = {}
    if gmm is not None:
        out["gmm"] = gmm
    if vamp is not None:
        out["prior"] = vamp
    if "frechet" in scores:
        out["frechet"] = frechet_distance(real, fake, eps)["frechet"]
    if "kid" in scores:
        out.update(kernel_distance(real, fake, subset_size=kid_subset_size, seed=seed))
    if "prdc" in scores:
        out.update(prdc(real, fake, nearest_k))
    out["features"] = dict(real=real, fake=fake)
    out["indices"] = indices
    return out


# ---- the sliced-Wasserstein distance ----------------------------------------------------------------------------------
def sliced_wasserstein_directions(num_projections, dim, seed=0):
    """fp32 ``[num_projections, dim]`` N(0, I) draws from a private CPU ``torch.Generator`` seeded by ``seed`` (the kernel
    normalises the rows): torch's global generators are untouched."""
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randn((int(num_projections), int(dim)), generator=gen)


def sliced_wasserstein_distance(real, fake, num_projections=1024, seed=0):
    """``dict(swd, sw2, sw2_std, per)`` of the sliced-Wasserstein distance (Deshpande et al. 2018; csrc/sw.hip) between
    the fp32 device rows ``real [N, D]`` and ``fake [N, D]`` -- equal counts -- over ``num_projections`` random
    directions: ``sw2`` the mean over the directions of the squared 1-D Wasserstein-2 distances ``per`` (an fp64 device
    tensor), ``swd`` its square root, ``sw2_std`` the standard error of that mean over the directions (ddof = 1; 0.0 for
    one direction).  The directions are ``sliced_wasserstein_directions(num_projections, D, seed)``: the same seed gives
    the same bits.  One read-back."""
    if real.dim() != 2 or fake.shape != real.shape:
        raise ValueError(f"sliced_wasserstein_distance: real and fake must share one [N, D] shape: the distance pairs sorted "
                         f"samples of equal counts (got {tuple(real.shape)}, {tuple(fake.shape)})")
    L = int(num_projections)
    if not 1 <= L <= 4096:
        raise ValueError(f"sliced_wasserstein_distance: num_projections must lie in 1..4096 (got {num_projections!r})")
    t = sliced_wasserstein_directions(L, real.shape[1], seed).to(real.device)
    _, per = HF.sw_distance(real, fake, t)
    sw2 = per.sum() / L                                  # the kernel's own fold is fp32 once stored: this one stays fp64
    se = per.std(unbiased=True) / L ** 0.5 if L > 1 else per.new_zeros(())
    sw2, se = torch.stack([sw2, se]).tolist()            # the one read-back
    if not np.isfinite(sw2):
        raise ValueError("quality: the features contain non-finite values")
    return dict(swd=float(np.sqrt(sw2)), sw2=sw2, sw2_std=se, per=per)


def compute_sliced_wasserstein(source, model, num=10000, space="feature", prior=None, num_projections=1024, feature="encoder",
                               batch_size=64, seed=0, indices=None, gmm_params=None):
    """The sliced-Wasserstein distance of ``model`` on ``source``: ``sliced_wasserstein_distance``'s dict plus ``indices``
    and, for a fitted or given prior, ``gmm`` / ``prior`` as in ``compute_sample_quality``.

    ``space="feature"``: the features of ``num`` real images (``indices``, or ``inference.draw_indices``) against those
    of as many decoded prior samples -- the usual companion of Frechet / KID, over the same pluggable feature map
    (``real_features`` / ``generated_features``).  ``space="latent"``: as many samples of the encoder z = mu +
    eps exp(logvar / 2), eps from a private CPU generator, against as many prior samples: q(z) against p(z) read
    directly, without fitting a density first.  ``prior``: None or ``"normal"`` (N(0, I)), ``"gmm"`` (a mixture fitted to
    the real images' latents, ``fit_gmm(latents, **gmm_params)``), a ``GaussianMixture`` or a ``VampPrior``."""
    from . import density
    if space not in ("feature", "latent"):
        raise ValueError(f'compute_sliced_wasserstein: space must be "feature" or "latent" (got {space!r})')
    if prior is not None and not isinstance(prior, (density.GaussianMixture, density.VampPrior)) \
            and prior not in ("normal", "gmm"):
        raise ValueError('compute_sliced_wasserstein: prior must be None, "normal", "gmm", a GaussianMixture or a VampPrior '
                         f"(got {prior!r})")
    if indices is None:
        indices = draw_indices(len(source), num, seed)
    indices = np.asarray(indices, dtype=np.int64)
    n, out = len(indices), {}
    if isinstance(prior, str) and prior == "gmm":
        prior = density.fit_gmm(real_features(source, model, indices, batch_size), **{"seed": seed, **(gmm_params or {})})
    if isinstance(prior, density.GaussianMixture):
        out["gmm"] = prior
    elif isinstance(prior, density.VampPrior):
        out["prior"] = prior
    else:
        prior = None
    if space == "feature":
        real = real_features(source, model, indices, batch_size, feature)
        fake = generated_features(model, n, batch_size, seed, feature, prior)
    else:
        gen = torch.Generator().manual_seed(int(seed))

        def sample(x):
            mu, logvar = model.encode(x)[:2]
            return mu + torch.randn(mu.shape, generator=gen).to(mu.device) * torch.exp(0.5 * logvar)

        real = real_features(source, model, indices, batch_size, sample)
        if prior is None:
            fake = torch.randn((n, real.shape[1]), generator=gen).to(real.device)
        elif isinstance(prior, density.VampPrior):
            fake = density.vamp_sample(prior, n, seed)
        else:
            fake = density.gmm_sample(prior, n, seed)
        fake = fake.to(torch.float32)
    out.update(sliced_wasserstein_distance(real, fake, num_projections, seed))
    out["indices"] = indices
    return out


# ---- reconstructions: PSNR, SSIM, MS-SSIM --------------------------------------------------------------------------------
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)       # Wang et al. 2003, finest level first
RECONSTRUCTION_SCORES = ("psnr", "ssim", "ms_ssim", "mse", "l1")


def ms_ssim_levels(H, W, window=11):
    """The largest L <= 5 such that the coarsest of L levels, ``min(H, W) >> (L - 1)``, still holds one window."""
    if min(H, W) < window:
        raise ValueError(f"reconstruction_quality: H, W = {H}, {W} are below window = {window}")
    L = 1
    while L < len(MS_SSIM_WEIGHTS) and (min(H, W) >> L) >= window:
        L += 1
    return L


def reconstruction_quality(x, y, window=11, sigma=1.5, levels=None):
    """Per-image scores of the reconstructions ``y`` of ``x`` (fp32 [B, C, H, W] on the device, values in [0, 1]): a dict of
    fp64 device vectors [B], nothing is read back.

    ``mse`` and ``l1`` are the means over the image of (y - x)^2 and |y - x|; ``psnr`` = 10 log10(1 / mse), inf for an exact
    reconstruction; ``ssim`` the mean over channels and positions of the SSIM map (``ops.ssim_loss``'s definition).
    ``ms_ssim``: with (ssim_l, cs_l) the per-channel means of ``HF.ssim_stats`` at level l, level l + 1 being both images
    halved by a 2 x 2 mean (``F.avg_pool2d``, an odd last row or column dropped),
        prod_{l < L - 1} max(cs_l, 0)^{w_l} * max(ssim_{L-1}, 0)^{w_{L-1}},   averaged over channels,
    w the first L = ``levels`` of ``MS_SSIM_WEIGHTS`` renormalised to sum 1.  ``levels`` None: ``ms_ssim_levels``, the most
    that the image size allows, 5 from 176 pixels on."""
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"reconstruction_quality: x and y must be [B, C, H, W] images of one shape (got {tuple(x.shape)}, "
                         f"{tuple(y.shape)})")
    x, y = x.detach(), y.detach()
    H, W = x.shape[2:]
    most = ms_ssim_levels(H, W, int(window))
    L = most if levels is None else int(levels)
    if L < 1 or L > most:
        raise ValueError(f"reconstruction_quality: levels must lie in 1..{most} for {H} x {W} images and window = {window} "
                         f"(got {levels})")
    d = y.to(torch.float64) - x.to(torch.float64)
    mse, l1 = (d * d).flatten(1).mean(1), d.abs().flatten(1).mean(1)
    w = torch.tensor(MS_SSIM_WEIGHTS[:L], dtype=torch.float64)
    w = (w / w.sum()).tolist()
    ms = ssim = None
    xl, yl = x, y
    for lev in range(L):
        if lev:
            xl, yl = F.avg_pool2d(xl, 2), F.avg_pool2d(yl, 2)
        st = HF.ssim_stats(xl, yl, window, sigma)                       # [B, C, 2]
        if lev == 0:
            ssim = st[:, :, 0].mean(1)
        term = st[:, :, 0 if lev == L - 1 else 1].clamp_min(0.0) ** w[lev]
        ms = term if ms is None else ms * term
    return dict(psnr=10.0 * torch.log10(1.0 / mse), ssim=ssim, ms_ssim=ms.mean(1), mse=mse, l1=l1)


def compute_reconstruction_quality(source, model, num=10000, batch_size=64, seed=0, indices=None, **kw):
    """The means of ``reconstruction_quality`` over images of ``source`` (a ``DeviceImageTable`` or a dataset; no factors are
    needed) and their deterministic reconstructions ``model.decode(model.encode(x)[0])``: a dict with ``psnr``, ``ssim``,
    ``ms_ssim``, ``mse``, ``l1`` (Python floats), ``per_image`` (the five fp64 device vectors) and the ``indices`` used --
    ``indices``, or ``inference.draw_indices(len(source), num, seed)``.  ``kw`` goes to ``reconstruction_quality``.  The
    model runs in eval mode under ``no_grad``; its training flag is put back and its BatchNorm buffers are not written.  ``psnr``
    is the mean of the per-image values (inf as soon as one image is reconstructed exactly)."""
    if indices is None:
        indices = draw_indices(len(source), num, seed)
    indices = np.asarray(indices, dtype=np.int64)
    if indices.ndim != 1 or not len(indices):
        raise ValueError("compute_reconstruction_quality: indices must be a non-empty 1-D integer array")
    device, bs = device_of(model), int(batch_size)
    if bs < 1:
        raise ValueError(f"batch_size must be positive (got {batch_size})")
    parts = {k: [] for k in RECONSTRUCTION_SCORES}
    with eval_mode(model):
        for a in range(0, len(indices), bs):
            x = images(source, indices[a:a + bs], device)
            got = reconstruction_quality(x, model.decode(model.encode(x)[0]), **kw)
            for k in RECONSTRUCTION_SCORES:
                parts[k].append(got[k])
    per_image = {k: torch.cat(v, 0) for k, v in parts.items()}
    out = {k: float(v.mean()) for k, v in per_image.items()}
    out["per_image"] = per_image
    out["indices"] = indices
    return out
