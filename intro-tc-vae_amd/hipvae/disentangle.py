"""Disentanglement scores computed on the device: MIG and modularity.

The reference's ``evaluation`` package (evaluation/metrics.py:169-219, 293-304; evaluation/utils.py:245-273, 323-335)
pulls every encoded batch to the host, bins each latent column with ``np.histogram`` / ``np.digitize`` and calls
``sklearn.metrics.mutual_info_score`` once per (latent, factor) pair.  Both scores are closed-form arithmetic on one
table -- the joint histogram of (latent bin, factor value) per pair -- so here the representations stay on the device:

    minmax -> joint histograms (integer, LDS + global atomics) -> MI[D, K], H[K] in fp64        (csrc/disent.hip)

and the two scores are a few fp64 tensor operations on MI and H.  One host read-back returns the scores together with
the two error flags.  Nothing here needs sklearn or xgboost; the classifier-based scores (beta-VAE, DCI, explicitness)
stay with the reference's package.

The binning rule is fixed (include/itcv_hip.h): with lo / hi the column's minimum / maximum as fp64 (lo -= 0.5, hi += 0.5
when they are equal), ``bin(x) = #{j in 0..bins-1 : x >= lo + j * ((hi - lo) / bins)}`` -- ``np.histogram``'s edges
followed by ``np.digitize(x, edges[:-1])``, so the column maximum lands in bin ``bins`` and the minimum in bin 1.

Degenerate inputs are not special-cased; they follow IEEE arithmetic exactly as the reference's numpy does: a factor
that takes one value has H = 0 and makes MIG ``nan`` (0 / 0) or ``inf``; a latent with no information about any factor
(theta = 0) or a single factor (K = 1) makes modularity ``nan``.  MIG of a single latent has no second-largest value and
raises, as the reference's indexing does.  Non-finite representations and factor values outside ``[0, size)`` raise
``ValueError`` (``np.histogram`` raises on the former too).
"""
import numpy as np
import torch

from . import functional as HF

__all__ = ["discretize", "factor_counts", "mutual_info", "mig_score", "modularity_score", "scores", "FactorSampler",
           "factor_representations", "compute_mig_score", "compute_modularity_score", "compute_scores"]


def _raise_on(flags):
    if flags[0]:
        raise ValueError("disentangle: the representations contain non-finite values")
    if flags[1]:
        raise ValueError("disentangle: a factor value lies outside [0, factor_size)")


def discretize(mu, bins):
    """int32 ``[N, D]`` device tensor of bin numbers in 1..bins (evaluation/utils.py:245-253)."""
    flags = HF.disent_flags(mu.device)
    mn, mx = HF.disent_minmax(mu, flags)
    out = HF.disent_bins(mu, mn, mx, bins)
    _raise_on(flags.tolist())
    return out


def _tables(mu, factors, factor_sizes, bins, flags, minmax=None):
    mn, mx = minmax if minmax is not None else HF.disent_minmax(mu, flags)
    return HF.disent_hist(mu, factors, factor_sizes, mn, mx, bins, flags)


def _mutual_info(mu, factors, factor_sizes, bins, flags, minmax=None):
    counts, vcount = _tables(mu, factors, factor_sizes, bins, flags, minmax)
    return HF.disent_mi(counts, vcount, mu.shape[0], mu.shape[1], factor_sizes, bins)


def factor_counts(mu, factors, factor_sizes, bins):
    """The integer tables: a list of K tensors ``[D, bins, size_k]`` (samples with latent d in bin b + 1 and factor k at
    value f) and a list of K marginals ``[size_k]``.  uint32 counts, returned as int32 tensors."""
    flags = HF.disent_flags(mu.device)
    counts, vcount = _tables(mu, factors, factor_sizes, bins, flags)
    _raise_on(flags.tolist())
    sizes = [int(s) for s in factor_sizes]
    D, bins = mu.shape[1], int(bins)
    per_d = counts.view(D, bins * sum(sizes))
    joint, marg, off = [], [], 0
    for s in sizes:
        joint.append(per_d[:, bins * off:bins * (off + s)].reshape(D, bins, s))
        marg.append(vcount[off:off + s])
        off += s
    return joint, marg


def mutual_info(mu, factors, factor_sizes, bins):
    """``(MI [D, K], H [K])`` as fp64 device tensors, in nats (evaluation/utils.py:256-273)."""
    flags = HF.disent_flags(mu.device)
    mi, h = _mutual_info(mu, factors, factor_sizes, bins, flags)
    _raise_on(flags.tolist())
    return mi, h


def _mig(mi, h):
    """mean_k (top1_k - top2_k) / H[k] over the latents (evaluation/metrics.py:215-219)."""
    if mi.shape[0] < 2:
        raise IndexError("MIG needs at least two latents (there is no second-largest mutual information)")
    top = mi.topk(2, dim=0).values
    return ((top[0] - top[1]) / h).mean()


def _modularity(mi):
    """evaluation/utils.py:323-335: the template keeps each latent's largest MI at its first argmax."""
    theta, idx = mi.max(dim=1, keepdim=True)
    template = torch.zeros_like(mi).scatter_(1, idx, theta)
    deltas = ((mi - template) ** 2).sum(dim=1) / (theta[:, 0] ** 2 * (mi.shape[1] - 1))
    return (1 - deltas).mean()


def _read(values, flags):
    """The one host read-back: the score scalars and the two flags."""
    out = torch.cat([torch.stack(values), flags.to(torch.float64)]).tolist()
    _raise_on(out[-2:])
    return out[:-2]


def mig_score(mu, factors, factor_sizes, bins=10):
    flags = HF.disent_flags(mu.device)
    mi, h = _mutual_info(mu, factors, factor_sizes, bins, flags)
    return _read([_mig(mi, h)], flags)[0]


def modularity_score(mu, factors, factor_sizes, bins=20):
    flags = HF.disent_flags(mu.device)
    mi, _ = _mutual_info(mu, factors, factor_sizes, bins, flags)
    return _read([_modularity(mi)], flags)[0]


def scores(mu, factors, factor_sizes, mig_bins=10, modularity_bins=20):
    """Both scores of one set of representations: ``{"mig": float, "modularity": float}``.  The scores use different bin
    counts, so the histogram pass runs twice over the same ``mu`` (one minmax pass, one read-back)."""
    flags = HF.disent_flags(mu.device)
    minmax = HF.disent_minmax(mu, flags)
    mi, h = _mutual_info(mu, factors, factor_sizes, mig_bins, flags, minmax)
    mi2 = mi if int(modularity_bins) == int(mig_bins) else \
        _mutual_info(mu, factors, factor_sizes, modularity_bins, flags, minmax)[0]
    mig, mod = _read([_mig(mi, h), _modularity(mi2)], flags)
    return {"mig": mig, "modularity": mod}


class FactorSampler:
    """Draws ground-truth factor vectors and looks up the images they generate, for a dataset ordered by its factors
    (``dataset.factor_sizes``: the size of every factor, most significant first; ``dataset.latent_indices``: the factors
    that vary).  Offers what the scores need of the reference's ``LatentGenerator``: ``factor_sizes``,
    ``latent_indices``, ``num_latents``, ``sample_factors_of_variation``, ``sample_observations_from_factors``,
    ``sample`` and ``generate``.  All randomness comes from a private ``np.random.RandomState(seed)``."""

    def __init__(self, dataset, device, seed=None):
        self.data_source, self.device, self.seed = dataset, device, seed
        self.factor_sizes = [int(s) for s in dataset.factor_sizes]
        self.latent_indices = [int(i) for i in dataset.latent_indices]
        self.num_factors, self.num_latents = len(self.factor_sizes), len(self.latent_indices)
        self.observed_factor_indices = [i for i in range(self.num_factors) if i not in self.latent_indices]
        # place value of factor i in the image index: the product of the sizes of the less significant factors
        self.factor_bases = [int(np.prod(self.factor_sizes[i + 1:], dtype=np.int64)) for i in range(self.num_factors)]
        self.random_state = np.random.RandomState(seed)

    @property
    def latent_factor_sizes(self):
        return [self.factor_sizes[i] for i in self.latent_indices]

    def sample_factors_of_variation(self, n):
        """int64 ``[n, num_latents]``: column j is uniform over the values of factor ``latent_indices[j]``."""
        out = np.empty((n, self.num_latents), dtype=np.int64)
        for j, i in enumerate(self.latent_indices):
            out[:, j] = self.random_state.randint(self.factor_sizes[i], size=n)
        return out

    def indices_from_factors(self, factors):
        """Image index of every row: the varying factors as given, the remaining ones drawn at random, read as one
        mixed-radix number with the first factor most significant."""
        factors = np.asarray(factors)
        full = np.empty((len(factors), self.num_factors), dtype=np.int64)
        full[:, self.latent_indices] = factors
        for i in self.observed_factor_indices:
            full[:, i] = self.random_state.randint(self.factor_sizes[i], size=len(factors))
        return full @ np.asarray(self.factor_bases, dtype=np.int64)

    def sample_observations_from_factors(self, factors):
        idx = self.indices_from_factors(factors)
        return torch.stack([self.data_source[int(i)][0] for i in idx], 0).to(self.device)

    def sample(self, n):
        factors = self.sample_factors_of_variation(n)
        return factors, self.sample_observations_from_factors(factors)

    def generate(self, n_samples=1000, batch_size=64, drop_last=False):
        sizes = [batch_size] * (n_samples // batch_size)
        if not drop_last and n_samples % batch_size:
            sizes.append(n_samples % batch_size)
        for n in sizes:
            yield self.sample(n)


def _latent_sizes(generator):
    return [int(generator.factor_sizes[i]) for i in generator.latent_indices]


def factor_representations(sampler, model, num_samples, batch_size):
    """``(mu [N, D] fp32, factors [N, K] int32)`` on the device: ``model.encode`` of ``num_samples`` sampled images, batch
    by batch, in eval mode and without gradients (evaluation/utils.py:14-56).  Every batch's means are written into one
    preallocated buffer; nothing is read back.  ``sampler``: a ``FactorSampler`` or the reference's generator."""
    was_training = model.training
    model.eval()
    mu, factors, row = None, [], 0
    try:
        with torch.no_grad():
            for f, obs in sampler.generate(num_samples, batch_size, drop_last=False):
                m, _ = model.encode(obs)
                if mu is None:
                    mu = torch.empty((num_samples, m.shape[1]), dtype=m.dtype, device=m.device)
                mu[row:row + m.shape[0]].copy_(m)
                row += m.shape[0]
                factors.append(np.asarray(f))
    finally:
        model.train(was_training)
    if mu is None or row != num_samples:
        raise ValueError(f"factor_representations: the sampler produced {row} of {num_samples} samples")
    v = torch.from_numpy(np.concatenate(factors, 0).astype(np.int32)).to(mu.device)
    return mu, v


def compute_mig_score(latent_generator, model, num_samples=10000, batch_size=64, params=None):
    """evaluation/metrics.py:169-219 with the reference's argument names; a Python float."""
    bins = (params or {}).get("bins", 10)
    mu, v = factor_representations(latent_generator, model, num_samples, batch_size)
    return mig_score(mu, v, _latent_sizes(latent_generator), bins)


def compute_modularity_score(latent_generator, model, num_samples=10000, batch_size=64, params=None):
    """The modularity half of evaluation/metrics.py:237-304 (explicitness needs logistic regression: not here)."""
    bins = (params or {}).get("bins", 20)
    mu, v = factor_representations(latent_generator, model, num_samples, batch_size)
    return modularity_score(mu, v, _latent_sizes(latent_generator), bins)


def compute_scores(latent_generator, model, num_samples=10000, batch_size=64, params=None):
    """Both scores from ONE encode of ``num_samples`` images: ``{"mig": float, "modularity": float}``
    (``params``: ``mig_bins`` / ``modularity_bins``)."""
    params = params or {}
    mu, v = factor_representations(latent_generator, model, num_samples, batch_size)
    return scores(mu, v, _latent_sizes(latent_generator), params.get("mig_bins", 10), params.get("modularity_bins", 20))
