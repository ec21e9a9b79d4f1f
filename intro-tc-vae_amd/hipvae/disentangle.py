"""Disentanglement scores computed on the device: MIG, modularity, beta-VAE, explicitness, DCI, FactorVAE and SAP.

The reference's ``evaluation`` package (evaluation/metrics.py:169-219, 293-304; evaluation/utils.py:245-273, 323-335)
pulls every encoded batch to the host, bins each latent column with ``np.histogram`` / ``np.digitize`` and calls
``sklearn.metrics.mutual_info_score`` once per (latent, factor) pair.  Both scores are closed-form arithmetic on one
table -- the joint histogram of (latent bin, factor value) per pair -- so here the representations stay on the device:

    minmax -> joint histograms (integer, LDS + global atomics) -> MI[D, K], H[K] in fp64        (csrc/disent.hip)

and the two scores are a few fp64 tensor operations on MI and H.  One host read-back returns the scores together with
the two error flags.  Nothing here needs sklearn or xgboost.

The beta-VAE score (evaluation/metrics.py:20-79, utils.py:60-174) and explicitness (metrics.py:237-304,
utils.py:277-320) are classifier-based, but they are mathematics too: each is read off the optimum of an L2-regularised
softmax regression (C = 1), which is strictly convex in the weights and so does not depend on the solver.  The rule is
in include/itcv_hip.h; csrc/logreg.hip evaluates all K problems in one launch in fp64, hipvae/logreg.py minimises them
to ``max|grad F_p| <= gtol`` for every problem (or raises), accuracy comes from the predictions and one-vs-rest ROC AUC
from integer pair counts.

DCI (evaluation/metrics.py:82-161, utils.py:178-241) needs a gradient-boosted tree classifier per factor; the reference
asks xgboost for ``tree_method="gpu_hist"``.  Here the booster is a fixed rule after xgboost's documented ``hist``
algorithm and defaults (include/itcv_hip.h; csrc/gbt.hip, hipvae/gbt.py): quantile cuts, uint8 bins, gradients
quantised to integers so that every histogram is an exact, order-free integer sum and a fit is bitwise reproducible.
Informativeness is the mean test accuracy; completeness and disentanglement are the reference's closed forms
(utils.py:220-241 with ops.entropy, eps = 1e-9) on the ``[K, D]`` matrix of xgboost's ``gain`` importances, a few fp64
tensor operations.  With that, no score of the reference's writer needs its ``evaluation`` package.

The binning rule is fixed (include/itcv_hip.h): with lo / hi the column's minimum / maximum as fp64 (lo -= 0.5, hi += 0.5
when they are equal), ``bin(x) = #{j in 0..bins-1 : x >= lo + j * ((hi - lo) / bins)}`` -- ``np.histogram``'s edges
followed by ``np.digitize(x, edges[:-1])``, so the column maximum lands in bin ``bins`` and the minimum in bin 1.

Degenerate inputs are not special-cased; they follow IEEE arithmetic exactly as the reference's numpy does: a factor
that takes one value has H = 0 and makes MIG ``nan`` (0 / 0) or ``inf``; a latent with no information about any factor
(theta = 0) or a single factor (K = 1) makes modularity ``nan``.  MIG of a single latent has no second-largest value and
raises, as the reference's indexing does.  Non-finite representations and factor values outside ``[0, size)`` raise
``ValueError`` (``np.histogram`` raises on the former too).

The FactorVAE score (Kim & Mnih 2018) and the SAP score (Kumar et al. 2018) are not in the reference; they complete the
usual seven-metric table.  Both are fixed rules (include/itcv_hip.h, csrc/extra_scores.hip): FactorVAE is a majority-vote
classifier on integer vote tables, one wave per group of images with one factor held fixed; SAP's default form fits
``D x sum(sizes)`` two-parameter squared-hinge classifiers (liblinear's ``LinearSVC(C=0.01, class_weight="balanced")``
objective, whose optimum is unique) to convergence in one launch and counts correct test predictions as integers.

The unsupervised scores and IRS (disentanglement_lib's ``unsupervised_metrics`` and ``irs``; not in the reference) are
fixed rules too (include/itcv_hip.h, csrc/unsup_scores.hip), all in fp64 on the fp32 representations ``x[N][D]``, every
reduction in a fixed order, no floating-point atomics, the same bits from run to run:

* covariance: ``m[d] = (sum_n x[n][d]) / N``, ``C[i][j] = sum_n (x[n][i] - m[i]) (x[n][j] - m[j]) / (N - 1)`` (two passes
  over centred values as ``np.cov``; the products on the f64 matrix cores; one triangle mirrored);  N >= 2, D <= 512.
* Gaussian total correlation ``tc = (sum_d log C[d][d] - logdet C) / 2``, ``logdet C = 2 sum_d log L[d][d]`` from the
  Cholesky factor.  C must be positive definite: a pivot <= 0 raises ``ValueError`` naming the dimension (the library
  returns nan or inf there).
* Gaussian Wasserstein correlation ``w = 2 tr C - 2 sum_i sqrt(max(lambda_i(S), 0))``, ``S = D^1/2 C D^1/2``, ``D =
  diag(C)`` (similar to the matrix whose ``sqrtm`` the library takes); ``lambda`` by a cyclic Jacobi iteration with a
  fixed round-robin rotation order, stopped at ``off(S)_F <= 1e-14 |S|_F``, ``RuntimeError`` after 60 sweeps;
  ``w_norm = w / tr C``.
* mutual information score: every column in 20 bins by ``discretize``; ``MI[i][j]`` in nats between the bin numbers of
  columns i and j (the existing histogram and MI kernels, 16 columns a call; the upper triangle mirrored); the score is
  ``sum_{i != j} MI[i][j] / (D^2 - D)``, ``nan`` for D = 1 as in the library.
* IRS: active dimensions are those with min < max (the library tests var > 0, whose result for a constant column depends
  on rounding); ``maxdev[d] = max_n |x[n][d] - m[d]|``; for every factor k and every value v present in the sample, with
  G its rows and n = |G|: ``e[d]`` the mean of the group, ``a`` the ascending sort of ``|x[g][d] - e[d]|``, ``h = (n - 1)
  q`` (q = 0.99), ``lo = floor(h)``, ``t = h - lo``, ``hi = min(lo + 1, n - 1)``, ``Q = a[lo] + (a[hi] - a[lo]) t`` if
  ``t < 0.5`` else ``a[hi] - (a[hi] - a[lo]) (1 - t)`` (``np.percentile``, bit for bit; the two order statistics are
  selected exactly); ``cum[d][k] = (sum_v Q) / #present``; ``M = 1 - cum / maxdev``; ``score[d] = max_k M[d][k]``,
  ``parent[d]`` its first arg-max; ``IRS = sum_d score[d] maxdev[d] / sum_d maxdev[d]``; no active dimension: 0.0.

The Unsupervised Disentanglement Ranking (Duan et al. 2020; disentanglement_lib's ``udr``; not in the reference) needs no
factors: M >= 2 models encode the same N images, and a model ranks high when each of its informative latents matches
exactly one latent of every other model.  Fixed rules (include/itcv_hip.h, csrc/udr.hip):

* ``kl_d = mean_n (mu^2 + exp(logvar) - logvar - 1) / 2`` per model and dimension in fp64; a dimension is informative iff
  ``kl_d > kl_filter_threshold`` (0.01).
* the similarity of the latents of models i and j, a matrix ``[D_i, D_j]``: in the Spearman form ``|R|`` of the cross block
  of the covariance of the doubled tie-averaged ranks ``[r2(a) | r2(b)]`` (``r2 = L + H + 1``, exact integers),
  ``R_kl = C_kl / sqrt(C_kk C_ll)`` with the row and column of a constant column set to 0; in the Lasso form (the library's
  default) ``|w|`` of the Lasso (alpha = 0.1) that predicts each standardised latent of j from the standardised latents of
  i, solved by cyclic coordinate descent on the same normalised covariance until the subgradient condition holds to 1e-12.
* ``relative_strength``: ``sx = mean_j (max_i c_ij)^2 / sum_i c_ij`` over the informative rows and columns, ``sy`` the same
  over rows, a term whose sum is 0 counts as 0, the result ``(sx + sy) / 2``; all sums in index order.
* ``model_scores[i]``: the median over ``j != i`` of the non-nan ``pairwise[j, i]``.
"""
import numpy as np
import torch

from . import functional as HF
from . import gbt
from . import logreg
from .inference import draw_indices, eval_mode

__all__ = ["discretize", "factor_counts", "mutual_info", "mig_score", "modularity_score", "scores", "FactorSampler",
           "factor_representations", "compute_mig_score", "compute_modularity_score", "compute_scores",
           "fit_softmax", "factor_change_accuracy", "explicitness", "factor_change_rows", "compute_bvae_score",
           "compute_explicitness_score", "compute_mod_expl_score", "fit_boosted_trees", "dci_completeness",
           "dci_disentanglement", "dci", "compute_dci_score", "factor_vae_votes", "factor_vae_score",
           "compute_factor_vae_score", "fit_sap_classifiers", "sap_score_matrix", "sap_score", "compute_sap_score",
           "covariance", "unsupervised_scores", "gaussian_scores", "compute_unsupervised_scores", "irs_score_matrix",
           "irs_score", "compute_irs_score", "spearman_matrix", "lasso_matrix", "relative_strength", "udr_scores",
           "compute_udr_score"]


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

    def sample_fixed_factor(self, n, k):
        """``(factors, observations)`` of one FactorVAE group: n factor vectors whose column ``k`` is overwritten with row
        0's value.  Draws, in this order: the factors, then (inside the observation lookup) the factors that do not vary."""
        factors = self.sample_factors_of_variation(n)
        factors[:, k] = factors[0, k]
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
    mu, factors, row = None, [], 0
    with eval_mode(model):
        for f, obs in sampler.generate(num_samples, batch_size, drop_last=False):
            m, _ = model.encode(obs)
            if mu is None:
                mu = torch.empty((num_samples, m.shape[1]), dtype=m.dtype, device=m.device)
            mu[row:row + m.shape[0]].copy_(m)
            row += m.shape[0]
            factors.append(np.asarray(f))
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


# ---- classifier-based scores: beta-VAE and explicitness --------------------------------------------------------------
def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + int(s))
    return off


def _present(y, sizes):
    """int32 [csum] device mask: class c of problem k occurs in column k of y (labels outside the range are left to the
    kernels' flag)."""
    off = _offsets(sizes)
    out = torch.zeros((off[-1],), dtype=torch.int32, device=y.device)
    for k, s in enumerate(sizes):
        col = y[:, k].long()
        ok = (col >= 0) & (col < s)
        out[off[k]:off[k + 1]] = (torch.bincount(col[ok], minlength=s) > 0).to(torch.int32)
    return out


def fit_softmax(x, y, class_sizes, cvalid, stats=None, C=1.0, gtol=1e-9, max_iter=2000, flags=None):
    """Fit the K softmax regressions of (x[N, D], y[N, K]) jointly.  Returns ``(problem, theta, info)``: the
    ``HF.LogregProblem``, the optimum ``theta[(D + 1), csum]`` and the solver's report.  A problem with fewer than two
    valid classes raises ``ValueError`` (as sklearn's ``fit``); non-convergence raises ``RuntimeError``."""
    sizes = [int(s) for s in class_sizes]
    off = _offsets(sizes)
    flags = HF.disent_flags(x.device) if flags is None else flags
    prob = HF.LogregProblem(x, y, sizes, cvalid, flags, stats=stats, C=C)
    nvalid = [int(v) for v in torch.stack([prob.cvalid[a:b].ne(0).sum() for a, b in zip(off[:-1], off[1:])]).tolist()]
    for k, nv in enumerate(nvalid):
        if nv < 2:
            raise ValueError(f"logreg: problem {k} needs samples of at least 2 classes, but the data contains {nv}")
    theta, info = logreg.minimize(prob.valgrad, (prob.D + 1, prob.csum), off, prob.x.device, gtol=gtol, max_iter=max_iter,
                                  check=(lambda: flags, _raise_on))
    return prob, theta, info


def _macro_auc(count2, pos, neg, cvalid, sizes):
    """Mean over the problems of the mean AUC over each problem's valid classes: an fp64 device scalar."""
    off = _offsets(sizes)
    auc = count2.to(torch.float64) / (2.0 * pos.to(torch.float64) * neg.to(torch.float64))
    per = [auc[a:b][cvalid[a:b].ne(0)].mean() for a, b in zip(off[:-1], off[1:])]
    return torch.stack(per).mean()


def factor_change_accuracy(x_train, y_train, x_test, y_test, num_classes, scale=False, gtol=1e-9, max_iter=2000):
    """evaluation/utils.py:156-174 at the optimum: accuracy on the test rows of the softmax regression fitted on the
    training rows (optionally standardised with the training statistics).  A test label unseen in training counts as wrong."""
    flags = HF.disent_flags(x_train.device)
    y_train, y_test = y_train.reshape(-1, 1), y_test.reshape(-1, 1)
    stats = HF.logreg_colstats(x_train, flags) if scale else None
    yt = torch.as_tensor(y_train).to(device=x_train.device, dtype=torch.int32)
    prob, theta, _ = fit_softmax(x_train, yt, [num_classes], _present(yt, [num_classes]), stats=stats, gtol=gtol,
                                 max_iter=max_iter, flags=flags)
    ye = torch.as_tensor(y_test).to(device=x_train.device, dtype=torch.int32)
    _, pred = prob.proba(theta, x_test, ye)
    return _read([(pred == ye).sum().to(torch.float64)], flags)[0] / ye.shape[0]      # an integer count: exact


def explicitness(x_train, y_train, x_test, y_test, factor_sizes, gtol=1e-9, max_iter=2000):
    """``(train, test)`` explicitness (evaluation/metrics.py:296-302, utils.py:285-320) at the optimum: both sets are
    standardised with the training statistics, per factor the classes present in BOTH sets take part, and the score is the
    mean over factors of the macro one-vs-rest AUC of the fitted probabilities."""
    sizes = [int(s) for s in factor_sizes]
    flags = HF.disent_flags(x_train.device)
    y_train = torch.as_tensor(y_train).to(device=x_train.device, dtype=torch.int32)
    y_test = torch.as_tensor(y_test).to(device=x_train.device, dtype=torch.int32)
    cvalid = _present(y_train, sizes) * _present(y_test, sizes)
    stats = HF.logreg_colstats(x_train, flags)
    prob, theta, _ = fit_softmax(x_train, y_train, sizes, cvalid, stats=stats, gtol=gtol, max_iter=max_iter, flags=flags)
    out = []
    for x, y in ((None, None), (x_test, y_test)):
        P, _ = prob.proba(theta, x, y)
        yy = prob.y if y is None else y
        out.append(_macro_auc(*HF.logreg_auc(P, yy, sizes, cvalid, flags), cvalid, sizes))
    return tuple(_read(out, flags))


def factor_change_rows(latent_generator, model, num_samples, batch_size, index_state=None):
    """``(z_diff [num_batches, D] fp32 on the device, y [num_batches] numpy int64)``: evaluation/utils.py:60-153.  Each row
    comes from two factor draws that share one column, two observation draws and ONE eval-mode encode of the 2 B stacked
    images (eval BatchNorm makes stacking exact).  The fixed factor's index is drawn, as the reference writes it, from a
    fresh ``RandomState(latent_generator.seed)`` per batch, or from ``index_state`` if given."""
    nb = int(np.ceil(num_samples / batch_size))
    rows, y = None, np.empty((nb,), dtype=np.int64)
    with eval_mode(model):
        for r in range(nb):
            rs = index_state if index_state is not None else np.random.RandomState(latent_generator.seed)
            y[r] = k = rs.randint(latent_generator.num_latents)
            v_li = latent_generator.sample_factors_of_variation(batch_size)
            v_lj = latent_generator.sample_factors_of_variation(batch_size)
            v_li[:, k] = v_lj[:, k]
            x_li = latent_generator.sample_observations_from_factors(v_li)
            x_lj = latent_generator.sample_observations_from_factors(v_lj)
            mu, _ = model.encode(torch.cat([x_li, x_lj], 0))
            mu = mu.reshape(2 * batch_size, -1)
            if rows is None:
                rows = torch.empty((nb, mu.shape[1]), dtype=torch.float32, device=mu.device)
            HF.zdiff_row(mu[:batch_size], mu[batch_size:], rows[r])
    return rows, y


def compute_bvae_score(latent_generator, model, num_samples=10000, batch_size=64, index_state=None, gtol=1e-9,
                       max_iter=2000):
    """evaluation/metrics.py:20-79 with the reference's argument names: ``(score, score_scaled)``."""
    nl = int(latent_generator.num_latents)
    xtr, ytr = factor_change_rows(latent_generator, model, num_samples, batch_size, index_state)
    xte, yte = factor_change_rows(latent_generator, model, num_samples, batch_size, index_state)
    return tuple(factor_change_accuracy(xtr, ytr, xte, yte, nl, scale=s, gtol=gtol, max_iter=max_iter)
                 for s in (False, True))


def _train_test(latent_generator, model, num_samples, batch_size):
    return (factor_representations(latent_generator, model, num_samples, batch_size),
            factor_representations(latent_generator, model, num_samples, batch_size))


def compute_explicitness_score(latent_generator, model, num_samples=10000, batch_size=64, params=None,
                               return_train=False):
    """The explicitness half of evaluation/metrics.py:237-304: the test score (``return_train``: ``(train, test)``).
    ``params``: ``gtol`` / ``max_iter`` of the solver."""
    params = params or {}
    (xtr, ytr), (xte, yte) = _train_test(latent_generator, model, num_samples, batch_size)
    got = explicitness(xtr, ytr, xte, yte, _latent_sizes(latent_generator), params.get("gtol", 1e-9),
                       params.get("max_iter", 2000))
    return got if return_train else got[1]


def compute_mod_expl_score(latent_generator, model, num_samples=10000, batch_size=64, params=None):
    """evaluation/metrics.py:237-304: ``(modularity, explicitness)``; modularity from the TRAIN representations."""
    params = params or {}
    sizes = _latent_sizes(latent_generator)
    (xtr, ytr), (xte, yte) = _train_test(latent_generator, model, num_samples, batch_size)
    mod = modularity_score(xtr, ytr, sizes, params.get("bins", 20))
    return mod, explicitness(xtr, ytr, xte, yte, sizes, params.get("gtol", 1e-9), params.get("max_iter", 2000))[1]


# ---- DCI: boosted trees, then closed forms on the importance matrix ---------------------------------------------------
fit_boosted_trees = gbt.fit_boosted_trees


def _entropy(x, base, dim, eps=1e-9):
    """ops.entropy (ops.py:125-133) along ``dim`` of an fp64 tensor."""
    p = (x + eps) / (x + eps).sum(dim=dim, keepdim=True)
    return -(p * torch.log(p + eps)).sum(dim=dim) / float(np.log(base + eps))


def _weights(P, dim):
    """utils.py:226-228 / 238-240: the share of every column (dim = 0) or row (dim = 1); uniform when P is all zero."""
    Q = torch.where(P.sum() == 0, torch.ones_like(P), P)
    return Q.sum(dim=dim) / Q.sum()


def dci_disentanglement(P):
    """evaluation/utils.py:220-229 on the fp64 ``[K, D]`` importance matrix: an fp64 device scalar."""
    return (_weights(P, 0) * (1.0 - _entropy(P, P.shape[0], 0))).sum()


def dci_completeness(P):
    """evaluation/utils.py:232-241: an fp64 device scalar."""
    return (_weights(P, 1) * (1.0 - _entropy(P, P.shape[1], 1))).sum()


def dci(x_train, y_train, x_test, y_test, factor_sizes, **booster):
    """``(informativeness, completeness, disentanglement)`` (evaluation/metrics.py:157-161): the mean test accuracy of the
    K boosted-tree classifiers and the closed forms on their importances.  ``booster``: ``rounds``, ``max_depth``,
    ``max_bin``, ``eta``, ``lam`` of ``fit_boosted_trees``.  One host read-back."""
    fit = gbt.fit_device(x_train, y_train, x_test, y_test, factor_sizes, **booster)
    P = fit["importance"]
    _, test, (comp, dis) = gbt.read_back(fit, (dci_completeness(P), dci_disentanglement(P)))
    return float(np.mean([c / fit["Nt"] for c in test])), comp, dis


_BOOSTER_KEYS = {"n_estimators": "rounds", "max_depth": "max_depth", "learning_rate": "eta", "reg_lambda": "lam",
                 "max_bin": "max_bin"}


def compute_dci_score(latent_generator, model, num_samples=10000, batch_size=64, params=None):
    """evaluation/metrics.py:106-161 with the reference's arguments and return order: ``(informativeness, completeness,
    disentanglement)``.  ``params["informativeness_params"]`` may carry ``n_estimators``, ``max_depth``,
    ``learning_rate``, ``reg_lambda`` and ``max_bin``; other keys (the reference passes xgboost's ``tree_method``,
    ``gpu_id``, ``eval_metric``, ``use_label_encoder``) select nothing here and are ignored."""
    params = params or {}
    method = params.get("informativeness_method")
    if method not in (None, "xgb"):
        raise NotImplementedError(f"compute_dci_score: informativeness_method = {method!r} (only None / 'xgb': the "
                                  "device-side histogram booster)")
    given = params.get("informativeness_params") or {}
    booster = {ours: given[theirs] for theirs, ours in _BOOSTER_KEYS.items() if theirs in given}
    (xtr, ytr), (xte, yte) = _train_test(latent_generator, model, num_samples, batch_size)
    return dci(xtr, ytr, xte, yte, _latent_sizes(latent_generator), **booster)


# ---- FactorVAE score: majority vote on the arg-min normalised variance ------------------------------------------------
def _raise_on_extra(flags):
    _raise_on(flags[:2])
    if len(flags) > 2 and flags[2]:
        raise RuntimeError("sap: a squared-hinge classifier did not converge (raise max_iter, or check the representations)")


def factor_vae_votes(mu_var, mu_train, fidx_train, mu_eval, fidx_eval, L, num_factors, threshold=0.05):
    """Everything the score is made of, for inspection: a dict of ``gvar [D]`` fp64, ``votes_train`` / ``votes_eval
    [D, K]`` int64, ``classifier [D]`` int32 (device tensors) and the floats ``train_accuracy``, ``eval_accuracy``,
    ``num_active``.  One host read-back."""
    L = int(L)
    if L < 2:
        raise ValueError(f"factor_vae: a group needs L >= 2 rows for a ddof = 1 variance (got L = {L})")
    if mu_var.dim() != 2 or mu_var.shape[0] < 2:
        raise ValueError("factor_vae: the variance estimate needs at least 2 rows of [N, D] representations")
    flags = HF.extra_flags(mu_var.device)
    gvar = HF.fvae_gvar(mu_var, flags)
    vt = HF.fvae_votes(mu_train, L, gvar, threshold, fidx_train, num_factors, flags)
    ve = HF.fvae_votes(mu_eval, L, gvar, threshold, fidx_eval, num_factors, flags)
    classifier, res = HF.fvae_classify(vt, ve, mu_train.shape[0] // L, mu_eval.shape[0] // L, gvar, threshold)
    out = torch.cat([res, flags.to(torch.float64)]).tolist()
    _raise_on_extra(out[3:])
    return dict(gvar=gvar, votes_train=vt, votes_eval=ve, classifier=classifier, train_accuracy=out[0],
                eval_accuracy=out[1], num_active=int(out[2]))


def factor_vae_score(mu_var, mu_train, fidx_train, mu_eval, fidx_eval, L, num_factors, threshold=0.05):
    """``(train_accuracy, eval_accuracy)`` of the FactorVAE majority-vote classifier (rule: include/itcv_hip.h).
    ``mu_train [Mt * L, D]`` / ``mu_eval [Me * L, D]``: groups of L consecutive rows with one factor held fixed,
    ``fidx_*``: that factor's index per group; ``mu_var [Nv, D]``: the rows of the global variance estimate."""
    got = factor_vae_votes(mu_var, mu_train, fidx_train, mu_eval, fidx_eval, L, num_factors, threshold)
    return got["train_accuracy"], got["eval_accuracy"]


def _index_state(generator):
    rs = getattr(generator, "random_state", None)
    return rs if rs is not None else np.random.RandomState(getattr(generator, "seed", None))


def _fixed_factor_group(generator, n, k):
    if hasattr(generator, "sample_fixed_factor"):
        return generator.sample_fixed_factor(n, k)
    factors = np.asarray(generator.sample_factors_of_variation(n)).copy()
    factors[:, k] = factors[0, k]
    return factors, generator.sample_observations_from_factors(factors)


def _fixed_factor_representations(generator, model, num_groups, L, stack):
    """``(mu [num_groups * L, D] fp32 on the device, fidx [num_groups] numpy int64)``: per group the factor index is drawn
    first, then the group.  ``stack`` groups go through one eval-mode forward call (eval BatchNorm normalises every image
    with the running statistics, so stacking is exact per image); the means land in one preallocated buffer."""
    rs = _index_state(generator)
    fidx = np.empty((num_groups,), dtype=np.int64)
    mu, row = None, 0
    for g0 in range(0, num_groups, stack):
        obs = []
        for g in range(g0, min(num_groups, g0 + stack)):
            fidx[g] = k = rs.randint(generator.num_latents)
            obs.append(_fixed_factor_group(generator, L, k)[1])
        m, _ = model.encode(torch.cat(obs, 0) if len(obs) > 1 else obs[0])
        m = m.reshape(m.shape[0], -1)
        if mu is None:
            mu = torch.empty((num_groups * L, m.shape[1]), dtype=m.dtype, device=m.device)
        mu[row:row + m.shape[0]].copy_(m)
        row += m.shape[0]
    return mu, fidx


def compute_factor_vae_score(latent_generator, model, batch_size=64, num_train=10000, num_eval=5000,
                             num_variance_estimate=10000, params=None):
    """``(train_accuracy, eval_accuracy)``: ``num_variance_estimate`` images for the global variances, then ``num_train`` /
    ``num_eval`` groups of ``batch_size`` images with one factor fixed, all encoded in eval mode without gradients (as many
    groups per forward call as fit in 1024 images).  ``params`` may override any of the counts and carry ``threshold``."""
    params = params or {}
    L = int(params.get("batch_size", batch_size))
    if L < 2:
        raise ValueError(f"factor_vae: a group needs L >= 2 rows for a ddof = 1 variance (got L = {L})")
    nt, ne = int(params.get("num_train", num_train)), int(params.get("num_eval", num_eval))
    nv = int(params.get("num_variance_estimate", num_variance_estimate))
    mu_var, _ = factor_representations(latent_generator, model, nv, L)
    stack = max(1, 1024 // L)
    with eval_mode(model):
        mu_t, f_t = _fixed_factor_representations(latent_generator, model, nt, L, stack)
        mu_e, f_e = _fixed_factor_representations(latent_generator, model, ne, L, stack)
    return factor_vae_score(mu_var, mu_t, f_t, mu_e, f_e, L, int(latent_generator.num_latents),
                            params.get("threshold", 0.05))


# ---- SAP score: separated attribute predictability --------------------------------------------------------------------
def _sap_inputs(x_train, x_test):
    for x in (x_train, x_test):
        if x.dim() != 2 or x.shape[1] < 2:
            raise ValueError(f"sap: the score needs at least two latents, representations [N, D >= 2] (got "
                             f"{tuple(x.shape)}): there is no second-largest predictability")
    if x_train.shape[1] != x_test.shape[1]:
        raise ValueError("sap: train and test representations differ in width")


def fit_sap_classifiers(x_train, y_train, factor_sizes, C=0.01, gtol=1e-10, max_iter=100, flags=None):
    """The classifiers alone: ``(theta [D, csum, 2], gnorm [D, csum], iters [D, csum], cvalid [csum])`` as device tensors.
    With ``flags`` None the flags are read back and raise; else the caller owns them."""
    own = flags is None
    flags = HF.extra_flags(x_train.device) if own else flags
    out = HF.sap_svc_fit(x_train, y_train, factor_sizes, flags, C, gtol, max_iter)
    if own:
        _raise_on_extra(flags.tolist())
    return out


def _sap_matrix(x_train, y_train, x_test, y_test, factor_sizes, continuous_factors, C, gtol, max_iter, flags):
    _sap_inputs(x_train, x_test)
    if continuous_factors:
        x = HF._disent_mu(x_train).to(torch.float64)
        y = torch.as_tensor(y_train).to(device=x.device, dtype=torch.float64)
        if y.dim() != 2 or y.shape[0] != x.shape[0] or x.shape[0] < 2:
            raise ValueError("sap: continuous factors must be [N >= 2, K], one row per representation")
        flags[0:1].bitwise_or_((~torch.isfinite(x).all()).to(torch.int32))
        xc, yc = x - x.mean(0, keepdim=True), y - y.mean(0, keepdim=True)
        cov = xc.t() @ yc / (x.shape[0] - 1)
        vx, vy = (xc * xc).sum(0) / (x.shape[0] - 1), (yc * yc).sum(0) / (x.shape[0] - 1)
        S = cov * cov / (vx[:, None] * vy[None, :])
        return torch.where(vx[:, None] > 1e-12, S, torch.zeros_like(S))
    theta, _, _, cvalid = HF.sap_svc_fit(x_train, y_train, factor_sizes, flags, C, gtol, max_iter)
    correct = HF.sap_svc_score(x_test, y_test, factor_sizes, cvalid, theta, flags)
    # integer counts over a TENSOR divisor: a true fp64 division (a Python divisor becomes a product with 1 / N_test)
    return correct.to(torch.float64) / torch.full((), float(x_test.shape[0]), dtype=torch.float64, device=correct.device)


def _sap(S):
    """mean_j (largest - second largest of S[:, j]); the sum runs in factor order, so the bits are defined."""
    top = S.topk(2, dim=0).values
    diff = top[0] - top[1]
    tot = diff[0]
    for j in range(1, diff.shape[0]):
        tot = tot + diff[j]
    return tot / torch.full((), float(diff.shape[0]), dtype=torch.float64, device=S.device)


def sap_score_matrix(x_train, y_train, x_test, y_test, factor_sizes, continuous_factors=False, C=0.01, gtol=1e-10,
                     max_iter=100):
    """fp64 device tensor ``S [D, K]``: test accuracy of the classifier that predicts factor j from latent i alone, or,
    with ``continuous_factors``, the squared correlation of the pair on the train rows (0 where var(x_i) <= 1e-12)."""
    flags = HF.extra_flags(x_train.device)
    S = _sap_matrix(x_train, y_train, x_test, y_test, factor_sizes, continuous_factors, C, gtol, max_iter, flags)
    _raise_on_extra(flags.tolist())
    return S


def sap_score(x_train, y_train, x_test, y_test, factor_sizes, continuous_factors=False, C=0.01, gtol=1e-10,
              max_iter=100):
    """The SAP score: the mean over the factors of (largest - second largest entry of the column of S).  One read-back."""
    flags = HF.extra_flags(x_train.device)
    S = _sap_matrix(x_train, y_train, x_test, y_test, factor_sizes, continuous_factors, C, gtol, max_iter, flags)
    out = torch.cat([_sap(S).reshape(1), flags.to(torch.float64)]).tolist()
    _raise_on_extra(out[1:])
    return out[0]


def compute_sap_score(latent_generator, model, num_train=10000, num_test=5000, batch_size=64, params=None):
    """SAP of ``num_train`` / ``num_test`` sampled images encoded in eval mode.  ``params`` may override the counts and
    carry ``continuous_factors``, ``C``, ``gtol``, ``max_iter``."""
    params = params or {}
    bs = int(params.get("batch_size", batch_size))
    xtr, ytr = factor_representations(latent_generator, model, int(params.get("num_train", num_train)), bs)
    xte, yte = factor_representations(latent_generator, model, int(params.get("num_test", num_test)), bs)
    return sap_score(xtr, ytr, xte, yte, _latent_sizes(latent_generator), params.get("continuous_factors", False),
                     params.get("C", 0.01), params.get("gtol", 1e-10), params.get("max_iter", 100))


# ---- unsupervised scores: Gaussian total correlation, Gaussian Wasserstein correlation, mutual information ----------
_MI_BINS = 20          # disentanglement_lib's unsupervised_metrics discretises every latent into 20 bins
_MI_CHUNK = 16         # factors per call of the histogram / MI kernels (kDisMaxK)


def covariance(mu):
    """``(mean [D], cov [D, D])`` as fp64 device tensors: the ddof = 1 covariance of ``mu [N >= 2, D <= 512]`` (``np.cov``'s
    two passes over centred values; rule: include/itcv_hip.h), symmetric bit for bit."""
    flags = HF.disent_flags(mu.device)
    mean, cov = HF.unsup_cov(mu, flags)
    _raise_on(flags.tolist())
    return mean, cov


def _mutual_info_matrix(mu, flags):
    """fp64 ``MI [D, D]``: the mutual information in nats of the bin numbers of every pair of columns.  The bin numbers
    minus 1 are handed to the histogram and MI kernels as "factors" of size 20, 16 columns a call; the upper triangle is
    kept and mirrored."""
    N, D = mu.shape
    mn, mx = HF.disent_minmax(mu, flags)
    b = HF.disent_bins(mu, mn, mx, _MI_BINS) - 1
    cols = []
    for c0 in range(0, D, _MI_CHUNK):
        f = b[:, c0:c0 + _MI_CHUNK].contiguous()
        sizes = [_MI_BINS] * f.shape[1]
        counts, vcount = HF.disent_hist(mu, f, sizes, mn, mx, _MI_BINS, flags)
        cols.append(HF.disent_mi(counts, vcount, N, D, sizes, _MI_BINS)[0])
    mi = torch.cat(cols, 1)
    return torch.triu(mi) + torch.triu(mi, 1).t()


def unsupervised_scores(mu):
    """The unsupervised scores of ``mu [N >= 2, D <= 512]`` (disentanglement_lib's ``unsupervised_metrics``; rules:
    include/itcv_hip.h): the floats ``gaussian_total_correlation``, ``gaussian_wasserstein_correlation``,
    ``gaussian_wasserstein_correlation_norm`` and ``mutual_info_score`` (``nan`` for D = 1), and the fp64 device tensors
    ``covariance [D, D]``, ``eigenvalues [D]`` (of S = D^1/2 C D^1/2, ascending) and ``mutual_info_matrix [D, D]``.  The
    covariance must be positive definite: a Cholesky pivot <= 0 (a constant column, two identical columns) raises
    ``ValueError`` naming the dimension, where the library returns nan or inf.  One host read-back."""
    flags = HF.disent_flags(mu.device)
    _, cov = HF.unsup_cov(mu, flags)
    res, eig, info = HF.unsup_gauss(cov)
    mi = _mutual_info_matrix(mu, flags)
    D = mu.shape[1]
    off = mi.masked_fill(torch.eye(D, dtype=torch.bool, device=mi.device), 0.0)
    mis = off.sum() / torch.full((), float(D * D - D), dtype=torch.float64, device=mi.device)
    out = torch.cat([res, mis.reshape(1), info.to(torch.float64), flags.to(torch.float64)]).tolist()
    _raise_on(out[10:12])
    _raise_on_gauss(out[6:10])
    return dict(gaussian_total_correlation=out[0], gaussian_wasserstein_correlation=out[1],
                gaussian_wasserstein_correlation_norm=out[2], mutual_info_score=out[5], covariance=cov,
                eigenvalues=torch.sort(eig).values, mutual_info_matrix=mi)


def _raise_on_gauss(info):
    if info[0]:
        raise ValueError(f"unsupervised scores: the covariance is not positive definite (the Cholesky pivot of dimension "
                         f"{int(info[1])} is not positive: a constant column, or one that depends linearly on the ones "
                         "before it)")
    if info[2]:
        raise RuntimeError("unsupervised scores: the Jacobi iteration did not converge in 60 sweeps")


def gaussian_scores(cov):
    """``(tc, w, w_norm, eigenvalues)`` of a given symmetric fp64 device ``cov [D, D]``: the Cholesky / Jacobi launch
    alone (the eigenvalues of S in the kernel's index order, a device tensor)."""
    res, eig, info = HF.unsup_gauss(cov)
    out = torch.cat([res, info.to(torch.float64)]).tolist()
    _raise_on_gauss(out[5:9])
    return out[0], out[1], out[2], eig


def compute_unsupervised_scores(source, model, num_train=10000, batch_size=64, seed=0):
    """``unsupervised_scores`` of the mean representations of ``num_train`` images of ``source`` (a ``DeviceImageTable``
    or a dataset; no factors are needed): the images ``inference.draw_indices(len(source), num_train, seed)``, encoded by
    ``hipvae.aggregate.dataset_posteriors`` in eval mode without gradients.  torch's generators, the BatchNorm buffers and
    the training flag are left as found."""
    from . import aggregate
    mu, _ = aggregate.dataset_posteriors(source, model, draw_indices(len(source), num_train, seed), batch_size)
    return unsupervised_scores(mu)


# ---- IRS: interventional robustness score ----------------------------------------------------------------------------
def irs_score_matrix(mu, factors, factor_sizes, diff_quantile=0.99):
    """Everything the IRS is made of (Suter et al. 2019; disentanglement_lib's ``irs.scalable_disentanglement_score`` on the
    active dimensions; rule: include/itcv_hip.h): ``avg_score`` (the IRS, a float), ``num_active_dims`` (int) and, over the
    active dimensions only, the device tensors ``disentanglement_scores [A]``, ``parents [A]`` (int64), ``IRS_matrix
    [A, K]``, ``max_deviations [A]``, ``cum_deviations [A, K]``; ``active_dims [A]`` lists them.  A dimension is active iff
    its minimum is below its maximum (the library tests var > 0, whose result for a constant column depends on rounding).
    No active dimension: ``avg_score`` 0.0."""
    flags = HF.disent_flags(mu.device)
    mn, mx = HF.disent_minmax(mu, flags)
    got = HF.irs(mu, factors, factor_sizes, mn, mx, flags, diff_quantile)
    out = torch.cat([got["res"], flags.to(torch.float64)]).tolist()
    _raise_on(out[2:])
    act = got["active"].nonzero().reshape(-1)
    return dict(avg_score=out[0], num_active_dims=int(out[1]), disentanglement_scores=got["score"][act],
                parents=got["parent"][act].long(), IRS_matrix=got["M"][act], max_deviations=got["maxdev"][act],
                cum_deviations=got["cum"][act], active_dims=act)


def irs_score(mu, factors, factor_sizes, diff_quantile=0.99):
    """The IRS alone, a Python float."""
    return irs_score_matrix(mu, factors, factor_sizes, diff_quantile)["avg_score"]


def compute_irs_score(latent_generator, model, num_train=10000, batch_size=64, params=None):
    """``irs_score_matrix`` of ``num_train`` sampled images encoded in eval mode (``factor_representations``); ``params``
    may override ``num_train`` / ``batch_size`` and carry ``diff_quantile``.  The IRS is ``["avg_score"]``."""
    params = params or {}
    mu, v = factor_representations(latent_generator, model, int(params.get("num_train", num_train)),
                                   int(params.get("batch_size", batch_size)))
    return irs_score_matrix(mu, v, _latent_sizes(latent_generator), params.get("diff_quantile", 0.99))


# ---- UDR: unsupervised disentanglement ranking -----------------------------------------------------------------------
def _ordered_sum(t, dim):
    """The sum of ``t`` along ``dim`` taken slice by slice in index order, so that the bits are defined (as ``_sap``)."""
    parts = t.unbind(dim)
    tot = parts[0]
    for part in parts[1:]:
        tot = tot + part
    return tot


def _correlation_of(cov):
    """``R_kl = C_kl / sqrt(C_kk C_ll)`` of a covariance; the row and column of a column with ``C_kk == 0`` are 0."""
    d = torch.diagonal(cov)
    live = (d != 0)[:, None] & (d != 0)[None, :]
    return torch.where(live, cov / torch.sqrt(d[:, None] * d[None, :]), torch.zeros_like(cov))


def _spearman(a, b, flags):
    cols = torch.cat([HF.udr_ranks(a, flags), HF.udr_ranks(b, flags)], 1)
    _, cov = HF.unsup_cov(cols, flags)
    return _correlation_of(cov)[:a.shape[1], a.shape[1]:].abs().contiguous()


def _same_rows(a, b):
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"udr: the representations must be [N, D_i] tensors of the same N inputs (got {tuple(a.shape)} "
                         f"and {tuple(b.shape)})")
    if a.shape[1] + b.shape[1] > 512:
        raise ValueError(f"udr: the two models have {a.shape[1]} + {b.shape[1]} latents, more than 512 together")


def spearman_matrix(a, b):
    """fp64 device ``[Da, Db]``: ``|rho|`` of Spearman's rank correlation (ties averaged, as ``scipy.stats.spearmanr``)
    between every column of ``a [N, Da]`` and every column of ``b [N, Db]``; a constant column gives zeros.  Exact ranks by
    ``itcv_udr_ranks``, their covariance by ``itcv_unsup_cov``."""
    _same_rows(a, b)
    flags = HF.disent_flags(a.device)
    out = _spearman(a, b, flags)
    _raise_on(flags.tolist())
    return out


def _raise_on_lasso(info):
    if info[0]:
        raise RuntimeError(f"udr: the Lasso coordinate descent did not converge for {int(info[1])} target(s) in "
                           f"{int(info[2])} sweeps (raise max_sweeps or gtol)")


def lasso_matrix(a, b, alpha=0.1, gtol=1e-12, max_sweeps=1000):
    """fp64 device ``[Da, Db]``: column t holds ``|w|`` of the Lasso that predicts the standardised column t of ``b`` from
    the standardised columns of ``a`` (``StandardScaler`` + ``sklearn.linear_model.Lasso(alpha)``, the library's
    ``transpose(abs(coef_))``), solved to ``gtol`` in the subgradient condition; ``RuntimeError`` when ``max_sweeps``
    sweeps do not reach it."""
    _same_rows(a, b)
    flags = HF.disent_flags(a.device)
    _, cov = HF.unsup_cov(torch.cat([HF._disent_mu(a), HF._disent_mu(b)], 1), flags)
    W, info = HF.udr_lasso(cov, a.shape[1], b.shape[1], alpha, gtol, max_sweeps)
    out = torch.cat([flags, info]).tolist()
    _raise_on(out[:2])
    _raise_on_lasso(out[2:])
    return W


def _relative_strength(corr, rows, cols):
    """``relative_strength`` of ``corr[rows][:, cols]`` (boolean device masks) without compacting it: a masked entry enters
    the ordered sums as +0, which changes no bit of a sum of non-negative terms, and never wins a maximum.  Leading
    dimensions are a batch: ``corr [..., Da, Db]``, ``rows [..., Da]``, ``cols [..., Db]`` give one score each from the same
    elementwise operations, so the bits do not depend on the batch."""
    zero = torch.zeros((), dtype=torch.float64, device=corr.device)
    c = torch.where(rows[..., :, None] & cols[..., None, :], corr, zero)

    def side(c, keep, n):
        top, tot = c.max(dim=-2).values, _ordered_sum(c, -2)
        term = torch.where(keep & (tot != 0), top * top / tot, zero)
        return _ordered_sum(term, -1) / n

    nr, nc = rows.sum(-1).to(torch.float64), cols.sum(-1).to(torch.float64)
    score = (side(c, cols, nc) + side(c.transpose(-1, -2), rows, nr)) / 2.0
    return torch.where((nr > 0) & (nc > 0), score, torch.full_like(zero, float("nan")))


def relative_strength(corr):
    """0-dim fp64 device tensor: ``(sx + sy) / 2`` with ``sx = mean_j (max_i c_ij)^2 / sum_i c_ij`` and ``sy`` the same
    over rows (disentanglement_lib's ``relative_strength_disentanglement``); a term whose sum is 0 counts as 0, a matrix
    with no rows or no columns gives nan.  The sums run in index order."""
    if corr.dim() != 2 or corr.dtype != torch.float64 or not corr.is_cuda:
        raise HF.abi.HipExtensionError("udr: relative_strength needs an fp64 [Da, Db] device tensor; there is no CPU path")
    if corr.shape[0] == 0 or corr.shape[1] == 0:
        return torch.full((), float("nan"), dtype=torch.float64, device=corr.device)
    return _relative_strength(corr, torch.ones(corr.shape[0], dtype=torch.bool, device=corr.device),
                              torch.ones(corr.shape[1], dtype=torch.bool, device=corr.device))


def _median(values):
    v = sorted(values)
    n = len(v)
    if not n:
        return float("nan")
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def udr_scores(mus, logvars=None, correlation="lasso", kl_filter_threshold=0.01, alpha=0.1):
    """The Unsupervised Disentanglement Ranking of M >= 2 models from their mean representations ``mus[i] [N, D_i]`` (and
    ``logvars[i]``) of the same N inputs.  A dict: ``model_scores`` (M floats: the median over the other models j of the
    non-nan ``pairwise[j, i]``, nan if there is none), ``pairwise_disentanglement_scores`` (fp64 numpy ``[M, M]``, nan on the
    diagonal: ``relative_strength`` of the similarity matrix of (i, j) restricted to the informative dimensions of both),
    ``raw_correlations`` ((i, j) -> the unrestricted fp64 device matrix ``[D_i, D_j]``), ``kl_masks`` (bool numpy arrays,
    ``kl_divergence > kl_filter_threshold``; everything when ``logvars`` is None) and ``kl_divergence`` (fp64 numpy arrays,
    None without ``logvars``).  ``correlation``: "lasso" (the library's default) or "spearman".  One covariance per
    unordered pair, one host read-back."""
    if correlation not in ("lasso", "spearman"):
        raise ValueError(f"udr: correlation must be 'lasso' or 'spearman' (got {correlation!r})")
    mus = [HF._disent_mu(m) for m in mus]
    M = len(mus)
    if M < 2:
        raise ValueError(f"udr: at least two models are needed (got {M})")
    if logvars is not None and (len(logvars) != M or any(lv.shape != m.shape for lv, m in zip(logvars, mus))):
        raise ValueError("udr: logvars must match mus, one [N, D_i] tensor per model")
    for m in mus[1:]:
        _same_rows(mus[0], m)
    dev = mus[0].device
    flags = HF.disent_flags(dev)
    if logvars is None:
        kls = None
        masks = [torch.ones(m.shape[1], dtype=torch.bool, device=dev) for m in mus]
    else:
        kls = []
        for m, lv in zip(mus, logvars):
            m64, lv64 = m.to(torch.float64), lv.detach().to(torch.float64)
            kls.append((0.5 * (m64 * m64 + torch.exp(lv64) - lv64 - 1.0)).mean(0))
        masks = [k > kl_filter_threshold for k in kls]
    raw, infos = {}, []
    nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
    pair = [[nan] * M for _ in range(M)]
    for i in range(M):
        for j in range(i + 1, M):
            Di, Dj = mus[i].shape[1], mus[j].shape[1]
            if correlation == "spearman":
                raw[i, j] = _spearman(mus[i], mus[j], flags)
                raw[j, i] = raw[i, j].t().contiguous()
            else:
                _, cov = HF.unsup_cov(torch.cat([mus[i], mus[j]], 1), flags)
                raw[i, j], info = HF.udr_lasso(cov, Di, Dj, alpha)
                infos.append(info)
                # the covariance of [b | a] is the same matrix with its blocks swapped
                raw[j, i], info = HF.udr_lasso(cov.roll((Dj, Dj), (0, 1)).contiguous(), Dj, Di, alpha)
                infos.append(info)
    shapes = {}                                                         # matrices of one shape are scored as one batch
    for key, mat in raw.items():
        shapes.setdefault(tuple(mat.shape), []).append(key)
    for keys in shapes.values():
        got = _relative_strength(torch.stack([raw[k] for k in keys]), torch.stack([masks[k[0]] for k in keys]),
                                 torch.stack([masks[k[1]] for k in keys]))
        for n, (i, j) in enumerate(keys):
            pair[i][j] = got[n]
    worst = torch.stack(infos).max(0).values if infos else torch.zeros(3, dtype=torch.int32, device=dev)
    head = torch.cat([torch.stack([p for row in pair for p in row]), flags.to(torch.float64), worst.to(torch.float64)])
    out = torch.cat([head] + (kls or [])).cpu().numpy()                 # the one read-back
    _raise_on(out[M * M:M * M + 2])
    _raise_on_lasso(out[M * M + 2:M * M + 5])
    pairwise = out[:M * M].reshape(M, M).copy()
    scores = [_median([float(pairwise[j, i]) for j in range(M) if j != i and not np.isnan(pairwise[j, i])])
              for i in range(M)]
    kl_np, kl_masks, at = None, [np.ones(m.shape[1], dtype=bool) for m in mus], M * M + 5
    if kls is not None:
        kl_np = []
        for m in mus:
            kl_np.append(out[at:at + m.shape[1]].copy())
            at += m.shape[1]
        kl_masks = [k > kl_filter_threshold for k in kl_np]
    return dict(model_scores=scores, pairwise_disentanglement_scores=pairwise, raw_correlations=raw, kl_masks=kl_masks,
                kl_divergence=kl_np)


def compute_udr_score(source, models, num_train=10000, batch_size=64, seed=0, params=None):
    """``udr_scores`` of ``models`` (M >= 2 networks with the same input) on ``num_train`` images of ``source`` (a
    ``DeviceImageTable`` or a dataset; no factors are needed): the images ``inference.draw_indices(len(source), num_train,
    seed)``, the ones ``compute_unsupervised_scores`` sees, encoded once per model by
    ``hipvae.aggregate.dataset_posteriors`` in eval mode without gradients.  torch's generators, the BatchNorm buffers
    and the training flags are left as found.  ``params`` may carry ``correlation``, ``kl_filter_threshold``, ``alpha``
    and ``num_train``."""
    from . import aggregate
    params = params or {}
    idx = draw_indices(len(source), params.get("num_train", num_train), seed)
    post = [aggregate.dataset_posteriors(source, model, idx, batch_size) for model in models]
    return udr_scores([p[0] for p in post], [p[1] for p in post], params.get("correlation", "lasso"),
                      params.get("kl_filter_threshold", 0.01), params.get("alpha", 0.1))
