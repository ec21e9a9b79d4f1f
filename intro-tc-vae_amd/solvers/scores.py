"""The scores ``VAESolver.write_disentanglemnt_scores`` can write, one record each.  ``TABLE`` holds those a user asks for
by name in ``extra_scores`` (the writer derives the known names, the factor / non-factor split and the order from it);
``DEVICE`` the four records of the ``device_scores`` ladder, which the writer selects itself.

Adding a score: one record here and one ``self.<name>_params = None`` line in ``VAESolver.__init__``."""
from dataclasses import dataclass
from typing import Callable, Optional

from hipvae import aggregate, density, disentangle, likelihood, quality


@dataclass(frozen=True)
class Score:
    """``name``: as it appears in ``extra_scores``.  ``added``: the score's place in the order in which the scores were
    added, which is the order of the unknown-name message (tests pin its tail); the order of writing is the table's.
    ``factors``: computed from the solver's ``latent_generator`` (a ``DisentanglementDataset`` only) rather than from the
    images alone.  ``params``: the solver attribute that feeds it.  ``tag``: the writer's record.  ``keys``: ``(written,
    read)`` pairs for ``add_scalars``, ``read`` a key or a position of what ``compute`` returns; None: the returned value
    goes to ``add_scalar``.  ``compute(solver, source)``: ``source`` is the latent generator for a factor score, else the
    device table or the dataset."""
    name: str
    added: int
    factors: bool
    params: Optional[str]
    tag: str
    keys: Optional[tuple]
    compute: Callable


def write(score, solver, source, cur_iter, *args):
    """Compute, then write: the one place a record reaches the writer."""
    got = score.compute(solver, source, *args)
    if score.keys is None:
        solver.writer.add_scalar(score.tag, got, global_step=cur_iter)
    else:
        solver.writer.add_scalars(score.tag, {w: got[r] for w, r in score.keys}, global_step=cur_iter)


def _same(*keys):
    return tuple((k, k) for k in keys)


def _keywords(s, params, **own):
    """The solver's batch size, then what the solver itself knows, then the user's ``params`` on top."""
    return {"batch_size": s.batch_size, **own, **(getattr(s, params) or {})}


def _prior(s):
    """``prior=`` of the solver's own learned prior, when it has one (``_eval_prior``)."""
    own = s._eval_prior()
    return {} if own is None else {"prior": own}


def _udr(s, source):
    if not s.udr_peers:
        raise ValueError('extra_scores: "udr" compares this model with models trained from other seeds: set '
                         "udr_peers to a sequence of them")
    got = disentangle.compute_udr_score(source, [s.model, *s.udr_peers], batch_size=s.batch_size, params=s.udr_params)
    mine = [float(v) for v in got["pairwise_disentanglement_scores"][1:, 0] if v == v]
    return dict(model_score=got["model_scores"][0], mean_pairwise=sum(mine) / len(mine) if mine else float("nan"))


TABLE = {r.name: r for r in (
    # factor_vae {train_accuracy, eval_accuracy}: FactorVAE's majority-vote classifier; ``params=factor_vae_params``
    Score("factor_vae", 1, True, "factor_vae_params", "factor_vae", (("train_accuracy", 0), ("eval_accuracy", 1)),
          lambda s, g: disentangle.compute_factor_vae_score(g, s.model, batch_size=s.batch_size,
                                                            params=s.factor_vae_params)),
    # sap_score: separated attribute predictability; ``params=sap_params``
    Score("sap", 2, True, "sap_params", "sap_score", None,
          lambda s, g: disentangle.compute_sap_score(g, s.model, batch_size=s.batch_size, params=s.sap_params)),
    # irs {IRS, num_active_dims}: interventional robustness; ``params=irs_params``
    Score("irs", 4, True, "irs_params", "irs", (("IRS", "avg_score"), ("num_active_dims", "num_active_dims")),
          lambda s, g: disentangle.compute_irs_score(g, s.model, batch_size=s.batch_size, params=s.irs_params)),
    # aggregate_decomp: the aggregate KL over the dataset's aggregate posterior, decomposed; keywords ``elbo_params``
    Score("elbo_decomposition", 3, False, "elbo_params", "aggregate_decomp",
          _same("mi", "tc", "dwkl", "kl", "kl_analytic"),
          lambda s, src: aggregate.compute_elbo_decomposition(src, s.model, **_keywords(s, "elbo_params"))),
    # unsupervised: Gaussian total / Wasserstein correlation and mutual information; keywords ``unsupervised_params``
    Score("unsupervised", 5, False, "unsupervised_params", "unsupervised",
          _same("gaussian_total_correlation", "gaussian_wasserstein_correlation", "gaussian_wasserstein_correlation_norm",
                "mutual_info_score"),
          lambda s, src: disentangle.compute_unsupervised_scores(src, s.model, **_keywords(s, "unsupervised_params"))),
    # udr {model_score, mean_pairwise}: this model's rank among ``[model, *udr_peers]`` and the mean of its non-nan
    # pairwise scores; ``params=udr_params``, ``udr_peers`` required
    Score("udr", 6, False, "udr_params", "udr", _same("model_score", "mean_pairwise"), _udr),
    # log_likelihood: the importance-weighted log p(x); keywords ``likelihood_params`` over the solver's reconstruction
    # loss and ``beta_rec``
    Score("log_likelihood", 9, False, "likelihood_params", "log_likelihood",
          _same("log_px", "bits_per_dim", "elbo", "ess"),
          lambda s, src: likelihood.compute_log_likelihood(
              src, s.model, **_keywords(s, "likelihood_params", loss_type=s.recon_loss_type, beta_rec=s.beta_rec))),
    # sample_quality: decoded prior samples against the images, over the model's own encoder means unless
    # ``quality_params`` names a feature (so not a published FID / KID); keywords ``quality_params`` over the solver's own
    # prior; ``dict(prior="gmm")`` decodes samples of an ex-post mixture instead
    Score("sample_quality", 10, False, "quality_params", "sample_quality",
          _same("frechet", "kid", "precision", "recall", "density", "coverage"),
          lambda s, src: quality.compute_sample_quality(src, s.model, **_keywords(s, "quality_params", **_prior(s)))),
    # reconstruction_quality: pixel-space means over deterministic reconstructions; keywords ``reconstruction_params``
    Score("reconstruction_quality", 7, False, "reconstruction_params", "reconstruction_quality",
          _same(*quality.RECONSTRUCTION_SCORES),
          lambda s, src: quality.compute_reconstruction_quality(src, s.model, **_keywords(s, "reconstruction_params"))),
    # latent_density: a Gaussian mixture fitted to one part of the latents and scored on another; ``gap`` is what the prior
    # loses against it, in nats per image; keywords ``density_params`` over the solver's own prior
    Score("latent_density", 8, False, "density_params", "latent_density",
          _same("loglik_heldout", "loglik_prior", "gap", "n_iter"),
          lambda s, src: density.compute_latent_density(src, s.model, **_keywords(s, "density_params", **_prior(s)))),
)}

# the names the unknown-name message lists, in its order
KNOWN = tuple(sorted(TABLE, key=lambda name: TABLE[name].added))

# the records of the ``device_scores`` ladder, by tag; ``compute(solver, generator, n)``: ``n`` sampled images
DEVICE = {r.tag: r for r in (
    Score("bvae", 0, True, None, "bvae_score", (("score", 0), ("scaled", 1)),
          lambda s, g, n: disentangle.compute_bvae_score(g, s.model, num_samples=n, batch_size=s.batch_size)),
    Score("mig", 0, True, None, "mig_score", None,
          lambda s, g, n: disentangle.compute_mig_score(g, s.model, num_samples=n, batch_size=s.batch_size)),
    Score("mod_expl", 0, True, None, "mod_expl", (("modularity_score", 0), ("explicitness_score", 1)),
          lambda s, g, n: disentangle.compute_mod_expl_score(g, s.model, num_samples=n, batch_size=s.batch_size)),
    Score("dci", 0, True, "dci_params", "dci",
          (("dci_informativeness_score", 0), ("dci_completeness_score", 1), ("dci_disentanglement_score", 2)),
          lambda s, g, n: disentangle.compute_dci_score(g, s.model, params=s.dci_params, num_samples=n,
                                                        batch_size=s.batch_size)),
)}
