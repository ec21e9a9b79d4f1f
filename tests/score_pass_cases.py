"""Every ``compute_*`` entry point of the evaluation modules whose encode loop or image draw goes through
``hipvae.inference``, on the smallest inputs that still take every branch: a tail batch, a draw below and one at or above
the number of images, a dataset and a ``DeviceImageTable`` of the same images.  ``tests/golden/make_golden_score_pass.py``
records what they return, ``tests/test_hip_score_pass_bits.py`` requires the same bytes.  Needs a GPU."""
import dataclasses

import numpy as np
import torch

NET = dict(cdim=3, zdim=8, channels=(8, 16), image_size=32)
FACTOR_SIZES = (6, 5, 4)
N_IMAGES = 120
SOURCES = ("dataset", "table")
# the untrained model spreads its means by less than FactorVAE's default threshold of 0.05: keep its dimensions active.
# 100 images per group: ten groups per forward call, so 13 groups take a full and a partial call
FACTOR_VAE = dict(num_train=13, num_eval=4, num_variance_estimate=250, batch_size=100, threshold=1e-6)
DCI = dict(informativeness_method="xgb", informativeness_params=dict(n_estimators=4, max_depth=3))


def dev():
    return torch.device("cuda:0")


def make_dataset():
    from solvers.vae import DisentanglementDataset

    class Synthetic(DisentanglementDataset):
        """120 seeded 3 x 32 x 32 uint8 images ordered by their factors (sizes 6, 5, 4, all varying), stored as the
        reference classes store them; ``__getitem__`` is ``imgs[i] / 255`` as ``ToTensor`` makes it."""
        factor_sizes = list(FACTOR_SIZES)
        latent_indices = [0, 1, 2]

        def __init__(self):
            rng = np.random.RandomState(11)
            a = rng.randint(0, 128, size=(N_IMAGES, 32, 32, 3)).astype(np.uint8)
            f = np.stack(np.unravel_index(np.arange(N_IMAGES), FACTOR_SIZES), 1)
            a[:, :16] += (f[:, 0] * 20).astype(np.uint8)[:, None, None, None]
            a[:, :, 16:] += (f[:, 1] * 25).astype(np.uint8)[:, None, None, None]
            a[..., 2] += (f[:, 2] * 30).astype(np.uint8)[:, None, None]
            self.imgs, self.resize, self.latents_values = a, 32, f

        def __len__(self):
            return N_IMAGES

        def __getitem__(self, i):
            a = np.ascontiguousarray(self.imgs[i].transpose(2, 0, 1))
            return torch.from_numpy(a).float().div(255), self.latents_values[i]

    return Synthetic()


class Context:
    """The dataset, its device table, the model under test (seeded, left in train mode), two peers for UDR and seeded
    pseudo-inputs; built once and left unchanged."""

    def __init__(self):
        import models
        from hipvae.dataset import DeviceImageTable
        self.dataset = make_dataset()
        self.table = DeviceImageTable.from_dataset(self.dataset, dev())
        nets = []
        for seed in (0, 1, 2):
            torch.manual_seed(seed)
            nets.append(models.SoftIntroVAE(arch="conv", **NET).to(dev()).train())
        self.model, self.peers = nets[0], nets[1:]
        self.pseudo = torch.rand(7, 3, 32, 32, generator=torch.Generator().manual_seed(5))

    def source(self, kind):
        return self.dataset if kind == "dataset" else self.table

    def sampler(self, kind):
        from hipvae.dataset import DeviceFactorSampler
        from hipvae.disentangle import FactorSampler
        if kind == "dataset":
            return FactorSampler(self.dataset, dev(), seed=3)
        return DeviceFactorSampler(self.dataset, dev(), seed=3, table=self.table)


def _calls():
    from hipvae import aggregate as A, density as Dn, disentangle as DS, likelihood as L, quality as Q
    rs = np.random.RandomState
    on_sampler = dict(
        scores=lambda s, m, c: DS.compute_scores(s, m, num_samples=150, batch_size=64),
        bvae=lambda s, m, c: DS.compute_bvae_score(s, m, num_samples=96, batch_size=8, index_state=rs(5)),
        mod_expl=lambda s, m, c: DS.compute_mod_expl_score(s, m, num_samples=150, batch_size=64),
        dci=lambda s, m, c: DS.compute_dci_score(s, m, num_samples=100, batch_size=48, params=DCI),
        factor_vae=lambda s, m, c: DS.compute_factor_vae_score(s, m, params=FACTOR_VAE),
        sap=lambda s, m, c: DS.compute_sap_score(s, m, params=dict(num_train=70, num_test=40, batch_size=16)),
        irs=lambda s, m, c: DS.compute_irs_score(s, m, params=dict(num_train=100, batch_size=16)),
    )
    on_source = dict(
        unsupervised_drawn=lambda s, m, c: DS.compute_unsupervised_scores(s, m, num_train=50, batch_size=16, seed=3),
        unsupervised_all=lambda s, m, c: DS.compute_unsupervised_scores(s, m, num_train=N_IMAGES, batch_size=16),
        udr_drawn=lambda s, m, c: DS.compute_udr_score(s, [m, *c.peers], num_train=80, batch_size=32, seed=3),
        udr_all=lambda s, m, c: DS.compute_udr_score(s, [m, *c.peers], batch_size=32, params=dict(correlation="spearman")),
        elbo_drawn=lambda s, m, c: A.compute_elbo_decomposition(s, m, num_samples=40, num_components=50, batch_size=16,
                                                                seed=3, return_inputs=True),
        elbo_all=lambda s, m, c: A.compute_elbo_decomposition(s, m, num_samples=40, batch_size=16, seed=3),
        log_likelihood=lambda s, m, c: L.compute_log_likelihood(s, m, num_samples=20, chunk=7, batch_size=16, num_images=40,
                                                                seed=3),
        sample_quality_normal=lambda s, m, c: Q.compute_sample_quality(s, m, num_real=50, num_fake=48, batch_size=16, seed=3,
                                                                       prior="normal"),
        sample_quality_gmm=lambda s, m, c: Q.compute_sample_quality(s, m, num_real=200, num_fake=48, batch_size=16, seed=3,
                                                                    prior="gmm", gmm_params=dict(n_components=2)),
        reconstruction_drawn=lambda s, m, c: Q.compute_reconstruction_quality(s, m, num=50, batch_size=16, seed=1),
        reconstruction_all=lambda s, m, c: Q.compute_reconstruction_quality(s, m, num=N_IMAGES, batch_size=16),
        latent_density=lambda s, m, c: Dn.compute_latent_density(s, m, num_fit=60, num_eval=30, batch_size=16, seed=2,
                                                                 n_components=2),
        vamp_prior=lambda s, m, c: Dn.vamp_prior(m, c.pseudo, batch_size=3),
    )
    return on_sampler, on_source


NAMES = ("scores", "bvae", "mod_expl", "dci", "factor_vae", "sap", "irs", "unsupervised_drawn", "unsupervised_all",
         "udr_drawn", "udr_all", "elbo_drawn", "elbo_all", "log_likelihood", "sample_quality_normal", "sample_quality_gmm",
         "reconstruction_drawn", "reconstruction_all", "latent_density", "vamp_prior")


def flatten(prefix, value, out):
    """``value`` (what a ``compute_*`` returned) as numpy arrays under ``prefix``-ed keys of ``out``."""
    if isinstance(value, dict):
        for k, v in value.items():
            flatten(f"{prefix}.{k}", v, out)
    elif dataclasses.is_dataclass(value):
        flatten(prefix, {f.name: getattr(value, f.name) for f in dataclasses.fields(value)}, out)
    elif isinstance(value, torch.Tensor):
        out[prefix] = value.detach().cpu().numpy()
    elif isinstance(value, (list, tuple)) and any(isinstance(v, (torch.Tensor, dict, tuple, list)) for v in value):
        for i, v in enumerate(value):
            flatten(f"{prefix}.{i}", v, out)
    elif value is not None:
        out[prefix] = np.asarray(value)
        assert out[prefix].dtype != object, prefix


def run(ctx, name, kind):
    """``{key: array}`` of one call on one kind of source.  The model's training flag and every buffer (the BatchNorm
    running statistics among them) must come back as they went in."""
    on_sampler, on_source = _calls()
    model = ctx.model
    before = [b.clone() for b in model.buffers()]
    assert model.training and before
    if name in on_sampler:
        got = on_sampler[name](ctx.sampler(kind), model, ctx)
    else:
        got = on_source[name](ctx.source(kind), model, ctx)
    assert model.training and all(p.training for p in ctx.peers)
    assert all(torch.equal(a, b) for a, b in zip(before, model.buffers()))
    out = {}
    flatten(f"{name}.{kind}", got, out)
    return out


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
