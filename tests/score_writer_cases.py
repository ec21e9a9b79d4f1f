"""What ``VAESolver.write_disentanglemnt_scores`` calls, in which order and with what, on the CPU: stubs for every
``compute_*`` entry point of the evaluation modules, a logging writer, a fake ``evaluation.metrics`` and the case list that
``tests/golden/make_golden_score_writer.py`` records and ``tests/test_score_writer_host.py`` replays.  No case touches a
device: the stubs return fixed values, so a log states the writer's own decisions and nothing else."""
import contextlib
import json
import sys
import types

import torch

NET = dict(cdim=3, zdim=8, channels=(8, 16), image_size=32)
NON_FACTOR = ("elbo_decomposition", "unsupervised", "udr", "log_likelihood", "sample_quality", "reconstruction_quality",
              "latent_density")
FACTOR = ("factor_vae", "sap", "irs")
ALL_EXTRAS = ("factor_vae", "sap", "elbo_decomposition", "irs", "unsupervised", "udr", "reconstruction_quality",
              "latent_density", "log_likelihood", "sample_quality")
PARAMS_OF = dict(elbo_decomposition="elbo_params", unsupervised="unsupervised_params", udr="udr_params",
                 log_likelihood="likelihood_params", sample_quality="quality_params",
                 reconstruction_quality="reconstruction_params", latent_density="density_params",
                 factor_vae="factor_vae_params", sap="sap_params", irs="irs_params")
NAN = float("nan")


class Table:
    """Stands for a ``DeviceImageTable``: the writer only passes it on."""

    def __len__(self):
        return 100


class Prior:
    """What a solver's ``_eval_prior()`` may return."""


def _plain(value):
    """A JSON value that says what was passed: numbers, strings and containers as they are, nan as a string (nan != nan
    would fail every comparison), any other object as its type's name."""
    if isinstance(value, float) and value != value:
        return "nan"
    if value is None or isinstance(value, (bool, int, float, str)):
        return value
    if isinstance(value, dict):
        return {str(k): _plain(v) for k, v in sorted(value.items(), key=lambda kv: str(kv[0]))}
    if isinstance(value, (list, tuple)):
        return [_plain(v) for v in value]
    return type(value).__name__


def _source(arg):
    if isinstance(arg, Table):
        return "table"
    return "dataset" if hasattr(arg, "__getitem__") and hasattr(arg, "__len__") and not isinstance(arg, (list, tuple)) \
        else None


def _udr_result(all_nan):
    import numpy as np
    col = [NAN, NAN, NAN] if all_nan else [NAN, 0.25, NAN]
    pairwise = np.array([[NAN, 0.1, 0.2], [col[1], NAN, 0.3], [col[2], 0.4, NAN]])
    return dict(model_scores=[0.625, 0.5, 0.375], pairwise_disentanglement_scores=pairwise, extra=1.0)


RETURNS = {
    ("disentangle", "compute_bvae_score"): (0.11, 0.12),
    ("disentangle", "compute_mig_score"): 0.13,
    ("disentangle", "compute_modularity_score"): 0.14,
    ("disentangle", "compute_explicitness_score"): 0.15,
    ("disentangle", "compute_mod_expl_score"): (0.16, 0.17),
    ("disentangle", "compute_dci_score"): (0.18, 0.19, 0.21),
    ("disentangle", "compute_scores"): dict(mig=0.22, modularity=0.23, extra=9.0),
    ("disentangle", "compute_factor_vae_score"): (0.24, 0.26),
    ("disentangle", "compute_sap_score"): 0.27,
    ("disentangle", "compute_irs_score"): dict(avg_score=0.28, num_active_dims=3, parents=None),
    ("disentangle", "compute_unsupervised_scores"): dict(
        gaussian_total_correlation=0.31, gaussian_wasserstein_correlation=0.32, gaussian_wasserstein_correlation_norm=0.33,
        mutual_info_score=0.34, covariance=None),
    ("disentangle", "compute_udr_score"): None,            # per case: ``_udr_result``
    ("aggregate", "compute_elbo_decomposition"): dict(mi=0.41, tc=0.42, dwkl=0.43, kl=0.44, kl_analytic=0.45,
                                                      joint_entropy=0.46, marginal_entropies=None, dimwise_kl=None),
    ("likelihood", "compute_log_likelihood"): dict(log_px=-0.51, bits_per_dim=0.52, elbo=-0.53, ess=0.54, per_image=None),
    ("quality", "compute_sample_quality"): dict(frechet=0.61, kid=0.62, kid_std=0.63, precision=0.64, recall=0.65,
                                                density=0.66, coverage=0.67, features=None, indices=None),
    ("quality", "compute_reconstruction_quality"): dict(psnr=0.71, ssim=0.72, ms_ssim=0.73, mse=0.74, l1=0.75,
                                                        per_image=None, indices=None),
    ("density", "compute_latent_density"): dict(gmm=None, loglik_fit=0.81, loglik_heldout=0.82, loglik_prior=0.83, gap=0.84,
                                                n_iter=5, converged=True, latents=None, indices=None),
}


@contextlib.contextmanager
def stubbed(log, evaluation="absent", udr_all_nan=False, raises=None):
    """Every ``compute_*`` above replaced by a function that appends ``["compute", "module.name", positional type names,
    source, keyword arguments, the model's training flag]`` to ``log`` and returns its fixed value; ``density.vamp_prior``
    likewise (a ``Prior``); ``sys.modules["evaluation"]`` a fake whose ``metrics.write_*`` log (``"fake"``) or None, so
    that the import fails (``"absent"``).  ``raises``: the ``module.name`` of one stub that raises ``RuntimeError`` after
    logging.  Everything is put back on the way out."""
    from hipvae import aggregate, density, disentangle, likelihood, quality
    mods = dict(aggregate=aggregate, density=density, disentangle=disentangle, likelihood=likelihood, quality=quality)
    saved = []

    def stub(mod, name, value):
        full = f"{mod}.{name}"

        def fn(*args, **kw):
            src = [s for s in map(_source, args) if s]
            mode = [a.training for a in args if isinstance(a, torch.nn.Module)]
            log.append(["compute", full, [type(a).__name__ for a in args], src[0] if src else None, _plain(kw),
                        mode[0] if mode else None])
            if raises == full:
                raise RuntimeError(f"{full} failed")
            return value

        saved.append((mods[mod], name, getattr(mods[mod], name)))
        setattr(mods[mod], name, fn)

    for (mod, name), value in RETURNS.items():
        stub(mod, name, _udr_result(udr_all_nan) if name == "compute_udr_score" else value)
    stub("density", "vamp_prior", Prior())

    def metric(name):
        def fn(writer, cur_iter, **kw):
            log.append(["metrics", name, type(writer).__name__, cur_iter, _plain(kw), kw["model"].training])
        return fn

    fake = None
    if evaluation == "fake":
        fake = types.ModuleType("evaluation")
        fake.metrics = types.ModuleType("evaluation.metrics")
        for name in ("write_bvae_score", "write_dci_score", "write_mig_score", "write_mod_expl_score"):
            setattr(fake.metrics, name, metric(name))
    had = {k: sys.modules.get(k, KeyError) for k in ("evaluation", "evaluation.metrics")}
    sys.modules["evaluation"] = fake
    sys.modules["evaluation.metrics"] = fake.metrics if fake is not None else None
    try:
        yield
    finally:
        for k, v in had.items():
            if v is KeyError:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for mod, name, fn in saved:
            setattr(mod, name, fn)


class Writer:
    def __init__(self, log):
        self.log = log

    def add_scalar(self, tag, value, global_step=None):
        self.log.append(["add_scalar", tag, _plain(value), global_step])

    def add_scalars(self, tag, values, global_step=None):
        self.log.append(["add_scalars", tag, [[k, _plain(v)] for k, v in values.items()], global_step])


def _datasets():
    from solvers.vae import DisentanglementDataset

    class Factored(DisentanglementDataset):
        factor_sizes, latent_indices = [1, 5, 4, 5], [1, 2, 3]

        def __init__(self, n=100):
            self.n = n

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            return torch.zeros(3, 32, 32), 0

    class Plain:
        def __len__(self):
            return 100

        def __getitem__(self, i):
            return torch.zeros(3, 32, 32)

    return Factored, Plain


def case(name, factored=False, extras=(), device_scores=None, evaluation="absent", writer=True, step=0, test_iter=1,
         table=False, attrs=None, eval_prior=False, peers=0, udr_all_nan=False, solver="vae", num_samples=None, length=100,
         raises=None):
    return dict(name=name, factored=factored, extras=list(extras), device_scores=device_scores, evaluation=evaluation,
                writer=writer, step=step, test_iter=test_iter, table=table, attrs=attrs or {}, eval_prior=eval_prior,
                peers=peers, udr_all_nan=udr_all_nan, solver=solver, num_samples=num_samples, length=length, raises=raises)


def cases():
    out = [case("no writer", factored=True, extras=ALL_EXTRAS, device_scores="all+dci", peers=1, writer=False),
           case("off the test iteration", factored=True, extras=ALL_EXTRAS, device_scores="all+dci", peers=1, step=3,
                test_iter=5),
           case("on a later test iteration", factored=True, extras=("sap", "elbo_decomposition"), device_scores=True,
                step=10, test_iter=5),
           case("plain, nothing asked"), case("plain, unknown name alone is silent", extras=("mig",)),
           case("plain, factor extra alone is silent", extras=("sap",)),
           case("plain, unknown name next to a known one", extras=("mig", "unsupervised")),
           case("factored, unknown names", factored=True, extras=("irs", "mig", "nope")),
           case("factored, unknown name, no writer", factored=True, extras=("mig",), writer=False)]
    params = dict(elbo_decomposition=dict(num_samples=64, seed=3), unsupervised=dict(num_train=50, batch_size=7),
                  udr=dict(correlation="spearman"), log_likelihood=dict(num_samples=5, loss_type="bce", beta_rec=1.0),
                  sample_quality=dict(num_real=40, batch_size=9), reconstruction_quality=dict(num=30, window=7),
                  latent_density=dict(num_fit=20, n_components=2))
    for e in NON_FACTOR:
        peers = 2 if e == "udr" else 0
        for table in (False, True):
            out.append(case(f"{e} alone, table={table}", extras=(e,), table=table, peers=peers))
        out.append(case(f"{e} alone, with params", extras=(e,), attrs={PARAMS_OF[e]: params[e]}, peers=peers, table=True))
        out.append(case(f"{e} alone, factored dataset, nothing native", factored=True, extras=(e,), device_scores=False,
                        peers=peers))
    every = {PARAMS_OF[e]: params[e] for e in NON_FACTOR}
    for table in (False, True):
        out.append(case(f"every non-factor extra, table={table}", extras=NON_FACTOR, table=table, peers=2))
        out.append(case(f"every non-factor extra, with params, table={table}", extras=NON_FACTOR, attrs=every, table=table,
                        peers=2))
    out.append(case("every non-factor extra, reversed order in extra_scores", extras=NON_FACTOR[::-1], peers=1))
    for table in (False, True):
        out.append(case(f"own prior, table={table}", extras=("sample_quality", "latent_density"), eval_prior=True,
                        table=table))
    out.append(case("own prior, params name a prior", extras=("sample_quality", "latent_density"), eval_prior=True,
                    attrs=dict(quality_params=dict(prior="gmm", num_real=20), density_params=dict(prior=None, num_fit=10))))
    out.append(case("own prior, params name none", extras=("sample_quality", "latent_density"), eval_prior=True,
                    attrs=dict(quality_params=dict(num_real=20), density_params=dict(num_fit=10))))
    dci = dict(informativeness_params=dict(n_estimators=5, max_depth=2))
    for ev in ("fake", "absent"):
        for ds in (None, True, False, "all", "all+dci"):
            out.append(case(f"factored, device_scores={ds!r}, evaluation {ev}", factored=True, device_scores=ds,
                            evaluation=ev))
            out.append(case(f"factored, device_scores={ds!r}, evaluation {ev}, dci_params and factor extras, table",
                            factored=True, device_scores=ds, evaluation=ev, extras=FACTOR, table=True,
                            attrs=dict(dci_params=dci, factor_vae_params=dict(num_train=20), sap_params=dict(C=0.5),
                                       irs_params=dict(diff_quantile=0.9))))
            for e in FACTOR:
                out.append(case(f"factored, device_scores={ds!r}, evaluation {ev}, {e} alone", factored=True,
                                device_scores=ds, evaluation=ev, extras=(e,)))
            for num, length in ((64, 100), (100, 100), (101, 100), (None, 100), (None, 10000), (None, 10001)):
                out.append(case(f"factored, device_scores={ds!r}, evaluation {ev}, num_samples={num}, len={length}",
                                factored=True, device_scores=ds, evaluation=ev, num_samples=num, length=length))
    out.append(case("everything at once", factored=True, extras=ALL_EXTRAS, device_scores="all+dci", peers=1, table=True,
                    attrs=dict(dci_params=dci, **every)))
    out.append(case("everything at once, evaluation fake, device_scores None", factored=True, extras=ALL_EXTRAS,
                    evaluation="fake", peers=1))
    out.append(case("udr with peers", extras=("udr",), peers=2))
    out.append(case("udr with peers, all-nan column", extras=("udr",), peers=2, udr_all_nan=True))
    out.append(case("udr without peers", extras=("udr",)))
    out.append(case("udr without peers, after the factor block", factored=True, extras=("sap", "udr"), device_scores=True))
    out.append(case("udr with an empty peer list", extras=("udr",), attrs=dict(udr_peers=[])))
    out.append(case("vamp, log_likelihood", extras=("log_likelihood",), solver="vamp"))
    out.append(case("vamp, log_likelihood, no writer", extras=("log_likelihood",), solver="vamp", writer=False))
    out.append(case("vamp, own prior", extras=("sample_quality", "latent_density"), solver="vamp"))
    out.append(case("vamp, own prior, factored", factored=True, extras=("sample_quality", "irs"), solver="vamp",
                    device_scores="all"))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


def make_solver(c, log):
    import models
    import solvers
    Factored, Plain = _datasets()
    model = models.SoftIntroVAE(arch="conv", **NET).train()
    dataset = Factored(c["length"]) if c["factored"] else Plain()
    args = (dataset, model, 4, torch.optim.Adam(model.encoder.parameters()), torch.optim.Adam(model.decoder.parameters()),
            "mse", 0.5, 0.75, torch.device("cpu"), False, None)
    if c["solver"] == "vamp":
        pseudo = models.PseudoInputs(7, NET["cdim"], NET["image_size"])
        s = solvers.VampSolver(*args, pseudo_inputs=pseudo, optimizer_prior=torch.optim.Adam(pseudo.parameters()))
    else:
        s = solvers.VAESolver(*args)
    s.writer, s.test_iter = (Writer(log) if c["writer"] else None), c["test_iter"]
    s.extra_scores, s.device_scores = tuple(c["extras"]), c["device_scores"]
    if c["peers"]:
        s.udr_peers = [models.SoftIntroVAE(arch="conv", **NET) for _ in range(c["peers"])]
    if c["table"]:
        s._device_table = Table()
    if c["eval_prior"]:
        s._eval_prior = Prior
    for k, v in c["attrs"].items():
        setattr(s, k, v)
    return s


def run_case(c):
    """The log of one case: the calls in order, then ``["raised", type, message up to "(known: "]`` if the writer raised,
    then ``["training", flag]``: the model's training flag afterwards (it went in as True)."""
    log = []
    with stubbed(log, c["evaluation"], c["udr_all_nan"], c["raises"]):
        s = make_solver(c, log)
        try:
            if c["num_samples"] is None:
                s.write_disentanglemnt_scores(c["step"])
            else:
                s.write_disentanglemnt_scores(c["step"], c["num_samples"])
        except Exception as e:  # noqa: BLE001  the log states which
            msg = str(e)
            cut = msg.find("(known: ")
            log.append(["raised", type(e).__name__, msg if cut < 0 else msg[:cut + len("(known: ")]])
        log.append(["training", s.model.training])
    return json.loads(json.dumps(log))
