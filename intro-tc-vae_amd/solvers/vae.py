"""VAESolver with the reference's constructor / hook / ``train_step`` surface
(/root/reference/solvers/vae.py:26-136), running the step on HIP kernels.

Shared machinery for all four solvers lives here: flat gradient buffers, the fused
clip-norm + optimiser tail, the single end-of-step host read-back and the data-parallel hooks.
"""
from typing import Optional

import torch
from torch import Tensor

from hipvae import ddp
from hipvae.functional import LinCombFn, conv_math_scope, deferred_wgrad_reduces, direct_grad_accumulation
from hipvae.flat import FlatGroup, clip_grad_norm, fused_update
from hipvae.inference import eval_mode
from models import grad_free_parameters
from ops import kl_divergence, reconstruction_loss
from utils import SingletonWriter

try:  # present when dropped into the reference tree; the hot path does not need them
    from dataset import DisentanglementDataset
except Exception:  # noqa: BLE001
    class DisentanglementDataset:  # type: ignore
        pass


class VAESolver:
    def __init__(self, dataset, model, batch_size: int, optimizer_e, optimizer_d, recon_loss_type: str,
                 beta_kl: float, beta_rec: float, device: torch.device, use_amp: bool, grad_scaler,
                 writer=None, test_iter: int = 1000, clip: Optional[float] = None):
        self.dataset = dataset
        if isinstance(dataset, DisentanglementDataset):
            try:
                from evaluation.generator import LatentGenerator
                self.latent_generator = LatentGenerator(dataset, device)
            except Exception:  # noqa: BLE001  evaluation stack is outside the hot path
                self.latent_generator = None
        self.model = model
        self.batch_size = batch_size
        self.optimizer_e, self.optimizer_d = optimizer_e, optimizer_d
        self.beta_kl, self.beta_rec = beta_kl, beta_rec
        self.device = device
        # The reference stores use_amp / grad_scaler and never uses them (no autocast anywhere).  Here use_amp selects the
        # arithmetic of the conv GEMMs: True -> "f16x3": operands as two scaled fp16 planes, three matrix-core products,
        # fp32 accumulate -- fp32 in/out and fp32-class accuracy (every parity test holds it to the exact-fp32 bar) at
        # ~5x the exact-fp32 MFMA rate; False -> exact fp32 MFMA.  ``conv_math`` may be set to "fp32" / "f16x3" /
        # "bf16x6" / "bf16x3" directly ("bf16x3" is 5 % faster than "f16x3" and 2^-16 per product: looser than the
        # reference's own fp32 on the ill-conditioned gradients); the ITCV_CONV_MATH environment variable overrides both.
        self.use_amp, self.grad_scaler = use_amp, grad_scaler
        import os as _os
        self.conv_math = _os.environ.get("ITCV_CONV_MATH") or ("f16x3" if use_amp else "fp32")
        self.writer, self.test_iter, self.clip = writer, test_iter, clip
        # MIG and modularity on the device (hipvae.disentangle): None -> when the reference's ``evaluation`` package cannot
        # be imported; True -> always (its classifier-based writers are still called when it imports); False -> never;
        # "all" -> the beta-VAE score and explicitness too; "all+dci" -> DCI as well, nothing delegated
        self.device_scores = None
        self.dci_params = None       # ``params`` of hipvae.disentangle.compute_dci_score (None: 100 rounds, depth 6)
        # scores the reference does not have, written from the device on top of the above: a tuple of names of
        # solvers.scores.TABLE, whose records say what each writes and which of the attributes below feeds it: ``params``
        # of hipvae.disentangle.compute_factor_vae_score / compute_sap_score / compute_irs_score; keyword arguments of
        # hipvae.aggregate.compute_elbo_decomposition / hipvae.disentangle.compute_unsupervised_scores (None: their
        # defaults, with this solver's batch size)
        self.extra_scores = ()
        self.factor_vae_params = None
        self.sap_params = None
        self.elbo_params = None
        self.irs_params = None
        self.unsupervised_params = None
        self.likelihood_params = None     # keyword arguments of hipvae.likelihood.compute_log_likelihood
        self.quality_params = None        # keyword arguments of hipvae.quality.compute_sample_quality
        self.reconstruction_params = None  # keyword arguments of hipvae.quality.compute_reconstruction_quality
        self.density_params = None        # keyword arguments of hipvae.density.compute_latent_density
        # "udr" ranks this model against ``udr_peers``: models trained from other seeds on the same data (a sequence of
        # networks; required by that score); ``udr_params``: ``params`` of hipvae.disentangle.compute_udr_score
        self.udr_peers = None
        self.udr_params = None
        self._device_table = None
        self.recon_loss_type = recon_loss_type
        self.scale = 1 / (self.model.cdim * self.model.encoder.image_size ** 2)   # solvers/vae.py:61
        self._flat = {}

    def use_device_dataset(self, table=None, seed=None, device_resize=None):
        """Opt in to device-resident images (hipvae.dataset): build the ``DeviceImageTable`` of ``self.dataset`` (or take
        ``table``, built earlier for the same dataset) and score through a ``DeviceFactorSampler`` on it, which draws what
        ``FactorSampler(self.dataset, self.device, seed)`` draws and looks the images up with one kernel launch instead
        of one ``__getitem__`` each.  Returns the table, so that the training loop can hand the same one to
        ``hipvae.dataset.DeviceLoader``.  ``device_resize`` ("table", "gather" or "auto") lets a dataset that resizes its
        images do so on the device (``DeviceImageTable.from_dataset``).  Without this call nothing changes."""
        from hipvae.dataset import DeviceFactorSampler, DeviceImageTable
        if table is None:
            table = DeviceImageTable.from_dataset(self.dataset, self.device, device_resize=device_resize)
        self.latent_generator = DeviceFactorSampler(self.dataset, self.device, seed=seed, table=table)
        self._device_table = table
        return table

    # ---- overridable loss hooks (solvers/vae.py:63-87) -----------------------------------
    def compute_kl_loss(self, z: Optional[Tensor], mu: Tensor, logvar: Tensor, reduce: str = "mean",
                        beta: float = None, write: bool = False) -> Tensor:
        if beta is None:
            beta = self.beta_kl
        if not (write and self.writer):
            return kl_divergence(logvar, mu, reduce=reduce, scale=beta)      # beta * kl inside the one launch
        kl = kl_divergence(logvar, mu, reduce=reduce)
        self.write_scalar(SingletonWriter().cur_iter, "kl_loss_unscaled", kl)
        return beta * kl

    def compute_rec_loss(self, x, recon_x, reduction="sum", beta: float = None, write: bool = False) -> Tensor:
        if beta is None:
            beta = self.beta_rec
        if not (write and self.writer):
            return reconstruction_loss(x, recon_x, self.recon_loss_type, reduction, scale=beta)
        rec = reconstruction_loss(x, recon_x, self.recon_loss_type, reduction)
        self.write_scalar(SingletonWriter().cur_iter, "r_loss_unscaled", rec)
        return beta * rec

    @staticmethod
    def _lincomb(weights, *terms):
        """sum_k weights[k] * terms[k] for scalar loss terms in one launch (overridden hooks that return anything but a
        device scalar fall back to torch arithmetic)."""
        if all(isinstance(t, Tensor) and t.numel() == 1 and t.is_cuda for t in terms):
            return LinCombFn.apply(tuple(weights), *terms)
        return sum(w * t for w, t in zip(weights, terms))

    # ---- optimiser tail shared by all solvers ----------------------------------------------
    def _module(self, part):
        """The module of a parameter group; with ``_optimizer`` all a solver with a further group overrides."""
        return getattr(self.model, part)

    def _optimizer(self, part):
        return self.optimizer_e if part == "encoder" else self.optimizer_d

    def _params(self, part):
        """Parameter list of one group, walked once per (solver, module) -- ``module.parameters()`` re-walks the
        module tree on every call (~1.5 ms of host time per step over the handful of calls a step makes)."""
        mod = self._module(part)
        ent = self.__dict__.setdefault("_plists", {}).get(part)
        if ent is None or ent[0] is not mod:
            ent = self._plists[part] = (mod, list(mod.parameters()))
        return ent[1]

    def _group(self, part) -> FlatGroup:
        params = self._params(part)
        g = self._flat.get(part)
        if g is None or not g.owns(params):
            # ownership lost (model.to() / .float() / load_state_dict(assign=True) after the first step): the new group
            # inherits the optimiser state and step count instead of restarting them
            g = self._flat[part] = FlatGroup(params, inherit=g,
                                             grad_free=grad_free_parameters(self._module(part)))
        return g

    def _set_trainable(self, encoder: bool, decoder: bool):
        for p in self._params("encoder"):
            p.requires_grad = encoder
        for p in self._params("decoder"):
            p.requires_grad = decoder

    def _backward(self, loss, parts, defer_average=False, retain_graph=False, inputs=None):
        """optimizer.zero_grad() of ``parts`` + loss.backward() + gradient averaging over ranks.  With
        ``defer_average`` the all-reduces are only started; the returned callable finishes them (data-parallel runs
        overlap them with work that does not depend on the averaged gradients).  ``retain_graph`` / ``inputs``: those of
        ``Tensor.backward`` (``inputs``: the walk runs only the nodes that lead to these tensors)."""
        groups = [self._group(p) for p in parts]
        for g in groups:
            g.zero_grad()
        # wgrad / BN / bias kernels add straight into the flat buffers; the planes weight gradients' slab reduces of the whole
        # backward pass are folded by one launch when it is over
        with direct_grad_accumulation(), deferred_wgrad_reduces():
            loss.backward(retain_graph=retain_graph, inputs=inputs)
        if defer_average:
            pending = [ddp.average_async(g.flat_g) for g in groups]
            return lambda: [f() for f in pending]
        for g in groups:
            ddp.average_(g.flat_g)
        return None

    def _clip(self):
        """clip_grad_norm_ over ALL parameters with a gradient, stale frozen-half gradients included
        (solvers/intro.py:113-115,157-159).  Returns the norm as a device scalar (or None)."""
        if not self.clip:
            return None
        return clip_grad_norm([self._group("encoder"), self._group("decoder")], self.clip)

    def _step(self, part):
        opt = self._optimizer(part)
        spec = fused_update(opt)
        if spec is None:
            opt.step()                       # an optimiser config without a fused update: torch's own
        else:
            g = self._group(part)
            g.bind_optimizer(opt, spec)      # state visible in (and adopted from) opt.state / state_dict()
            g.fused_step(spec)

    # ---- step execution: eager, or one hipGraph replay -----------------------------------------
    def enable_graph(self, flag: bool = True):
        """Capture the whole training step (every kernel of both phases, the optimiser tail and the
        RNG draws) into ONE hipGraph after a few eager warm-up steps and replay it per step: the
        ~1.4 k launches of a step then cost one submission.  Used without a writer, with device-side noise, and
        single-rank unless ``ddp.graph_capturable()`` (RCCL collectives captured in the graph; opt-in, see there);
        anything else silently runs eagerly."""
        self._graph_on = bool(flag)
        self._graph = None
        self._graphs, self._graph_warm = {}, {}
        return self

    def _graph_ok(self, specs=None):
        """``specs``: (fused_update(optimizer_e), fused_update(optimizer_d)) when the caller has them already."""
        import ops
        if not (getattr(self, "_graph_on", False) and self.writer is None
                and (ddp.get() is None or ddp.graph_capturable())
                and ops._noise["queue"] is None and ops._noise["mode"] == "device"):
            return False
        if specs is None:
            specs = (fused_update(self.optimizer_e), fused_update(self.optimizer_d))
        return specs[0] is not None and specs[1] is not None

    def _run(self, real: Tensor) -> Tensor:
        """Runs ``_device_step`` eagerly or through the captured graph; returns the device stats vector."""
        with conv_math_scope(self.conv_math):
            return self._run_scoped(real)

    def _run_scoped(self, real: Tensor) -> Tensor:
        specs = (fused_update(self.optimizer_e), fused_update(self.optimizer_d)) if getattr(self, "_graph_on", False) \
            else None
        if not self._graph_ok(specs):
            return self._device_step(real)
        # the optimiser hyper-parameters are scalar kernel arguments frozen into a captured graph: the update specs are
        # part of its key, so a scheduler or manual decay of param_groups[0]["lr"] re-captures instead of being ignored
        # the TC solvers' KL hook ("simple" | "full") selects different kernels: a switch re-captures too
        # the conv entry: the arithmetic, and the module-level routing threshold of the upsampled convs' data gradient
        # (both select kernels; one element, so that the specs and everything behind them keep their places)
        from hipvae.functional import UP2_FOLD_MIN_BYTES, bump_weight_epoch
        key = (tuple(real.shape), real.dtype, (self.conv_math, UP2_FOLD_MIN_BYTES[0])) + specs + self._graph_key_extra() \
            + self._schedule_key() + (getattr(self, "kl_loss", None),)
        graphs = self.__dict__.setdefault("_graphs", {})
        ent = graphs.get(key)
        if ent is None:
            # eager warm-up before a capture: 3 steps for the first graph (allocator, flat buffers, caches), one for
            # every further key (a new batch shape -- the last partial batch of an epoch -- or new hyper-parameters)
            warm = self.__dict__.setdefault("_graph_warm", {})
            warm[key] = warm.get(key, 0) + 1
            if warm[key] <= (3 if not graphs else 1):
                return self._device_step(real)
            while len(graphs) >= 4:                       # keep a handful of shapes alive; the oldest goes first
                graphs.pop(next(iter(graphs)))
            ent = dict(inp=real.clone())
            bump_weight_epoch()                          # every weight gets re-packed inside the graph
            torch.cuda.synchronize()
            ent["graph"] = torch.cuda.CUDAGraph()
            # thread-local capture mode: the input pipeline's staging thread (hipvae.loader) may allocate pinned memory or
            # issue copies on its own stream while this thread captures, and RCCL's watchdog thread may query events.
            # Data-parallel capture additionally needs the watchdog's work list EMPTY before the capture begins: the
            # watchdog polls the end events of the eager steps' collectives, those events live on the communicator's
            # stream, that stream joins the capture, and HIP refuses a query on such an event ("operation not permitted
            # on an event last recorded in a capturing stream" / "... when stream is capturing" -> abort()).
            # ddp.drain_pending_collectives() blocks on exactly that condition (ProcessGroupNCCL::waitForPendingWorks: the
            # watchdog has retired every enqueued Work); the device is idle (synchronize above) so it terminates, and
            # collectives issued DURING a capture are never handed to the watchdog (c10d skips the enqueue when the
            # current stream is capturing) -- nothing is left for it to poll until the first eager collective after the
            # capture.  No timing assumption.
            ddp.drain_pending_collectives()
            mode = "thread_local"
            with torch.cuda.graph(ent["graph"], capture_error_mode=mode):
                ent["out"] = self._device_step(ent["inp"])
            graphs[key] = ent
        self._graph, self._graph_key, self._graph_in, self._graph_out = ent["graph"], key, ent["inp"], ent["out"]
        ent["inp"].copy_(real)
        ent["graph"].replay()
        bump_weight_epoch()                              # eager users after a replay must re-pack
        return ent["out"]

    def _schedule_key(self) -> tuple:
        """What else selects the kernels of a step (part of the captured graph's key)."""
        return ()

    def _graph_key_extra(self) -> tuple:
        """Further kernel-selecting switches of a solver; they sit behind the update specs and in front of the schedule
        key, so the specs keep their places at the front of the graph key and the schedule key and the KL mode at its end."""
        return ()

    # ---- solvers/vae.py:89-136 ---------------------------------------------------------------
    # The one VAE step.  An objective supplies what differs: ``_losses`` (how z and the two loss terms come out of the
    # batch, and its further device scalars), ``_batch`` (the batch check), ``_write_losses`` / ``_extra_results`` (what
    # it logs and returns for those scalars); FactorVAE also ``_side_walk`` and ``_updates`` for its third group; the
    # VampPrior solver ``_walk``: its third group takes its gradient from the VAE's own backward.
    _updates = ("encoder", "decoder")
    _walk = ("decoder", "encoder")

    def _losses(self, real: Tensor):
        """(z, loss_rec, loss_kl, extra): ``extra`` a device vector of further scalars for the stats, or None."""
        mu, logvar, z, rec = self.model(real)
        loss_rec = self.compute_rec_loss(real, rec, reduction="mean", write=True)
        return z, loss_rec, self.compute_kl_loss(z, mu, logvar, write=True), None

    def _side_walk(self, z: Tensor):
        """Between the VAE's backward and the clip: a further loss and walk over a group of its own."""

    def _total_loss(self, loss_rec: Tensor, loss_kl: Tensor) -> Tensor:
        """The scalar the step differentiates, from what ``_losses`` returned: scale * (loss_rec + loss_kl), vae.py:106.
        An objective whose loss is not that sum overrides this."""
        return self._lincomb((self.scale, self.scale), loss_rec, loss_kl)

    def _device_step(self, real: Tensor) -> Tensor:
        """Returns the stats vector [loss, loss_kl, loss_rec, *extra, norm]."""
        self._set_trainable(True, True)
        z, loss_rec, loss_kl, extra = self._losses(real)
        loss = self._total_loss(loss_rec, loss_kl)
        self._backward(loss, self._walk)
        self._side_walk(z)
        norm = self._clip()
        for part in self._updates:
            self._step(part)
        stats = torch.stack([loss.detach(), loss_kl.detach(), loss_rec.detach()])
        if extra is not None:
            stats = torch.cat([stats, extra])
        ddp.mean_scalars_(stats)
        return torch.cat([stats, norm if norm is not None else stats.new_zeros(1)])

    def _batch(self, batch: Tensor) -> Tensor:
        return batch.unsqueeze(0) if batch.dim() == 3 else batch

    def _write_losses(self, cur_iter: int, v_kl: float, v_rec: float, *extra):
        self.write_scalars(cur_iter, losses=dict(r_loss=v_rec, kl_loss=v_kl))

    def _extra_results(self, *extra) -> dict:
        return {}

    def train_step(self, batch: Tensor, cur_iter: int) -> dict:
        real = self._batch(batch).to(self.device)
        v_loss, v_kl, v_rec, *extra, v_norm = self._run(real).tolist()     # the step's only host read-back
        if v_loss != v_loss:
            raise RuntimeError
        if self.writer:
            self._write_losses(cur_iter, v_kl, v_rec, *extra)
            if self.clip:
                self.writer.add_scalar("total_norm", v_norm, global_step=cur_iter)
            self.write_gradient_norm(cur_iter)
            self._write_images_helper(real, cur_iter)
            self.write_disentanglemnt_scores(cur_iter)
            self.writer.flush()
        # the reference leaves L2 unbound when clip is falsy (vae.py:135); None is returned instead
        return {"loss_enc": v_loss, "loss_dec": v_loss, "loss_kl": v_kl, "loss_rec": v_rec,
                "L2": v_norm if self.clip else None, **self._extra_results(*extra)}

    # ---- TensorBoard side channel (solvers/vae.py:138-254); all no-ops without a writer ------
    def _eval_prior(self):
        """The model's own prior for "sample_quality" and "latent_density" when their params name none: None is N(0, I);
        a solver with a learned prior returns what ``hipvae.quality.compute_sample_quality(prior=...)`` takes."""
        return None

    def _write_images_helper(self, batch, cur_iter):
        if self.writer is not None and cur_iter % self.test_iter == 0:
            noise = torch.randn(size=(batch.size(0), self.model.zdim), device=self.device)
            with torch.no_grad():
                fake = self.model.sample(noise)
            self.write_images(batch, fake, cur_iter)

    def write_images(self, batch, fake_batch, cur_iter):
        if self.writer is not None and cur_iter % self.test_iter == 0:
            with torch.no_grad():
                _, _, _, rec_det = self.model(batch, deterministic=True)
            k = min(batch.size(0), 16)
            grid = torch.cat([batch[:k], rec_det[:k], fake_batch[:k]], dim=0).data.cpu()
            self.writer.add_images("reconstructions", grid, global_step=cur_iter)

    def write_gradient_norm(self, cur_iter: int):
        grads = [p.grad.detach().norm(2) for p in self.model.encoder.fc.parameters() if p.grad is not None]
        if grads:
            self.writer.add_scalar("fc_grad_norm", torch.stack(grads).norm(2).item(), global_step=cur_iter)

    def write_scalar(self, cur_iter: int, tag: str, value: Tensor):
        if self.writer and value.dim() == 0:
            self.writer.add_scalar(tag, value.data.item(), global_step=cur_iter)

    def write_scalars(self, cur_iter: int, losses: dict, **kwargs):
        if self.writer is not None:
            self.write_losses(cur_iter, losses)
            for name, value in kwargs.items():
                self.writer.add_scalar(name, value, global_step=cur_iter)

    def write_losses(self, cur_iter: int, losses: dict):
        if self.writer is not None:
            self.writer.add_scalars("losses", losses, global_step=cur_iter)

    def write_disentanglemnt_scores(self, cur_iter: int, num_samples: int = 10000):
        """solvers/vae.py:188-213, at a test iteration and with a writer.  For a ``DisentanglementDataset`` the factor scores
        come first.  The reference's ``evaluation`` package writes all four of its scores when it imports (it needs sklearn
        and xgboost).  MIG and modularity do not need it: they are computed on the device (``device_scores``,
        hipvae.disentangle) from one encode of the sampled images, in eval mode, with a private numpy generator (torch's
        RNG streams and the BatchNorm running buffers are untouched).  The classifier-based scores stay delegated unless
        ``device_scores == "all"``: then ``bvae_score`` {score, scaled} and ``mod_expl`` {modularity_score,
        explicitness_score} are written from the device too (metrics.py:11-17, 222-234) and only DCI is delegated.
        ``device_scores == "all+dci"`` writes those three records and then ``dci`` {dci_informativeness_score,
        dci_completeness_score, dci_disentanglement_score} from the device (metrics.py:82-103; ``dci_params``) and
        delegates nothing: ``evaluation`` is not imported.
        ``extra_scores`` adds, after all of the above and whatever ``device_scores`` says, the records of
        ``solvers.scores.TABLE`` that it names, in the table's order: the factor scores among them for a
        ``DisentanglementDataset`` only, the others for any dataset, from the device table when ``use_device_dataset``
        was called."""
        from solvers import scores              # with the evaluation modules behind it: not needed to train
        extras = tuple(self.extra_scores or ())
        factored = isinstance(self.dataset, DisentanglementDataset)
        if self.writer is None or not (factored or any(e in scores.TABLE and not scores.TABLE[e].factors for e in extras)) \
                or cur_iter % self.test_iter:
            return
        unknown = [e for e in extras if e not in scores.TABLE]
        if unknown:
            raise ValueError(f"extra_scores: unknown score(s) {unknown} (known: {', '.join(map(repr, scores.KNOWN))})")
        wanted = [score for score in scores.TABLE.values() if score.name in extras]
        if factored:
            self._write_factor_scores(cur_iter, num_samples, [score for score in wanted if score.factors])
        source = self.dataset if self._device_table is None else self._device_table
        for score in wanted:
            if not score.factors:
                scores.write(score, self, source, cur_iter)

    def _write_factor_scores(self, cur_iter: int, num_samples: int, extras: list):
        """The factor-based scores of ``write_disentanglemnt_scores`` (a ``DisentanglementDataset``, at a test iteration):
        the ``device_scores`` ladder, then the factor records of ``extra_scores``, all with the model in eval mode."""
        from solvers import scores
        with_dci = isinstance(self.device_scores, str) and self.device_scores == "all+dci"
        M = None
        if not with_dci:
            try:
                from evaluation import metrics as M
            except Exception:  # noqa: BLE001
                M = None
        native = (M is None) if self.device_scores is None else bool(self.device_scores)
        if M is None and not native and not extras:
            return
        if native or extras:
            from hipvae import disentangle
            if getattr(self, "latent_generator", None) is None:
                self.latent_generator = disentangle.FactorSampler(self.dataset, self.device)
        n = num_samples if len(self.dataset) >= num_samples else len(self.dataset) // 2
        everything = with_dci or (isinstance(self.device_scores, str) and self.device_scores == "all")
        with eval_mode(self.model):
            if M is not None:
                kw = dict(latent_generator=self.latent_generator, model=self.model, num_samples=n,
                          batch_size=self.batch_size)
                writers = (() if everything else (M.write_bvae_score,)) + (M.write_dci_score,) + \
                    (() if native else (M.write_mig_score, M.write_mod_expl_score))
                for fn in writers:
                    fn(self.writer, cur_iter, **kw)
            if everything:
                for tag in ("bvae_score", "mig_score", "mod_expl") + (("dci",) if with_dci else ()):
                    scores.write(scores.DEVICE[tag], self, self.latent_generator, cur_iter, n)
            elif native:        # MIG and modularity from ONE encode
                got = disentangle.compute_scores(self.latent_generator, self.model, num_samples=n,
                                                 batch_size=self.batch_size)
                self.writer.add_scalar("mig_score", got["mig"], global_step=cur_iter)
                self.writer.add_scalars("mod_expl", dict(modularity_score=got["modularity"]), global_step=cur_iter)
            for score in extras:
                scores.write(score, self, self.latent_generator, cur_iter)

    def write_gradient_flow(self, cur_iter, named_parameters):
        """Matplotlib figure of per-layer gradient magnitudes in the reference; not reproduced."""
        return None
