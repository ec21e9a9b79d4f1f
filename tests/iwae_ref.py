"""fp64 restatement of the importance-weighted bound (Burda, Grosse and Salakhutdinov 2016) and of its three gradient
estimators into the encoder (plain reparameterised; sticking the landing, Roeder et al. 2017; doubly reparameterised, Tucker
et al. 2019), the yardstick of csrc/iwae.hip: numpy for the kernel tests, torch (autograd, fp64) as the independent
expression.  Inputs mu, logvar [B, D], eps [K B, D], images x [B, P], reconstructions recon [K B, P]; row r = k B + b is
sample k of image b.  With s_b = exp(logvar_b / 2):

    z_r     = mu_b + s_b eps_r
    lat_r   = 1/2 sum_d (z_rd^2 - eps_rd^2 - logvar_bd)          log q(z_r | x_b) - log p(z_r); no clamp, no variance floor
    rows_r  = sum_p err(recon_rp, x_bp)                          err of ops.reconstruction_loss: mse | l1 | bce
    logw_r  = -(beta_rec rows_r + beta_kl lat_r)
    bound_b = logsumexp_k logw_(kB+b) - log K,   w_r = softmax_k(logw)_r,   ess_b = 1 / sum_k w_r^2
    loss    = -mean_b bound_b
    terms   = rec: beta_rec mean_b sum_k w_r rows_r, kl: beta_kl mean_b sum_k w_r lat_r, bound: mean_b bound_b, ess: mean_b ess_b

Gradients for an upstream g, a_r = g w_r / B:  d loss / d rows_r = beta_rec a_r,  d loss / d lat_r = beta_kl a_r = h_r.
With dz_r what the decoder's backward hands down:

    iwae:  t_r = dz_r + h_r z_r;                  dmu_b = sum_k t_r,  dlogvar_b = sum_k (t_r eps_r s_b / 2 - h_r / 2)
    stl:   p_r = dz_r + h_r (z_r - eps_r / s_b);  dmu_b = sum_k p_r,  dlogvar_b = sum_k p_r eps_r s_b / 2
    dreg:  as stl with p_r multiplied by w_r once more
"""
import numpy as np

ESTIMATORS = ("iwae", "stl", "dreg")
LOSS_TYPES = ("mse", "l1", "bce")


def _f64(*a):
    return tuple(np.asarray(v, np.float64) for v in a)


def sample(mu, logvar, eps):
    """(z [K B, D], lat [K B]) in fp64."""
    mu, logvar, eps = _f64(mu, logvar, eps)
    B, D = mu.shape
    K = eps.shape[0] // B
    assert eps.shape == (K * B, D)
    m, l = np.tile(mu, (K, 1)), np.tile(logvar, (K, 1))
    z = m + np.exp(0.5 * l) * eps
    return z, 0.5 * (z * z - eps * eps - l).sum(1)


def err(recon, x, loss_type):
    """The per-element error of ops.reconstruction_loss in fp64 (bce clamps both logs at -100, as torch does)."""
    recon, x = _f64(recon, x)
    if loss_type == "mse":
        return (recon - x) ** 2
    if loss_type == "l1":
        return np.abs(recon - x)
    if loss_type == "bce":
        with np.errstate(divide="ignore"):
            return -(x * np.maximum(np.log(recon), -100.0) + (1.0 - x) * np.maximum(np.log(1.0 - recon), -100.0))
    raise NotImplementedError(loss_type)


def derr(recon, x, loss_type):
    """d err / d recon, as the kernels define it (l1: the sign, 0 at 0; bce: ATen's (r - t) / max((1 - r) r, 1e-12))."""
    recon, x = _f64(recon, x)
    if loss_type == "mse":
        return 2.0 * (recon - x)
    if loss_type == "l1":
        return np.sign(recon - x)
    if loss_type == "bce":
        return (recon - x) / np.maximum((1.0 - recon) * recon, 1e-12)
    raise NotImplementedError(loss_type)


def rows(recon, x, loss_type):
    """rows [K B] in fp64: x [B, P] is broadcast over the K slabs of recon [K B, P]."""
    recon, x = _f64(recon, x)
    K = recon.shape[0] // x.shape[0]
    return err(recon, np.tile(x, (K, 1)), loss_type).sum(1)


def combine(rows_, lat, B, beta_rec, beta_kl):
    """dict(loss, rec, kl, bound, ess, w [K B], bound_b, ess_b [B], logw [K B]) from the per-row terms, max-shifted."""
    rows_, lat = _f64(rows_, lat)
    K = rows_.shape[0] // B
    logw = -(beta_rec * rows_ + beta_kl * lat)
    lw = logw.reshape(K, B)
    m = lw.max(0)
    e = np.exp(lw - m)
    s1 = e.sum(0)
    w = e / s1
    bound_b = m + np.log(s1) - np.log(float(K))
    ess_b = 1.0 / (w * w).sum(0)
    return dict(loss=-bound_b.mean(), rec=beta_rec * (w * rows_.reshape(K, B)).sum(0).mean(),
                kl=beta_kl * (w * lat.reshape(K, B)).sum(0).mean(), bound=bound_b.mean(), ess=ess_b.mean(),
                w=w.reshape(-1), bound_b=bound_b, ess_b=ess_b, logw=logw, elbo_b=lw.mean(0))


def combine_grads(w, B, beta_rec, beta_kl, g=1.0):
    """(d loss / d rows, d loss / d lat), each [K B]."""
    a = g * np.asarray(w, np.float64) / B
    return beta_rec * a, beta_kl * a


def encoder_grads(mu, logvar, eps, dz, h, w, estimator):
    """(dmu, dlogvar) [B, D] from dz [K B, D], h [K B] = d loss / d lat and the normalised weights w [K B]."""
    mu, logvar, eps, dz, h, w = _f64(mu, logvar, eps, dz, h, w)
    B, D = mu.shape
    K = eps.shape[0] // B
    z, _ = sample(mu, logvar, eps)
    s = np.tile(np.exp(0.5 * logvar), (K, 1))
    hc = h[:, None]
    if estimator == "iwae":
        t = dz + hc * z
        dmu, dlv = t, t * eps * s / 2.0 - hc / 2.0
    elif estimator in ("stl", "dreg"):
        p = dz + hc * (z - eps / s)
        if estimator == "dreg":
            p = p * w[:, None]
        dmu, dlv = p, p * eps * s / 2.0
    else:
        raise ValueError(estimator)
    return dmu.reshape(K, B, D).sum(0), dlv.reshape(K, B, D).sum(0)


def full(mu, logvar, eps, x, decoder, beta_rec, beta_kl, loss_type, estimator, g=1.0):
    """The whole objective for a LINEAR stand-in decoder recon = act(z @ decoder), act the identity (mse, l1) or the logistic
    function (bce): dict(loss, terms.., dmu, dlogvar, ddecoder)."""
    mu, logvar, eps, x, W = _f64(mu, logvar, eps, x, decoder)
    B = mu.shape[0]
    K = eps.shape[0] // B
    z, lat = sample(mu, logvar, eps)
    pre = z @ W
    recon = 1.0 / (1.0 + np.exp(-pre)) if loss_type == "bce" else pre
    r = rows(recon, x, loss_type)
    out = combine(r, lat, B, beta_rec, beta_kl)
    g_rows, g_lat = combine_grads(out["w"], B, beta_rec, beta_kl, g)
    drecon = g_rows[:, None] * derr(recon, np.tile(x, (K, 1)), loss_type)
    dpre = drecon * recon * (1.0 - recon) if loss_type == "bce" else drecon
    dz = dpre @ W.T
    out["dmu"], out["dlogvar"] = encoder_grads(mu, logvar, eps, dz, g_lat, out["w"], estimator)
    out["ddecoder"] = z.T @ dpre
    out.update(z=z, lat=lat, rows=r, dz=dz, g_lat=g_lat)
    return out


# ---- the streaming form ------------------------------------------------------------------------------------------------
def accumulate(state, rows_, lat, B, beta_rec, beta_kl):
    """Merge one chunk into state = dict(m, s1, s2, sl, n) of [B] fp64 arrays (None: empty); returns the new state."""
    rows_, lat = _f64(rows_, lat)
    K = rows_.shape[0] // B
    lw = (-(beta_rec * rows_ + beta_kl * lat)).reshape(K, B)
    m = lw.max(0)
    e = np.exp(lw - m)
    new = dict(m=m, s1=e.sum(0), s2=(e * e).sum(0), sl=lw.sum(0), n=np.full(B, float(K)))
    if state is None:
        return new
    M = np.maximum(state["m"], m)
    f0, f1 = np.exp(state["m"] - M), np.exp(m - M)
    return dict(m=M, s1=state["s1"] * f0 + new["s1"] * f1, s2=state["s2"] * f0 * f0 + new["s2"] * f1 * f1,
                sl=state["sl"] + new["sl"], n=state["n"] + K)


def finalize(state):
    """(log_px, elbo, ess), each [B]."""
    return (state["m"] + np.log(state["s1"]) - np.log(state["n"]), state["sl"] / state["n"],
            state["s1"] ** 2 / state["s2"])


# ---- the independent torch expressions -------------------------------------------------------------------------------------
def torch_rows(recon, x, loss_type):
    """rows [K B] with x [B, P] repeated, in recon's dtype: torch's own losses."""
    import torch
    F = torch.nn.functional
    xr = x.repeat(recon.shape[0] // x.shape[0], 1)
    fn = {"mse": F.mse_loss, "l1": F.l1_loss, "bce": F.binary_cross_entropy}[loss_type]
    return fn(recon, xr, reduction="none").sum(1)


def torch_loss(mu, logvar, eps, x, decode, beta_rec, beta_kl, loss_type, estimator, dreg_by_row=False):
    """(surrogate, value): ``surrogate`` is a scalar whose autograd gradient is the estimator's (in every parameter that
    ``decode`` and ``mu`` / ``logvar`` depend on); ``value`` a dict of detached scalars (loss, rec, kl, bound, ess).
    iwae: the bound itself.  stl: log q evaluated at detached (mu, logvar).  dreg: in addition the surrogate
    -mean_b sum_k sg(w)^2 logw for the encoder's path and -mean_b sum_k sg(w) logw for the decoder, separated by routing z
    through a function that is the identity forward and hands the two consumers their own gradients.
    ``dreg_by_row``: "dreg" as the kernels define it for ANY decoder: the "stl" surrogate with the gradient that arrives at
    z_r multiplied by w_r on its way into (mu, logvar).  For a decoder that treats its rows independently the two forms are
    the same gradient; a decoder with BatchNorm in training mode couples the rows of a batch, and then only this form is what
    the step computes (the weight goes with the row the gradient arrives at, not with the row whose logw it came from)."""
    import math
    import torch
    B, D = mu.shape
    K = eps.shape[0] // B
    s = torch.exp(0.5 * logvar)
    z = mu.repeat(K, 1) + s.repeat(K, 1) * eps

    def log_ratio(zz, m, l):            # log q(z | m, l) - log p(z)
        return 0.5 * (zz * zz - (zz - m.repeat(K, 1)) ** 2 * torch.exp(-l).repeat(K, 1) - l.repeat(K, 1)).sum(1)

    def logw_of(zz, m, l):
        r = torch_rows(decode(zz), x, loss_type)
        return -(beta_rec * r + beta_kl * log_ratio(zz, m, l)), r

    if estimator == "iwae":
        logw, r = logw_of(z, mu, logvar)
        lw = logw.reshape(K, B)
        surrogate = -(torch.logsumexp(lw, 0) - math.log(K)).mean()
    else:
        logw, r = logw_of(z, mu.detach(), logvar.detach())
        lw = logw.reshape(K, B)
        w = torch.softmax(lw, 0).detach()
        if estimator == "stl" or (estimator == "dreg" and dreg_by_row):
            surrogate = -(w * lw).sum(0).mean()
            if estimator == "dreg":
                z.register_hook(lambda g: g * w.reshape(-1, 1))
        elif estimator == "dreg":
            # decoder: z detached, single weight; encoder: decoder's parameters untouched, squared weight
            logw_dec, _ = logw_of(z.detach(), mu.detach(), logvar.detach())
            dec = -(w * logw_dec.reshape(K, B)).sum(0).mean()
            (gz,) = torch.autograd.grad(-(w * w * lw).sum(0).mean(), (z,), retain_graph=True)
            surrogate = dec + (z * gz.detach()).sum()
        else:
            raise ValueError(estimator)
    with torch.no_grad():
        lat = log_ratio(z, mu, logvar)
        lwv = lw.detach()
        w = torch.softmax(lwv, 0)
        bound = (torch.logsumexp(lwv, 0) - math.log(K)).mean()
        value = dict(loss=-bound, bound=bound, rec=beta_rec * (w * r.detach().reshape(K, B)).sum(0).mean(),
                     kl=beta_kl * (w * lat.reshape(K, B)).sum(0).mean(), ess=(1.0 / (w * w).sum(0)).mean())
    return surrogate, value


def make_inputs(B, K, D, seed):
    """The generator of the stored vectors: mu ~ N(0, 1), logvar ~ N(-1, 0.5^2), eps ~ N(0, 1), fp32."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(B, D)).astype(np.float32)
    logvar = (rng.normal(size=(B, D)) * 0.5 - 1.0).astype(np.float32)
    eps = rng.normal(size=(K * B, D)).astype(np.float32)
    return mu, logvar, eps


def make_images(B, K, P, seed, loss_type="mse"):
    """x [B, P] and recon [K B, P] in (0, 1), fp32; for bce a few values of recon sit at exactly 0 and 1 (the log clamp)
    and x is binary there."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(B, P)).astype(np.float32)
    recon = rng.uniform(0.02, 0.98, size=(K * B, P)).astype(np.float32)
    if loss_type == "bce":
        recon[0, 0], recon[-1, -1] = 0.0, 1.0
        x[0, 0], x[-1, -1] = 1.0, 1.0
    return x, recon
