"""fp64 restatement of the latent op of Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020; disentanglement_lib's ``weak``
module, ``GroupVAEBase`` with ``aggregate_argmax``), the yardstick of csrc/ada.hip: numpy (forward and the analytic
backward) for the kernel tests, torch (autograd, any dtype; a transcription of the library's own lines) for the step tests.

2B stacked rows, rows b and B + b a pair (m1, l1), (m2, l2); per dimension d:

    delta = exp(l1 - l2) + (m2 - m1)^2 exp(-l2) - 1 + l2 - l1     (the library's compute_kl: no 1/2, one direction)
    tau   = (min_d delta + max_d delta) / 2,   own = delta >= tau  (an external mask replaces it)
    gvae:   mb = (m1 + m2) / 2, vb = (e^l1 + e^l2) / 2;   mlvae:  vb = 2 e^l1 e^l2 / (e^l1 + e^l2), mb = vb (m1 e^-l1 + m2 e^-l2) / 2
    (mt_i, lt_i) = own ? (m_i, l_i) : (mb, log vb);   z_i = mt_i + eps_i exp(lt_i / 2)
    loss  = beta * mean_{2B rows} -1/2 sum_d (1 + lt - mt^2 - e^lt)

The backward holds the mask fixed.  With G_z = dz (the gradient of z), g the gradient of the loss, g_k = g beta / (2B):

    own:    dm_i = G_zi + g_k m_i,   dl_i = G_zi eps_i e^(l_i / 2) / 2 + g_k (e^l_i - 1) / 2
    shared: G_m = G_z1 + G_z2 + 2 g_k mb          (both rows of the pair carry mb: through z, and through the KL twice)
            G_l = sqrt(vb) (G_z1 eps_1 + G_z2 eps_2) / 2 + g_k (vb - 1)        (d / d log vb)
      gvae:   d mb / d m_i = 1/2;  d log vb / d l_i = e^l_i / (e^l1 + e^l2)
              dm_i = G_m / 2,   dl_i = G_l e^l_i / (e^l1 + e^l2)
      mlvae:  with the precisions p_i = e^-l_i, P = p_1 + p_2:  mb = (m_1 p_1 + m_2 p_2) / P,  log vb = log 2 - log P,
              d p_i / d l_i = -p_i, so with w_i = p_i / P
              d mb / d m_i = w_i,   d mb / d l_i = (-m_i p_i P + (m_1 p_1 + m_2 p_2) p_i) / P^2 = w_i (mb - m_i),
              d log vb / d l_i = w_i
              dm_i = G_m w_i,   dl_i = G_l w_i + G_m w_i (mb - m_i)

``defect`` names one deliberate mistake a kernel could make (DEFECTS): tests/test_ada_ref_host.py shows that each of them
moves a quantity the GPU test compares above that test's bar.
"""
import numpy as np

AVERAGINGS = ("gvae", "mlvae")
MASKS = ("threshold", "external")
MARGIN = 1e-9
DEFECTS = ("half_in_delta",            # 1/2 on the log term of delta (log sigma for log variance); a 1/2 on ALL of delta
                                       # scales the threshold with it and is no defect
           "symmetric_delta",          # the mean of both directions of the KL
           "mask_inverted",            # the LOWER bin kept as own
           "threshold_at_mean",        # tau = mean_d delta instead of the middle of the range
           "average_logvar_not_var",   # log vb = (l1 + l2) / 2
           "kl_of_unadapted",          # the KL of the encoder's posteriors, not of the adapted ones
           "mean_over_B_not_2B",       # the KL sum divided by the number of pairs
           "grad_to_one_row_only",     # a shared dimension's gradient reaches the first row of the pair only
           "drop_tail",                # the columns past the last full 64 are left out of min / max and of the KL
           "mlvae_mean_unweighted",    # mlvae with the plain mean of the means
           "eps_of_first_row")         # the second row of a pair sampled with the first row's draw


def delta(m1, l1, m2, l2, defect=None):
    d = np.exp(l1 - l2) + (m2 - m1) ** 2 * np.exp(-l2) - 1.0
    if defect == "half_in_delta":
        return d + 0.5 * (l2 - l1)
    d = d + l2 - l1
    if defect == "symmetric_delta":
        return 0.5 * (d + np.exp(l2 - l1) + (m1 - m2) ** 2 * np.exp(-l1) - 1.0 + l1 - l2)
    return d


def threshold_mask(dl, defect=None):
    """own [B, D] of delta [B, D]; with ``drop_tail`` the tail columns are no part of min / max."""
    D = dl.shape[1]
    keep = D - D % 64 if (defect == "drop_tail" and D > 64) else D
    head = dl[:, :keep]
    tau = head.mean(1) if defect == "threshold_at_mean" else 0.5 * (head.min(1) + head.max(1))
    own = dl >= tau[:, None]
    return ~own if defect == "mask_inverted" else own


def average(m1, l1, m2, l2, averaging, defect=None):
    """(mb, vb) of every element."""
    e1, e2 = np.exp(l1), np.exp(l2)
    if averaging == "gvae":
        mb, vb = 0.5 * (m1 + m2), 0.5 * (e1 + e2)
    elif averaging == "mlvae":
        vb = 2.0 * e1 * e2 / (e1 + e2)
        mb = 0.5 * (m1 + m2) if defect == "mlvae_mean_unweighted" else 0.5 * vb * (m1 * np.exp(-l1) + m2 * np.exp(-l2))
    else:
        raise ValueError(averaging)
    if defect == "average_logvar_not_var":
        vb = np.exp(0.5 * (l1 + l2))
    return mb, vb


def ada(mu, logvar, eps, beta, averaging, own=None, dz=None, g=1.0, defect=None):
    """dict(z [2B, D], own [B, D] bool, kl_rows [2B], loss, terms = (mean KL, mean shared dimensions per pair), dmu,
    dlogvar): the op and the gradients of  sum(dz * z) + g * loss  (``dz`` None: zeros) with the mask held fixed."""
    mu, lv, eps = (np.asarray(a, np.float64) for a in (mu, logvar, eps))
    R, D = mu.shape
    B = R // 2
    assert R == 2 * B and B >= 1
    m1, m2, l1, l2, n1, n2 = mu[:B], mu[B:], lv[:B], lv[B:], eps[:B], eps[B:]
    if defect == "eps_of_first_row":
        n2 = n1
    own = threshold_mask(delta(m1, l1, m2, l2, defect), defect) if own is None else np.asarray(own) != 0
    mb, vb = average(m1, l1, m2, l2, averaging, defect)
    mt1, mt2 = np.where(own, m1, mb), np.where(own, m2, mb)
    vt1, vt2 = np.where(own, np.exp(l1), vb), np.where(own, np.exp(l2), vb)
    lt1, lt2 = np.where(own, l1, np.log(vb)), np.where(own, l2, np.log(vb))
    z = np.concatenate([mt1 + n1 * np.sqrt(vt1), mt2 + n2 * np.sqrt(vt2)])
    if defect == "kl_of_unadapted":
        per = np.concatenate([1.0 + l1 - m1 * m1 - np.exp(l1), 1.0 + l2 - m2 * m2 - np.exp(l2)])
    else:
        per = np.concatenate([1.0 + lt1 - mt1 * mt1 - vt1, 1.0 + lt2 - mt2 * mt2 - vt2])
    if defect == "drop_tail" and D > 64:
        per = per[:, :D - D % 64]
    kl_rows = -0.5 * per.sum(1)
    mean_kl = kl_rows.sum() / (B if defect == "mean_over_B_not_2B" else 2 * B)
    shared = (~own).sum() / B
    # ---- backward
    dz = np.zeros_like(mu) if dz is None else np.asarray(dz, np.float64)
    g1, g2 = dz[:B], dz[B:]
    gk = g * beta / (2 * B) if beta != 0.0 else 0.0
    if defect == "mean_over_B_not_2B":
        gk *= 2.0
    o = [g1 + gk * m1, g2 + gk * m2, 0.5 * np.exp(0.5 * l1) * (g1 * n1) + gk * (0.5 * (np.exp(l1) - 1.0)),
         0.5 * np.exp(0.5 * l2) * (g2 * n2) + gk * (0.5 * (np.exp(l2) - 1.0))]
    Gm = (g1 + g2) + 2.0 * gk * mb
    Gl = 0.5 * np.sqrt(vb) * (g1 * n1 + g2 * n2) + gk * (vb - 1.0)
    if averaging == "gvae":
        e1, e2 = np.exp(l1), np.exp(l2)
        s = [0.5 * Gm, 0.5 * Gm, Gl * (e1 / (e1 + e2)), Gl * (e2 / (e1 + e2))]
    else:
        p1, p2 = np.exp(-l1), np.exp(-l2)
        w1, w2 = p1 / (p1 + p2), p2 / (p1 + p2)
        s = [Gm * w1, Gm * w2, Gl * w1 + Gm * (w1 * (mb - m1)), Gl * w2 + Gm * (w2 * (mb - m2))]
    if defect == "grad_to_one_row_only":
        s[1], s[3] = np.zeros_like(s[1]), np.zeros_like(s[3])
    dm1, dm2, dl1, dl2 = (np.where(own, a, b) for a, b in zip(o, s))
    return dict(z=z, own=own, kl_rows=kl_rows, loss=beta * mean_kl if beta != 0.0 else 0.0,
                terms=np.array([mean_kl, shared]), dmu=np.concatenate([dm1, dm2]), dlogvar=np.concatenate([dl1, dl2]))


def scalar(mu, logvar, eps, beta, averaging, own, dz, g):
    """sum(dz * z) + g * loss with the given (fixed) mask: what ``ada``'s gradients differentiate."""
    r = ada(mu, logvar, eps, beta, averaging, own=own)
    return float((np.asarray(dz, np.float64) * r["z"]).sum() + g * r["loss"])


def central_differences(mu, logvar, eps, beta, averaging, own, dz, g, h=1e-6):
    """(dmu, dlogvar) of ``scalar`` by central differences in fp64, the mask held fixed."""
    mu, lv = np.array(mu, np.float64), np.array(logvar, np.float64)
    out = []
    for k in range(2):
        grad = np.zeros_like(mu)
        for idx in np.ndindex(*mu.shape):
            pair = [mu.copy(), lv.copy()]
            pair[k][idx] += h
            up = scalar(pair[0], pair[1], eps, beta, averaging, own, dz, g)
            pair[k][idx] -= 2 * h
            dn = scalar(pair[0], pair[1], eps, beta, averaging, own, dz, g)
            grad[idx] = (up - dn) / (2 * h)
        out.append(grad)
    return out


def torch_op(mu, logvar, eps, beta, averaging, own=None):
    """The library's lines on torch tensors of any dtype, differentiable by autograd: compute_kl, aggregate_argmax's
    two-bin histogram (``torch.where`` on the mask, a constant), aggregate_labels' averages, the reparameterisation and
    the KL of the adapted posteriors.  Returns (z, loss, own, terms)."""
    import torch
    B = mu.shape[0] // 2
    z_mean, z_mean_2, z_logvar, z_logvar_2 = mu[:B], mu[B:], logvar[:B], logvar[B:]
    var_1, var_2 = z_logvar.exp(), z_logvar_2.exp()
    if own is None:
        with torch.no_grad():
            kl_per_point = var_1 / var_2 + (z_mean_2 - z_mean) ** 2 / var_2 - 1.0 + z_logvar_2 - z_logvar
            lo, hi = kl_per_point.min(1, keepdim=True)[0], kl_per_point.max(1, keepdim=True)[0]
            own = kl_per_point >= 0.5 * (lo + hi)         # histogram_fixed_width_bins(nbins=2) == 1
    else:
        own = own != 0
    if averaging == "gvae":
        new_mean = 0.5 * z_mean + 0.5 * z_mean_2
        new_log_var = (0.5 * var_1 + 0.5 * var_2).log()
    elif averaging == "mlvae":
        new_var = 2.0 * var_1 * var_2 / (var_1 + var_2)
        new_mean = (z_mean / var_1 + z_mean_2 / var_2) * new_var * 0.5
        new_log_var = new_var.log()
    else:
        raise ValueError(averaging)
    mt = torch.cat([torch.where(own, z_mean, new_mean), torch.where(own, z_mean_2, new_mean)])
    lt = torch.cat([torch.where(own, z_logvar, new_log_var), torch.where(own, z_logvar_2, new_log_var)])
    z = mt + eps * (0.5 * lt).exp()
    kl = (-0.5 * (1.0 + lt - mt * mt - lt.exp()).sum(1)).mean()
    terms = torch.stack([kl.detach(), (~own).sum().to(kl.dtype) / B])
    return z, beta * kl, own, terms


def margin_holds(mu, logvar):
    """|delta - tau| >= MARGIN (max delta - min delta) for every element of every pair with max delta > min delta: the
    mask of such inputs does not depend on the last bits of an exp."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    B = mu.shape[0] // 2
    dl = delta(mu[:B], lv[:B], mu[B:], lv[B:])
    lo, hi = dl.min(1, keepdims=True), dl.max(1, keepdims=True)
    return bool((np.abs(dl - 0.5 * (lo + hi)) >= MARGIN * (hi - lo)).all())


def make_inputs(B, D, seed):
    """(mu, logvar, eps [2B, D] fp32, the seed used).  Pairs shaped like a trained encoder's -- every second pair has one to
    three clearly different dimensions and the rest near-equal -- between fully random pairs; with three pairs or more
    the last one is two equal rows (all-equal delta: every dimension own).  The margin condition is asserted: the
    generator moves to the next seed until it holds, and returns the seed it used."""
    while True:
        rng = np.random.default_rng(seed)
        m1 = rng.normal(size=(B, D))
        l1 = rng.normal(-2.0, 0.7, size=(B, D))
        m2 = rng.normal(size=(B, D))
        l2 = rng.normal(-2.0, 0.7, size=(B, D))
        for b in range(0, B, 2):
            near_m = m1[b] + rng.normal(0.0, 0.02, size=D)
            near_l = l1[b] + rng.normal(0.0, 0.02, size=D)
            diff = rng.choice(D, size=min(D, int(rng.integers(1, 4))), replace=False)
            near_m[diff], near_l[diff] = m2[b, diff] + np.sign(m2[b, diff] - m1[b, diff]) * 1.5, l2[b, diff]
            m2[b], l2[b] = near_m, near_l
        if B >= 3:
            m2[B - 1], l2[B - 1] = m1[B - 1], l1[B - 1]
        mu = np.concatenate([m1, m2]).astype(np.float32)
        lv = np.concatenate([l1, l2]).astype(np.float32)
        eps = rng.normal(size=(2 * B, D)).astype(np.float32)
        if margin_holds(mu, lv):
            return mu, lv, eps, seed
        seed += 1


def make_mask(B, D, seed):
    """An external own mask [B, D] uint8 for the inputs of ``seed``: about half the dimensions, the first pair all
    shared and (two pairs or more) the second all own."""
    own = (np.random.default_rng(seed + 100003).random((B, D)) < 0.5).astype(np.uint8)
    own[0] = 0
    if B >= 2:
        own[1] = 1
    return own


def make_dz(B, D, seed):
    """An incoming gradient of z [2B, D] fp32."""
    return np.random.default_rng(seed + 200003).normal(size=(2 * B, D)).astype(np.float32)
