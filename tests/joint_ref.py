"""fp64 restatement of the latent op of JointVAE (Dupont 2018, "Learning Disentangled Joint Continuous and Discrete
Representations") and, without discrete variables, of AnnealedVAE (Burgess et al. 2018; disentanglement_lib's
``annealed_vae``), the yardstick of csrc/joint.hip: numpy (forward and the analytic backward) for the kernel tests, torch
(autograd, any dtype) for the step tests.

mu, logvar [B, D], D = n_cont + sum K_i: columns [0, n_cont) are the continuous posterior (m, l), the remaining columns of mu
the logits a of G categorical variables with K_1 .. K_G categories side by side; those columns of logvar are unused.

    z_cont = m + eps exp(l / 2)                                KL_z = mean_b -1/2 sum_d (1 + l - m^2 - e^l)
    per group: log alpha = a - logsumexp(a),  u' = u if u > 0 else 2^-25,  g = -log(-log u')
               y = softmax((a + g) / tau)                      KL_i = mean_b (log K + sum_k alpha_k log alpha_k)
    KL_c = sum_i KL_i,    loss = beta (gamma_z |KL_z - C_z| + gamma_c |KL_c - C_c|)

With dz the gradient of z, g_L that of the loss, s = sign(KL - C) (0 at 0), k_z = g_L beta gamma_z s_z / B and k_c alike:

    dm_cont = dz + k_z m                    dl_cont = dz eps e^(l / 2) / 2 + k_z (e^l - 1) / 2
    da_k    = y_k (dz_k - sum_j y_j dz_j) / tau + k_c alpha_k (log alpha_k - sum_j alpha_j log alpha_j)     per group
    dl_disc = 0 exactly

``defect`` names one deliberate mistake a kernel could make (DEFECTS): tests/test_joint_ref_host.py shows that each of
them moves a quantity the GPU test compares above that test's bar.
"""
import numpy as np

TINY_U = 2.0 ** -25
SIGNS = ((1, 1), (1, -1), (-1, 1), (-1, -1))      # (sign of KL_z - C_z, sign of KL_c - C_c) a pair of capacities gives
DEFECTS = ("mean_over_BD",            # the KL means taken over B * D instead of B
           "no_abs",                  # KL - C without the absolute value
           "capacity_per_group",      # |KL_i - C_c| per discrete variable instead of |sum_i KL_i - C_c|
           "tau_missing_bwd",         # the softmax gradient without its 1 / tau
           "gumbel_after_tau",        # y = softmax(a / tau + g)
           "kl_of_tempered",          # the KL of alpha = softmax(a / tau)
           "no_log_K",                # log K left out of the KL
           "drop_tail",               # the columns past the last full 64 are left out of the KL sums
           "cut_at_64",               # a group that straddles a multiple of 64 columns is treated as two
           "u_zero_kept",             # u = 0 not replaced: g = -inf
           "disc_logvar_grad")        # the unused logvar columns get the continuous formula's gradient


def groups(n_cont, disc, cut=False):
    """[(first, one past last)] absolute columns of every discrete variable; ``cut``: split at multiples of 64."""
    out, s = [], n_cont
    for k in disc:
        e = s + k
        if cut:
            while s // 64 != (e - 1) // 64:
                mid = (s // 64 + 1) * 64
                out.append((s, mid))
                s = mid
        out.append((s, e))
        s = e
    return out


def _sign(v):
    return float(v > 0) - float(v < 0)


def joint(mu, logvar, eps, u, n_cont, disc, cap, gamma_z, gamma_c, beta=1.0, tau=0.67, dz=None, g=1.0, defect=None):
    """dict(z [B, D], loss, terms = (KL_z, KL_c, C_z, C_c), kl_groups, dmu, dlogvar): the op and the gradients of
    sum(dz * z) + g * loss (``dz`` None: zeros).  ``eps`` [B, n_cont], ``u`` [B, n_disc]; ``cap`` = (C_z, C_c)."""
    mu, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    B, D = mu.shape
    nc = int(n_cont)
    assert nc + sum(disc) == D
    eps = np.zeros((B, 0)) if nc == 0 else np.asarray(eps, np.float64)
    u = np.zeros((B, 0)) if nc == D else np.asarray(u, np.float64)
    cz, cc = float(cap[0]), float(cap[1])
    keep = D - D % 64 if (defect == "drop_tail" and D > 64) else D
    nB = B * D if defect == "mean_over_BD" else B
    dz = np.zeros((B, D)) if dz is None else np.asarray(dz, np.float64)
    z, dmu, dlv = np.zeros((B, D)), np.zeros((B, D)), np.zeros((B, D))
    # ---- continuous block
    m, l = mu[:, :nc], lv[:, :nc]
    wz = (np.arange(nc) < keep).astype(np.float64)
    z[:, :nc] = m + eps * np.exp(0.5 * l)
    klz = (-0.5 * ((1.0 + l - m * m - np.exp(l)) * wz).sum(1)).sum() / nB
    # ---- discrete block
    per = []
    for s, e in groups(nc, disc, cut=defect == "cut_at_64"):
        a, uu = mu[:, s:e], u[:, s - nc:e - nc]
        with np.errstate(divide="ignore"):
            gum = -np.log(-np.log(uu if defect == "u_zero_kept" else np.where(uu > 0, uu, TINY_U)))
        t = a / tau + gum if defect == "gumbel_after_tau" else (a + gum) / tau
        y = np.exp(t - t.max(1, keepdims=True))
        y /= y.sum(1, keepdims=True)
        akl = a / tau if defect == "kl_of_tempered" else a
        mx = akl.max(1, keepdims=True)
        la = akl - (mx + np.log(np.exp(akl - mx).sum(1, keepdims=True)))
        al = np.exp(la)
        wc = (np.arange(s, e) < keep).astype(np.float64)
        ent = (al * la * wc).sum(1, keepdims=True)
        kl_i = ((0.0 if defect == "no_log_K" else np.log(e - s)) + ent[:, 0]).sum() / nB
        z[:, s:e] = y
        per.append(dict(s=s, e=e, y=y, la=la, al=al, ent=ent, wc=wc, kl=kl_i))
    klc = float(sum(p["kl"] for p in per))
    if defect == "no_abs":
        lz, sz, lc, sc = klz - cz, 1.0, klc - cc, [1.0] * len(per)
    else:
        lz, sz = abs(klz - cz), _sign(klz - cz)
        if defect == "capacity_per_group":
            lc, sc = sum(abs(p["kl"] - cc) for p in per), [_sign(p["kl"] - cc) for p in per]
        else:
            lc, sc = abs(klc - cc), [_sign(klc - cc)] * len(per)
    loss = beta * (gamma_z * lz + gamma_c * lc)
    # ---- backward
    kz = g * beta * gamma_z * sz / nB
    gzc = dz[:, :nc]
    dmu[:, :nc] = gzc + kz * m * wz
    dlv[:, :nc] = 0.5 * np.exp(0.5 * l) * (gzc * eps) + kz * (0.5 * (np.exp(l) - 1.0)) * wz
    for p, s_i in zip(per, sc):
        s, e = p["s"], p["e"]
        kc = g * beta * gamma_c * s_i / nB
        gy = dz[:, s:e]
        soft = p["y"] * (gy - (p["y"] * gy).sum(1, keepdims=True))
        dmu[:, s:e] = soft / (1.0 if defect == "tau_missing_bwd" else tau) + kc * (p["al"] * (p["la"] - p["ent"])) * p["wc"]
        if defect == "disc_logvar_grad":
            dlv[:, s:e] = 0.5 * gy
    return dict(z=z, loss=float(loss), terms=np.array([klz, klc, cz, cc]), kl_groups=np.array([p["kl"] for p in per]),
                dmu=dmu, dlogvar=dlv)


def hard(mu, n_cont, disc):
    """The deterministic code: z_cont = mu, and per group the one-hot of the FIRST maximum of the fp32 logits."""
    mu = np.asarray(mu, np.float32)
    z = np.zeros_like(mu)
    z[:, :n_cont] = mu[:, :n_cont]
    for s, e in groups(n_cont, disc):
        z[np.arange(mu.shape[0]), s + np.argmax(mu[:, s:e], axis=1)] = 1.0       # np.argmax: the first of equal maxima
    return z


def torch_op(mu, logvar, eps, u, n_cont, disc, cap, gamma_z, gamma_c, beta=1.0, tau=0.67):
    """The same lines on torch tensors of any dtype, differentiable by autograd (Dupont's model and loss with the exact
    log-softmax in place of his EPS guards).  Returns (z, loss, terms [4])."""
    import torch
    nc = int(n_cont)
    m, l = mu[:, :nc], logvar[:, :nc]
    cols = [m + eps * (0.5 * l).exp()] if nc else []
    klz = (-0.5 * (1.0 + l - m * m - l.exp()).sum(1)).mean() if nc else mu.new_zeros(())
    klc = mu.new_zeros(())
    for s, e in groups(nc, disc):
        a, uu = mu[:, s:e], u[:, s - nc:e - nc]
        uu = torch.where(uu > 0, uu, torch.full_like(uu, TINY_U))
        gum = -torch.log(-torch.log(uu))
        cols.append(torch.softmax((a + gum) / tau, dim=1))
        la = torch.log_softmax(a, dim=1)
        klc = klc + (float(np.log(e - s)) + (la.exp() * la).sum(1)).mean()
    cz, cc = (torch.as_tensor(c, dtype=mu.dtype, device=mu.device) for c in (cap[0], cap[1]))
    loss = beta * (gamma_z * (klz - cz).abs() + gamma_c * (klc - cc).abs())
    return torch.cat(cols, dim=1), loss, torch.stack([klz.detach(), klc.detach(), cz, cc])


def capacity_at(t, c_min, c_max, iters, ceiling=None):
    """C(t) = min(C_max, C_min + (C_max - C_min) t / iters), optionally capped (the discrete one at sum_i log K_i)."""
    c = min(c_max, c_min + (c_max - c_min) * t / iters)
    return c if ceiling is None else min(c, ceiling)


def make_inputs(B, n_cont, disc, seed):
    """(mu, logvar [B, D], eps [B, n_cont], u [B, n_disc], all fp32, and caps): ``caps[(s_z, s_c)]`` is a pair (C_z, C_c)
    under which sign(KL_z - C_z) = s_z and sign(KL_c - C_c) = s_c WITH A MARGIN -- C = KL / 2 or 3 KL / 2 of the
    restatement's own KLs, so |KL - C| = KL / 2 >= 0.1 KL and no sign hangs on a last bit.  An empty block has KL = C = 0
    and the sign 0.  The logvar columns of the discrete block hold numbers that nothing may depend on; u has no zero."""
    disc = tuple(disc)
    nd, D = sum(disc), n_cont + sum(disc)
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(B, D))
    mu[:, n_cont:] *= 1.5
    lv = rng.normal(-2.0, 0.7, size=(B, D))
    mu, lv = mu.astype(np.float32), lv.astype(np.float32)
    eps = rng.normal(size=(B, n_cont)).astype(np.float32)
    u = rng.random(size=(B, nd), dtype=np.float32)
    u[u == 0] = 0.5
    base = joint(mu, lv, eps, u, n_cont, disc, (0.0, 0.0), 1.0, 1.0)["terms"]
    caps = {(sz, sc): (float(base[0]) * (1.0 - 0.5 * sz), float(base[1]) * (1.0 - 0.5 * sc)) for sz, sc in SIGNS}
    for (sz, sc), (cz, cc) in caps.items():
        assert abs(base[0] - cz) >= 0.1 * base[0] and abs(base[1] - cc) >= 0.1 * base[1]
        assert (_sign(base[0] - cz), _sign(base[1] - cc)) == (sz if n_cont else 0, sc if nd else 0)
    return mu, lv, eps, u, caps


# the cases (B, n_cont, disc) on which the edge draws are tried: groups small enough for one column with g = -2.85 to count
EDGE_CASES = ((4, 61, (2,)), (7, 6, (3,)), (33, 10, (10,)), (9, 60, (3, 7, 59)))


def edge_draws(u, mu, n_cont, disc):
    """A copy of ``u`` [B, n_disc >= 2] with the two ends of torch.rand's range: 1 - 2^-24 in its last element (that draw's
    g = 16.6 decides its group whatever else is in it) and exactly 0 in the first row (B >= 2: another row), at the
    column that keeps the largest share of its softmax with g = -log(25 log 2) = -2.85: the one whose a + g stands
    highest above the other columns of its group."""
    u = np.array(u, np.float32)
    u[-1, -1] = np.float32(1.0 - 2.0 ** -24)
    t = np.asarray(mu, np.float64)[0, n_cont:] - np.log(-np.log(u[0].astype(np.float64)))
    best, at = -np.inf, 0
    for s, e in groups(0, disc):
        for j in range(s, e):
            lead = t[j] - np.delete(t[s:e], j - s).max()
            best, at = (lead, j) if lead > best else (best, at)
    u[0, at] = 0.0
    assert u.max() < 1.0 and u.min() == 0.0
    return u


def make_dz(B, D, seed):
    """An incoming gradient of z [B, D] fp32."""
    return np.random.default_rng(seed + 200003).normal(size=(B, D)).astype(np.float32)
