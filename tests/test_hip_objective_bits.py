"""GPU: the objective ops (DIP, MMD, Ada-GVAE, JointVAE / Annealed, the S2 label term, IWAE) give the bits they gave at
the commit before their kernels were put on the shared header csrc/objective.h.
tests/golden/objective_bits.npz was recorded from a build of that commit; every comparison is an equality of bytes, with
no tolerance.  Only the ``ops`` surface is called, so the file runs on both trees (the one output ``ops`` drops, the
per-image ``img`` of the IWAE combine, is picked up where ``ops.iwae_bound`` receives it).

Every input is an exact integer hash (the same floats on any host).  Per case: every forward output (``z``, the loss,
``terms``, the mask, ``lat``, the importance weights, ``img``) and every gradient, taken with a hashed upstream gradient
of the loss and, for the ops that return ``z``, a hashed NON-contiguous one of ``z``.  The shapes are the smallest that
reach each path: ada at D = 1, 65, 130, 300 (the instances of 1, 2, 4 and 8 registers a lane), 5 pairs (not a multiple of
the four pairs a block takes) and 300 pairs (the ordered sum folds more than one element a thread), both averagings,
the adaptive and a given mask, dense inputs and the halves of one packed tensor; joint with a group across a 64-lane
edge, with an empty continuous and an empty discrete block, both signs of the capacity terms, 300 rows, and the hard
code; sup in its three forms, cov also over more than one tile, 300 rows, gamma as a number and on the device; dip in
both kinds at D = 10 and 70, local rows inside the batch, dense and packed; mmd with both kernels and with local rows;
iwae at (B, K, D) = (3, 5, 10) and (300, 2, 3) under its three estimators, mse and bce.

    python tests/test_hip_objective_bits.py OUT.npz        # re-record (on a GPU, from a build of the PARENT commit)
"""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_bits.npz")


def _hash(n, seed):
    """n floats in [-0.5, 0.5), multiples of 2^-24: integer arithmetic only."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 69069 + 12345)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    return ((h >> np.uint64(8)).astype(np.float64) * (1.0 / (1 << 24)) - 0.5).astype(np.float32)


def _t(shape, seed, mul=1.0, add=0.0):
    """A device tensor of hashes times ``mul`` (a power of two) plus ``add``."""
    h = _hash(int(np.prod(shape, dtype=np.int64)), seed) * np.float32(mul) + np.float32(add)
    return torch.from_numpy(h).reshape(shape).to("cuda:0")


def _pair(rows, D, seed, packed):
    """(mu, logvar, leaves): two dense leaves, or the halves of one packed [rows, 2D] leaf."""
    if packed:
        pk = _t((rows, 2 * D), seed, 2.0).requires_grad_()
        return pk[:, :D], pk[:, D:], [pk]
    mu, lv = _t((rows, D), seed, 4.0).requires_grad_(), _t((rows, D), seed + 1, 2.0).requires_grad_()
    return mu, lv, [mu, lv]


def _strided(rows, D, seed):
    """A hashed [rows, D] upstream gradient with a row stride of 2 D."""
    return _t((rows, 2 * D), seed)[:, D:]


def _scalar(seed):
    return _t((), seed, 1.0, 1.0)


def _np(**tensors):
    return {k: v.detach().cpu().contiguous().numpy() for k, v in tensors.items()}


def _grads(outputs, leaves, upstream):
    got = torch.autograd.grad(outputs, leaves, upstream)
    return {f"grad{i}": g for i, g in enumerate(got)}


def ada(D, B, averaging, given, packed):
    import ops
    seed = 100 + D + B
    mu, lv, leaves = _pair(2 * B, D, seed, packed)
    eps = _t((2 * B, D), seed + 2, 4.0)
    own = (_t((B, D), seed + 3) > 0).to(torch.uint8) if given else None
    z, loss, mask, terms = ops.ada_group(mu, lv, 0.5, averaging, own=own, eps=eps, with_terms=True)
    return _np(z=z, loss=loss, mask=mask, terms=terms,
               **_grads([z, loss], leaves, [_strided(2 * B, D, seed + 4), _scalar(seed + 5)]))


def joint(B, n_cont, disc, cap, hard=False):
    import ops
    n_disc = sum(disc)
    D, seed = n_cont + n_disc, 200 + B + n_cont
    mu, lv, leaves = _pair(B, D, seed, False)
    if hard:
        return _np(z=ops.joint_latent(mu, lv, n_cont, disc, None, 1.0, 1.0, hard=True))
    eps = _t((B, n_cont), seed + 2, 4.0) if n_cont else None
    u = _t((B, n_disc), seed + 3, 1.0, 0.5) if n_disc else None
    capacity = torch.tensor([cap, cap], dtype=torch.float64, device="cuda:0")
    z, loss, terms = ops.joint_latent(mu, lv, n_cont, disc, capacity, 3.0, 2.0, beta=0.5, temperature=0.67, eps=eps, u=u,
                                      with_terms=True)
    return _np(z=z, loss=loss, terms=terms, **_grads([z, loss], leaves, [_strided(B, D, seed + 4), _scalar(seed + 5)]))


def sup(kind, B, D, F, gamma_on_device):
    import ops
    seed = 300 + B + D + F
    mu = _t((B, D), seed, 4.0).requires_grad_()
    sizes = tuple(3 + f % 5 for f in range(F))
    y = np.floor((_hash(B * F, seed + 1).reshape(B, F).astype(np.float64) + 0.5) * np.array(sizes)).astype(np.float32)
    gamma = torch.tensor([1.5], dtype=torch.float64, device="cuda:0") if gamma_on_device else 1.5
    out, terms = ops.supervised_regularizer(mu, torch.from_numpy(y).to("cuda:0"), kind,
                                            factor_sizes=sizes if kind == "xent" else None, gamma=gamma, scale=0.75,
                                            with_terms=True)
    return _np(loss=out, terms=terms, **_grads([out], [mu], [_scalar(seed + 2)]))


def dip(kind, D, packed, local):
    import ops
    Bt, seed = 5, 400 + D
    mu_all, lv_all, leaves = _pair(Bt, D, seed, packed)
    Bl, off = (3, 1) if local else (Bt, 0)
    out, terms = ops.dip_kl_loss(mu_all[off:off + Bl], lv_all[off:off + Bl], 0.5, 2.0, 3.0, kind, mu_all=mu_all,
                                 logvar_all=lv_all, row_offset=off, with_terms=True)
    return _np(loss=out, terms=terms, **_grads([out], leaves, [_scalar(seed + 2)]))


def mmd(kernel, Bl):
    import ops
    Bt, P, D, seed = 5, 7, 10, 500 + Bl
    z_all, prior = _t((Bt, D), seed, 4.0).requires_grad_(), _t((P, D), seed + 1, 4.0)
    mu, lv, leaves = _pair(Bl, D, seed + 2, False)
    out, terms = ops.mmd_kl_loss(z_all, mu, lv, prior, 0.5, 5.0, kernel, z_all=z_all, prior_all=prior, with_terms=True)
    return _np(loss=out, terms=terms, **_grads([out], [z_all] + leaves, [_scalar(seed + 4)]))


@contextlib.contextmanager
def _combine_outputs(log):
    """What ``ops.iwae_bound`` receives from the combine, ``img`` included, appended to ``log``."""
    from hipvae import functional as HF
    inner = HF.IwaeCombineFn.apply

    def apply(*args):
        log.append(inner(*args))
        return log[-1]

    HF.IwaeCombineFn.apply = apply
    try:
        yield
    finally:
        del HF.IwaeCombineFn.apply              # the inherited classmethod shows again


def iwae(B, K, D, estimator, loss_type):
    import ops
    P, seed = (8 if B < 100 else 5), 600 + B
    mu, lv, leaves = _pair(B, D, seed, False)
    eps = _t((K * B, D), seed + 2, 4.0)
    x = _t((B, P), seed + 3, 1.0, 0.5)
    recon = _t((K * B, P), seed + 4, 0.5, 0.5).requires_grad_()          # inside (0.25, 0.75): bce is finite
    sample = ops.iwae_sample(mu, lv, K, eps=eps)
    log = []
    with _combine_outputs(log):
        loss, terms = ops.iwae_bound(x, recon, sample, 0.75, 0.5, loss_type, estimator, with_terms=True)
    return _np(z=sample.z, lat=sample.lat, loss=loss, terms=terms, img=log[0][2], weights=sample.weights,
               **_grads([loss, sample.z], leaves + [recon], [_scalar(seed + 5), _strided(K * B, D, seed + 6)]))


def _cases():
    c = {}
    layouts = [(False, False), (True, True), (True, False), (False, True)]       # (given mask, packed)
    for i, D in enumerate((1, 65, 130, 300)):
        for j, averaging in enumerate(("gvae", "mlvae")):
            given, packed = layouts[(i + 2 * j) % 4]
            c[f"ada-{D}-{averaging}"] = (ada, (D, 5, averaging, given, packed))
    c["ada-300pairs"] = (ada, (3, 300, "mlvae", False, False))
    for k, (n_cont, disc) in enumerate(((3, (2, 70)), (0, (4,)), (10, ()))):
        c[f"joint-{k}-above"] = (joint, (5, n_cont, disc, 0.0))
        c[f"joint-{k}-below"] = (joint, (5, n_cont, disc, 1000.0))
    c["joint-300rows"] = (joint, (300, 2, (3,), 0.0))
    c["joint-hard"] = (joint, (5, 3, (2, 70), 0.0, True))
    for k, kind in enumerate(("xent", "l2", "cov")):
        c[f"sup-{kind}"] = (sup, (kind, 5, 10, 3, k % 2 == 1))
    c["sup-cov-tiles"] = (sup, ("cov", 5, 40, 33, True))
    c["sup-xent-300rows"] = (sup, ("xent", 300, 10, 3, False))
    c["sup-cov-300rows"] = (sup, ("cov", 300, 10, 3, False))
    for kind in ("i", "ii"):
        for D in (10, 70):
            for packed in (False, True):
                local = ((kind == "ii") + (D == 70) + packed) % 2 == 1
                c[f"dip-{kind}-{D}-{'packed' if packed else 'dense'}"] = (dip, (kind, D, packed, local))
    c["mmd-rbf"], c["mmd-imq"], c["mmd-rbf-local"] = (mmd, ("rbf", 5)), (mmd, ("imq", 5)), (mmd, ("rbf", 3))
    for estimator in ("iwae", "stl", "dreg"):
        c[f"iwae-small-{estimator}"] = (iwae, (3, 5, 10, estimator, "mse"))
        c[f"iwae-300-{estimator}"] = (iwae, (300, 2, 3, estimator, "mse"))
    c["iwae-small-bce"] = (iwae, (3, 5, 10, "iwae", "bce"))
    return c


CASES = _cases()


def run(name):
    fn, args = CASES[name]
    out = fn(*args)
    torch.cuda.synchronize()
    return out


_golden = []


def golden():
    if not _golden:
        _golden.append(np.load(GOLDEN))
    return _golden[0]


def test_golden_covers_every_case():
    assert sorted({k.split("/")[0] for k in golden().files}) == sorted(CASES)
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("name", list(CASES))
def test_ops_give_the_recorded_bits(name):
    got = run(name)
    want = {k.split("/")[1]: golden()[k] for k in golden().files if k.split("/")[0] == name}
    assert sorted(got) == sorted(want)
    for k, a in got.items():
        b = want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.isfinite(a.astype(np.float64)).all(), (name, k)
        assert a.tobytes() == b.tobytes(), (name, k, int((a != b).sum()), "of", a.size, "values differ")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "intro-tc-vae_amd"), os.path.dirname(here)):
        sys.path.insert(0, p)
    rec = {}
    for c in CASES:
        rec.update({f"{c}/{k}": v for k, v in run(c).items()})
    np.savez_compressed(sys.argv[1], **rec)
    print(f"recorded {len(CASES)} cases -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)")
