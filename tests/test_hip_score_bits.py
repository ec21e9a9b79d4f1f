"""GPU: the score and density kernels that share csrc/dense.h (the covariance pass, the block Cholesky, the cyclic Jacobi
sweep) give the bits they gave at the commit before they were put on that header (DESIGN, "What the score kernels share").
tests/golden/score_bits.npz was recorded from a build of that commit; every comparison is an equality of bytes, with no
tolerance.  Only ``hipvae.functional`` wrappers are called, so the file runs on both trees.

Every input is an exact integer hash (the same numbers on any host; no BLAS and no ``randn`` makes them).  A symmetric
positive definite matrix is H + (0.5 D + 1) I with H symmetric and hashed, multiples of 2^-24 in [-0.5, 0.5): strictly
diagonally dominant and exact in fp64.  A matrix whose pivot p is exactly 0 is L L^T in integers with L[p][p] = 0 and
every other diagonal element 2, so each step of the factorisation is exact.  Responsibilities are (hash + 0.5) times an
exact power of two.  A strided input is the same values at a row stride of 2 D; a case that takes both asserts that the
two runs agree byte for byte and records one.

Sweeps of the Jacobi iteration with these matrices (tests/unsup_ref.ref_jacobi on the CPU; the recorded info[3] of the
device agree): unsup_gauss D = 1: 0, 2: 1, 7: 5, 128: 8, 131: 9; frechet D = 1: 0, 2: 1, 33: 7 (eps = 0 and
0.125), 128: 9, 131: 9.  Every D >= 7 case takes at least two sweeps with the diagonal as stated, so it is not lowered.

An array above 32 KiB is recorded as the SHA-256 of its bytes (with its dtype and shape), which keeps the recording
small; equal digests are equal bytes.

    python tests/test_hip_score_bits.py OUT.npz        # re-record (on a GPU, from a build of the PARENT commit)
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_bits.npz")
DIGEST_ABOVE = 32 * 1024


def _hash(n, seed):
    """n fp64 values in [-0.5, 0.5), multiples of 2^-24: integer arithmetic only."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(seed * 69069 + 12345)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(13))) * np.uint64(0x45D9F3B)) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    return (h >> np.uint64(8)).astype(np.float64) * (1.0 / (1 << 24)) - 0.5


def spd(D, seed, diag=None):
    """H + diag I (0.5 D + 1 unless given), H symmetric and hashed."""
    H = np.triu(_hash(D * D, seed).reshape(D, D))
    H = H + np.triu(H, 1).T
    return H + (0.5 * D + 1.0 if diag is None else diag) * np.eye(D)


def singular(D, p, seed):
    """L L^T in exact integers: L lower triangular with hashed entries in -2..2, 2 on the diagonal, 0 at [p][p]."""
    L = np.tril(np.floor((_hash(D * D, seed).reshape(D, D) + 0.5) * 5.0).astype(np.int64) - 2, -1)
    L += 2 * np.eye(D, dtype=np.int64)
    L[p, p] = 0
    return (L @ L.T).astype(np.float64)


def rows(N, D, seed):
    """(dense, strided): the same hashed fp32 [N, D] values on the device, the second at a row stride of 2 D."""
    x = torch.from_numpy((_hash(N * D, seed) * 4.0).astype(np.float32).reshape(N, D)).to("cuda:0")
    wide = torch.zeros((N, 2 * D), dtype=torch.float32, device="cuda:0")
    wide[:, D:] = x
    return x, wide[:, D:]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _np(**tensors):
    return {k: v.detach().cpu().contiguous().numpy() for k, v in tensors.items()}


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, "the dense and the strided run differ")
    return a


def unsup_cov(N, D):
    from hipvae import functional as HF
    out = []
    for x in rows(N, D, 1000 + N + D):
        flags = HF.disent_flags(x.device)
        mean, cov = HF.unsup_cov(x, flags)
        out.append(_np(mean=mean, cov=cov, flags=flags))
    return _same(out[0], out[1], "unsup_cov")


def unsup_gauss(cov):
    from hipvae import functional as HF
    res, eig, info = HF.unsup_gauss(_dev(cov))
    return _np(res=res, eig=eig, info=info)


def frechet(c1, c2, eps):
    from hipvae import functional as HF
    D = c1.shape[0]
    res, eig, info = HF.frechet(_dev(_hash(D, 31)), _dev(c1), _dev(_hash(D, 32)), _dev(c2), eps)
    return _np(res=res, eig=eig, info=info)


def gmm_factor(covs):
    from hipvae import functional as HF
    chol, linv, logdet, info = HF.gmm_factor(_dev(np.stack(covs)))
    return _np(chol=chol, linv=linv, logdet=logdet, info=info)


def gmm_resp(N, K, seed):
    K2 = 1
    while K2 < K:
        K2 *= 2
    return (_hash(N * K, seed).reshape(N, K) + 0.5) * (1.0 / K2)


def gmm_mstep(N, D, K, with_cov):
    from hipvae import functional as HF
    resp = _dev(gmm_resp(N, K, 2000 + N))
    out = []
    for x in rows(N, D, 2100 + N + D):
        flags = HF.disent_flags(x.device)
        nk, w, mean, cov = HF.gmm_mstep(x, resp, flags, reg=2.0 ** -20, with_cov=with_cov)
        got = dict(nk=nk, w=w, mean=mean, flags=flags)
        if with_cov:
            got["cov"] = cov
        out.append(_np(**got))
    return _same(out[0], out[1], "gmm_mstep")


def _cases():
    c = {}
    for N, D in ((2, 5), (67, 16), (600, 131), (33000, 3)):
        c[f"unsup_cov-{N}-{D}"] = (unsup_cov, (N, D))
    for D in (1, 2, 7, 128, 131):
        c[f"unsup_gauss-{D}"] = (unsup_gauss, (spd(D, 40 + D),))
    c["unsup_gauss-pivot3"] = (unsup_gauss, (singular(6, 3, 47),))
    for D in (1, 2, 33, 128, 131):
        c[f"frechet-{D}"] = (frechet, (spd(D, 50 + D), spd(D, 60 + D), 0.0))
    c["frechet-33-eps"] = (frechet, (spd(33, 83), spd(33, 93), 0.125))
    c["frechet-pivot"] = (frechet, (singular(6, 3, 57), spd(6, 66), 0.0))
    c["gmm_factor-1-1"] = (gmm_factor, ([spd(1, 70)],))
    c["gmm_factor-17-3"] = (gmm_factor, ([spd(17, 71), singular(17, 3, 72), singular(17, 9, 73)],))
    for D in (128, 131):
        c[f"gmm_factor-{D}-2"] = (gmm_factor, ([spd(D, 74 + D), spd(D, 75 + D)],))
    for N, D, K in ((5, 1, 1), (130, 17, 3), (700, 131, 2)):
        for with_cov in (True, False):
            c[f"gmm_mstep-{N}-{D}-{K}-{'cov' if with_cov else 'means'}"] = (gmm_mstep, (N, D, K, with_cov))
    return c


CASES = _cases()


def run(name):
    fn, args = CASES[name]
    out = fn(*args)
    torch.cuda.synchronize()
    return out


def _record(a):
    """What the recording keeps of an output: the array, or above DIGEST_ABOVE the digest of (dtype, shape, bytes)."""
    if a.nbytes <= DIGEST_ABOVE:
        return a
    head = f"{a.dtype.str}{a.shape}".encode()
    return np.frombuffer(hashlib.sha256(head + a.tobytes()).digest(), dtype=np.uint8)


_golden = []


def golden():
    if not _golden:
        _golden.append(np.load(GOLDEN))
    return _golden[0]


def test_golden_covers_every_case():
    assert sorted({k.split("/")[0] for k in golden().files}) == sorted(CASES)
    assert os.path.getsize(GOLDEN) < 400 * 1024


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_give_the_recorded_bits(name):
    got = run(name)
    want = {k.split("/")[1]: golden()[k] for k in golden().files if k.split("/")[0] == name}
    assert sorted(got) == sorted(want)
    for k, full in got.items():
        a, b = _record(full), want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, k, a.dtype, b.dtype, a.shape, b.shape)
        differ = "digest" if a is not full else int(
            (a.reshape(-1, 1).view(np.uint8) != b.reshape(-1, 1).view(np.uint8)).any(1).sum())
        assert a.tobytes() == b.tobytes(), (name, k, differ, "of", full.size, "values differ")


def test_mstep_means_of_unit_responsibilities_are_the_cov_means():
    """K = 1 and responsibilities exactly 1.0: the M-step adds what unsup_cov adds, in its order."""
    from hipvae import functional as HF
    x, _ = rows(1200, 40, 3000)
    flags = HF.disent_flags(x.device)
    mean, _ = HF.unsup_cov(x, flags)
    resp = torch.ones((1200, 1), dtype=torch.float64, device=x.device)
    _, _, gm, _ = HF.gmm_mstep(x, resp, flags, with_cov=False)
    a, b = _np(a=mean, b=gm[0]).values()
    assert a.tobytes() == b.tobytes(), int((a != b).sum())


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.join(os.path.dirname(here), "intro-tc-vae_amd"), os.path.dirname(here)):
        sys.path.insert(0, p)
    rec = {}
    for c in CASES:
        got = run(c)
        if "info" in got:
            print(c, "info", got["info"].tolist())
        rec.update({f"{c}/{k}": _record(v) for k, v in got.items()})
    np.savez_compressed(sys.argv[1], **rec)
    print(f"recorded {len(CASES)} cases -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)")
