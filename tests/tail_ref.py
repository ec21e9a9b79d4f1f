"""fp64 restatement of the kernels a training step runs around the convolutions -- the loss heads, the scalar algebra,
the gradient norm / clip pair and the flip of csrc/loss_optim.hip, the skinny GEMMs and the bias gradient of
csrc/conv_igemm.hip, the pointwise / resampling kernels of csrc/norm_act.hip -- for tests/test_hip_tail.py and
tests/test_tail_ref_host.py: torch and numpy on the CPU only, dtype-generic, every gradient written out (no autograd;
the host test holds them to torch's fp64 autograd).

``defect`` names one deliberate mistake of a kernel (DEFECTS below): the host test uses them to show that a checked
quantity moves far beyond the tolerance on a named case when the kernel makes that mistake.  The plan arithmetic of the
host dispatch (``recon_splits``, ``gemm_plan``, ``bias_splits``) is restated in plain Python and held to the library's
workspace queries."""
import math

import torch

# ---- tolerances of tests/test_hip_tail.py on rel_err (max |got - ref| / max |ref|, per array) -------------------------
TOL_LINEAR = 2e-5        # fp32 fma chains against fp64 (the bar of test_hip_ops.py's linear / conv tests)
TOL_LOSS = 1e-5          # loss heads, values and gradients
TOL_SCALAR = 1e-6        # exp-ELBO and linear-combination values
TOL_POINT = 1e-6         # avg-pool, upsample adjoint, sigmoid
TOL_NORM = 1e-5          # the fp32 norm clip_grad_norm returns
# itcv_sumsq itself writes a double: fp32 squares are exact in fp64 and a sum of n positive terms in any order is within
# (n - 1) * 2^-53 of the exact one -- 2.4e-10 at the largest n (2^21 + 3).  4x that:
TOL_SUMSQ = 1e-9

LOSSES = ("mse", "l1", "bce")
REDUCTIONS = ("none", "sum", "mean")

DEFECTS = ("chunk_unrounded",    # recon slice chunk not rounded to 4: the float4 reads run over the slice's end
           "end_unclamped",      # recon slice end not clamped to P: the last slice runs into the next row
           "sumsq_tail_dropped",  # the n % 4 tail is left out of the sum of squares
           "scale_tail_twice",   # the n % 4 tail is scaled by every block, not by block 0 alone (here: twice)
           "bce_fwd_unclamped",  # log terms not floored at -100
           "bce_bwd_unclamped",  # (1 - r) r not floored at 1e-12
           "mean_over_P",        # reduction mean divides by the row length instead of the batch
           "l1_tie_sign",        # the L1 gradient at r == t is +-1 instead of 0
           "bias_per_split",     # every split-K slab adds the bias
           "accumulate_ignored",  # the split-K reduce overwrites the gradient it should add to
           "k_tail_kept",        # the clamped reads past K in the last K-tile are not zeroed
           "full_last_split",    # the short last split walks a full kps tiles: the ones before it are counted twice
           "flip_off_by_one",    # mirror index W - w instead of W - 1 - w
           "elbo_weight_no_B")   # the exp-ELBO gradient weight misses the 1 / B


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def moved(bad, ref):
    """rel_err of a defective result; anything not finite has moved without bound."""
    bad = bad.detach().double()
    if not bool(torch.isfinite(bad).all()):
        return math.inf
    return rel_err(bad, ref)


def cdiv(a, b):
    return (a + b - 1) // b


# ---- plan arithmetic -------------------------------------------------------------------------------------------------
def recon_splits(B, P):
    """Slices per row of recon_partial_kernel: about 1024 blocks in all, at least 2048 elements a slice."""
    return max(min(cdiv(1024, B), cdiv(P, 2048)), 1)


def recon_chunk(B, P, rounded=True):
    c = cdiv(P, recon_splits(B, P))
    return (c + 3) // 4 * 4 if rounded else c


def gemm_plan(M, N, K):
    """(mt, nt, ktiles, splits, kps) of gemm64_kernel for C[M][N] = A[M][K] B[K][N]: 64 x 64 tiles, K-tiles of 32; split-K
    only with fewer than 128 tiles and at least 4 K-tiles, at most 32 splits of at least 2 K-tiles; ``splits`` is then
    recomputed from the K-tiles per split, so the last split may be short."""
    mt, nt, ktiles = cdiv(M, 64), cdiv(N, 64), cdiv(K, 32)
    tiles, splits = mt * nt, 1
    if tiles < 128 and ktiles >= 4:
        splits = max(min(cdiv(256, tiles), 32, ktiles // 2), 1)
    kps = cdiv(ktiles, splits)
    return mt, nt, ktiles, cdiv(ktiles, kps), kps


def linear_gemms(B, K, N):
    """(M, N, K) of the three GEMMs of nn.Linear(K -> N) at batch B."""
    return {"fwd": (B, N, K), "dgrad": (B, K, N), "wgrad": (N, K, B)}


def gemm_instances(B, K, N):
    """(A_KC, B_KC) -- is the operand's k stride 1? -- of the three GEMMs, as run_gemm64 decides it from the strides
    itcv_linear_* pass: x [B][K] and w [N][K] forward, dy [B][N] and w as [N][K] for dx, dy as [N][B] and x as [B][K]
    for dw."""
    return {"fwd": (True, True), "dgrad": (True, K == 1), "wgrad": (N == 1, K == 1)}


def gemm_workspace(M, N, K):
    s = gemm_plan(M, N, K)[3]
    return s * M * N * 4 if s > 1 else 0


def linear_workspace(B, K, N):
    return max(gemm_workspace(*g) for g in linear_gemms(B, K, N).values())


def bias_splits(B, C, HW):
    return max(min(cdiv(1024, C), cdiv(B * HW, 2048), 256), 1)


# ---- case tables -----------------------------------------------------------------------------------------------------
RECON_SHAPES = [(3, 7), (5, 2048), (4, 2049), (4, 4100), (2, 4099), (1, 2048 * 3 + 4), (300, 192), (1100, 12), (8, 12288)]
# (B, P): (splits, rounded chunk) -- what the shape is in the list for
RECON_PLANS = {(3, 7): (1, 8), (5, 2048): (1, 2048), (4, 2049): (2, 1028), (4, 4100): (3, 1368), (2, 4099): (3, 1368),
               (1, 6148): (4, 1540), (300, 192): (1, 192), (1100, 12): (1, 12), (8, 12288): (6, 2048)}

# (B, K, N).  The weight gradient is a GEMM over K = B: no shape with B <= 127 gives it the four K-tiles split-K starts
# at, so (200, 70, 40) and (130, 1, 9) are what sends ``accumulate`` through the split-K reduce.  run_gemm64 picks the
# kernel instance from the operands' k strides (gemm_instances): the K = 1 and N = 1 shapes reach the two instances
# that the weight gradient of a wider layer never takes.
LINEAR_SHAPES = [(1, 1, 1), (3, 31, 5), (64, 33, 64), (65, 97, 65), (5, 283, 70), (7, 351, 40), (64, 2049, 48),
                 (64, 2048, 64), (5, 40, 8192), (64, 8192, 40), (200, 70, 40), (3, 1, 5), (130, 1, 9), (5, 7, 1)]
# the plans the shapes are in the list for: (B, K, N) -> {gemm: (mt, nt, ktiles, splits, kps)}
LINEAR_PLANS = {
    (1, 1, 1): {"fwd": (1, 1, 1, 1, 1), "dgrad": (1, 1, 1, 1, 1), "wgrad": (1, 1, 1, 1, 1)},
    (3, 31, 5): {"fwd": (1, 1, 1, 1, 1)},
    (5, 283, 70): {"fwd": (1, 2, 9, 3, 3)},                    # wanted 4 splits, 3 K-tiles each: 3 splits
    (7, 351, 40): {"fwd": (1, 1, 11, 4, 3)},                   # wanted 5: 4 splits, the last of 2 K-tiles
    (64, 2049, 48): {"fwd": (1, 1, 65, 22, 3)},                # wanted 32: 22 splits, the last of 2 K-tiles, one element
    (64, 2048, 64): {"fwd": (1, 1, 64, 32, 2)},                # exactly the cap
    (5, 40, 8192): {"fwd": (1, 128, 2, 1, 2), "dgrad": (1, 1, 256, 32, 8), "wgrad": (128, 1, 1, 1, 1)},
    (64, 8192, 40): {"fwd": (1, 1, 256, 32, 8), "dgrad": (1, 128, 2, 1, 2)},
    (200, 70, 40): {"wgrad": (1, 2, 7, 3, 3)},                 # split-K weight gradient: 3 + 3 + 1 K-tiles
    (3, 1, 5): {"fwd": (1, 1, 1, 1, 1), "dgrad": (1, 1, 1, 1, 1), "wgrad": (1, 1, 1, 1, 1)},
    (130, 1, 9): {"wgrad": (1, 1, 5, 2, 3)},                   # <false, true> through the reduce: 3 + 2 K-tiles
    (5, 7, 1): {"wgrad": (1, 1, 1, 1, 1)},
}
# (A_KC, B_KC) of gemm64_kernel the shapes are in the list for (gemm_instances)
LINEAR_INSTANCES = {(3, 1, 5): {"wgrad": (False, True), "dgrad": (True, True)},
                    (130, 1, 9): {"wgrad": (False, True)},
                    (5, 7, 1): {"wgrad": (True, False), "dgrad": (True, False)},
                    (1, 1, 1): {"wgrad": (True, True)},
                    (3, 31, 5): {"fwd": (True, True), "dgrad": (True, False), "wgrad": (False, False)}}

# (B, C, HW): (splits) of itcv_bias_grad
BIAS_SHAPES = {(3, 1, 1): 1, (3, 257, 1): 1, (2, 257, 7): 1, (5, 1, 1024): 3, (3, 257, 700): 2}

SUMSQ_SIZES = [1, 3, 4, 1027, 2 * 1048576 + 3]
# itcv_scale_by_dev's grid covers 2048 * 256 float4: one more, and a tail of 2, for the second trip of its stride loop
SCALE_SIZES = SUMSQ_SIZES + [4 * 524289 + 2]
ELBO_SIZES = [1, 255, 256, 257, 1000]
ELBO_COEFS = [-2.0 / 12288, -0.05]
FLIP_SHAPES = [(3, 6, 1), (4, 12, 5), (5, 192, 577)]
POINT_SIZES = [1, 255, 524288 + 77]


# ---- seeded inputs ---------------------------------------------------------------------------------------------------
BCE_EPS = float(torch.tensor(1e-12, dtype=torch.float32))      # ATen's EPSILON is a float constant: 9.99999996e-13
BCE_RECON = (0.0, 1.0, 2.0 ** -149, 1.0 - 2.0 ** -24)
BCE_TARGET = (0.0, 1.0, 0.3)
BCE_PLANTS = [(r, t) for r in BCE_RECON for t in BCE_TARGET]       # 12 pairs; a row holds 8 of them, rotating


def plant_positions(B, P):
    """8 distinct positions of a row -- P // 2 of them where P < 16 (3 at P = 7, 6 at P = 12), so that such a row keeps
    unplanted elements -- the same in every row: the row's two ends and
    both sides of the first slice boundary, as it is (rounded chunk) and as it would be unrounded; the rest spread."""
    want = min(8, P // 2)
    c4, c = recon_chunk(B, P), recon_chunk(B, P, rounded=False)
    cand = [0, P - 1, c - 1, c, c4 - 1, c4, P // 3, P // 5, 2 * P // 3, P // 7, 1, 2, 3]
    pos = []
    for p in cand:
        if 0 <= p < P and p not in pos:
            pos.append(p)
    return sorted(pos[:want])


def recon_inputs(B, P, loss, seed=0):
    """fp32 (x, recon [B, P], planted [B, P] bool).  bce: recon in [0.01, 0.99] with the 12 (recon, target) pairs of
    BCE_PLANTS planted, both clamps of ATen firing; l1: exact ties planted; mse: nothing planted."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + P)
    x, r = torch.rand(B, P, generator=g), torch.rand(B, P, generator=g)
    planted = torch.zeros(B, P, dtype=torch.bool)
    pos = plant_positions(B, P)
    if loss == "bce":
        r = r * 0.98 + 0.01
        for b in range(B):
            for k, p in enumerate(pos):
                rv, tv = BCE_PLANTS[(5 * b + k) % 12]
                r[b, p], x[b, p] = rv, tv
        planted[:, pos] = True
    elif loss == "l1":
        r[:, pos] = x[:, pos]
        planted[:, pos] = True
    return x, r, planted


def linear_inputs(B, K, N):
    """fp32 (x [B, K], w [N, K], bias [N], dy [B, N], and the non-zero gradients dw / db are accumulated into)."""
    g = torch.Generator().manual_seed(3 + B + N)
    x, w = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b, dy = torch.randn(N, generator=g), torch.randn(B, N, generator=g)
    return x, w, b, dy, torch.randn(N, K, generator=g), torch.randn(N, generator=g)


def sumsq_input(n, recipe, seed=0):
    """fp32 [n].  ``span``: magnitudes log-uniform over 1e-12 .. 1e12, random signs, the two ends present where n >= 2;
    ``tail``: the same below 1, and the last n % 4 elements (all of them where n < 4) at +-1e12 -- they carry the norm."""
    g = torch.Generator().manual_seed(50 + seed + n % 1000)
    hi = 12.0 if recipe == "span" else 0.0
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * (hi + 12.0) - 12.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    v = mag * sign
    if recipe == "span":
        v[0] = 1e12
        if n >= 2:
            v[n // 2] = -1e-12
    else:
        t = n % 4 if n >= 4 else n
        if t:
            v[n - t:] = 1e12 * sign[n - t:]
    return v.float()


def flip_input(B, rows, W, seed=0):
    g = torch.Generator().manual_seed(70 + seed + B + W)
    x = torch.randn(B, rows, W, generator=g)
    flip = torch.tensor([(0, 1, 2, 0, 255)[b % 5] for b in range(B)], dtype=torch.uint8)
    return x, flip


# ---- reconstruction losses -------------------------------------------------------------------------------------------
def recon_elem(r, t, loss, defect=None):
    """Per-element error, ATen's clamps included (binary_cross_entropy floors both log terms at -100)."""
    if loss == "mse":
        return (r - t) ** 2
    if loss == "l1":
        return (r - t).abs()
    lr, l1r = torch.log(r), torch.log(1 - r)
    if defect != "bce_fwd_unclamped":
        lr, l1r = lr.clamp(min=-100.0), l1r.clamp(min=-100.0)
    return -(t * lr + (1 - t) * l1r)


def recon_delem(r, t, loss, defect=None):
    """d error / d recon: 2 (r - t); sign(r - t) with 0 at a tie; ATen's (r - t) / max((1 - r) r, 1e-12f)."""
    if loss == "mse":
        return 2 * (r - t)
    if loss == "l1":
        s = torch.sign(r - t)
        return torch.where(s == 0, torch.ones_like(s), s) if defect == "l1_tie_sign" else s
    den = (1 - r) * r
    return (r - t) / (den if defect == "bce_bwd_unclamped" else den.clamp(min=BCE_EPS))


def recon_rows(x, r, loss, defect=None):
    """Per-sample sums [B].  The two slicing defects are emulated on the kernel's own slices: the float4 loop of a slice
    reads whole groups of 4 from its start (so an unrounded chunk runs over its end), an unclamped end runs into the
    next row (the storage is walked flat; past its end nothing is added)."""
    B, P = r.shape
    if defect not in ("chunk_unrounded", "end_unclamped"):
        return recon_elem(r, x, loss, defect).sum(1)
    e = recon_elem(r, x, loss).reshape(-1)
    splits = recon_splits(B, P)
    chunk = recon_chunk(B, P, rounded=defect != "chunk_unrounded")
    vec = P % 4 == 0
    rows = torch.zeros(B, dtype=r.dtype)
    for b in range(B):
        for s in range(splits):
            beg = s * chunk
            end = beg + chunk if defect == "end_unclamped" else min(beg + chunk, P)
            if end <= beg:
                continue
            if vec:
                end = beg + cdiv(end - beg, 4) * 4
            rows[b] += e[b * P + beg:min(b * P + end, B * P)].sum()
    return rows


def reduce_rows(rows, reduction, scale=1.0, defect=None, P=None):
    if reduction == "none":
        return scale * rows
    if reduction == "sum":
        return scale * rows.sum()
    return scale * rows.sum() / (P if defect == "mean_over_P" else rows.shape[0])


def recon_loss(x, r, loss, reduction, scale=1.0, defect=None):
    return reduce_rows(recon_rows(x, r, loss, defect), reduction, scale, defect, r.shape[1])


def recon_loss_grad(x, r, g, loss, reduction, scale=1.0, defect=None):
    """d (g . loss) / d recon; g is [B] for reduction none, a scalar otherwise."""
    B, P = r.shape
    d = recon_delem(r, x, loss, defect)
    if reduction == "none":
        return (scale * g).reshape(B, 1) * d
    return (scale * g / ((P if defect == "mean_over_P" else B) if reduction == "mean" else 1)) * d


# ---- scalar heads ----------------------------------------------------------------------------------------------------
def exp_elbo(a, b, c):
    return torch.exp(c * (a + b)).mean()


def exp_elbo_grad(a, b, c, g, defect=None):
    """d (g * exp_elbo) / d a = d / d b."""
    w = torch.exp(c * (a + b)) * c
    return g * (w if defect == "elbo_weight_no_B" else w / a.shape[0])


def lincomb(weights, terms):
    out = terms[0] * 0
    for w, t in zip(weights, terms):
        out = out + w * t
    return out


# ---- gradient norm and clip ------------------------------------------------------------------------------------------
def sumsq(x, defect=None):
    x = x.double().reshape(-1)
    if defect == "sumsq_tail_dropped":
        x = x[:x.numel() // 4 * 4]
    return (x * x).sum()


def total_norm(parts, defect=None):
    return math.sqrt(sum(float(sumsq(p, defect)) for p in parts))


def clip_coef(norm, clip):
    """torch.nn.utils.clip_grad_norm_: min(1, clip / (norm + 1e-6))."""
    return min(1.0, clip / (norm + 1e-6))


def scale_by(x, coef, defect=None):
    y = x * coef
    if defect == "scale_tail_twice":
        n = x.numel()
        y.reshape(-1)[n // 4 * 4:] *= coef
    return y


# ---- nn.Linear -------------------------------------------------------------------------------------------------------
def _split_gemm(A, Bm, defect):
    """A [M, K] @ Bm [K, N] with the two K-walk defects of the plan of that GEMM."""
    M, K = A.shape
    N = Bm.shape[1]
    out = A @ Bm
    _, _, ktiles, splits, kps = gemm_plan(M, N, K)
    if defect == "k_tail_kept" and ktiles * 32 > K:
        out = out + (ktiles * 32 - K) * torch.outer(A[:, K - 1], Bm[K - 1])
    if defect == "full_last_split" and splits > 1 and splits * kps > ktiles:
        lo, hi = (ktiles - kps) * 32, (splits - 1) * kps * 32
        out = out + A[:, lo:hi] @ Bm[lo:hi]
    return out


def linear_fwd(x, w, bias=None, defect=None):
    y = _split_gemm(x, w.t(), defect)
    if bias is not None:
        s = gemm_plan(x.shape[0], w.shape[0], x.shape[1])[3]
        y = y + (s if defect == "bias_per_split" else 1) * bias
    return y


def linear_dgrad(dy, w, defect=None):
    return _split_gemm(dy, w, defect)


def linear_wgrad(dy, x, into=None, defect=None):
    dw = _split_gemm(dy.t(), x, defect)
    if into is None:
        return dw
    s = gemm_plan(dy.shape[1], x.shape[1], x.shape[0])[3]
    return dw if (defect == "accumulate_ignored" and s > 1) else into + dw


def bias_grad(dy, into=None):
    """dy [B, C] or [B, C, HW] -> [C]."""
    db = dy.sum(0) if dy.dim() == 2 else dy.sum((0, 2))
    return db if into is None else into + db


# ---- pointwise / resampling ------------------------------------------------------------------------------------------
def avgpool2(x):
    B, C, H, W = x.shape
    v = x.reshape(B, C, H // 2, 2, W // 2, 2)
    return 0.25 * ((v[:, :, :, 0, :, 0] + v[:, :, :, 0, :, 1]) + (v[:, :, :, 1, :, 0] + v[:, :, :, 1, :, 1]))


def upsample2(x):
    return x.repeat_interleave(2, 2).repeat_interleave(2, 3)


def avgpool2_adjoint(dy):
    return 0.25 * upsample2(dy)


def upsample2_adjoint(dy):
    B, C, H2, W2 = dy.shape
    v = dy.reshape(B, C, H2 // 2, 2, W2 // 2, 2)
    return (v[:, :, :, 0, :, 0] + v[:, :, :, 0, :, 1]) + (v[:, :, :, 1, :, 0] + v[:, :, :, 1, :, 1])


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def sigmoid_grad(x, dy):
    s = sigmoid(x)
    return dy * (1 - s) * s


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def lrelu_grad(x, dy, slope):
    return torch.where(x > 0, dy, dy * slope)


def hflip(x, flip, defect=None):
    """x [B, rows, W]: image b mirrored along W where flip[b] != 0.  The defective index W - w reads one element further
    on in the flat storage (nothing past its end: 0)."""
    B, rows, W = x.shape
    if defect != "flip_off_by_one":
        return torch.where((flip != 0).reshape(B, 1, 1), x.flip(2), x)
    flat = torch.cat([x.reshape(-1), x.new_zeros(1)])
    w = torch.arange(W)
    idx = (torch.arange(B * rows).reshape(-1, 1) * W + (W - w)).reshape(B, rows, W)
    return torch.where((flip != 0).reshape(B, 1, 1), flat[idx], x)
