"""Case tables of the exact-fp32 gather GEMMs (conv_igemm.hip), the direct kernels (conv_small.hip) and the
in-kernel-split kernels, with the fp64 reference they are compared against.  Importable without a GPU:
test_conv_cases_host.py proves on the CPU that the tables reach every kernel instance and every listed edge,
test_hip_conv_fp32.py runs them on the device.

A case is ``(id, (B, Ci, H, W, Co, KS, up2, bias, accumulate))``.  H, W are the conv's output size (with up2 its input
is H/2 x W/2); ``bias`` and ``accumulate`` are 0 / 1.  The id names the instance or edge the case is there for.

Table A (forward-type GEMM, itcv_conv2d_fwd): every case runs twice, as the forward Ci -> Co with the for_dgrad = 0
packing and as the data gradient Co -> Ci on dy with the for_dgrad = 1 packing (never up2, never a bias).
Table B (weight gradient, itcv_conv2d_wgrad).  Table C (direct kernels): a layer with at most 4 output channels runs
its forward on small_cout<KS, Co> and its data gradient on small_cin<KS, Co, DGRAD>; a layer with at most 4 input
channels its forward on small_cin<KS, Ci> and its data gradient on small_cout<KS, Ci, DGRAD>.  Table D (in-kernel-split
kernels): every case runs under bf16x3 and bf16x6, forward, data gradient where the split kernel takes the exchanged
shape, and weight gradient where it takes the shape.

The planning rules the instance of a case follows from are mirrored here in a few lines (``fwd_launch``,
``wgrad_launch``); the host test pins the mirrors against literals and against the library's ``*_variant`` words."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

Case = namedtuple("Case", "B Ci H W Co KS up2 bias accumulate")

CEILING = 2e-5              # exact-fp32 kernels, direct kernels, bf16x6: of the output scale
CEILING_BF16X3 = 5e-5
E32_MARGIN, E32_FLOOR = 4.0, 2.0 ** -22


def cdiv(a, b):
    return -(-a // b)


def tile_rows(M):
    return 32 if M <= 32 else (64 if M <= 64 else 128)


# ---- mirrors of the host's planning rules ---------------------------------------------------------------------------
FwdLaunch = namedtuple("FwdLaunch", "KS BM up2 tail BN mt nt ktiles splits kps")
WgradLaunch = namedtuple("WgradLaunch", "KS up2 CB BM swapped ktiles splits kps small_reduce w_pow2 hw_pow2")


def variant_fields(word):
    """(BM, KS, up2, splits) of an itcv_conv2d_*_variant word."""
    return word & 255, (word >> 8) & 255, (word >> 16) & 1, word >> 20


def fwd_launch(lib, B, Ci, H, W, Co, KS, up2):
    """What itcv_conv2d_fwd launches for a forward-type GEMM Ci -> Co: BM, KS, up2 and the split count from the
    library's variant word; CI_TAIL, the pixel tile and the K tiles mirrored."""
    BM, ks, u, splits = variant_fields(lib.itcv_conv2d_fwd_variant(B, Ci, H, W, Co, KS, int(up2)))
    BN = 128 if BM == 128 else 256
    ktiles = KS * KS * cdiv(Ci, 16)
    return FwdLaunch(ks, BM, u, int(Ci & 15 != 0), BN, cdiv(Co, BM), cdiv(B * H * W, BN), ktiles, splits, cdiv(ktiles, splits))


def col_block(Ci):
    """CB of conv_wgrad_kernel: reduction channels per 128-column tile."""
    return 4 if Ci <= 4 else 16 if Ci <= 16 else 32 if Ci <= 32 else 64 if Ci <= 64 else 128


def swapped(Ci, Co, up2):
    return Co <= 4 < Ci and not up2


def wgrad_launch(lib, B, Ci, H, W, Co, KS, up2):
    """What itcv_conv2d_wgrad launches: with few output channels the operands are exchanged, and tile rows, column block
    and split count are those of the exchanged shape; the small reduce takes weight tensors of at most 65536 elements
    from 32 slices on."""
    sw = swapped(Ci, Co, up2)
    ci, co = (Co, Ci) if sw else (Ci, Co)
    BM, ks, u, splits = variant_fields(lib.itcv_conv2d_wgrad_variant(B, ci, H, W, co, KS, int(up2)))
    ktiles = cdiv(B * H * W, 32)
    small = Co * Ci * KS * KS <= 65536 and splits >= 32
    pow2 = lambda n: n & (n - 1) == 0
    return WgradLaunch(ks, u, col_block(ci), BM, int(sw), ktiles, splits, cdiv(ktiles, splits), int(small), int(pow2(W)),
                       int(pow2(H * W)))


# The library has no variant query for the in-kernel-split kernels; these two restate plan_fwd(kFwdSplit) (64 rows up to
# Co = 64, else 128) and plan_wgrad(min_bm = 64) of conv_igemm.hip, and the host test pins them as literals.
def split_fwd_instance(B, Ci, H, W, Co, KS, up2, ns):
    """conv_fwd_bf16s_ws_kernel<KS, ns, BM, UP2>."""
    return KS, ns, 64 if Co <= 64 else 128, int(up2)


def split_wgrad_instance(B, Ci, H, W, Co, KS, ns):
    """conv_wgrad_bf16s_kernel<KS, ns, CB, BM> (CB: the fp32 kernel's rule, no block narrower than 32 as Ci % 32 == 0)."""
    return KS, ns, col_block(Ci), 64 if Co <= 64 else 128


# ---- table A: forward-type GEMM ------------------------------------------------------------------------------------
# id: k<KS>-m<BM>[-up2][-tail] of the forward launch, then what else the case is there for
TABLE_A = [
    # KS = 1: Ci < 128 has fewer than 8 K tiles -> no K split, the bias is added inside the kernel
    ("k1-m32-images-in-tile-unsplit-bias", (2, 16, 6, 10, 5, 1, 0, 1, 0)),
    ("k1-m32-tail-co1-5x3-unsplit", (3, 17, 5, 3, 1, 1, 0, 0, 0)),
    ("k1-m32-up2-src1x1", (2, 32, 2, 2, 8, 1, 1, 1, 0)),
    ("k1-m32-up2-tail", (1, 17, 4, 6, 32, 1, 1, 0, 0)),
    ("k1-m64-hw400", (1, 32, 20, 20, 64, 1, 0, 0, 0)),
    ("k1-m64-tail-ci24", (2, 24, 5, 3, 40, 1, 0, 1, 0)),
    ("k1-m64-up2", (2, 16, 8, 4, 64, 1, 1, 0, 0)),
    ("k1-m64-up2-tail-co33-6x10", (2, 24, 6, 10, 33, 1, 1, 1, 0)),
    ("k1-m128-nt10-unsplit-bias", (3, 16, 20, 20, 129, 1, 0, 1, 0)),
    ("k1-m128-tail-h1", (2, 17, 1, 7, 130, 1, 0, 0, 0)),
    ("k1-m128-up2", (1, 32, 6, 10, 130, 1, 1, 1, 0)),
    ("k1-m128-up2-tail-ci1-co65", (2, 1, 4, 4, 65, 1, 1, 0, 0)),
    ("k1-m32-nt10-two-grid-groups", (6, 16, 20, 20, 8, 1, 0, 1, 0)),
    ("k1-m32-split-even", (2, 128, 4, 4, 16, 1, 0, 1, 0)),
    ("k1-m64-split-short-nobias", (1, 144, 3, 5, 64, 1, 0, 0, 0)),
    # KS = 3: nine K tiles at least, so every small shape writes slabs
    ("k3-m32-short-slice-bias", (2, 16, 6, 10, 5, 3, 0, 1, 0)),
    ("k3-m32-tail-co1-5x3", (1, 17, 5, 3, 1, 3, 0, 0, 0)),
    ("k3-m32-up2", (2, 32, 4, 4, 24, 3, 1, 1, 0)),
    ("k3-m32-up2-src1x1", (2, 16, 2, 2, 8, 3, 1, 0, 0)),
    ("k3-m32-up2-tail-ci1", (3, 1, 6, 6, 5, 3, 1, 0, 0)),
    ("k3-m64-hw400-bias", (1, 16, 20, 20, 33, 3, 0, 1, 0)),
    ("k3-m64-tail-ci24", (2, 24, 8, 8, 40, 3, 0, 0, 0)),
    ("k3-m64-up2", (2, 32, 8, 8, 33, 3, 1, 0, 0)),
    ("k3-m64-up2-tail-6x10", (2, 24, 6, 10, 64, 3, 1, 1, 0)),
    ("k3-m128-co129", (2, 32, 6, 10, 129, 3, 0, 0, 0)),
    ("k3-m128-tail-nt10-co130", (3, 24, 20, 20, 130, 3, 0, 1, 0)),
    ("k3-m128-up2", (1, 16, 8, 12, 130, 3, 1, 1, 0)),
    ("k3-m128-up2-tail-co65", (2, 17, 4, 4, 65, 3, 1, 0, 0)),
    ("k3-m32-even-slices", (2, 64, 4, 4, 8, 3, 0, 1, 0)),
    ("k3-m32-w1", (2, 16, 9, 1, 16, 3, 0, 0, 0)),
    ("k3-m128-unsplit-192-tiles-bias", (2, 16, 64, 64, 260, 3, 0, 1, 0)),
    # KS = 5
    ("k5-m32-images-in-tile", (2, 16, 6, 10, 5, 5, 0, 1, 0)),
    ("k5-m32-tail-ci1-w2", (2, 1, 5, 2, 32, 5, 0, 0, 0)),
    ("k5-m32-up2-src1x1", (1, 32, 2, 2, 8, 5, 1, 0, 0)),
    ("k5-m32-up2-tail", (2, 17, 4, 6, 20, 5, 1, 1, 0)),
    ("k5-m64-h1", (2, 16, 1, 9, 64, 5, 0, 0, 0)),
    ("k5-m64-tail-w1-co33", (1, 24, 7, 1, 33, 5, 0, 1, 0)),
    ("k5-m64-up2", (2, 32, 4, 8, 48, 5, 1, 0, 0)),
    ("k5-m64-up2-tail-6x10", (1, 24, 6, 10, 64, 5, 1, 1, 0)),
    ("k5-m128-nt10-co129", (3, 16, 20, 20, 129, 5, 0, 0, 0)),
    ("k5-m128-tail-5x3-co130", (1, 17, 5, 3, 130, 5, 0, 1, 0)),
    ("k5-m128-up2", (2, 16, 8, 8, 72, 5, 1, 0, 0)),
    ("k5-m128-up2-tail-ci1-co65", (1, 1, 6, 10, 65, 5, 1, 1, 0)),
    ("k5-m32-64-slices", (1, 528, 4, 4, 8, 5, 0, 1, 0)),
    ("k5-m128-tail-unsplit-192-tiles", (2, 2, 64, 64, 260, 5, 0, 0, 0)),
]

# ---- table B: weight gradient --------------------------------------------------------------------------------------
# id: k<KS>[-up2]-c<CB>-m<BM> of the launch (the exchanged shape's where the operands are exchanged), then the edge
TABLE_B = [
    # one case per <KS, UP2, CB, BM>
    ("k1-c4-m32-ci3-co5-8x8", (2, 3, 8, 8, 5, 1, 0, 0, 0)),
    ("k1-c4-m64-ci4-co33-3x8-acc", (1, 4, 3, 8, 33, 1, 0, 0, 1)),
    ("k1-c4-m128-ci1-co65-6x10", (3, 1, 6, 10, 65, 1, 0, 0, 0)),
    ("k1-c16-m32-ci5-co32-5x3-acc", (1, 5, 5, 3, 32, 1, 0, 0, 1)),
    ("k1-c16-m64-ci12-co64-4x16", (2, 12, 4, 16, 64, 1, 0, 0, 0)),
    ("k1-c16-m128-ci16-co129-20x20-acc", (3, 16, 20, 20, 129, 1, 0, 0, 1)),
    ("k1-c32-m32-ci17-co8-1x7", (1, 17, 1, 7, 8, 1, 0, 0, 0)),
    ("k1-c32-m64-ci32-co40-2x2-acc", (2, 32, 2, 2, 40, 1, 0, 0, 1)),
    ("k1-c32-m128-ci24-co130-16x16", (2, 24, 16, 16, 130, 1, 0, 0, 0)),
    ("k1-c64-m32-ci33-co16-7x1-acc", (1, 33, 7, 1, 16, 1, 0, 0, 1)),
    ("k1-c64-m64-ci48-co33-8x8", (2, 48, 8, 8, 33, 1, 0, 0, 0)),
    ("k1-c64-m128-ci64-co65-3x8-acc", (1, 64, 3, 8, 65, 1, 0, 0, 1)),
    ("k1-c128-m32-ci65-co5-6x10", (3, 65, 6, 10, 5, 1, 0, 0, 0)),
    ("k1-c128-m64-ci129-co48-5x3-acc", (1, 129, 5, 3, 48, 1, 0, 0, 1)),
    ("k1-c128-m128-ci200-co129-4x16", (2, 200, 4, 16, 129, 1, 0, 0, 0)),
    ("k1-up2-c4-m32-ci2-co24-2x16-acc", (1, 2, 2, 16, 24, 1, 1, 0, 1)),
    ("k1-up2-c4-m64-ci4-co64-8x8", (2, 4, 8, 8, 64, 1, 1, 0, 0)),
    ("k1-up2-c4-m128-ci3-co72-6x8-acc", (1, 3, 6, 8, 72, 1, 1, 0, 1)),
    ("k1-up2-c16-m32-ci5-co5-6x10", (3, 5, 6, 10, 5, 1, 1, 0, 0)),
    ("k1-up2-c16-m64-ci16-co33-2x2-acc", (2, 16, 2, 2, 33, 1, 1, 0, 1)),
    ("k1-up2-c16-m128-ci8-co65-4x6", (1, 8, 4, 6, 65, 1, 1, 0, 0)),
    ("k1-up2-c32-m32-ci17-co32-20x20-acc", (2, 17, 20, 20, 32, 1, 1, 0, 1)),
    ("k1-up2-c32-m64-ci32-co64-4x4", (3, 32, 4, 4, 64, 1, 1, 0, 0)),
    ("k1-up2-c32-m128-ci20-co129-2x16-acc", (1, 20, 2, 16, 129, 1, 1, 0, 1)),
    ("k1-up2-c64-m32-ci33-co8-8x8", (2, 33, 8, 8, 8, 1, 1, 0, 0)),
    ("k1-up2-c64-m64-ci64-co40-6x8-acc", (1, 64, 6, 8, 40, 1, 1, 0, 1)),
    ("k1-up2-c64-m128-ci40-co130-6x10", (3, 40, 6, 10, 130, 1, 1, 0, 0)),
    ("k1-up2-c128-m32-ci256-co16-2x2-acc", (2, 256, 2, 2, 16, 1, 1, 0, 1)),
    ("k1-up2-c128-m64-ci128-co33-4x6", (1, 128, 4, 6, 33, 1, 1, 0, 0)),
    ("k1-up2-c128-m128-ci65-co65-20x20-acc", (2, 65, 20, 20, 65, 1, 1, 0, 1)),
    ("k3-c4-m32-ci3-co5-8x8", (2, 3, 8, 8, 5, 3, 0, 0, 0)),
    ("k3-c4-m64-ci4-co48-3x8-acc", (1, 4, 3, 8, 48, 3, 0, 0, 1)),
    ("k3-c4-m128-ci1-co129-6x10", (3, 1, 6, 10, 129, 3, 0, 0, 0)),
    ("k3-c16-m32-ci5-co24-5x3-acc", (1, 5, 5, 3, 24, 3, 0, 0, 1)),
    ("k3-c16-m64-ci12-co64-4x16", (2, 12, 4, 16, 64, 3, 0, 0, 0)),
    ("k3-c16-m128-ci16-co72-20x20-acc", (3, 16, 20, 20, 72, 3, 0, 0, 1)),
    ("k3-c32-m32-ci17-co5-1x7", (1, 17, 1, 7, 5, 3, 0, 0, 0)),
    ("k3-c32-m64-ci32-co33-2x2-acc", (2, 32, 2, 2, 33, 3, 0, 0, 1)),
    ("k3-c32-m128-ci24-co65-16x16", (2, 24, 16, 16, 65, 3, 0, 0, 0)),
    ("k3-c64-m32-ci33-co32-7x1-acc", (1, 33, 7, 1, 32, 3, 0, 0, 1)),
    ("k3-c64-m64-ci48-co64-8x8", (2, 48, 8, 8, 64, 3, 0, 0, 0)),
    ("k3-c64-m128-ci64-co129-3x8-acc", (1, 64, 3, 8, 129, 3, 0, 0, 1)),
    ("k3-c128-m32-ci65-co8-6x10", (3, 65, 6, 10, 8, 3, 0, 0, 0)),
    ("k3-c128-m64-ci129-co40-5x3-acc", (1, 129, 5, 3, 40, 3, 0, 0, 1)),
    ("k3-c128-m128-ci200-co130-4x16", (2, 200, 4, 16, 130, 3, 0, 0, 0)),
    ("k3-up2-c4-m32-ci2-co16-20x20-acc", (2, 2, 20, 20, 16, 3, 1, 0, 1)),
    ("k3-up2-c4-m64-ci4-co33-4x4", (3, 4, 4, 4, 33, 3, 1, 0, 0)),
    ("k3-up2-c4-m128-ci3-co65-2x16-acc", (1, 3, 2, 16, 65, 3, 1, 0, 1)),
    ("k3-up2-c16-m32-ci5-co5-8x8", (2, 5, 8, 8, 5, 3, 1, 0, 0)),
    ("k3-up2-c16-m64-ci16-co48-6x8-acc", (1, 16, 6, 8, 48, 3, 1, 0, 1)),
    ("k3-up2-c16-m128-ci8-co129-6x10", (3, 8, 6, 10, 129, 3, 1, 0, 0)),
    ("k3-up2-c32-m32-ci17-co24-2x2-acc", (2, 17, 2, 2, 24, 3, 1, 0, 1)),
    ("k3-up2-c32-m64-ci32-co64-4x6", (1, 32, 4, 6, 64, 3, 1, 0, 0)),
    ("k3-up2-c32-m128-ci20-co72-20x20-acc", (2, 20, 20, 20, 72, 3, 1, 0, 1)),
    ("k3-up2-c64-m32-ci33-co5-4x4", (3, 33, 4, 4, 5, 3, 1, 0, 0)),
    ("k3-up2-c64-m64-ci64-co33-2x16-acc", (1, 64, 2, 16, 33, 3, 1, 0, 1)),
    ("k3-up2-c64-m128-ci40-co65-8x8", (2, 40, 8, 8, 65, 3, 1, 0, 0)),
    ("k3-up2-c128-m32-ci256-co32-6x8-acc", (1, 256, 6, 8, 32, 3, 1, 0, 1)),
    ("k3-up2-c128-m64-ci128-co64-6x10", (3, 128, 6, 10, 64, 3, 1, 0, 0)),
    ("k3-up2-c128-m128-ci65-co129-2x2-acc", (2, 65, 2, 2, 129, 3, 1, 0, 1)),
    ("k5-c4-m32-ci3-co8-8x8", (2, 3, 8, 8, 8, 5, 0, 0, 0)),
    ("k5-c4-m64-ci4-co40-3x8-acc", (1, 4, 3, 8, 40, 5, 0, 0, 1)),
    ("k5-c4-m128-ci1-co130-6x10", (3, 1, 6, 10, 130, 5, 0, 0, 0)),
    ("k5-c16-m32-ci5-co16-5x3-acc", (1, 5, 5, 3, 16, 5, 0, 0, 1)),
    ("k5-c16-m64-ci12-co33-4x16", (2, 12, 4, 16, 33, 5, 0, 0, 0)),
    ("k5-c16-m128-ci16-co65-20x20-acc", (3, 16, 20, 20, 65, 5, 0, 0, 1)),
    ("k5-c32-m32-ci17-co5-1x7", (1, 17, 1, 7, 5, 5, 0, 0, 0)),
    ("k5-c32-m64-ci32-co48-2x2-acc", (2, 32, 2, 2, 48, 5, 0, 0, 1)),
    ("k5-c32-m128-ci24-co129-16x16", (2, 24, 16, 16, 129, 5, 0, 0, 0)),
    ("k5-c64-m32-ci33-co24-7x1-acc", (1, 33, 7, 1, 24, 5, 0, 0, 1)),
    ("k5-c64-m64-ci48-co64-8x8", (2, 48, 8, 8, 64, 5, 0, 0, 0)),
    ("k5-c64-m128-ci64-co72-3x8-acc", (1, 64, 3, 8, 72, 5, 0, 0, 1)),
    ("k5-c128-m32-ci65-co5-6x10", (3, 65, 6, 10, 5, 5, 0, 0, 0)),
    ("k5-c128-m64-ci129-co33-5x3-acc", (1, 129, 5, 3, 33, 5, 0, 0, 1)),
    ("k5-c128-m128-ci200-co65-4x16", (2, 200, 4, 16, 65, 5, 0, 0, 0)),
    ("k5-up2-c4-m32-ci2-co32-2x2-acc", (2, 2, 2, 2, 32, 5, 1, 0, 1)),
    ("k5-up2-c4-m64-ci4-co64-4x6", (1, 4, 4, 6, 64, 5, 1, 0, 0)),
    ("k5-up2-c4-m128-ci3-co129-20x20-acc", (2, 3, 20, 20, 129, 5, 1, 0, 1)),
    ("k5-up2-c16-m32-ci5-co8-4x4", (3, 5, 4, 4, 8, 5, 1, 0, 0)),
    ("k5-up2-c16-m64-ci16-co40-2x16-acc", (1, 16, 2, 16, 40, 5, 1, 0, 1)),
    ("k5-up2-c16-m128-ci8-co130-8x8", (2, 8, 8, 8, 130, 5, 1, 0, 0)),
    ("k5-up2-c32-m32-ci17-co16-6x8-acc", (1, 17, 6, 8, 16, 5, 1, 0, 1)),
    ("k5-up2-c32-m64-ci32-co33-6x10", (3, 32, 6, 10, 33, 5, 1, 0, 0)),
    ("k5-up2-c32-m128-ci20-co65-2x2-acc", (2, 20, 2, 2, 65, 5, 1, 0, 1)),
    ("k5-up2-c64-m32-ci33-co5-4x6", (1, 33, 4, 6, 5, 5, 1, 0, 0)),
    ("k5-up2-c64-m64-ci64-co48-20x20-acc", (2, 64, 20, 20, 48, 5, 1, 0, 1)),
    ("k5-up2-c64-m128-ci40-co129-4x4", (3, 40, 4, 4, 129, 5, 1, 0, 0)),
    ("k5-up2-c128-m32-ci256-co24-2x16-acc", (1, 256, 2, 16, 24, 5, 1, 0, 1)),
    ("k5-up2-c128-m64-ci128-co64-8x8", (2, 128, 8, 8, 64, 5, 1, 0, 0)),
    ("k5-up2-c128-m128-ci65-co72-6x8-acc", (1, 65, 6, 8, 72, 5, 1, 0, 1)),
    # the swapped form (Co <= 4 < Ci, not up2: the kernel runs the exchanged shape) through both reduce kernels, its neighbours
    ("k5-c4-m64-swapped-ci64-co3", (2, 64, 8, 8, 3, 5, 0, 0, 0)),
    ("k3-c4-m128-swapped-ci200-co4-6x10-acc", (1, 200, 6, 10, 4, 3, 0, 0, 1)),
    ("k1-c4-m32-swapped-ci17-co1-5x3", (3, 17, 5, 3, 1, 1, 0, 0, 0)),
    ("k5-c4-m64-swapped-small-reduce-32-slices", (2, 64, 64, 64, 3, 5, 0, 0, 0)),
    ("k3-c4-m64-swapped-small-reduce-acc", (2, 33, 64, 64, 2, 3, 0, 0, 1)),
    ("k3-c4-m32-ci4-co4-not-swapped", (1, 4, 6, 10, 4, 3, 0, 0, 0)),
    ("k3-c4-m32-ci5-co4-swapped-acc", (1, 5, 6, 10, 4, 3, 0, 0, 1)),
    ("k3-c4-m32-ci4-co5-acc", (1, 4, 6, 10, 5, 3, 0, 0, 1)),
    ("k3-c16-m32-ci5-co5", (1, 5, 6, 10, 5, 3, 0, 0, 0)),
    ("k3-up2-c64-m32-co3-not-swapped", (2, 64, 8, 8, 3, 3, 1, 0, 0)),
    # K slices: several with a short last one, a count above 8 that is no multiple of 8, exactly even ones
    ("k3-c16-m32-4-slices-short-acc", (3, 8, 20, 20, 16, 3, 0, 0, 1)),
    ("k3-c16-m32-9-slices-short", (6, 8, 20, 20, 16, 3, 0, 0, 0)),
    ("k3-c16-m32-12-slices-even", (3, 8, 32, 32, 16, 3, 0, 0, 0)),
    # the small reduce: at most 65536 weights from 32 slices on (8192 pixels and few tiles), 16 k and 16 k + 5 slices
    ("k5-c4-m64-small-reduce-32-slices", (2, 3, 64, 64, 64, 5, 0, 0, 0)),
    ("k5-c4-m64-small-reduce-37-slices-acc", (2, 3, 64, 74, 64, 5, 0, 0, 1)),
]

# ---- table C: direct kernels ---------------------------------------------------------------------------------------
# small_cout: Co <= 4 output channels, Ci reduction channels in LDS chunks of 8.  id: out<KS>-<Co>
TABLE_C_COUT = [
    ("out3-1-c1-5x3", (2, 1, 5, 3, 1, 3, 0, 0, 0)),
    ("out3-2-c7-17x33-bias", (1, 7, 17, 33, 2, 3, 0, 1, 0)),
    ("out3-3-c8-16x16", (2, 8, 16, 16, 3, 3, 0, 0, 0)),
    ("out3-4-c9-16x40-bias", (1, 9, 16, 40, 4, 3, 0, 1, 0)),
    ("out5-1-c20-16x16-bias", (1, 20, 16, 16, 1, 5, 0, 1, 0)),
    ("out5-2-c9-5x3", (3, 9, 5, 3, 2, 5, 0, 0, 0)),
    ("out5-3-c7-16x40-bias", (2, 7, 16, 40, 3, 5, 0, 1, 0)),
    ("out5-4-c8-17x33", (1, 8, 17, 33, 4, 5, 0, 0, 0)),
    ("out3-3-c20-17x33-bias", (2, 20, 17, 33, 3, 3, 0, 1, 0)),
    ("out5-3-c1-17x33", (1, 1, 17, 33, 3, 5, 0, 0, 0)),
]
# small_cin: Ci <= 4 reduction channels held in registers.  id: in<KS>-<Ci>
TABLE_C_CIN = [
    ("in3-1-co1-5x3", (2, 1, 5, 3, 1, 3, 0, 0, 0)),
    ("in3-2-co5-17x33-bias", (1, 2, 17, 33, 5, 3, 0, 1, 0)),
    ("in3-3-co70-16x16", (1, 3, 16, 16, 70, 3, 0, 0, 0)),
    ("in3-4-co5-16x40-bias", (2, 4, 16, 40, 5, 3, 0, 1, 0)),
    ("in5-1-co5-16x16-bias", (2, 1, 16, 16, 5, 5, 0, 1, 0)),
    ("in5-2-co70-5x3", (1, 2, 5, 3, 70, 5, 0, 0, 0)),
    ("in5-3-co70-17x33-bias", (1, 3, 17, 33, 70, 5, 0, 1, 0)),
    ("in5-4-co1-16x40", (2, 4, 16, 40, 1, 5, 0, 0, 0)),
]

# ---- table D: in-kernel-split kernels ------------------------------------------------------------------------------
# the smaller shapes of test_hip_ops.SPLIT_CASES, then what they leave out: KS = 1 forms (with up2 on the forward), images
# 8 and 24 pixels wide (the weight gradient reads 8-pixel chunks and masks one pixel per row edge), accumulate
TABLE_D = [
    ("k3-m64-c32", (2, 32, 8, 8, 40, 3, 0, 0, 0)),
    ("k3-m64-c64", (3, 64, 16, 16, 64, 3, 0, 0, 0)),
    ("k3-m128-c128-12x24", (2, 96, 12, 24, 130, 3, 0, 0, 0)),
    ("k3-m128-c128-8x16", (3, 128, 8, 16, 96, 3, 0, 0, 0)),
    ("k1-m64-c64", (2, 64, 8, 8, 64, 1, 0, 0, 0)),
    ("k3-m64-up2-c32-w8", (3, 32, 24, 8, 64, 3, 1, 0, 0)),
    ("k1-m128-h1w1", (5, 64, 1, 1, 70, 1, 0, 0, 0)),
    ("k3-m64-up2-c64", (2, 64, 16, 16, 48, 3, 1, 0, 0)),
    ("k1-m64-up2-c32-w8-acc", (2, 32, 4, 8, 40, 1, 1, 1, 1)),
    ("k1-m128-up2-c64-w24", (1, 64, 6, 24, 130, 1, 1, 0, 0)),
    ("k1-m64-c128-w24-acc", (2, 128, 3, 24, 64, 1, 0, 1, 1)),
    ("k1-m128-c32-w8", (3, 32, 5, 8, 96, 1, 0, 0, 0)),
    ("k1-m128-c128-acc", (2, 160, 4, 16, 129, 1, 0, 0, 1)),
    ("k3-m128-c32-w24-acc", (1, 32, 6, 24, 72, 3, 0, 1, 1)),
    ("k3-m128-up2-c64-w8", (2, 64, 10, 8, 130, 3, 1, 0, 0)),
    ("k3-m64-c128-w8-acc", (3, 96, 7, 8, 33, 3, 0, 1, 1)),
]

TABLES = {"A": TABLE_A, "B": TABLE_B, "C_cout": TABLE_C_COUT, "C_cin": TABLE_C_CIN, "D": TABLE_D}


def cases(table):
    return [(cid, Case(*shape)) for cid, shape in TABLES[table]]


def ids(table):
    return [cid for cid, _ in TABLES[table]]


# ---- inputs and the fp64 reference ---------------------------------------------------------------------------------
def seed_of(shape, salt=0):
    """A fixed generator seed derived from the tuple (not hash(): that changes between interpreter runs)."""
    s = 1000003 * salt + 17
    for v in shape:
        s = (s * 131 + int(v) + 1) % (2 ** 31 - 1)
    return s


def rel_err(a, b):
    """max |a - b| / max |b|: the error of a whole array in units of its scale."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def bound_of(e32):
    """What an exact-fp32 array is held to: 4x the error of PyTorch's fp32 CPU operator on the same inputs (another
    summation order: MFMA 32x32x2 chains, split-K slabs folded in slice order), not below 2^-22, under the ceiling."""
    return min(CEILING, max(E32_MARGIN * e32, E32_FLOOR))


Reference = namedtuple("Reference", "x w b dy dw0 y dxu dx dw e32")


def _conv(x, w, b, c):
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if c.up2 else x
    xin.retain_grad()
    return xin, F.conv2d(xin, w, b, padding=c.KS // 2)


@functools.lru_cache(maxsize=8)
def reference(c, salt=0):
    """fp32 inputs of a case (as test_hip_ops draws them) and its fp64 results: y, dxu (the gradient of the conv's own
    input, [B, Ci, H, W]: what the data-gradient GEMM computes), dx (of x: through the upsampling's adjoint under up2),
    dw (with ``accumulate`` the sum includes the preloaded target dw0).  e32: the error of the fp32 CPU operator, per array."""
    c = Case(*c)
    g = torch.Generator().manual_seed(seed_of(c, salt))
    hs, ws = (c.H // 2, c.W // 2) if c.up2 else (c.H, c.W)
    x = torch.randn(c.B, c.Ci, hs, ws, generator=g)
    w = torch.randn(c.Co, c.Ci, c.KS, c.KS, generator=g) / (c.Ci * c.KS * c.KS) ** 0.5
    b = torch.randn(c.Co, generator=g) if c.bias else None
    dy = torch.randn(c.B, c.Co, c.H, c.W, generator=g)
    out = {}
    for dt in (torch.float64, torch.float32):
        xr, wr = x.to(dt, copy=True).requires_grad_(True), w.to(dt, copy=True).requires_grad_(True)
        xin, y = _conv(xr, wr, None if b is None else b.to(dt), c)
        y.backward(dy.to(dt))
        out[dt] = [y.detach(), xin.grad if c.up2 else xr.grad, xr.grad, wr.grad]
    y, dxu, dx, dw = out[torch.float64]
    dw0 = None
    if c.accumulate:     # at the gradient's own scale: a reduce that overwrites or adds twice moves the result by its size
        dw0 = torch.randn(w.shape, generator=g) * float(dw.pow(2).mean().sqrt())
        dw = dw + dw0.double()
        out[torch.float32][3] = out[torch.float32][3] + dw0
    e32 = dict(zip(("y", "dxu", "dx", "dw"), (rel_err(a, r) for a, r in zip(out[torch.float32], (y, dxu, dx, dw)))))
    return Reference(x, w, b, dy, dw0, y, dxu, dx, dw, e32)


def dw_fp32(r, c):
    """The weight gradient of a case by PyTorch's fp32 CPU operator (without the preloaded target)."""
    c = Case(*c)
    xr, wr = r.x.clone().requires_grad_(True), r.w.clone().requires_grad_(True)
    _conv(xr, wr, r.b, c)[1].backward(r.dy)
    return wr.grad
