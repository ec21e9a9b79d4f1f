/*
 * itcv_hip.h -- C ABI of libitcv_hip.so, the MI355X (gfx950) hot path of the Soft-Intro
 * beta-TC-VAE training step.
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream (as void*); no
 * torch / C++ types cross this boundary.  All tensors are fp32, dense, NCHW.  Entry points
 * return 0 on success and a non-zero code on error; itcv_last_error() returns the message
 * of the last failure on the calling thread.  Nothing here allocates: scratch memory is
 * passed in by the caller ("ws"), with the size given by the matching *_workspace() query.
 * All launches are asynchronous on `stream`; nothing synchronises the device.
 *
 * The reference (meffmadd/intro-tc-vae) is pure Python/PyTorch, so there is no FFI layer to
 * mirror; each entry point below names the reference call site (file:line under
 * /root/reference) whose ATen work it replaces.  The Python mirror of the reference's
 * module surface (models.py / ops.py / solvers) binds these with ctypes
 * (intro-tc-vae_amd/hipvae/abi.py); see INTEGRATION.md.
 */
#ifndef ITCV_HIP_H
#define ITCV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITCV_ABI_VERSION 4

/* ---- library ------------------------------------------------------------------------- */
int itcv_abi_version(void);
const char* itcv_last_error(void);
/* Launch-shape options (process-wide; the library reads NO environment variable).  Every option and value is part of
 * the test matrix: results are bit-identical for any band_persist_blocks, and equal to rounding for band_m16.
 *   "band_m16"             1 (default): v_mfma_f32_16x16x32_bf16 in the band / 128-pixel planes kernels; 0: 32x32x16
 *   "band_persist_blocks"  256 (default): blocks of the persistent band kernel (used when a launch has more tiles);
 *                          0: one tile per block; range 0..1024
 *   "wgrad_m16"            1 (default): v_mfma_f32_16x16x32 in itcv_conv2d_wgrad_bf16p; 0: 32x32x16 (equal to rounding)
 *   "planes_mfma_waves"    8 (default) or 4: MFMA waves of the 128 x 128 tile of the 128-pixel planes kernel (bit-identical)
 *   "sw_lds_rows"          0 (default: 4096): rows of itcv_sw_kl_fwd whose sort keys sit in LDS, above that in the workspace;
 *                          range 0..4096 (bit-identical: a test option that forces the workspace path at any Bt)
 *   "sw_max_blocks"        0 (default: 256): the grid cap of itcv_sw_kl_fwd's first launch; range 0..1024 (bit-identical)
 *   "stream_nt"            ITCV_STREAM_NT_DEFAULT (default): mask of ITCV_STREAM_NT_* bits below, one per kernel family; a set
 *                          bit makes the family's once-used streams non-temporal loads / stores (bit-identical: a cache
 *                          policy changes no value).  Any value >= 0 is taken; bits outside ITCV_STREAM_NT_ALL are dropped
 *                          (itcv_get_option reads back the kept bits).
 * itcv_set_option returns non-zero for an unknown name or a value out of range; itcv_get_option returns -1 for an unknown name. */
#define ITCV_STREAM_NT_BN_APPLY 0x1    /* x, dy, skip loads of the BatchNorm backward apply pass (last use) */
#define ITCV_STREAM_NT_WGRAD_SLABS 0x2 /* fp32 slab stores of a deferred planes weight gradient (read by the fold, far later) */
#define ITCV_STREAM_NT_FOLD 0x4        /* slab loads of the deferred weight-gradient fold, itcv_wgrad_reduce_many (last use) */
#define ITCV_STREAM_NT_WGRAD_OPS 0x8   /* reserved: operand loads of the weight gradient; no kernel reads this bit */
#define ITCV_STREAM_NT_OPTIM 0x10      /* reserved: optimiser streams; measured, no gain, no kernel reads this bit */
#define ITCV_STREAM_NT_BN_FWD 0x20     /* conv-output loads of the BatchNorm forward apply pass (next read: the backward) */
#define ITCV_STREAM_NT_ALL (ITCV_STREAM_NT_BN_APPLY | ITCV_STREAM_NT_WGRAD_SLABS | ITCV_STREAM_NT_FOLD | ITCV_STREAM_NT_WGRAD_OPS | ITCV_STREAM_NT_OPTIM | ITCV_STREAM_NT_BN_FWD)
#define ITCV_STREAM_NT_DEFAULT (ITCV_STREAM_NT_BN_APPLY | ITCV_STREAM_NT_WGRAD_SLABS | ITCV_STREAM_NT_FOLD | ITCV_STREAM_NT_BN_FWD)
int itcv_set_option(const char* name, int value);
int itcv_get_option(const char* name);

/* Optional per-launch timing of the GEMM-class kernels (bench.py's roofline leg): between _begin and
 * _end every conv entry point records a HIP event pair on its launch stream around its MAIN kernel
 * (not the split-K reduce).  _end waits for the events and returns the record count; record i is
 * (code = kind | KS<<4 | BM<<8 | up2<<16 | NS<<20 with kind 0 fwd fp32, 1 fwd split-bf16, 2 wgrad fp32,
 * 3 wgrad split-bf16, 4 small-Cout direct, 5 small-Cin direct, 6 fwd on planes, 7 wgrad on planes, 8 / 9 band-form fwd on planes (one tile / persistent) -- for 7..9 the KS field
 * holds log2(W) -- 10 small-Cout on planes, 11 small-Cin on the matrix cores, 12 5x5 weight gradient on planes (BM field = narrow side's channels);
 * algorithmic FLOP; elapsed ms). */
int itcv_profile_begin(void);
int itcv_profile_end(void);
int itcv_profile_get(int i, int* code, double* flop, float* ms);
int itcv_profile_clear(void);

/* ---- convolution / linear: implicit GEMM on v_mfma_f32_32x32x2_f32 -------------------
 * Stride 1, square odd kernel KS in {1,3,5}, zero padding KS/2 ("same"), groups 1.
 * Replaces nn.Conv2d / nn.Linear forward+backward: models.py:28-47 (3x3 blocks), :213
 * (5x5 stem), :290 (5x5 predict, with bias), :233 / :270 (Linear == KS 1, H=W=1).
 *
 * Weights are consumed in a packed, zero-padded, K-major layout wp[KS*KS*Cp][Mp] with the
 * reduction index ordered TAP-MAJOR, k = tap*Cp + c (Cp = reduction channels rounded up to 16,
 * Mp = M rounded up to the 32/64/128-row tile the kernel picks for M):
 *   for_dgrad = 0:  M = Co, c = ci:  wp[tap*Cp + ci][co] = w[co][ci][tap]
 *   for_dgrad = 1:  M = Ci, c = co:  wp[tap*Cp + co][ci] = w[co][ci][KK-1-tap]
 * so that the data-gradient is the same kernel run on dy with the roles of Ci/Co swapped. */
size_t itcv_conv2d_packed_weight_elems(int Co, int Ci, int KS, int for_dgrad);
int itcv_conv2d_pack_weight(const float* w, float* wp, int Co, int Ci, int KS, int for_dgrad,
                            void* stream);
/* y[B][Co][H][W] = conv(x[B][Ci][H][W], w) (+ bias[Co] if non-NULL).  `up2` != 0 reads x as the
 * nearest-neighbour x2 upsampling of a [B][Ci][H/2][W/2] tensor (models.py:284-286 fused into the
 * consumer). */
size_t itcv_conv2d_fwd_workspace(int B, int Ci, int H, int W, int Co, int KS);
int itcv_conv2d_fwd(const float* x, const float* wp, const float* bias, float* y, int B, int Ci,
                    int H, int W, int Co, int KS, int up2, void* ws, size_t ws_bytes, void* stream);
/* Split-bf16 throughput variant of itcv_conv2d_fwd (forward and data-gradient): every fp32 operand
 * is split into ns bf16 planes and the product is accumulated in fp32 on v_mfma_f32_32x32x16_bf16:
 * ns = 2 ("bf16x3", 3 MFMAs per product, ~2^-16 relative per product), ns = 3 ("bf16x6", 6 MFMAs,
 * fp32-class ~2^-23).  Supported for KS in {1,3}, Ci a multiple of 32, Co > 32 (see _supported);
 * weights come pre-split from itcv_conv2d_pack_weight_bf16s. */
int itcv_conv2d_bf16s_supported(int Ci, int Co, int KS);
size_t itcv_conv2d_packed_weight_bytes_bf16s(int Co, int Ci, int KS, int for_dgrad, int ns);
int itcv_conv2d_pack_weight_bf16s(const float* w, void* wp, int Co, int Ci, int KS, int for_dgrad, int ns,
                                  void* stream);
/* The same packing for many layers in ONE launch (the conv weights of a network after its optimiser step,
 * solvers/intro.py:116,160, solvers/vae.py:109-110): the caller fills a host array of n descriptors of itcv_pack_desc_bytes() each with
 * itcv_conv2d_pack_desc_bf16s (returns the number of blocks the layer adds, or a negative error; block0 = the running
 * sum of those), copies it to the device once and launches itcv_conv2d_pack_weights_bf16s with the total. */
size_t itcv_pack_desc_bytes(void);
int itcv_conv2d_pack_desc_bf16s(void* host_desc, const float* w, void* wp, int Co, int Ci, int KS, int for_dgrad,
                                int ns, int block0);
int itcv_conv2d_pack_weights_bf16s(const void* dev_table, int n, int total_blocks, int ns, void* stream);
size_t itcv_conv2d_fwd_bf16s_workspace(int B, int Ci, int H, int W, int Co, int KS);
int itcv_conv2d_fwd_bf16s(const float* x, const void* wp, const float* bias, float* y, int B, int Ci, int H,
                          int W, int Co, int KS, int up2, int ns, void* ws, size_t ws_bytes, void* stream);
/* Pre-split operand ("planes"): planes[p][b][c/8][h][w] = one 16-byte chunk of 8 bf16 = plane p of
 * channels c..c+7 of one pixel (C % 8 == 0; p < ns).  A producing pass (itcv_split_planes, or the
 * BatchNorm apply / backward kernels through their `planes` argument) writes it next to the fp32
 * tensor; itcv_conv2d_fwd_bf16p then moves both operands global -> LDS by LDS-DMA (no gather, no
 * conversion in the conv kernel).  Same contract and shapes (its own workspace query) and -- bit for bit -- results as
 * itcv_conv2d_fwd_bf16s (replaces the same ATen conv forward / data-gradient, models.py:28-47). */
/* Plane formats (the `ns` argument of every planes entry point):
 *   2  two bf16 planes  ("bf16x3": 3 products, ~2^-16 per product)
 *   3  three bf16 planes ("bf16x6": 6 products, fp32 class)
 *   4  ITCV_PLANES_F16X2: two FP16 planes hi = fp16(S x), lo = fp16(S x - hi) of the tensor times a power-of-two scale S
 *      ("f16x3": the same 3 products on v_mfma_f32_*_f16 carry 22 significand bits, ~2^-21 per product -- fp32 class at the
 *      bf16x3 rate).  The record {S, 1/S} (16 bytes) sits behind the second plane; producers write it, consumers multiply
 *      their result by the exact inverse.  Activations use S = 1 (O(1) values; |x| >= 65504 becomes inf and surfaces as a
 *      NaN loss); packed weights S = 2^8; gradient tensors a scale derived from a rigorous bound of their magnitude
 *      (BatchNorm backward: from per-channel maxima it computes anyway; itcv_absmax for loose fp32 tensors). */
#define ITCV_PLANES_F16X2 4
size_t itcv_planes_bytes(int B, int C, int HW, int ns);
int itcv_split_planes(const float* x, void* planes, int B, int C, int HW, int ns, void* stream);
/* parts[256] = block maxima of |x| (x 16-byte aligned); feeds the `amax` arguments below, which derive the power-of-two
 * scale of an fp16 split from them on the device (no host round trip).  amax == NULL means S = 1. */
int itcv_absmax(const float* x, size_t n, float* parts, void* stream);
int itcv_split_planes_scaled(const float* x, void* planes, int B, int C, int HW, int ns, const float* amax, void* stream);
size_t itcv_conv2d_fwd_bf16p_workspace(int B, int Ci, int H, int W, int Co, int KS, int ns);
int itcv_conv2d_fwd_bf16p(const void* xplanes, const void* wp, const float* bias, float* y, int B, int Ci, int H,
                          int W, int Co, int KS, int up2, int ns, void* ws, size_t ws_bytes, void* stream);
/* The same with the BatchNorm statistics of the consumer layer (models.py:37: conv -> BatchNorm) fused into the conv
 * epilogue: tile_stats[(k*Co + c)*T + t], k = 0: sum, k = 1: sum of squares of output channel c over the t-th tile of
 * 256 consecutive (image, pixel) positions, T = itcv_conv2d_fwd_bf16p_stat_tiles(...) (0 = not available for the shape:
 * pass NULL).  itcv_bn_train_fwd folds them (fp64) instead of reading the tensor once more. */
int itcv_conv2d_fwd_bf16p_stat_tiles(int B, int Ci, int H, int W, int Co, int KS, int ns);
int itcv_conv2d_fwd_bf16p_st(const void* xplanes, const void* wp, const float* bias, float* y, int B, int Ci, int H,
                             int W, int Co, int KS, int up2, int ns, float* tile_stats, void* ws, size_t ws_bytes,
                             void* stream);
/* itcv_conv2d_fwd_bf16p on the images [b0, b0 + nb) of the B-image tensors xplanes / y (both given WHOLE): the planes are
 * read at the whole tensor's plane stride and scale record, y is written in that image range only, and every written
 * value is bit for bit the one the full call writes -- tile shape, MFMA form and K split are planned for B, not nb.
 * Workspace: that of the full call.  Used for the data gradient of a batch of which only some images carry a gradient. */
int itcv_conv2d_fwd_bf16p_sub(const void* xplanes, const void* wp, const float* bias, float* y, int B, int Ci, int H,
                              int W, int Co, int KS, int up2, int ns, int b0, int nb, void* ws, size_t ws_bytes,
                              void* stream);
/* Data gradient of a conv that read its input through the nearest x2 upsample, with the upsample's adjoint folded into the
 * store: dx_lo[B][Co][H/2][W/2] = itcv_upsample2_bwd(itcv_conv2d_fwd_bf16p_sub(xplanes, wp, NULL, ..., up2 = 0, ...)), bit
 * for bit, without the H x W tensor in between.  xplanes: the planes of dy, [.][B][Ci/8][H][W]; wp: the data-gradient
 * packing of the weight; H, W: the high resolution; images [b0, b0 + nb) only (whole batch: 0, B), planned for B.
 * The band kernels' two-plane launches without a K split have this form: _supported answers 1 only where the plan of
 * the two-call path is a band launch (W 16..64) with splits == 1 whose kernel form exists (16x16x32 products: fp16 planes,
 * or bf16 planes with "band_m16" = 1) and H, W are even.  Host arithmetic only.  The entry point refuses any other
 * shape; ws / ws_bytes are not used (no slabs) and may be NULL / 0. */
int itcv_conv2d_dgrad_up2_supported(int B, int Ci, int H, int W, int Co, int KS, int fmt, int nb);
int itcv_conv2d_dgrad_up2_bf16p(const void* xplanes, const void* wp, float* dx_lo, int B, int Ci, int H, int W, int Co,
                                int KS, int fmt, int b0, int nb, void* ws, size_t ws_bytes, void* stream);
/* Weight gradient from the same planes (x: [2][B][Ci/8][Hs][Ws], dy: [2][B][Co/8][H][W]); the pixel
 * reduction runs through the gfx950 transposing LDS read, so no pixel-major copy is needed.  bf16x3
 * only; KS = 3, W a power of two in 4..64, H a power of two, B*H*W % 64 == 0 (see _supported).  Replaces
 * the ATen conv weight-gradient (backward of models.py:28-47).  Deterministic split-K (fp32 slabs). */
int itcv_conv2d_wgrad_bf16p_supported(int B, int Ci, int H, int W, int Co, int KS);
size_t itcv_conv2d_wgrad_bf16p_workspace(int B, int Ci, int H, int W, int Co, int KS);
int itcv_conv2d_wgrad_bf16p(const void* xplanes, const void* dyplanes, float* dw, int B, int Ci, int H, int W,
                            int Co, int KS, int up2, int ns /* 2 or 4 */, int accumulate, void* ws, size_t ws_bytes,
                            void* stream);
/* accumulate == 2 DEFERS the slab reduce of itcv_conv2d_wgrad_bf16p: the call leaves its itcv_conv2d_wgrad_bf16p_slabs(...)
 * fp32 slabs in `ws` (which must then stay alive), and ONE itcv_wgrad_reduce_many launch folds the slabs of many layers
 * into their dw (a whole backward pass: solvers/intro.py:109-116).  The caller fills a host array of n descriptors of
 * itcv_wgrad_reduce_desc_bytes() each (returns the blocks the layer adds, < 0 on error; block0 = their running sum; up to
 * four slab sources per dw, folded in the given order: a weight used by several passes of the backward), copies it to the
 * device and launches with the total.  Results are bitwise those of the per-call reduces. */
int itcv_conv2d_wgrad_bf16p_slabs(int B, int Ci, int H, int W, int Co, int KS);
size_t itcv_wgrad_reduce_desc_bytes(void);
int itcv_wgrad_reduce_desc(void* host_desc, const float* const* slabs, const int* splits, int nsrc, float* dw, int Co,
                           int Ci, int accumulate, int block0);
int itcv_wgrad_reduce_many(const void* dev_table, int n, int total_blocks, void* stream);
int itcv_wgrad_reduce_max_descs(void);   /* descriptors one table (one launch) may hold */
/* nn.Linear(K -> N) at batch B (models.py:233,270) as skinny exact-fp32 MFMA GEMMs, in every conv-math mode:
 * y[B][N] = x[B][K] w[N][K]^T + bias;  dx[B][K] = dy[B][N] w;  dw[N][K] (+)= dy^T x.  Deterministic
 * split-K; itcv_linear_workspace serves all three. */
size_t itcv_linear_workspace(int B, int K, int N);
int itcv_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, void* ws,
                    size_t ws_bytes, void* stream);
int itcv_linear_dgrad(const float* dy, const float* w, float* dx, int B, int K, int N, void* ws, size_t ws_bytes,
                      void* stream);
int itcv_linear_wgrad(const float* dy, const float* x, float* dw, int B, int K, int N, int accumulate, void* ws,
                      size_t ws_bytes, void* stream);
/* The hidden layers of the FactorVAE discriminator: the same GEMMs (same arithmetic, same plan, same deterministic
 * split-K, itcv_linear_workspace) with LeakyReLU(slope) in the epilogue of the GEMM or, under split-K, of its slab
 * reduce: no pointwise launch and no pre-activation in memory.
 *   _lrelu_fwd  : y[B][N] = lrelu(x[B][K] w[N][K]^T + bias)          x has row stride ldx >= K, bias may be NULL
 *   _dgrad_lrelu: dx[B][K] = (dy[B][N] w[N][K]) o lrelu'(y_prev[B][K])  dy / y_prev have row strides lddy >= N, ldy >= K
 * y_prev is the OUTPUT of the activation whose input gradient is wanted: y_prev > 0 <=> its input > 0 for slope > 0, and
 * an element that is exactly zero takes the derivative `slope`, as torch's leaky_relu does.  w, y and dx are dense.
 * Refused before any launch: a NULL x / dy / w / y / dx / y_prev, B, K or N < 1, a row stride below the row length,
 * slope <= 0 or not finite, a workspace that is too small. */
int itcv_linear_lrelu_fwd(const float* x, size_t ldx, const float* w, const float* bias, float* y, int B, int K, int N,
                          float slope, void* ws, size_t ws_bytes, void* stream);
int itcv_linear_dgrad_lrelu(const float* dy, size_t lddy, const float* w, const float* y_prev, size_t ldy, float* dx,
                            int B, int K, int N, float slope, void* ws, size_t ws_bytes, void* stream);
/* 5x5 weight gradients with a <= 3-channel side (stem 3 -> 64: stem = 1, small = x, big_planes = planes of dy;
 * predict 64 -> 3: stem = 0, small = dy, big_planes = planes of x), bf16x3 on the matrix cores: rows (small channel,
 * filter column), pixel reduction through the transposing LDS read.  W in {32, 64}.  Deterministic slab reduce. */
int itcv_conv2d_wgrad5_bf16p_supported(int Cs, int Cb, int H, int W);
size_t itcv_conv2d_wgrad5_bf16p_workspace(int B, int H);
int itcv_conv2d_wgrad5_bf16p(const float* small, const void* big_planes, float* dw, int B, int Cs, int H, int W,
                             int stem, int ns /* 2 or 4 */, const float* small_amax /* itcv_absmax of `small`, or NULL */,
                             int accumulate, void* ws, size_t ws_bytes, void* stream);
/* Direct (vector-ALU, exact fp32) convolution for layers with at most 4 output channels -- the 5x5
 * predict conv 64->3 (models.py:290) and the data-gradient of the 5x5 stem (models.py:213), where a
 * 32-row MFMA tile would be >90 % padding.  for_dgrad = 0: w is [Co][C][KS][KS]; for_dgrad = 1: w is the
 * forward layer's [C][Co][KS][KS] and its transposed, flipped filter is applied to x = dy. */
int itcv_conv2d_small_cout_supported(int Co, int KS);
/* The same layer on the bf16 matrix cores (bf16x3) from pre-split planes of a 64-channel input: MFMA rows are
 * (output channel, filter column), every operand fragment is one plane chunk loaded straight from global memory. */
int itcv_conv2d_small_cout_bf16p_supported(int C, int Co, int KS);
int itcv_conv2d_small_cout_fwd_bf16p(const void* xplanes, const float* w, const float* bias, float* y, int B, int C,
                                     int H, int W, int Co, int KS, int for_dgrad, int ns /* 2 or 4 */, void* stream);
int itcv_conv2d_small_cout_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C,
                               int H, int W, int Co, int KS, int for_dgrad, void* stream);
/* ... and for layers with at most 4 REDUCTION channels (the 5x5 stem 3->64 forward, models.py:213, and
 * the data-gradient of the predict conv): the pixel's input window lives in registers. */
int itcv_conv2d_small_cin_supported(int C, int KS);
int itcv_conv2d_small_cin_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int H,
                              int W, int Co, int KS, int for_dgrad, void* stream);

/* The same conv for C <= 3, Co == 64, KS == 5, W % 32 == 0 (the stem layer models.py:199-204 and the data-gradient of
 * the prediction layer models.py:271) as split-bf16 (bf16x3) products on the matrix cores. */
int itcv_conv2d_small_cin_bf16x3_supported(int C, int Co, int KS, int W);
int itcv_conv2d_small_cin_fwd_bf16x3(const float* x, const float* w, const float* bias, float* y, int B, int C, int H,
                                     int W, int Co, int KS, int for_dgrad, int ns /* 2 or 4 */,
                                     const float* x_amax /* itcv_absmax of x, or NULL */, void* stream);
/* Split-bf16 weight gradient (same arithmetic, same workspace size as itcv_conv2d_wgrad_workspace):
 * needs KS in {1,3}, Ci % 32 == 0, W % 8 == 0, Co > 32 and a materialised (not virtually upsampled) x. */
int itcv_conv2d_wgrad_bf16s_supported(int Ci, int H, int W, int Co, int KS);
int itcv_conv2d_wgrad_bf16s(const float* x, const float* dy, float* dw, int B, int Ci, int H, int W, int Co,
                            int KS, int ns, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dw[Co][Ci][KS][KS] (+)= sum_{b,h,w} dy[b][co][h][w] * x[b][ci][h+kh-p][w+kw-p]; `up2` as in _fwd
 * (x is the low-resolution [B][Ci][H/2][W/2] tensor, H/W are the dims of dy). */
size_t itcv_conv2d_wgrad_workspace(int B, int Ci, int H, int W, int Co, int KS);
int itcv_conv2d_wgrad(const float* x, const float* dy, float* dw, int B, int Ci, int H, int W,
                      int Co, int KS, int up2, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* Kernel instantiation a call resolves to, for profiling buckets: bits 0-7 block rows BM,
 * 8-15 KS, 16 up2, 20-31 split-K factor. */
int itcv_conv2d_fwd_variant(int B, int Ci, int H, int W, int Co, int KS, int up2);
int itcv_conv2d_wgrad_variant(int B, int Ci, int H, int W, int Co, int KS, int up2);
/* db[C] (+)= sum_{b,hw} dy[b][c][hw]  (bias gradients: models.py:290 predict, :233/:270 Linear) */
size_t itcv_bias_grad_workspace(int B, int C, int HW);
int itcv_bias_grad(const float* dy, float* db, int B, int C, int HW, int accumulate, void* ws,
                   size_t ws_bytes, void* stream);

/* ---- BatchNorm2d (+ LeakyReLU, + AvgPool2d(2)) ---------------------------------------
 * Replaces nn.BatchNorm2d(eps) -> nn.LeakyReLU(0.2) [-> nn.AvgPool2d(2)]: models.py:37-38,48-49,
 * 214-216,225.  Train-mode statistics are computed in fp64 from per-channel (sum, sum of
 * squares); the moments are exposed so that a data-parallel caller can all-reduce them
 * (Sync-BN) between _moments and _finalize. */
size_t itcv_bn_workspace(int B, int C, int HW);
/* sums[0..C) = sum x, sums[C..2C) = sum x^2 over (b,hw); deterministic two-stage reduction */
int itcv_bn_moments(const float* x, double* sums, int B, int C, int HW, void* ws, size_t ws_bytes,
                    void* stream);
/* single-rank fast path: moments + finalize of this rank's own batch in two launches */
int itcv_bn_train_stats(const float* x, int B, int C, int HW, float eps, float momentum, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, void* ws,
                        size_t ws_bytes, void* stream);
/* mean/rstd from the moments of `count` samples; updates running_mean/var (momentum, unbiased
 * variance) and num_batches_tracked when those pointers are non-NULL. */
int itcv_bn_finalize(const double* sums, double count, float eps, float momentum, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, int C,
                     void* stream);
/* The same, also writing the unbiased variance that running_var was blended with to unbiased_var [C] (may be NULL;
 * written only when running_var is given): see itcv_bn_replay_many. */
int itcv_bn_finalize_uv(const double* sums, double count, float eps, float momentum, float* running_mean,
                        float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd, float* unbiased_var,
                        int C, void* stream);
/* eval mode: mean = running_mean, rstd = 1/sqrt(running_var + eps) */
int itcv_bn_eval_stats(const float* running_mean, const float* running_var, float eps, float* mean,
                       float* rstd, int C, void* stream);
/* y = pool(lrelu(gamma*(x-mean)*rstd + beta, slope)); slope = 1 disables the activation; pool in
 * {0: none (y [B][C][H][W]), 1: 2x2 average (y [B][C][H/2][W/2])}.  If `skip` is non-NULL it is
 * added before the activation (ResidualBlock, models.py:113-114). */
int itcv_bn_act_fwd(const float* x, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, const float* skip, float* y, int B, int C, int H, int W,
                    float slope, int pool, void* planes, int ns, size_t plane_stride, void* stream);
/* `plane_stride` (16-byte chunks; also in itcv_bn_act_bwd_apply / itcv_bn_train_fwd / itcv_bn_train_bwd): distance
 * between consecutive planes of `planes` / `dx_planes`.  0 = B*(C/8)*Ho*Wo, i.e. the call covers the whole tensor.
 * Non-zero: x / y / planes point at ONE BatchNorm GROUP of a larger batched tensor -- the solvers push several
 * independent network passes (each a BatchNorm batch of its own, models.py:37) through the conv GEMMs as one batch,
 * and normalise every group with its own call: statistics, running-buffer updates and their order stay those of
 * separate passes.
 * `planes` (may be NULL): the same launch also writes the output as pre-split bf16 planes
 * [ns][B][C/8][Ho][Wo] for the consumer conv (itcv_conv2d_fwd_bf16p / _wgrad_bf16p); needs
 * itcv_bn_act_planes_supported(C, H, W, pool).  The fp32 output is bitwise unchanged; with planes given,
 * `y` may be NULL (fp32 output not written: the consumer GEMMs read only the planes).  The same holds
 * for `dx_planes` / `dx` of itcv_bn_act_bwd_apply (planes of dx, pool = 0 in the support query). */
int itcv_bn_act_planes_supported(int C, int H, int W, int pool);
/* backward, stage 1: dsums[0..C) = sum g, dsums[C..2C) = sum g*xhat where
 * g = unpool(dy) * lrelu'(bn_out (+skip)); `up2`!=0 means dy is the gradient of the x2-upsampled
 * output (dy [B][C][2H][2W], summed 2x2 on the fly: adjoint of models.py:284-286).  When non-NULL,
 * dgamma (+)= dsums[C+c] and dbeta (+)= dsums[c] are written by the same launch (the rank's own
 * sums are the parameter gradients, also under Sync-BN). */
int itcv_bn_act_bwd_reduce(const float* x, const float* dy, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, const float* skip, double* dsums,
                           float* dgamma, float* dbeta, int accumulate, int B, int C, int H, int W,
                           float slope, int pool, int up2, void* ws, size_t ws_bytes, void* stream);
/* backward, stage 2: dx = gamma*rstd*(g - dsums[c]/count - xhat*dsums[C+c]/count);
 * dgamma (+)= local_dsums[C+c], dbeta (+)= local_dsums[c] when non-NULL (local_dsums = the rank's
 * own sums; dsums may have been all-reduced for Sync-BN); dskip = g when non-NULL. */
int itcv_bn_act_bwd_apply(const float* x, const float* dy, const float* mean, const float* rstd,
                          const float* gamma, const float* beta, const float* skip, const double* dsums,
                          const double* local_dsums, double count, float* dx, float* dskip,
                          float* dgamma, float* dbeta, int accumulate, int B, int C, int H, int W,
                          float slope, int pool, int up2, void* dx_planes, int ns, size_t plane_stride, void* stream);

/* Single-rank training forms: itcv_bn_train_fwd == itcv_bn_train_stats + itcv_bn_act_fwd and
 * itcv_bn_train_bwd == itcv_bn_act_bwd_reduce + itcv_bn_act_bwd_apply (count = B*H*W), same arguments and results;
 * where the planes kernels apply and the reduction is sliced, the apply launch folds the slices itself (two
 * launches per layer instead of three).  Workspace: itcv_bn_workspace. */
int itcv_bn_train_fwd(const float* x, const float* gamma, const float* beta, const float* skip, float* y, void* planes,
                      int ns, int B, int C, int H, int W, float slope, int pool, float eps, float momentum,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd,
                      void* ws, size_t ws_bytes, size_t plane_stride, const float* tile_stats, int tiles, int tile_pitch,
                      int groups, void* stream);
/* itcv_bn_train_fwd_uv == itcv_bn_train_fwd, also leaving in unbiased_var [groups][C] (may be NULL; written only when
 * running_var is given) the float every group blended into running_var.  With mean [groups][C] these are the values a
 * later replay of the running-buffer update needs (itcv_bn_replay_many); rstd does not give the second back bit for bit. */
int itcv_bn_train_fwd_uv(const float* x, const float* gamma, const float* beta, const float* skip, float* y, void* planes,
                         int ns, int B, int C, int H, int W, float slope, int pool, float eps, float momentum,
                         float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* rstd,
                         float* unbiased_var, void* ws, size_t ws_bytes, size_t plane_stride, const float* tile_stats,
                         int tiles, int tile_pitch, int groups, void* stream);
/* Replay of running-buffer updates: when a network pass is reused instead of recomputed (same weights, same input, batch
 * statistics: solvers/intro.py:119-120 repeats :70,75), every BatchNorm layer still owes the update the repeated pass
 * would have made, at that point of the stream.  ONE launch for all layers: the caller fills a host array of n
 * descriptors of itcv_bn_replay_desc_bytes() each (returns the blocks the layer adds, 0 when all three buffers are NULL
 * -- leave such a layer out -- and < 0 on error; block0 = their running sum), copies it to the device and launches with
 * the total.  Per channel, group by group in order: running = (1 - momentum) * running + momentum * saved, the
 * expression of the forward; num_batches_tracked += groups.  Bitwise the buffers the repeated forward would leave.  The
 * device table must stay alive as long as a captured graph may replay the launch. */
size_t itcv_bn_replay_desc_bytes(void);
int itcv_bn_replay_desc(void* host_desc, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                        const float* mean, const float* unbiased_var, int C, int groups, float momentum, int block0);
int itcv_bn_replay_many(const void* dev_table, int n, int total_blocks, void* stream);
int itcv_bn_replay_max_descs(void);   /* descriptors one table (one launch) may hold */
/* groups > 1 (itcv_bn_train_fwd / _bwd): x / y / planes (dy / dx / dx_planes) hold `groups` BatchNorm groups of B images
 * each, stacked along the batch dimension; mean / rstd are [groups][C], dsums [groups][2C]; plane_stride is that of the
 * whole tensor.  Every group is normalised with its own statistics and advances the running buffers on its own, in
 * order; small layers do it in one statistics launch + one apply launch for all groups. */
/* tile_stats (may be NULL): per-tile sums of x written by the producing conv (itcv_conv2d_fwd_bf16p_st):
 * sum at tile_stats[c*tile_pitch + t], sum of squares at tile_stats[(C + c)*tile_pitch + t], t < tiles -- the tiles
 * that make up THIS call's B images; the statistics are then folded from them and x is read once (apply) only. */
int itcv_bn_train_bwd(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, const float* skip, double* dsums, float* dx, float* dskip, void* dx_planes,
                      int ns, float* dgamma, float* dbeta, int accumulate, int B, int C, int H, int W, float slope,
                      int pool, int up2, void* ws, size_t ws_bytes, size_t plane_stride, int groups, void* stream);
/* itcv_bn_train_bwd for a dy that is exactly zero outside the groups [live0, live0 + nlive) (the caller's guarantee; a
 * batched pass of which one half only feeds constants).  Live groups: launches, arithmetic and results of the full call on
 * every path of itcv_bn_plan_query.  Dead groups: dy and skip are not read, dx / dskip / dx_planes are not written, their
 * dsums are 0 and the parameter gradients receive nothing from them.  fp16 planes: the reduce pass still reads a dead
 * group's x for max|xhat|, so the scale record -- one per tensor, where the whole tensor's planes put it -- and the live
 * groups' chunks are bit for bit those of the full call.  live0 = 0, nlive = groups is itcv_bn_train_bwd. */
int itcv_bn_train_bwd_live(const float* x, const float* dy, const float* mean, const float* rstd, const float* gamma,
                           const float* beta, const float* skip, double* dsums, float* dx, float* dskip, void* dx_planes,
                           int ns, float* dgamma, float* dbeta, int accumulate, int B, int C, int H, int W, float slope,
                           int pool, int up2, void* ws, size_t ws_bytes, size_t plane_stride, int groups, int live0,
                           int nlive, void* stream);

/* Which launches a BatchNorm training call gets.  Pure host arithmetic (no launch, no device): the decision
 * itcv_bn_train_fwd (bwd = 0) / itcv_bn_train_bwd (bwd = 1) make for one group of (B, C, H, W), `planes` != 0 when
 * planes are requested in format `ns`, `ws_bytes` the workspace handed in, `tile_stats` != 0 when the conv epilogue's
 * tile sums are given.  *path receives one of ITCV_BN_PATH_*, *splits the slices per channel of the reduction (either
 * may be NULL).  Tests pin the path of every shape they run; returns non-zero for non-positive dimensions. */
#define ITCV_BN_PATH_ONE_BLOCK 0      /* one block per channel reduces and finalises (all groups, in order); planes apply */
#define ITCV_BN_PATH_SLICED_FOLD 1    /* sliced reduce; the planes apply launch folds the slices itself */
#define ITCV_BN_PATH_SLICED_COMBINE 2 /* sliced reduce, a combine launch, planes apply (fewer than 64 threads a plane) */
#define ITCV_BN_PATH_FALLBACK 3       /* no planes, or a shape the planes kernels do not take: plain apply kernels */
#define ITCV_BN_PATH_PER_GROUP 4      /* groups > 1 that cannot go out as one launch: one call per group */
#define ITCV_BN_PATH_TILE_STATS 5     /* forward: statistics from the producing conv's tile sums, then the apply pass */
int itcv_bn_plan_query(int bwd, int B, int C, int H, int W, int pool, int up2, int groups, int planes, int ns,
                       size_t ws_bytes, int tile_stats, int* path, int* splits);

/* ---- pointwise / resampling ----------------------------------------------------------- */
int itcv_lrelu_fwd(const float* x, float* y, size_t n, float slope, void* stream);     /* models.py:271 */
int itcv_lrelu_bwd(const float* x, const float* dy, float* dx, size_t n, float slope, void* stream);
int itcv_sigmoid_fwd(const float* x, float* y, size_t n, void* stream);                /* models.py:291 */
int itcv_sigmoid_bwd(const float* y, const float* dy, float* dx, size_t n, void* stream);
int itcv_avgpool2_fwd(const float* x, float* y, int BC, int H, int W, void* stream);   /* models.py:216,225 */
int itcv_avgpool2_bwd(const float* dy, float* dx, int BC, int H, int W, void* stream);
int itcv_upsample2_fwd(const float* x, float* y, int BC, int H, int W, void* stream);  /* models.py:284 */
int itcv_upsample2_bwd(const float* dy, float* dx, int BC, int H, int W, void* stream);
int itcv_add(const float* a, const float* b, float* out, size_t n, void* stream);      /* models.py:114,182 */

/* ---- latent math (ops.py) ------------------------------------------------------------- */
/* ops.py:166-185  z = mu + eps*exp(0.5*logvar) */
int itcv_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z, size_t n,
                     void* stream);
int itcv_reparam_bwd(const float* dz, const float* logvar, const float* eps, float* dmu, float* dlogvar,
                     size_t n, void* stream);
/* ops.py:161-163  kl[j] = -0.5 * sum_l (1 + lv - exp(lv) - mu^2) */
int itcv_kl_rows_fwd(const float* logvar, const float* mu, float* kl, int B, int D, void* stream);
int itcv_kl_rows_bwd(const float* g, const float* logvar, const float* mu, float* dlogvar, float* dmu,
                     int B, int D, void* stream);

/* ops.py:15-29,32-49,52-115: pairwise Gaussian log-density + minibatch stratified / weighted
 * sampling, fused; the [B,B,D] tensor is never materialised.
 *   rows j: the caller's local samples z[Bl][D] (global row index = row_offset + j)
 *   cols i: all samples' means mu_all[Bt][D] (all-gathered in data-parallel runs)
 *   logvar: [Bl][D] (rows) with ITCV_TC_VAR_FROM_ROW, else [Bt][D] (columns)
 *   flags: ITCV_TC_*   variance source, density flavour and sampler
 * Outputs: prodm[Bl] = sum_l logsumexp_i(logW[j,i] + lp[j,i,l]),
 *          logqz[Bl] = logsumexp_i(logW[j,i] + sum_l lp[j,i,l]),
 *          lse[Bl][D]      (saved per-dimension logsumexp, needed by the backward),
 *          sjoint[Bl][Bt]  (the joint terms logW[j,i] + sum_l lp[j,i,l] -- without logW for the weighted sampler --
 *                           saved for the backward, which does not recompute the forward).
 * Workspace: itcv_tc_fwd_workspace (per-chunk logsumexp partials). */
#define ITCV_TC_VAR_FROM_ROW 0x1 /* ops.py:81 logvar.unsqueeze(1): variance of sample row j (live path) */
#define ITCV_TC_EPS_DENSITY 0x2  /* ops.py:15-21 density (var clamp 1e-4, straight-through) else ops.py:24-29 */
#define ITCV_TC_WEIGHTED 0x4     /* ops.py:92-101 MWS; default ops.py:104-115 MSS */
#define ITCV_TC_LIVE (ITCV_TC_VAR_FROM_ROW | ITCV_TC_EPS_DENSITY)
size_t itcv_tc_fwd_workspace(int Bl, int Bt, int D);
int itcv_tc_fwd(const float* z, const float* mu_all, const float* logvar, float* prodm, float* logqz,
                float* lse, float* sjoint, int Bl, int Bt, int row_offset, int D, int64_t dataset_size, int flags,
                void* ws, size_t ws_bytes, void* stream);
/* gradient of sum_j g[j] * (logqz[j] - prodm[j]) for the live path (flags == ITCV_TC_LIVE):
 * dz[Bl][D], dlogvar[Bl][D] (rows) and dmu_all[Bt][D] (columns; partial over this rank's rows). */
size_t itcv_tc_bwd_workspace(int Bl, int Bt);
int itcv_tc_bwd(const float* g, const float* z, const float* mu_all, const float* logvar,
                const float* logqz, const float* lse, const float* sjoint, float* dz, float* dmu_all,
                float* dlogvar, int Bl, int Bt, int row_offset, int D, int64_t dataset_size, int flags, void* ws,
                size_t ws_bytes, void* stream);
/* The whole KL hook of the TC solvers, solvers/tc.py:69-89: (beta - 1) * total_correlation + kl_divergence with the
 * hook's reduction, fused into the estimator's launches: out[Bl] (reduction 0 none) or out[1] (1 sum, 2 mean) of
 * coef_tc * (logqz_j - prodm_j) + coef_kl * kl_j, kl_j = ops.py:161-163 on this rank's rows (mu_all + row_offset*D, logvar).
 * rows[Bl]: scratch of the reduced forms.  prodm / logqz / lse / sjoint as itcv_tc_fwd (kept for _bwd).
 * _bwd: g is [Bl] (none) or [1]; dz, dlogvar (rows) and dmu_all (columns; the KL's d/dmu added at this rank's rows). */
int itcv_tc_kl_fwd(const float* z, const float* mu_all, const float* logvar, float* out, float* rows, float* prodm,
                   float* logqz, float* lse, float* sjoint, int Bl, int Bt, int row_offset, int D, int64_t dataset_size,
                   float coef_tc, float coef_kl, int reduction, void* ws, size_t ws_bytes, void* stream);
int itcv_tc_kl_bwd(const float* g, const float* z, const float* mu_all, const float* logvar, const float* logqz,
                   const float* lse, const float* sjoint, float* dz, float* dmu_all, float* dlogvar, int Bl, int Bt,
                   int row_offset, int D, int64_t dataset_size, float coef_tc, float coef_kl, int reduction, void* ws,
                   size_t ws_bytes, void* stream);
/* The full beta-TC decomposition of solvers/tc.py:91-144 (_compute_kl_loss_full) as a trainable loss, with weights:
 *   r_j = alpha (logqcx_j - logqz_j) + beta (logqz_j - prodm_j) + gamma (prodm_j - logpz_j)   (the reference: alpha = gamma = 1)
 * with the ops.py:24-29 density (no variance floor), the variance of COMPONENT i (logvar.unsqueeze(0)) and the stratified
 * sampler (ops.py:32-49,104-115); logqcx_j / logpz_j: ops.py:24-29 at (mu_j, logvar_j) / (0, 0), summed over l.
 *   rows j: z[Bl][D] (global row row_offset + j);  cols i: mu_all / logvar_all [Bt][D] with row stride ld >= D (ld = 2D
 *   reads the two halves of one packed [Bt][2D] all-gather in place).  This rank's own means and variances are rows
 *   row_offset .. row_offset+Bl-1 of the column operands.
 * out[Bl] (reduction 0 none) or out[1] (1 sum, 2 mean) of r_j; rows[Bl]: scratch of the reduced forms; comps[3][Bl]
 * (may be NULL): the per-sample (mi, tc, dwkl).  prodm / logqz / lse / sjoint as itcv_tc_fwd; ivar[Bt][D] = exp(-logvar_all),
 * the coefficients the forward used.  Workspace: itcv_tc_full_fwd_workspace.  3 launches at most.
 * _bwd: g is [Bl] (none) or [1]; dz[Bl][D] (rows), dmu_all / dlogvar_all [Bt][D] with row stride ld (columns: the partial
 * over this rank's rows, plus the d/dmu, d/dlogvar of logqcx on this rank's own rows).  Workspace: itcv_tc_full_bwd_workspace.
 * 2 launches, fixed summation orders (bitwise reproducible). */
size_t itcv_tc_full_fwd_workspace(int Bl, int Bt, int D);
int itcv_tc_full_fwd(const float* z, const float* mu_all, const float* logvar_all, int ld, float* out, float* rows,
                     float* comps, float* prodm, float* logqz, float* lse, float* sjoint, float* ivar, int Bl, int Bt,
                     int row_offset, int D, int64_t dataset_size, float alpha, float beta, float gamma, int reduction,
                     void* ws, size_t ws_bytes, void* stream);
size_t itcv_tc_full_bwd_workspace(int Bl, int Bt);
int itcv_tc_full_bwd(const float* g, const float* z, const float* mu_all, const float* logvar_all, int ld,
                     const float* logqz, const float* lse, const float* sjoint, const float* ivar, float* dz, float* dmu_all,
                     float* dlogvar_all, int Bl, int Bt, int row_offset, int D, int64_t dataset_size, float alpha,
                     float beta, float gamma, int reduction, void* ws, size_t ws_bytes, void* stream);
/* ops.kl_divergence with its reduction and the hook's `beta *` (ops.py:136-163, solvers/vae.py:63-77) in one launch:
 * reduction 0: out[B] = scale * kl_j; 1 / 2: out[1] = scale * sum_j kl_j [/ B]; _bwd for g of that shape. */
int itcv_kl_loss_fwd(const float* logvar, const float* mu, float* out, int B, int D, int reduction, float scale, void* stream);
int itcv_kl_loss_bwd(const float* g, const float* logvar, const float* mu, float* dlogvar, float* dmu, int B, int D,
                     int reduction, float scale, void* stream);
/* The KL hook of DIP-VAE-I (kind 1) / DIP-VAE-II (kind 2) (Kumar et al. 2018; disentanglement_lib's dip_vae) with its
 * gradient (csrc/dip.hip).  mu_all / logvar_all [Bt][D] fp32 are the whole global batch, row stride ld = D, or ld = 2D for
 * the two halves of one packed [Bt][2D] all-gather read in place; this rank's rows are row_offset .. row_offset+Bl-1.
 *   m = mean_b mu_all[b], X = mu_all - m, C = X^T X / Bt (centred two-pass form, fp64; divisor Bt),
 *   kind 2: C += diag(mean_b exp(logvar_all[b]));
 *   out[0]   = coef_kl * mean_{local rows} kl_j (ops.py:161-163) + lambda_od sum_{i != j} C_ij^2 + lambda_d sum_i (C_ii - 1)^2
 *   terms[3] = {mean kl_j, the lambda_od term, the lambda_d term}
 *   W[D][D]  = 2 lambda_od offdiag(C) + diag(2 lambda_d (C_ii - 1)) (fp32, symmetric), mean[D] = m (fp64): kept for _bwd.
 * coef_kl == 0 leaves the KL out of out[0] and of the gradients whatever its value.  Workspace: itcv_dip_kl_workspace (the
 * fp64 loss partials of the 32 x 32 tiles of C).  2 launches: the tiles over a grid, then a one-block finish.
 * _bwd, ONE launch: g[1]; dmu_all / dlogvar_all [Bt][D] with row stride ld (every element written):
 *   dmu_all = g ((2 / Bt) X W + (coef_kl / Bl) mu on the local rows)
 *   dlogvar_all = g (exp(logvar_all) diag(W) / Bt [kind 2] + (coef_kl / Bl) (-1/2)(1 - exp(logvar)) on the local rows).
 * Every sum is fp64 in a fixed order, there are no atomics: results are bitwise reproducible and do not depend on the grid.
 * Refused before any launch: a NULL pointer, Bt outside 2..2^24, D outside 1..512, rows outside the global batch, another
 * kind, a negative or non-finite lambda, a non-finite coef_kl, a row stride that is neither D nor 2D. */
size_t itcv_dip_kl_workspace(int Bt, int D);
int itcv_dip_kl_fwd(const float* mu_all, const float* logvar_all, int ld, float* out, float* terms, float* W, double* mean,
                    int Bl, int Bt, int row_offset, int D, int kind, double lambda_od, double lambda_d, double coef_kl,
                    void* ws, size_t ws_bytes, void* stream);
int itcv_dip_kl_bwd(const float* g, const float* mu_all, const float* logvar_all, int ld, const float* W, const double* mean,
                    float* dmu_all, float* dlogvar_all, int Bl, int Bt, int row_offset, int D, int kind, double coef_kl,
                    void* stream);
/* The KL hook of InfoVAE / MMD-VAE (Zhao et al. 2017) and WAE-MMD (Tolstikhin et al. 2018) with its gradient
 * (csrc/mmd.hip).  z_all [Bt][D] fp32: the reparameterised samples of the whole global batch (the gradient flows to it);
 * prior [P][D] fp32: draws from N(0, I), a constant; mu / logvar [Bl][D] fp32: this rank's rows, read for the KL only.
 * All four are dense (row stride D).
 *   d2(a, b) = sum_l (a_l - b_l)^2 in fp64 from the fp32 inputs (difference form); bandwidth h > 0;
 *   kernel 1 "rbf": k = exp(-d2 / h), k' = -k / h;
 *   kernel 2 "imq": k = sum_s C_s / (C_s + d2), k' = -sum_s C_s / (C_s + d2)^2, C_s = s h, s in (.1, .2, .5, 1, 2, 5, 10);
 *   S_zz = sum_{i != j} k(d2(z_i, z_j)) / (Bt (Bt - 1)), S_pp = sum_{i != j} k(d2(p_i, p_j)) / (P (P - 1)),
 *   S_zp = sum_{i, j} k(d2(z_i, p_j)) / (Bt P), MMD^2 = S_zz + S_pp - 2 S_zp (the unbiased U-statistic; may be negative);
 *   out[0]   = coef_kl * mean_{b < Bl} kl_b (ops.py:161-163) + lambda_mmd * MMD^2
 *   terms[5] = {mean kl_b, MMD^2, S_zz, S_pp, S_zp}
 *   Wt[Bt][Bt + P] = (A | C) (fp32), A_ij = k'(d2(z_i, z_j)) 2 / (Bt (Bt - 1)) (A_ii = 0; symmetric bit for bit),
 *   C_ij = k'(d2(z_i, p_j)) (-2) / (Bt P); rs[Bt] (fp64) = the row sums of (A | C), accumulated from the fp64 values in a
 *   fixed order: both kept for _bwd.
 * coef_kl == 0 leaves the KL out of out[0] and of the gradients whatever its value.  Workspace: itcv_mmd_kl_workspace (one
 * fp64 partial per 32 x 32 tile of the pair matrix of [z_all ; prior] and one fp64 row sum per strip of 32 points and row
 * of z_all: at most 8.5 MiB).  2 launches: the upper tiles over a grid (zz upper tiles mirrored, zp in full, pp sums only),
 * then a finish whose first block folds the partials and the KL and whose other blocks fold rs.
 * _bwd, ONE launch: g[1]; every element of dz_all [Bt][D], dmu and dlogvar [Bl][D] is written:
 *   dz_all = g lambda_mmd 2 (rs o z_all - Wt [z_all ; prior]) (fp64 accumulation, fp32 store)
 *   dmu = g (coef_kl / Bl) mu, dlogvar = g (coef_kl / Bl) (-1/2)(1 - exp(logvar)).
 * Every sum is fp64 in a fixed order, there are no atomics: results are bitwise reproducible and do not depend on the grid.
 * Refused before any launch: a NULL pointer, Bt or P outside 2..4096, Bl outside 1..2^24, D outside 1..512, another
 * kernel id, h not finite or <= 0, a negative or non-finite lambda_mmd, a non-finite coef_kl, a workspace that is too
 * small.  The limits bound Wt at 4096 x 8192 x 4 bytes = 128 MiB. */
size_t itcv_mmd_kl_workspace(int Bt, int P);
int itcv_mmd_kl_fwd(const float* z_all, const float* prior, const float* mu, const float* logvar, float* out, float* terms,
                    float* Wt, double* rs, int Bl, int Bt, int P, int D, int kernel, double h, double lambda_mmd,
                    double coef_kl, void* ws, size_t ws_bytes, void* stream);
int itcv_mmd_kl_bwd(const float* g, const float* z_all, const float* prior, const float* mu, const float* logvar,
                    const float* Wt, const double* rs, float* dz_all, float* dmu, float* dlogvar, int Bl, int Bt, int P,
                    int D, double lambda_mmd, double coef_kl, void* stream);
/* The KL hook of the sliced-Wasserstein autoencoder (Kolouri et al. 2018) with its gradient, and the sliced-Wasserstein
 * distance as a score (Deshpande et al. 2018) (csrc/sw.hip).  z_all [Bt][D] fp32 with row stride ldz >= D, read in place:
 * the reparameterised samples of the whole global batch (the gradient flows to it); prior [Bt][D] fp32 with row stride
 * ldp >= D: as many draws from N(0, I), a constant; t [L][D] fp32, dense: N(0, I) draws, a constant; mu / logvar [Bl][D]
 * fp32, dense: this rank's rows, read for the KL only.
 *   theta_l = t_l / |t_l|, the norm in fp64; a row of norm 0 gives theta_l = 0;
 *   u_l[i] = sum_d theta_ld z_id, v_l[i] = sum_d theta_ld p_id in fp64 from the fp32 inputs, in an order that depends on
 *   D alone (equal rows get equal bits wherever they stand);
 *   pi_l = the ascending order of u_l, ties broken by the smaller row index (the stable sort; the order is total for any
 *   keys, +0 and -0 are one key); v_l is sorted ascending;
 *   SW_l^2 = (1 / Bt) sum_i (u_l[pi_l(i)] - v_l(i))^2, SW^2 = (1 / L) sum_l SW_l^2, both sums in index order;
 *   out[0]   = coef_kl * mean_{b < Bl} kl_b (ops.py:161-163) + lambda_sw * SW^2
 *   terms[3] = {mean kl_b, SW^2, max_l SW_l^2};  per[L] (fp64) = the SW_l^2
 *   Theta[L][D] (fp64) = the theta_l;  G[L][Bt] (fp64), G[l][pi_l(i)] = u_l[pi_l(i)] - v_l(i): the difference of every row,
 *   written to the row it came from, so that _bwd needs no permutation.  Both are kept for _bwd.  G == NULL is the
 *   forward-only form of the score: nothing of size L x Bt is written.  mu and logvar may both be NULL when coef_kl == 0:
 *   no KL is read and terms[0] = 0.
 * coef_kl == 0 leaves the KL out of out[0] and of the gradients whatever its value.  2 launches: one block per projection
 * (the grid is capped at 256 blocks; a block walks further projections by the grid stride) normalises, projects, sorts
 * (key, row) pairs with a bitonic network and folds; then a one-block finish.  The sort keys sit in LDS up to
 * Bt = itcv_sw_lds_rows() (4096 rows of 20 bytes), above that in the workspace: itcv_sw_workspace bytes, one slice of
 * Bt rows per resident block (0 when the keys sit in LDS; ws may then be NULL).  There the steps of the network that stay
 * inside an aligned chunk of 4096 rows run on the chunk staged in LDS, the steps across chunks on the workspace in place;
 * the step is one function, and the sorted sequence -- unique, (key, row) being a total order -- is the same.
 * _bwd, ONE launch: g[1]; every element of dz_all [Bt][D], dmu and dlogvar [Bl][D] (all dense) is written:
 *   dz_all = g lambda_sw (2 / (L Bt)) sum_l G[l][i] Theta[l][d] (l ascending, fp64 accumulation, fp32 store)
 *   dmu = g (coef_kl / Bl) mu, dlogvar = g (coef_kl / Bl) (-1/2)(1 - exp(logvar)).
 * There is no gradient to prior or t.  lambda_sw == 0 gives an exactly zero dz_all.
 * Every sum is fp64 in a fixed order, there are no atomics: results are bitwise reproducible and do not depend on the
 * grid or on where the keys sit.  Refused before any launch: a NULL pointer, Bt outside 1..2^20, L outside 1..4096, D
 * outside 1..2048, Bl outside 1..2^24, L * Bt above 2^26 when G is asked for, a negative or non-finite lambda_sw, a
 * non-finite coef_kl, a row stride below D, a workspace that is too small. */
int itcv_sw_lds_rows(void);
size_t itcv_sw_workspace(int Bt, int L, int D);
int itcv_sw_kl_fwd(const float* z_all, size_t ldz, const float* prior, size_t ldp, const float* t, const float* mu,
                   const float* logvar, float* out, float* terms, double* per, double* Theta, double* G, int Bl, int Bt,
                   int L, int D, double lambda_sw, double coef_kl, void* ws, size_t ws_bytes, void* stream);
int itcv_sw_kl_bwd(const float* g, const float* mu, const float* logvar, const double* G, const double* Theta,
                   float* dz_all, float* dmu, float* dlogvar, int Bl, int Bt, int L, int D, double lambda_sw,
                   double coef_kl, void* stream);
/* The latent op of Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020; disentanglement_lib's `weak` module: GroupVAEBase with
 * aggregate_argmax) with its gradient (csrc/ada.hip).  mu, logvar, eps [2B][D] fp32 with unit column stride and row strides
 * ld_mu, ld_logvar, ld_eps >= D (mu and logvar may be the halves of one [2B][2D] tensor); rows b and B + b are a pair
 * (m1, l1), (m2, l2).  Per pair and dimension d, in fp64 from the fp32 inputs:
 *   delta = exp(l1 - l2) + (m2 - m1)^2 exp(-l2) - 1 + l2 - l1        (the library's compute_kl: one direction, no 1/2)
 *   tau   = (min_d delta + max_d delta) / 2,   own = delta >= tau    (D = 1 or all-equal delta: every dimension is own);
 *           own_in [B][D] uint8 (may be NULL), when given, replaces the threshold: own = own_in != 0
 *   averaging 1 "gvae":  mb = (m1 + m2) / 2, vb = (e^l1 + e^l2) / 2
 *   averaging 2 "mlvae": vb = 2 e^l1 e^l2 / (e^l1 + e^l2), mb = vb (m1 e^-l1 + m2 e^-l2) / 2
 *   (mt_i, lt_i) = own ? (m_i, l_i) : (mb, log vb);   z_i = mt_i + eps_i exp(lt_i / 2)
 *   part[r] = -1/2 sum_d (1 + lt - mt^2 - e^lt) for r < 2B (the KL of adapted row r), part[2B + b] = the number of shared
 *           (not own) dimensions of pair b: part [3B] fp64 is the op's workspace
 *   out[0]   = beta * mean_{r < 2B} part[r];  terms[2] = {that mean, mean_b part[2B + b]}
 * z [2B][D] fp32 and own [B][D] uint8 are dense and written in full.  2 launches: a wave per pair (four pairs a block, the
 * blocks stride over the pairs), then a one-block finish that adds the partials in row order.
 * _bwd, ONE launch, the mask a constant: dz [2B][D] (row stride ld_dz >= D) and g[1] are the gradients of z and out[0];
 * every element of the dense dmu, dlogvar [2B][D] is written.  With g_k = g beta / (2B):
 *   own:    dm_i = dz_i + g_k m_i,  dl_i = dz_i eps_i e^(l_i / 2) / 2 + g_k (e^l_i - 1) / 2
 *   shared: G_m = dz_1 + dz_2 + 2 g_k mb,  G_l = sqrt(vb) (dz_1 eps_1 + dz_2 eps_2) / 2 + g_k (vb - 1)
 *     gvae:  dm_i = G_m / 2,  dl_i = G_l e^l_i / (e^l1 + e^l2)
 *     mlvae: w_i = e^-l_i / (e^-l1 + e^-l2):  dm_i = G_m w_i,  dl_i = G_l w_i + G_m w_i (mb - m_i)
 * beta == 0 leaves the KL out of out[0] and of the gradients whatever its value.  Every sum is fp64 in a fixed order, there
 * are no atomics: results are bitwise reproducible and do not depend on the grid.  Refused before any launch: a NULL
 * pointer (own_in excepted), B outside 1..2^30, D outside 1..512, another averaging, a non-finite beta, a row stride
 * below D. */
int itcv_ada_group_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps,
                       size_t ld_eps, const uint8_t* own_in, float* z, uint8_t* own, double* part, float* out,
                       float* terms, int B, int D, int averaging, double beta, void* stream);
int itcv_ada_group_bwd(const float* dz, size_t ld_dz, const float* g, const float* mu, size_t ld_mu, const float* logvar,
                       size_t ld_logvar, const float* eps, size_t ld_eps, const uint8_t* own, float* dmu, float* dlogvar,
                       int B, int D, int averaging, double beta, void* stream);
/* The latent op of JointVAE (Dupont 2018, "Learning Disentangled Joint Continuous and Discrete Representations") and, with
 * n_disc = 0, of AnnealedVAE (Burgess et al. 2018; disentanglement_lib's `annealed_vae`) with its gradient (csrc/joint.hip).
 * mu, logvar [B][D] fp32, D = n_cont + n_disc, unit column stride and row strides ld_mu, ld_logvar >= D (they may be the
 * halves of one [B][2D] tensor).  Columns [0, n_cont) are the continuous posterior; columns [n_cont, D) of mu are the LOGITS
 * a of G categorical variables laid side by side, and the same columns of logvar are never read.  eps [B][n_cont] ~ N(0, 1)
 * (ld_eps >= n_cont), u [B][n_disc] ~ U[0, 1) (ld_u >= n_disc).  seg [n_disc][2] int32 on the device: the first and the
 * one-past-last column of the group of discrete column j, both counted from the first discrete column (the kernels hold
 * them inside 0 <= first <= j < last <= n_disc).  cap [2] fp64 ON THE DEVICE = (C_z, C_c), read by the second launch when it
 * runs: a captured graph replays with whatever it holds then.  In fp64 from the fp32 inputs, every sum in column order:
 *   z_d   = m + eps exp(l / 2),   part[b] = -1/2 sum_d (1 + l - m^2 - e^l)                                   (d < n_cont)
 *   per group of K columns: log alpha = a - logsumexp(a),  u' = u > 0 ? u : 2^-25,  g = -log(-log u'),
 *           y = softmax((a + g) / tau) -> z,   part[B + b] = sum over the groups of (log K + sum_k alpha_k log alpha_k)
 *   KL_z = mean_b part[b], KL_c = mean_b part[B + b]                     (part [2B] fp64 is the op's workspace)
 *   out[0] = beta (gamma_cont |KL_z - C_z| + gamma_disc |KL_c - C_c|),  sgn[2] = the signs of the two differences (0 at 0),
 *   terms[4] = {KL_z, KL_c, C_z, C_c}
 * z [B][D] fp32 is dense and written in full.  2 launches: a wave per row (four rows a block, the blocks stride over the
 * rows), then a one-block finish that adds the partials in row order.
 * hard != 0, ONE launch, the deterministic code: z_d = mu_d bit for bit (d < n_cont) and, per group, the one-hot of the FIRST
 * maximum of the fp32 logits (an exact comparison; ties take the lowest column).  Only mu, seg and z are touched then; every
 * other pointer may be NULL and tau, the gammas and beta are not looked at.
 * _bwd, ONE launch: dz [B][D] (row stride ld_dz >= D) and g[1] are the gradients of z and out[0], sgn the forward's; every
 * element of the dense dmu, dlogvar [B][D] is written.  With k_z = g beta gamma_cont sgn[0] / B, k_c = g beta gamma_disc
 * sgn[1] / B:
 *   d < n_cont:  dm = dz + k_z m,   dl = dz eps e^(l / 2) / 2 + k_z (e^l - 1) / 2
 *   per group:   da_k = y_k (dz_k - sum_j y_j dz_j) / tau + k_c alpha_k (log alpha_k - sum_j alpha_j log alpha_j),  dl = 0
 * Every sum is fp64 in a fixed order, there are no atomics: results are bitwise reproducible and do not depend on the grid.
 * Refused before any launch: a NULL pointer that the call needs (eps / logvar with n_cont = 0, u / seg with n_disc = 0 are
 * not needed), B outside 1..2^30, a negative n_cont or n_disc, D outside 1..512, a temperature that is not finite and above
 * 0, a gamma that is negative or not finite, a non-finite beta, a row stride below its width. */
int itcv_joint_latent_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps,
                          size_t ld_eps, const float* u, size_t ld_u, const int* seg, const double* cap, float* z,
                          double* part, float* out, float* sgn, float* terms, int B, int n_cont, int n_disc, int hard,
                          double tau, double gamma_cont, double gamma_disc, double beta, void* stream);
int itcv_joint_latent_bwd(const float* dz, size_t ld_dz, const float* g, const float* sgn, const float* mu, size_t ld_mu,
                          const float* logvar, size_t ld_logvar, const float* eps, size_t ld_eps, const float* u,
                          size_t ld_u, const int* seg, float* dmu, float* dlogvar, int B, int n_cont, int n_disc,
                          double tau, double gamma_cont, double gamma_disc, double beta, void* stream);
/* The label regulariser of the semi-supervised S2 objectives (Locatello et al. 2020, "Disentangling Factors of Variation
 * Using Few Labels"; disentanglement_lib's `semi_supervised_vae`: supervised_regularizer_xent / _l2 / _cov) with its gradient
 * (csrc/sup.hip).  mu [B][D] fp32: the encoder means of the B labelled rows, unit column stride and a row stride ld_mu >= D
 * (read in place: a row slice of a wider tensor, half of a packed [.][2D] tensor).  y [B][F] fp32 holding the integer factor
 * values, row stride ld_y >= F.  1 <= F <= min(D, 64), D <= 512.  All three forms are SUMS over the labelled batch, not means,
 * as the library defines them.  In fp64 from the fp32 inputs:
 *   form 1 "xent": t = y_bf / sizes[f];  sup = sum_b sum_{f<F} (max(m, 0) - m t + log1p(exp(-|m|))),  m = mu[b][f]
 *                  d sup / d m = sigmoid(m) - t.  sizes [F] int32 ON THE DEVICE; min_size is its smallest entry as the host
 *                  that built it knows it (only this form reads either).
 *   form 2 "l2":   sup = sum_b sum_{f<F} (scale mu[b][f] - y_bf)^2;   d sup / d m = 2 scale (scale m - y)
 *   form 3 "cov":  C = (1 / B) sum_b (mu[b] - mean)(y_b - ybar)^T  [D][F];  W = C with W_ii = 0 (i < min(D, F));
 *                  sup = sum_ij W_ij^2;   d sup / d mu[b][i] = (2 / B) sum_j W_ij (y_bj - ybar_j)
 * Columns >= F of mu get an exactly zero gradient under xent and l2 (they are not read); under cov every column counts.
 * gamma: gamma_dev, when not NULL, is a [1] fp64 value ON THE DEVICE that the second launch reads when it runs (a captured
 * graph replays with whatever it holds then) and the scalar argument gamma is not looked at; with gamma_dev NULL the scalar
 * is used.  out[0] = gamma * sup;  terms[2] = {sup, gamma};  keep [1 + F] fp64: keep[0] = the gamma that was used, and under
 * cov keep[1 + j] = ybar_j.  Wt [F][D] fp64 (cov only, may be NULL otherwise): Wt[j][i] = W_ij, so that the backward is the
 * row-major product (2 / B) Y_c Wt.  ws: itcv_sup_workspace(B, D, F, form) bytes (B fp64 row partials, or one per 32 x 32
 * tile of C; 0 for shapes the op refuses).
 * 2 launches forward: xent / l2 a wave per row (four rows a block, the blocks stride over the rows), cov a 32 x 32 tile of
 * C per block (column means first, then the rows in staged chunks of 64); then a one-block finish that adds the partials in
 * index order.
 * _bwd, ONE launch: g[1] is the gradient of out[0]; every element of the dense dmu [B][D] fp32 is written:
 * g keep[0] d sup / d mu.  It reads keep and Wt of the forward, not gamma_dev again.  gamma == 0 gives out[0] = 0 and an all-zero
 * dmu whatever sup is.  Every sum is fp64 in a fixed order, there are no atomics: results are bitwise reproducible and do
 * not depend on the grid.  Refused before any launch: a NULL pointer that the form needs, B outside 1..2^24, D outside
 * 1..512, F outside 1..64, F > D, another form, min_size < 1 under xent, a gamma (gamma_dev NULL) or scale that is not
 * finite, a row stride below its width, a workspace that is too small. */
size_t itcv_sup_workspace(int B, int D, int F, int form);
int itcv_sup_fwd(const float* mu, size_t ld_mu, const float* y, size_t ld_y, const int* sizes, int min_size,
                 const double* gamma_dev, double gamma, double scale, float* out, float* terms, double* Wt, double* keep,
                 void* ws, size_t ws_bytes, int B, int D, int F, int form, void* stream);
int itcv_sup_bwd(const float* g, const float* mu, size_t ld_mu, const float* y, size_t ld_y, const int* sizes, int min_size,
                 double scale, const double* Wt, const double* keep, float* dmu, int B, int D, int F, int form,
                 void* stream);
/* The importance-weighted bound (Burda, Grosse and Salakhutdinov 2016, "Importance Weighted Autoencoders") as a training
 * objective and as a streaming estimate of log p(x), with the gradient estimators of Roeder et al. 2017 ("sticking the
 * landing") and Tucker et al. 2019 (doubly reparameterised), csrc/iwae.hip.  K samples of each of B images: row r = k B + b is
 * sample k of image b, so slab k = 0 is the plain batch.  1 <= K <= 1024, B K <= 2^24, 1 <= D <= 512.  fp64 arithmetic from
 * the fp32 inputs; every sum in a fixed order, no atomics: results are bitwise reproducible and do not depend on the grid.
 * mu, logvar [B][D] fp32 with unit column stride and row strides ld_mu, ld_logvar >= D (read in place); eps [K B][D], row
 * stride ld_eps >= D.
 * itcv_iwae_sample_fwd, ONE launch (a wave per row): with s = exp(logvar / 2)
 *   z[r][d] = mu[b][d] + s eps[r][d]  (dense [K B][D] fp32),   lat[r] = 1/2 sum_d (z^2 - eps^2 - logvar)  ([K B] fp64)
 * lat is log q(z | x) - log p(z) of the sample; no clamp and no variance floor; it is formed from the fp64 z.
 * itcv_iwae_sample_bwd, ONE launch (a thread per element of [B][D], the K samples walked in k order): dz [K B][D] (row stride
 * ld_dz >= D) is the gradient of z, h [K B] fp64 that of lat, wt [K B] fp64 the normalised weights of itcv_iwae_combine_fwd
 * (read under estimator 2 only; may be NULL otherwise).  Every element of the dense dmu, dlogvar [B][D] fp32 is written:
 *   estimator 0 "iwae": t = dz + h z;                  dmu = sum_k t,  dlogvar = sum_k (t eps s / 2 - h / 2)
 *   estimator 1 "stl":  p = dz + h (z - eps / s);      dmu = sum_k p,  dlogvar = sum_k p eps s / 2
 *   estimator 2 "dreg": p as under 1, times wt[r]
 * (1 and 2 drop the direct dependence of log q on mu and logvar and keep the path through z.)
 * itcv_iwae_rows_fwd, 2 launches, the broadcast reconstruction rows: rows[r] = sum_p err(recon[r][p], x[r mod B][p]) for
 * x [B][P] and recon [K B][P], both dense; x is never copied K times.  A block takes one slice of one image and a k-strided
 * set of its rows, so the slice of x comes from HBM once.  err, the slicing and the order of every row's sum are those of
 * itcv_recon_rows_fwd at K B rows: with x repeated K times the two entries give the same bits (float4 reads under the same
 * condition: P % 4 == 0 and 16-byte aligned bases).  ws: itcv_iwae_rows_workspace(B, K, P) bytes (0 for refused shapes).
 * itcv_iwae_rows_bwd, ONE launch: drecon[r][p] = g[r] err'(recon[r][p], x[r mod B][p]), g [K B] fp32; the bits of
 * itcv_recon_rows_bwd on the repeated x.
 * itcv_iwae_combine_fwd, 2 launches (a wave per image, lanes striding over k; then a one-block finish that adds the per-image
 * values in image order): logw_r = -(beta_rec rows[r] + beta_kl lat[r]), m_b = max_k logw,
 *   wt[r] = e^(logw_r - m_b) / sum_k e^(logw - m_b)                                               ([K B] fp64)
 *   img [4][B] fp64 = {bound_b = m_b + log sum_k e^(logw - m_b) - log K,  ess_b = (sum_k e)^2 / sum_k e^2,
 *                      sum_k wt rows,  sum_k wt lat}
 *   out[0] = -mean_b bound_b,  terms[4] = {beta_rec mean_b sum_k wt rows, beta_kl mean_b sum_k wt lat, mean_b bound_b, mean_b ess_b}
 * K = 1 gives bound_b = logw, wt = 1 and ess = 1 exactly; K equal weights give ess = K exactly.
 * itcv_iwae_combine_bwd, ONE launch: with a_r = g[0] wt[r] / B, g_rows[r] = (float)(beta_rec a_r), g_lat[r] = beta_kl a_r (fp64).
 * itcv_iwae_accumulate, ONE launch, the streaming form: one chunk's rows, lat of K samples of B images is merged into
 * state [5][B] fp64 = {running max m, sum e^(logw - m), sum e^(2 (logw - m)), sum logw, count}; a count of 0 marks an empty
 * state (a zero-filled buffer is one).  The number of samples is unbounded across calls.  itcv_iwae_finalize, ONE launch:
 *   log_px[b] = m + log sum e - log count,  elbo[b] = sum logw / count,  ess[b] = (sum e)^2 / sum e^2     (all [B] fp64)
 * Refused before any launch, with every output untouched: a NULL pointer that the call needs, B < 1, K outside 1..1024,
 * B K above 2^24, D outside 1..512, a row stride below its width, P < 1, an unknown loss type or estimator, a beta that is
 * not finite, a workspace that is too small. */
int itcv_iwae_sample_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps,
                         size_t ld_eps, float* z, double* lat, int B, int K, int D, void* stream);
int itcv_iwae_sample_bwd(const float* dz, size_t ld_dz, const double* h, const double* wt, const float* mu, size_t ld_mu,
                         const float* logvar, size_t ld_logvar, const float* eps, size_t ld_eps, float* dmu, float* dlogvar,
                         int B, int K, int D, int estimator, void* stream);
size_t itcv_iwae_rows_workspace(int B, int K, size_t P);
int itcv_iwae_rows_fwd(const float* x, const float* recon, float* rows, int B, int K, size_t P, int loss_type, void* ws,
                       size_t ws_bytes, void* stream);
int itcv_iwae_rows_bwd(const float* x, const float* recon, const float* g, float* drecon, int B, int K, size_t P,
                       int loss_type, void* stream);
int itcv_iwae_combine_fwd(const float* rows, const double* lat, double beta_rec, double beta_kl, double* wt, double* img,
                          float* out, float* terms, int B, int K, void* stream);
int itcv_iwae_combine_bwd(const float* g, const double* wt, double beta_rec, double beta_kl, float* g_rows, double* g_lat,
                          int B, int K, void* stream);
int itcv_iwae_accumulate(const float* rows, const double* lat, double beta_rec, double beta_kl, double* state, int B, int K,
                         void* stream);
int itcv_iwae_finalize(const double* state, double* log_px, double* elbo, double* ess, int B, void* stream);
/* The KL term of a VAE with a VampPrior (Tomczak & Welling 2018, "VAE with a VampPrior") with its gradient, csrc/vamp.hip:
 * one sample per row against the uniform mixture of K diagonal Gaussians.  mu, logvar, eps [B][D] fp32 (the posterior and
 * its N(0, 1) draw) and p_mu, p_logvar [K][D] fp32 (the components), all with unit column stride and row strides >= D, read
 * in place (a pair may be the halves of one [.][2D] tensor).  1 <= B, K <= 4096, B K <= 2^22, 1 <= D <= 512.  In fp64 from
 * the fp32 inputs, with c = log 2 pi:
 *   z_bd   = fp32(mu + eps exp(logvar / 2))                  (dense [B][D]; L below is formed from this rounded value)
 *   logq_b = -1/2 sum_d (c + logvar_bd + eps_bd^2)           (exact in eps: no (z - mu) / sigma round trip)
 *   L_bk   = -1/2 (D c + sum_d p_logvar_kd + sum_d (z_bd - p_mu_kd)^2 exp(-p_logvar_kd))
 *   logp_b = logsumexp_k L_bk - log K,   r_bk = exp(L_bk - logsumexp_k L_bk)
 *   rows_b = beta (logq_b - logp_b)      (fp32 [B]);  out[0] = beta * mean_b (logq_b - logp_b), the sum under reduce 2
 *   terms[3] = {mean_b (logq_b - logp_b), mean_b logq_b, mean_b logp_b};   logq, logp: fp64 [B]
 * reduce: 0 "none" and 1 "mean" give the mean in out[0], 2 "sum" the sum; rows is written in every case.  L [B][K] fp64
 * holds r when the call returns: kept for _bwd.  The logsumexp is taken per tile of 32 components about the tile's own
 * maximum and the tiles are combined about the row's maximum, tiles ascending: a component astronomically far away gets
 * r_bk = 0.0 exactly and nothing overflows.  Row b of z, logq, logp and rows depends on row b of the inputs and on the
 * components alone.  Workspace: itcv_vamp_workspace (the max and sum partials per component tile and row, and the KL per
 * row: at most 2.2 MiB; 0 for shapes the op refuses).  2 launches: 32 x 32 tiles of L over a grid, D staged through LDS in
 * chunks of 32 with exp(-p_logvar) taken once per staged element; then a finish whose first block writes logp, rows, the
 * scalar and the terms and whose other blocks (at most 128) turn 16 rows of L a trip into r.
 * _bwd, ONE launch: gz [B][D] (row stride ld_gz >= D; NULL: zero) is the gradient of z; g (NULL: zero) that of out[0]
 * (g_rows == 0: g[1]) or of rows (g_rows != 0: g[B]); G_b = g_scale * g.  The caller passes g_scale = 1 / B for the mean.
 * z and r are the forward's.  Every element of the dense dmu, dlogvar [B][D] and dp_mu, dp_logvar [K][D] fp32 is written,
 * with iv = exp(-p_logvar):
 *   A_bd = sum_k r_bk (z_bd - p_mu_kd) iv_kd,   t_bd = gz_bd + G_b beta A_bd
 *   dmu = t,   dlogvar = exp(logvar / 2) eps t / 2 - G_b beta / 2
 *   dp_mu_kd = -beta sum_b G_b r_bk (z_bd - p_mu_kd) iv_kd,   dp_logvar_kd = beta / 2 sum_b G_b r_bk (1 - (z_bd - p_mu_kd)^2 iv_kd)
 * Blocks x < ceil(B / 16) take a 16 x 64 tile of [B][D] over chunks of 32 components, the blocks behind them a 16 x 64 tile
 * of [K][D] over chunks of 32 rows.  beta == 0 leaves the term out of out[0], rows and the gradients whatever its value.
 * itcv_vamp_logprob, 2 launches: logp [N] fp64 of given rows x [N][D] fp32 (row stride ld_x >= D) under the same mixture;
 * the same pair pass, so x = the z of _fwd gives its logp bit for bit.  N takes B's limits.
 * Every sum is fp64 in a fixed order, there are no atomics: results are bitwise reproducible and do not depend on the grid.
 * Refused before any launch: a NULL pointer (gz and g excepted), B (N) or K outside 1..4096, D outside 1..512, B K above
 * 2^22, a non-finite beta or g_scale, another reduce, a row stride below D, a workspace that is too small. */
size_t itcv_vamp_workspace(int B, int K, int D);
int itcv_vamp_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps, size_t ld_eps,
                  const float* p_mu, size_t ld_pmu, const float* p_logvar, size_t ld_plogvar, float* z, double* L,
                  double* logq, double* logp, float* rows, float* out, float* terms, int B, int K, int D, double beta,
                  int reduce, void* ws, size_t ws_bytes, void* stream);
int itcv_vamp_bwd(const float* gz, size_t ld_gz, const float* g, int g_rows, double g_scale, const float* logvar,
                  size_t ld_logvar, const float* eps, size_t ld_eps, const float* z, const float* p_mu, size_t ld_pmu,
                  const float* p_logvar, size_t ld_plogvar, const double* r, float* dmu, float* dlogvar, float* dp_mu,
                  float* dp_logvar, int B, int K, int D, double beta, void* stream);
int itcv_vamp_logprob(const float* x, size_t ld_x, const float* p_mu, size_t ld_pmu, const float* p_logvar,
                      size_t ld_plogvar, double* logp, int N, int K, int D, void* ws, size_t ws_bytes, void* stream);
/* The FactorVAE objective (Kim & Mnih 2018; disentanglement_lib's `factor_vae`), csrc/factor.hip.
 * itcv_permute_dims, ONE launch (a block per column): out[r][d] = z[i][d] where r is the rank of keys[i][d] in column d
 * of keys[B][D] -- ascending in the monotone uint32 image of the float's bits (the sign-flip map of itcv_udr_ranks, +0 and
 * -0 share one image), then in the row index i.  The result is a permutation of every column for ANY keys (ties, +-0,
 * +-inf, NaN).  z and keys have row strides ldz, ldk >= D; out is dense; zcopy (may be NULL) receives the dense copy of z
 * in the same launch.  Keys and indices are sorted in LDS.  Refused: a NULL z / keys / out, B outside 1..4096, D outside
 * 1..512, a row stride below D.
 * itcv_disc_head_fwd, ONE launch: logits[R][2] (dense), the first R0 rows labelled 0 and the rest 1; d_i = l_i0 - l_i1:
 *   out[0] = tc     = mean_{i < R0} d_i
 *   out[1] = d_loss = 0.5 mean_{i < R0} softplus(-d_i) + 0.5 mean_{i >= R0} softplus(d_i)   (cross entropy; the second
 *            term is 0 when R == R0), softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   out[2] = d_acc  = the share of the R rows whose argmax (the first of two equal logits) is their label.
 * itcv_disc_head_bwd, ONE launch, g[1] on the device: mode 0 writes the R0 rows dlogits[i] = (+w, -w), w = g / R0 (the
 * gradient of tc); mode 1 (needs R0 < R) writes all R rows, w = -g sigmoid(-d_i) / (2 R0) for i < R0 and
 * w = g sigmoid(d_i) / (2 (R - R0)) for the others (the gradient of d_loss).
 * Every sum is fp64 in a fixed order, there are no atomics; both are finite for any finite logits.  Refused: a NULL
 * pointer, R0 outside 1..R, R above 2^24, another mode. */
int itcv_permute_dims(const float* z, size_t ldz, const float* keys, size_t ldk, float* out, float* zcopy, int B, int D,
                      void* stream);
int itcv_disc_head_fwd(const float* logits, int R, int R0, float* out, void* stream);
int itcv_disc_head_bwd(const float* g, const float* logits, float* dlogits, int R, int R0, int mode, void* stream);
/* solvers/tc.py:104-121: per-sample log q(z|x) (ops.py:24-29 density, own mu/logvar) and log p(z) */
int itcv_diag_logdensity_rows(const float* z, const float* mu, const float* logvar, float* logq_cx,
                              float* logpz, int B, int D, void* stream);
/* Materialising forms of the reference's named helpers, for callers that use the pieces one by one
 * (`from ops import gaussian_log_density, ...`, solvers/tc.py:5-11); the training step uses the fused kernels above.
 * ops.py:15-21 (eps_density != 0: variance floor 1e-4, straight-through) / ops.py:24-29: out[n0][n1][n2] =
 * clamp(log N(x; mu, exp(logvar)), min=-50) with the three operands broadcast to dims[3] through element strides
 * sx/sm/sl[3] (0 = broadcast dimension).  _bwd: elementwise gradients at the broadcast shape, dx (dmu = -dx) and
 * dlogvar, zero where the clamp is active; the caller sums them over its broadcast dimensions. */
int itcv_gauss_logdensity_fwd(const float* x, const float* mu, const float* logvar, float* out, const int64_t* dims,
                              const int64_t* sx, const int64_t* sm, const int64_t* sl, int eps_density, void* stream);
int itcv_gauss_logdensity_bwd(const float* g, const float* x, const float* mu, const float* logvar, float* dx,
                              float* dlogvar, const int64_t* dims, const int64_t* sx, const int64_t* sm,
                              const int64_t* sl, int eps_density, void* stream);
/* ops.py:104-115 (weighted == 0) / ops.py:92-101 on a materialised lp[B][B][D]: prodm[B], logqz[B]; lse[B][D] and
 * sjoint[B][B] are kept for _bwd, which returns dlp[B][B][D] for gradients g_prodm[B], g_logqz[B]. */
int itcv_sampling_fwd(const float* lp, float* prodm, float* logqz, float* lse, float* sjoint, int B, int D,
                      int64_t dataset_size, int weighted, void* stream);
int itcv_sampling_bwd(const float* g_prodm, const float* g_logqz, const float* lp, const float* lse,
                      const float* sjoint, const float* logqz, float* dlp, int B, int D, int64_t dataset_size,
                      int weighted, void* stream);
/* ops.py:118-122 for x[m][n] with m == n or m == 1: diag[min(m,n)], off[m][n][n] = x - diag_embed(x) */
int itcv_on_off_diag(const float* x, float* diag, float* off, int m, int n, void* stream);
/* Log density of S samples under a mixture of N diagonal Gaussians -- a whole dataset's aggregate posterior -- and under
 * the product of its marginals, streamed (csrc/aggregate.hip): with lp[j][i][l] = max(log N(z_jl; mu_il, exp(logvar_il)),
 * -50) (the ops.py:24-29 density with the variance of component i; the clamp per element, inside the sum over l),
 *   logqz[j]  = logsumexp_i(logw_i + sum_l lp[j][i][l]),      lse[j][l] = logsumexp_i(logw_i + lp[j][i][l]).
 * logw: N finite log weights, or NULL for -log N each.  1 <= D <= 512, S >= 1, N >= 1; anything else, a null operand or
 * a short workspace returns non-zero before a launch.  splits: the number of slices the component range is cut into
 * (each leaves one (max, sum) partial per (row, l) and per row; a second kernel merges them in slice order); 0 lets the
 * library choose from S, N and D so that the grid fills the 256 CUs; values above min(N, 1024) are lowered to that, and
 * slices that would be empty are not made.  With s the slice count actually used,
 *   itcv_aggregate_workspace = 2 * S * s * (D + 1) * sizeof(float)      (s <= 1024: nothing grows with S * N).
 * No atomics and fixed summation orders: bitwise reproducible, and for a given splits row j's results depend only on
 * z[j] and the components, not on S or on the other rows of the call. */
size_t itcv_aggregate_workspace(int64_t S, int64_t N, int D, int splits);
int itcv_aggregate_logdensity(const float* z, const float* mu, const float* logvar, const float* logw, float* logqz,
                              float* lse, int64_t S, int64_t N, int D, int splits, void* ws, size_t ws_bytes,
                              void* stream);

/* ---- disentanglement scores (evaluation/utils.py:245-273,323-335, metrics.py:169-219) -- */
/* Mutual information between every discretised latent column of mu[N][D] (fp32, row stride ld elements) and every
 * ground-truth factor column of v[N][K] (int32, values 0..fsize[k]-1), from integer joint histograms.
 * Supported: 1 <= bins <= 32, 1 <= K <= 16, 1 <= fsize[k] <= 256, 1 <= N <= 2^30, any D >= 1; anything else returns non-zero
 * before a launch.  fsize is a HOST array of K ints.
 * Binning rule (np.histogram's edges + np.digitize(x, edges[:-1])), in fp64, each operation rounded on its own:
 *   lo = (double)min_d, hi = (double)max_d; if (lo == hi) lo -= 0.5, hi += 0.5;
 *   bin(x) = #{ j in 0..bins-1 : (double)x >= lo + j * ((hi - lo) / bins) }        (1..bins; stored 0-based in counts)
 * flags[2] (int, zeroed by the caller, only ever set): [0] a non-finite element of mu (minmax), [1] a factor value
 * outside [0, fsize[k]) (hist; that sample is not added for that factor).
 *   _minmax: mn[D], mx[D]; workspace itcv_disent_minmax_workspace.
 *   _bins:   out[N][D] = bin(mu[n][d]), dense int32.
 *   _hist:   counts[d][bins * off[k] + b * fsize[k] + f] (off = prefix sums of fsize; itcv_disent_counts_elems uint32,
 *            fsum = off[K]) and the factor marginals vcount[off[k] + f]; both are cleared by the call.  Integer sums:
 *            bitwise reproducible.
 *   _hist_tiling: host only, no GPU work: the launch plan _hist makes for (D, K, fsize, bins), as out[21] ints:
 *            [0] columns per block (a power of two, 1..64), [1] column tiles, [2] factor groups ng, [3] LDS bytes of a
 *            block, [4 .. 4 + ng] the first factor of every group and then K, zeros behind.  Refuses what _hist refuses.
 *   _mi:     mi[D][K] = max(0, sum_{c>0} (c/N)(log c - log r_b - log s_f + log N)) in nats (r, s: row / column sums of the
 *            pair's table) and h[K] = sum_{s>0} -(s/N) log(s/N), in fp64. */
size_t itcv_disent_minmax_workspace(int N, int D);
int itcv_disent_minmax(const float* mu, size_t ld, int N, int D, float* mn, float* mx, int* flags, void* ws,
                       size_t ws_bytes, void* stream);
int itcv_disent_bins(const float* mu, size_t ld, int N, int D, const float* mn, const float* mx, int bins, int* out,
                     void* stream);
size_t itcv_disent_counts_elems(int D, int fsum, int bins);
int itcv_disent_hist(const float* mu, size_t ld, const int* v, int N, int D, int K, const int* fsize, int bins,
                     const float* mn, const float* mx, unsigned* counts, unsigned* vcount, int* flags, void* stream);
int itcv_disent_hist_tiling(int D, int K, const int* fsize, int bins, int* out);
int itcv_disent_mi(const unsigned* counts, const unsigned* vcount, int N, int D, int K, const int* fsize, int bins,
                   double* mi, double* h, void* stream);

/* ---- classifier-based disentanglement scores (evaluation/metrics.py:20-79,237-304; utils.py:60-174,277-320) -- */
/* The beta-VAE score and explicitness are the optimum of an L2-regularised softmax regression plus accuracy / one-vs-rest
 * ROC AUC of its probabilities.  All arithmetic is fp64; x[N][D] is fp32 with row stride ld (elements).
 * K problems share x: y[N][K] int32 labels, csize[K] class counts (a HOST array; coff = prefix sums, csum = coff[K]),
 * cvalid[csum] int32 (non-zero: the class takes part), theta[(D + 1)][csum] fp64 (row D: the intercepts).
 * mean / scale: both NULL (raw x) or both given (x is standardised on the fly as (x - mean[d]) / scale[d]).
 * Rule for problem p, with V its valid classes, its valid rows those with y in V, n their number:
 *   F_p = (1/n) sum_valid [ logsumexp_{c in V}(x.W_c + b_c) - (x.W_y + b_y) ] + (lambda/2) sum_{c in V} |W_c|^2,
 *   lambda = m / (C n), m = 2 when |V| == 2 (sklearn's binary model), else 1; intercepts are not penalised; the gradient
 *   of an invalid class is exactly 0.
 * Supported: 1 <= K <= 16, 1 <= csize[k] <= 256, 1 <= D <= 512, 1 <= N <= 2^30; anything else returns non-zero before a
 * launch.  flags[2] as for itcv_disent_*: [0] a non-finite element of x, [1] a label outside [0, csize[k]).
 * Every floating-point reduction has a fixed order: two calls with the same inputs return the same bits.
 *   _colstats: mean[D], scale[D] = sqrt(population variance), 1 where the variance is 0 (StandardScaler).
 *   _valgrad:  f[K], grad[(D + 1)][csum]; workspace itcv_logreg_workspace(N, D, K, csum).
 *   _proba:    P[N][csum] (0 for invalid classes and for rows whose label is invalid), pred[N][K] = first argmax of the
 *              logits over the valid classes (every row).
 *   _auc:      per valid class c over the problem's valid rows, s = P[:, c]:
 *              count2[c] = sum_{i: y_i = c} sum_{j: y_j != c} (2 [s_i > s_j] + [s_i == s_j]), pos[c], neg[c] (uint64, cleared by
 *              the call); AUC_c = count2 / (2 pos neg).
 *   itcv_zdiff_row: out[d] = fp32( mean_b |a[b][d] - b[b][d]| ), accumulated in fp64 (utils.py:106-109). */
size_t itcv_logreg_colstats_workspace(int N, int D);
int itcv_logreg_colstats(const float* x, size_t ld, int N, int D, double* mean, double* scale, int* flags, void* ws,
                         size_t ws_bytes, void* stream);
size_t itcv_logreg_workspace(int N, int D, int K, int csum);
int itcv_logreg_valgrad(const float* x, size_t ld, const double* mean, const double* scale, const int* y, int N, int D,
                        int K, const int* csize, const int* cvalid, const double* theta, double C, double* f,
                        double* grad, int* flags, void* ws, size_t ws_bytes, void* stream);
int itcv_logreg_proba(const float* x, size_t ld, const double* mean, const double* scale, const int* y, int N, int D,
                      int K, const int* csize, const int* cvalid, const double* theta, double* P, int* pred, int* flags,
                      void* stream);
int itcv_logreg_auc(const double* P, const int* y, int N, int K, const int* csize, const int* cvalid,
                    unsigned long long* count2, unsigned long long* pos, unsigned long long* neg, int* flags,
                    void* stream);
int itcv_zdiff_row(const float* a, const float* b, size_t ld, int B, int D, float* out, void* stream);

/* ---- DCI: histogram gradient-boosted trees (evaluation/metrics.py:82-161; utils.py:178-241) -- */
/* A multi-class gradient-boosted tree classifier after xgboost's documented `hist` algorithm and defaults, as a fixed
 * rule.  K problems share x[N][D] (fp32, row stride ld): y[N][K] int32 labels, csize[K] class counts (a HOST array;
 * coff = prefix sums, csum = coff[K]), cvalid[csum] int32 (non-zero: the class takes part; hipvae sets it iff the class
 * occurs in the training labels).  A "class slot" c in 0..csum-1 is class c - coff[k] of its problem k.
 * Supported: 1 <= K <= 16, 1 <= csize[k] <= 256, 1 <= D <= 512, 2 <= N <= 2^30 training rows (1 <= N for the entry points
 * that only read rows), 1 <= max_depth <= 6, 2 <= max_bin <= 256, rounds >= 1; anything else returns non-zero before a
 * launch.  flags[2] as for itcv_disent_*: [0] a non-finite element of x (bin), [1] a label outside [0, csize[k]) (grad,
 * predict).
 * Cuts (per feature d; s = the training column sorted ascending, B = max_bin): the candidates s[(j * N) / B] (integer
 *   division), j = 1..B-1; kept are the distinct values greater than s[0], ascending.  bin(x) = #{cuts <= x}, uint8,
 *   stored feature-major bins[D][N]; nbins[d] = #cuts + 1.  Test rows are binned with the training cuts.
 * Round: every valid class of a problem starts from margin 0 (margins F[csum][N] fp64, class-major).  p = softmax over
 *   the problem's valid classes in fp64, max-subtracted; for class c: g = p_c - [y == c], h = max((2 p_c)(1 - p_c), 1e-16),
 *   quantised gq = llrint(g * 2^24), hq = llrint(h * 2^24) (int64).  Every sum of gradients below is an INTEGER sum of gq /
 *   hq (|sum| <= 2^54): exact, and free of any summation order.  A row whose label is not a valid class of problem k has
 *   gq = hq = 0 for the classes of problem k (it takes no part), but is still routed and its margins still advance.
 * Tree: one per valid class per round, grown level by level to max_depth; lambda (default 1), eta (default 0.3),
 *   gamma = 0, min_child_weight = 1.  Nodes are heap-indexed (root 0, children of i: 2 i + 1, 2 i + 2; ITCV_GBT_TREE_NODES
 *   slots per tree); node[csum][N] uint8 holds the node every row sits in.
 * Candidate (d, b), b = 0..nbins[d]-2: left is bin <= b; admissible iff HLq >= 2^24 and HRq >= 2^24 (integer compares).
 * Gain: G = (double)Gq * 2^-24, H likewise; score(G, H) = (G * G) / (H + lambda); gain = 0.5 * ((score_L + score_R) -
 *   score_P); each operation rounded on its own (no fused multiply-add).  A node splits on the admissible candidate of
 *   largest gain if that gain is > 1e-6; bit-equal gains go to the smallest d, then the smallest b; otherwise it is a leaf.
 *   Leaf value ((-G) / (H + lambda)) * eta; train and test margins advance by the leaf values at the end of the round.
 * Tree arrays, [rounds][csum][ITCV_GBT_TREE_NODES]: tfeat (int32, -1: leaf or absent; the caller fills -1 before the
 *   fit), tbin (int32), tvalue (fp64 leaf value of every node that exists), tgain (fp64, of the split nodes; 0 else).
 * Prediction: first argmax of the margins over the valid classes (-1 without one); a label that is not a valid class
 *   counts as wrong.  Importance of problem k: imp[d] = (total gain of the splits on d) / (number of splits on d), 0 without
 *   a split, then imp / sum_d imp (all 0 if no tree ever split): xgboost's `gain` importance.  The totals are fp64 sums in
 *   the order round, class, node index; the normaliser in the order d = 0..D-1.  Same inputs, same bits.
 *   _cuts:       sorted[D][N] (feature-major, each row ascending) -> cuts[D][max_bin - 1], nbins[D].
 *   _bin:        x -> bins[D][N] with given cuts.
 *   _grad:       F -> gq, hq [csum][N] (and g, h as fp64 when both are non-NULL).
 *   _hist:       tab[nc][2^level][D][max_bin][2] int64 (G, H) of class slots c0..c0+nc-1 and the nodes of `level`, from
 *                the rows whose node id lies in that level; cleared by the call; tab_bytes >= what that takes.
 *   _split:      reads tab, writes the level's nodes of the tree arrays (pointers to ONE round's [csum][NODES] slices) and
 *                nsum[csum][NODES][2] (int64 G, H of every node that exists).
 *   _advance:    node ids of `level` one level down.        _margins: F[c][n] += leaf value (node == NULL: rows walk the
 *                tree from the root, as the test rows do).
 *   _round:      the whole launch sequence of one boosting round; classes are taken in chunks of tab_bytes /
 *                (2^(max_depth-1) * D * max_bin * 16) slots.  itcv_gbt_workspace: the table bytes that keep a chunk inside
 *                the budget of ITCV_GBT_TABLE_BUDGET bytes (at least one class slot). */
#define ITCV_GBT_TREE_NODES 127
#define ITCV_GBT_TABLE_BUDGET ((size_t)512 << 20)
size_t itcv_gbt_workspace(int N, int D, int K, int csum, int max_depth, int max_bin);
int itcv_gbt_cuts(const float* sorted, int N, int D, int max_bin, float* cuts, int* nbins, void* stream);
int itcv_gbt_bin(const float* x, size_t ld, int N, int D, int max_bin, const float* cuts, const int* nbins,
                 unsigned char* bins, int* flags, void* stream);
int itcv_gbt_grad(const double* F, const int* y, int N, int K, const int* csize, const int* cvalid, long long* gq,
                  long long* hq, double* g, double* h, int* flags, void* stream);
int itcv_gbt_hist(const unsigned char* bins, int N, int D, int max_bin, const long long* gq, const long long* hq,
                  const unsigned char* node, const int* cvalid, int c0, int nc, int level, long long* tab,
                  size_t tab_bytes, void* stream);
int itcv_gbt_split(const long long* tab, const int* nbins, int D, int max_bin, const int* cvalid, int c0, int nc,
                   int level, double lam, double eta, long long* nsum, int* tfeat, int* tbin, double* tvalue,
                   double* tgain, void* stream);
int itcv_gbt_advance(const unsigned char* bins, int N, int csum, const int* cvalid, const int* tfeat, const int* tbin,
                     int level, unsigned char* node, void* stream);
int itcv_gbt_margins(const unsigned char* bins, int N, int csum, const int* cvalid, const unsigned char* node,
                     const int* tfeat, const int* tbin, const double* tvalue, int max_depth, double* F, void* stream);
int itcv_gbt_predict(const double* F, const int* y, int N, int K, const int* csize, const int* cvalid, int* pred,
                     unsigned long long* correct, int* flags, void* stream);
int itcv_gbt_importance(const int* tfeat, const double* tgain, int rounds, int K, const int* csize, int D, double* imp,
                        void* stream);
int itcv_gbt_round(const unsigned char* bins, int N, int D, int max_bin, const int* nbins, const int* y, int K,
                   const int* csize, const int* cvalid, double* F, const unsigned char* bins_test, int Nt, double* Ft,
                   int max_depth, double lam, double eta, long long* gq, long long* hq, unsigned char* node,
                   long long* nsum, long long* tab, size_t tab_bytes, int* tfeat, int* tbin, double* tvalue,
                   double* tgain, int* flags, void* stream);

/* ---- FactorVAE and SAP scores (not in the reference; Kim & Mnih 2018, Kumar et al. 2018) ------------------------ */
/* Both scores are fixed rules; all arithmetic is fp64 on fp32 representations (row stride ld elements), every operation
 * rounded on its own (no fused multiply-add), every floating-point sum in a fixed order: same inputs, same bits.
 * flags[3] (int, zeroed by the caller, only ever set): [0] a non-finite representation, [1] a factor index / label outside
 * its range, [2] a SAP classifier that did not converge.
 *
 * FactorVAE score.  Inputs mu_var[Nv][D]; mu_train[Mt * L][D] with fidx_train[Mt]; mu_eval[Me * L][D] with fidx_eval[Me].  A
 * group is L consecutive rows, encoded from L factor vectors whose column fidx was overwritten with row 0's value.
 *   1. gvar[d] = the ddof = 1 variance of mu_var[:, d] (the mean first, then the squared deviations).
 *   2. d is ACTIVE iff sqrt(gvar[d]) >= threshold (default 0.05).  No active dimension: both accuracies are 0.
 *   3. Per group, lvar[d] = (sum_r (x_r - m)^2) / (L - 1), m = (sum_r x_r) / L, both sums over the rows in ascending order.
 *   4. The group votes for d* = argmin over the active d of lvar[d] / gvar[d], ties to the smallest d: votes[d*][fidx] += 1
 *      (int64; integer atomics, so the table does not depend on the order of arrival).  d* indexes ALL dimensions.
 *   5. classifier[d] = argmax_k votes_train[d][k], ties to the smallest k;
 *      train_accuracy = sum_d votes_train[d][classifier[d]] / Mt, eval_accuracy = sum_d votes_eval[d][classifier[d]] / Me.
 * Supported: 2 <= L <= 2^16, 2 <= Nv <= 2^24, M * L <= 2^24, 1 <= D <= 512, 1 <= K <= 256; anything else returns non-zero
 * before a launch.
 *   _gvar:     gvar[D].
 *   _votes:    votes[D][K], cleared by the call; fidx[M] int32 on the device.
 *   _classify: classifier[D] int32 and res[3] = {train_accuracy, eval_accuracy, number of active dimensions}. */
int itcv_fvae_gvar(const float* mu, size_t ld, int N, int D, double* gvar, int* flags, void* stream);
int itcv_fvae_votes(const float* mu, size_t ld, int M, int L, int D, const double* gvar, double threshold, const int* fidx,
                    int K, long long* votes, int* flags, void* stream);
int itcv_fvae_classify(const long long* votes_train, const long long* votes_eval, int D, int K, int Mt, int Me,
                       const double* gvar, double threshold, int* classifier, double* res, void* stream);
/* SAP score, discrete factors.  K factors share x[N][D]: y[N][K] int32 labels, csize[K] class counts (a HOST array; coff =
 * prefix sums, csum = coff[K]).  For latent i and factor j: V = the classes present in the train labels, n = N the train
 * rows, bw_c = n / (|V| count_c), x = column i as fp64, C = 0.01 by default.
 *   |V| >= 3: for each c in V minimise F(w, b) = (w^2 + b^2) / 2 + sum_n C_n max(0, 1 - t_n (w x_n + b))^2 with t_n = +1 where
 *             y_n == c, else -1; C_n = C bw_c on the positive rows, C on the others (liblinear's one-vs-rest with
 *             class_weight = "balanced").  Prediction: argmax_{c in V} (w_c x + b_c), ties to the smallest c.
 *   |V| == 2: ONE problem, stored at the slot of the larger class value V[1], whose rows are the positives; every row carries
 *             its own class's weight C_n = C bw_{y_n}.  Prediction: V[1] iff w x + b > 0, else V[0].
 *   |V| == 1: that class is predicted; nothing is solved.
 *   S[i][j] = (test rows whose prediction equals the label) / N_test; a test label outside V counts as wrong.  The score is
 *   the mean over j of (largest - second largest of S[:, j]), summed in factor order.
 * Solve: F is 1-strongly convex, so the optimum is unique and |theta - theta*|_2 <= |grad F(theta)|_2.  From (0, 0): Newton
 *   steps d = -H^-1 g with the generalised Hessian H = I + 2 sum_{1 - t z > 0} C_n [x^2, x; x, 1]; the step length starts at
 *   1 and is halved (50 times at the most) until F(theta + a d) <= F(theta) + 1e-4 a g.d, or until the trial point itself
 *   meets the stopping rule max(|dF/dw|, |dF/db|) <= gtol (default 1e-10).  A problem that has not met it after max_iter
 *   (default 100) Newton steps, or whose step lengths are exhausted, sets flags[2].
 * Supported: 1 <= K <= 16, 1 <= csize[k] <= 256, 1 <= D <= 512, 1 <= N <= 2^24; anything else returns non-zero before a launch.
 *   _fit:   theta[D][csum][2] = (w, b), gnorm[D][csum] = the final max-norm of the gradient, iters[D][csum] = Newton steps
 *           taken (all 0 at a slot without a problem), cvalid[csum] = the class occurs in the train labels.  Two launches:
 *           feature-major copies xt[D][N] / yt[K][N] with the class counts (integer atomics), then ONE launch that solves
 *           every problem, a wave each; up to itcv_sap_svc_lds_rows() rows the column and the labels sit in LDS, above
 *           that they are streamed from the copies.  Workspace: itcv_sap_svc_workspace.
 *   _score: correct[D][K] int64 (cleared by the call) and, when non-NULL, pred[D][K][Nt] int32. */
int itcv_sap_svc_lds_rows(void);
size_t itcv_sap_svc_workspace(int N, int D, int K, int csum);
int itcv_sap_svc_fit(const float* x, size_t ld, const int* y, int N, int D, int K, const int* csize, double C, double gtol,
                     int max_iter, double* theta, double* gnorm, int* iters, int* cvalid, int* flags, void* ws,
                     size_t ws_bytes, void* stream);
int itcv_sap_svc_score(const float* x, size_t ld, const int* y, int Nt, int D, int K, const int* csize, const int* cvalid,
                       const double* theta, long long* correct, int* pred, int* flags, void* stream);

/* ---- unsupervised scores and IRS (not in the reference; Locatello et al. 2019, Suter et al. 2019) ---------------- */
/* Fixed rules; all arithmetic is fp64 on fp32 representations x[N][D] (row stride ld elements), every operation rounded
 * on its own (no fused multiply-add outside the matrix cores), every floating-point reduction in a fixed order that depends
 * on the shapes alone and never on the grid, no floating-point atomics: same inputs, same bits.
 *
 * Covariance.  m[d] = (sum_n x[n][d]) / N;  C[i][j] = (sum_n (x[n][i] - m[i]) (x[n][j] - m[j])) / (N - 1): two passes over
 *   centred values, as np.cov.  The centred products are accumulated on v_mfma_f64_16x16x4_f64 (D padded to 16 with zero
 *   columns) per slice of rows; the slice length is a function of N alone and the slices are added in ascending order.  One
 *   triangle is computed and mirrored: C is symmetric bit for bit.  flags[2] as for itcv_disent_*: [0] a non-finite x.
 *   Supported: 2 <= N <= 2^24, 1 <= D <= 512.
 * Gaussian total correlation.  tc = (sum_d log C[d][d] - logdet C) / 2 with logdet C = 2 sum_d log L[d][d], L the Cholesky
 *   factor of C; both sums in ascending d.  A pivot <= 0 or non-finite sets info[0] and records its dimension in info[1]
 *   (C must be positive definite; the results are then nan).
 * Gaussian Wasserstein correlation.  w = 2 tr C - 2 sum_i sqrt(max(lambda_i(S), 0)) with S = D^1/2 C D^1/2, D = diag(C),
 *   S[i][j] = (sqrt(C[i][i]) C[i][j]) sqrt(C[j][j]) for j <= i, mirrored (S is similar to C o diag(C)[:, None], whose matrix
 *   square root disentanglement_lib takes); w_norm = w / tr C.  lambda: cyclic Jacobi in fp64 inside one launch.  A sweep is
 *   Dp - 1 rounds (Dp = D rounded up to even) of the round-robin schedule: round r rotates the disjoint pairs (r, Dp - 1) and
 *   ((r + k) mod (Dp - 1), (r - k) mod (Dp - 1)), k = 1 .. Dp / 2 - 1, each ordered p < q; a pair with q >= D or with
 *   S[p][q] == 0 is skipped; an element with |S[p][p]| + |S[p][q]| == |S[p][p]| and |S[q][q]| + |S[p][q]| == |S[q][q]| (fp64)
 *   is negligible and takes the identity rotation c = 1, s = 0: it is set to 0 and nothing else moves (inside a cluster of
 *   equal eigenvalues tau would be a quotient of rounding errors).  Rotation of (p, q): tau = (S[q][q] - S[p][p]) / (2 S[p][q]), t = sign(tau) / (|tau| +
 *   sqrt(1 + tau^2)) (sign(0) = +1), c = 1 / sqrt(1 + t^2), s = t c; all rotations of a round are computed from the matrix
 *   as the round finds it, then rows p, q become (c row_p - s row_q, s row_p + c row_q), then the columns likewise, and the
 *   2 x 2 block takes its closed form S[p][p] - t S[p][q], S[q][q] + t S[p][q], 0.  Before every sweep: stop when
 *   off(S)_F <= 1e-14 |S|_F; after 60 sweeps without that, info[2] is set.  lambda_i is the diagonal in index order.
 *   _gauss: res[5] = {tc, w, w_norm, tr C, logdet C}, eig[D], info[4] = {pivot failed, its dimension (-1), Jacobi did not
 *   converge, sweeps taken}.  One block; the matrix sits in LDS up to D = itcv_unsup_gauss_lds_dim(), above that in the
 *   workspace (itcv_unsup_gauss_workspace).  Supported: 1 <= D <= 512.
 * IRS.  v[N][K] int32 factor values in [0, fsize[k]) (fsize: a HOST array), order[K][N] int32: for every factor the row
 *   numbers sorted by that factor's value, stable.  mn / mx: the column minima / maxima of itcv_disent_minmax.
 *   1. d is ACTIVE iff mn[d] < mx[d] (disentanglement_lib tests var > 0, whose result for a constant column depends on
 *      rounding).  No active dimension: IRS = 0.
 *   2. maxdev[d] = max_n |x[n][d] - m[d]|, m as above.
 *   3. For every factor k and every value v PRESENT in the sample, G its rows, n = |G|: e[d] = (sum_G x[g][d]) / n;
 *      a = |x[g][d] - e[d]| sorted ascending; h = (n - 1) q; lo = floor(h); t = h - lo; hi = min(lo + 1, n - 1);
 *      Q = a[lo] + (a[hi] - a[lo]) t if t < 0.5, else a[hi] - (a[hi] - a[lo]) (1 - t)       (np.percentile, linear).
 *      a[lo] and a[hi] are found exactly (a radix select on the bit patterns of the fp64 values).
 *   4. cum[d][k] = (sum_v Q, ascending v) / #present values;  M[d][k] = 1 - cum[d][k] / maxdev[d] (0 for an inactive d);
 *      score[d] = max_k M[d][k], parent[d] its first arg-max;
 *      IRS = (sum_d score[d] maxdev[d]) / (sum_d maxdev[d]) over the active d in ascending order.
 *   flags[2] as for itcv_disent_*: [1] a factor value outside its range (or a row number of `order` outside [0, N)).
 *   _irs: maxdev[D], cum[D][K], M[D][K], score[D] fp64; parent[D], active[D] int32; res[2] = {IRS, number of active d}.
 *   A fixed number of launches whatever the groups; workspace itcv_irs_workspace(N, D, K, fsum).
 *   Supported: 1 <= N <= 2^24, 1 <= D <= 512, 1 <= K <= 16, 1 <= fsize[k] <= 256, 0 <= q <= 1.
 * Anything unsupported returns non-zero before a launch. */
size_t itcv_unsup_cov_workspace(int N, int D);
int itcv_unsup_cov(const float* x, size_t ld, int N, int D, double* mean, double* cov, int* flags, void* ws,
                   size_t ws_bytes, void* stream);
int itcv_unsup_gauss_lds_dim(void);
size_t itcv_unsup_gauss_workspace(int D);
int itcv_unsup_gauss(const double* cov, int D, double* res, double* eig, int* info, void* ws, size_t ws_bytes,
                     void* stream);
size_t itcv_irs_workspace(int N, int D, int K, int fsum);
int itcv_irs(const float* x, size_t ld, const int* v, const int* order, int N, int D, int K, const int* fsize, double q,
             const float* mn, const float* mx, double* maxdev, double* cum, double* M, double* score, int* parent,
             int* active, double* res, int* flags, void* ws, size_t ws_bytes, void* stream);

/* ---- UDR: tie-averaged ranks and the Lasso matrix (not in the reference; Duan et al. 2020) ------------------------ */
/* The two device primitives of the Unsupervised Disentanglement Ranking (disentanglement_lib's `udr`); fixed rules, no
 * floating-point atomics, nothing depends on the grid: same inputs, same bits.
 *
 * Ranks.  x[N][D] fp32 (row stride ld elements; nothing left of a strided view is read), r2[N][D] fp32 dense:
 *   r2[n][d] = L + H + 1,  L = #{m : x[m][d] < x[n][d]},  H = #{m : x[m][d] <= x[n][d]},
 *   twice scipy.stats.rankdata's average rank: an integer <= 2 N, exact in fp32 up to N = 2^23 (rounded to nearest above).
 *   The comparison is numeric: -0.0 equals +0.0, denormals are ordinary values.  A non-finite element sets flags[0] as in
 *   itcv_unsup_cov; r2 is then unspecified.  One block per column: every value becomes a monotone uint32 key (u = bits of
 *   x, +-0 -> 0; key = ~u if the sign bit is set, else u | 2^31), the keys of the column are sorted in place (a bitonic
 *   network whose exchanges all point upwards, so any N needs no padding), and every row finds L and H by two binary
 *   searches.  The sorted keys sit in LDS up to N = itcv_udr_rank_lds_rows() (32768 keys = 128 KiB of the 160 KiB; the
 *   in-place sort needs nothing else), above that in the workspace (itcv_udr_ranks_workspace: N D uint32, else 0).
 *   Supported: 2 <= N <= 2^24, 1 <= D <= 512 (the limits of itcv_unsup_cov).
 * Lasso.  cov: the fp64 covariance [(Da + Db)][(Da + Db)] of the concatenated columns [a | b] as itcv_unsup_cov writes it.
 *   1. R[k][l] = C[k][l] / sqrt(C[k][k] C[l][l]); a column with C[k][k] == 0 (exactly what the covariance's two centred
 *      passes give for a constant fp32 column) has row and column k of R equal to 0, the diagonal included.  This is
 *      StandardScaler followed by sklearn.linear_model.Lasso(alpha) with its intercept: the 1 / n factors cancel.
 *   2. For every target column t of b: G = R[:Da][:Da], c = R[:Da][Da + t], w_t = argmin 1/2 w'Gw - c'w + alpha |w|_1 by
 *      cyclic coordinate descent in index order from w = 0:
 *        w[k] <- S(c[k] - sum_{l != k} G[k][l] w[l], alpha) / G[k][k],   S(r, a) = r - a if r > a, r + a if r < -a, else 0;
 *      a coordinate with G[k][k] == 0 stays 0.  The sum is taken by one wave: lane i adds its terms l = i, i + 64, ... in
 *      ascending l, the 64 partial sums are folded by the xor butterfly (32, 16, .., 1).
 *   3. After every sweep: g = G w - c (the same sum, l == k included),
 *        v = max_k (w[k] != 0 ? |g[k] + alpha sign(w[k])| : max(|g[k]| - alpha, 0)).
 *      Stop at v <= gtol (a nan never stops); otherwise stop after max_sweeps sweeps.
 *   4. W[Da][Db] fp64, W[k][t] = |w_t[k]| (rows of a, columns of b: the library's transpose(abs(coef_))).
 *      info[3] = {some target did not reach gtol, how many, the largest number of sweeps any target took}.
 *   One wave per target, eight targets a block, one launch; G sits in LDS up to Da = 128, above that its rows are read
 *   from the normalised copy in the workspace (itcv_udr_lasso_workspace).  All arithmetic is fp64, every operation rounded
 *   on its own.  Supported: Da, Db >= 1, Da + Db <= 512, alpha >= 0 finite, gtol >= 0, max_sweeps >= 1.
 * Anything unsupported returns non-zero before a launch; the workspace queries return 0 for it. */
int itcv_udr_rank_lds_rows(void);
size_t itcv_udr_ranks_workspace(int N, int D);
int itcv_udr_ranks(const float* x, size_t ld, int N, int D, float* r2, int* flags, void* ws, size_t ws_bytes,
                   void* stream);
size_t itcv_udr_lasso_workspace(int Da, int Db);
int itcv_udr_lasso(const double* cov, int Da, int Db, double alpha, double gtol, int max_sweeps, double* W, int* info,
                   void* ws, size_t ws_bytes, void* stream);

/* ---- sample quality: neighbour radii, PRDC counts, polynomial MMD, Frechet distance (not in the reference) ------- */
/* Scores of generated samples against real ones over feature rows x[N][D] (fp32, row stride ld elements, read in place;
 * nothing left of a strided view is read): Kynkaanniemi et al. 2019 and Naeem et al. 2020 (the `prdc` package), Binkowski
 * et al. 2018 (KID), Heusel et al. 2017 (the Frechet distance).  Fixed rules; all arithmetic is fp64, every operation
 * rounded on its own (no fused multiply-add outside the matrix cores), every floating-point sum in a fixed order that
 * depends on the shapes alone, counts and minima through integer atomics (order-free), no floating-point atomic: same
 * inputs, same bits.  flags[0] is set by a non-finite element, as for itcv_unsup_cov; the outputs are then unspecified.
 *
 * Distance.  d2(a, b) = sum_d (a_d - b_d)^2: the difference of the widened values, its square, added in ascending d (the
 *   difference form of csrc/mmd.hip; never |a|^2 + |b|^2 - 2 a.b).  Integer-valued features give exact integers.
 * Radii.  r2[i] = the (k + 1)-th smallest of {d2(x_i, x_j) : j = 0 .. N - 1}, row i's own 0 included: prdc's
 *   get_kth_value(dist, k + 1), squared.  A block owns 32 rows and streams the candidates through LDS, 64 rows by 32
 *   columns a step, keeping the k + 1 smallest values of every row; nothing of size N x N is written.  A selection does not
 *   depend on the visiting order, so the candidates are cut into `splits` slices (grid = row tiles x slices) whose lists a
 *   second kernel merges: r2 is the same for every `splits`, bit for bit.  splits = 0 lets the library choose: slices until
 *   the grid has 1024 blocks, ceil(1024 / ceil(N / 32)); any value is lowered to min(ceil(N / 64), 256), and slices that
 *   would be empty are not made.  With s the slice count used, itcv_knn_radius_workspace = s * N * (k + 1) * sizeof(double).
 *   Supported: 2 <= N <= 2^20, 1 <= D <= 2048, 1 <= k <= 16, k < N, splits >= 0.
 * Counts.  real[N][D], fake[M][D], r2_real[N], r2_fake[M] (radii of each set among itself):
 *     fake_hits[j]    = #{i : d2(real_i, fake_j) < r2_real[i]}          (int32)
 *     real_covered[i] = 1 if some j has d2(real_i, fake_j) < r2_fake[j], else 0      (int32)
 *     real_min[i]     = min_j d2(real_i, fake_j)                         (fp64)
 *   every comparison strict, as in prdc.  The scores are rationals of these integers: precision = #{j : fake_hits[j] > 0}
 *   / M, recall = sum real_covered / N, density = sum fake_hits / (k M), coverage = #{i : real_min[i] < r2_real[i]} / N.
 *   The same streamed pass, the fakes as the candidates, `splits` as above (of M, for N rows); the outputs are cleared by
 *   the call and need no workspace.  Supported: 2 <= N, M <= 2^20, 1 <= D <= 2048.
 * Polynomial MMD.  kappa(a, b) = (gamma a.b + coef0)^degree, gamma = 1 / D when passed as 0, degree 1..4 by repeated
 *   multiplication (t, t t, (t t) t, (t t)(t t)).  a.b runs on v_mfma_f64_16x16x4_f64 from the widened values (D padded to
 *   a multiple of 4 with zeros, ascending).  res[4] = {Sxx, Syy, Sxy, mmd2}: Sxx = sum_{i != j} kappa(x_i, x_j), Syy
 *   likewise, Sxy = sum_{i, j} kappa(x_i, y_j), mmd2 = (Sxx / (N (N - 1)) + Syy / (M (M - 1))) - 2 Sxy / (N M), the unbiased
 *   estimate.  The kernel matrix is cut into 64 x 64 tiles, t = (row tile) * (column tiles) + (column tile); G = min(tiles,
 *   1024) blocks take the tiles b, b + G, ... and add their sums in that order; the G partials are added in ascending b.
 *   itcv_poly_mmd_workspace = 3 * 1024 * sizeof(double).  Supported: 2 <= N, M <= 2^20, 1 <= D <= 2048, gamma >= 0.
 * Frechet distance.  m1, m2 [D] and c1, c2 [D][D] fp64 as itcv_unsup_cov writes them, eps >= 0; with A = c1 + eps I and
 *   B = c2 + eps I:  L = the Cholesky factor of A (the rules of itcv_unsup_gauss; a failed pivot sets info[0] and info[1],
 *   the results are then nan);  T = B L, T[i][j] = sum_{k = j}^{D-1} B[i][k] L[k][j];  M[i][j] = sum_{k = i}^{D-1} L[k][i]
 *   T[k][j] for i <= j, mirrored (both sums ascending);  lambda = the eigenvalues of M by the cyclic Jacobi rules of
 *   itcv_unsup_gauss, on M itself (stop at off(M)_F <= 1e-14 |M|_F, 60 sweeps at most).  M is similar to A B, so
 *   tr sqrt(A B) = sum_i sqrt(max(lambda_i, 0)) in index order.  Only A has to be positive definite.
 *   res[5] = {fd, |m1 - m2|^2, tr A, tr B, tr sqrt}, fd = ((|m1 - m2|^2 + tr A) + tr B) - 2 tr sqrt (the traces include
 *   eps, so equal inputs give 0 up to rounding); eig[D] = lambda in index order; info[5] = {pivot failed, its dimension
 *   (-1), Jacobi did not converge, sweeps taken, number of lambda < 0 clipped}.  One block; the matrix sits in LDS up to
 *   D = itcv_unsup_gauss_lds_dim(), above that in the workspace (itcv_frechet_workspace).  Supported: 1 <= D <= 512.
 * Anything unsupported, a null operand or a short workspace returns non-zero before a launch; the workspace queries
 * return 0 for it. */
size_t itcv_knn_radius_workspace(int N, int D, int k, int splits);
int itcv_knn_radius(const float* x, size_t ld, int N, int D, int k, int splits, double* r2, int* flags, void* ws,
                    size_t ws_bytes, void* stream);
int itcv_prdc_counts(const float* real, size_t ldr, const float* fake, size_t ldf, int N, int M, int D,
                     const double* r2_real, const double* r2_fake, int splits, int* fake_hits, int* real_covered,
                     double* real_min, int* flags, void* stream);
size_t itcv_poly_mmd_workspace(int N, int M, int D);
int itcv_poly_mmd(const float* x, size_t ldx, const float* y, size_t ldy, int N, int M, int D, int degree, double gamma,
                  double coef0, double* res, int* flags, void* ws, size_t ws_bytes, void* stream);
size_t itcv_frechet_workspace(int D);
int itcv_frechet(const double* m1, const double* c1, const double* m2, const double* c2, int D, double eps, double* res,
                 double* eig, int* info, void* ws, size_t ws_bytes, void* stream);

/* ---- ex-post latent density: full-covariance Gaussian mixture (not in the reference; Ghosh et al. 2020) ----------- */
/* The EM rules of sklearn.mixture.GaussianMixture(covariance_type="full") over rows x[N][D] (fp32, row stride ld elements,
 * read in place; nothing left of a strided view is read).  Fixed rules; all arithmetic is fp64, every operation rounded on
 * its own (no fused multiply-add outside the matrix cores), every floating-point sum in a fixed order that depends on the
 * shapes alone, no floating-point atomic: same inputs, same bits.  flags[2] as for itcv_disent_*: [0] a non-finite x (the
 * outputs are then unspecified), [1] a component number outside [0, K) (the sampler).  w[K], mean[K][D], cov / chol / linv
 * [K][D][D], logdet[K], nk[K] are fp64 and dense.
 * Factor.  chol holds C_k on entry and L_k on return, C_k = L_k L_k^T by the right-looking loop of itcv_unsup_gauss, the
 *   upper triangle zero; linv = L_k^-1 by forward substitution (X = I; for k ascending: row k / L[k][k], then X[i][j] -=
 *   L[i][k] X[k][j] for i > k, j <= k); logdet[k] = 2 sum_i log L[i][i], ascending.  info[k] = 0, or 1 + the dimension of the
 *   first pivot that is <= 0 or non-finite (chol, linv and logdet of that component are then nan).  One block per
 *   component; the matrix sits in LDS up to D = itcv_unsup_gauss_lds_dim(), above that the block works in chol itself.
 * E-step.  y = linv_k (x_n - mean_k) on v_mfma_f64_16x16x4_f64 from the widened, centred values (the 16 x 16 tiles of linv_k
 *   above its diagonal are skipped, elements above the diagonal enter as zeros); q = sum_i y_i^2 in ascending i;
 *     lp[n][k] = log w[k] - ((D log 2 pi + logdet[k]) + q) / 2.
 *   Then per row, with m = max_k lp[n][k]: lse = m + log sum_k exp(lp[n][k] - m) (ascending k), resp[n][k] = exp(lp[n][k] -
 *   lse), loglik[n] = lse.  hard != 0: resp[n] is the one-hot of the largest lp[n][k] (ties to the lowest k) and loglik[n]
 *   that value.  sum_loglik[0] = the sums of loglik over blocks of 256 rows, added in block order.  w need not sum to one.
 * M-step.  nk[k] = sum_n resp[n][k] + 10 DBL_EPSILON;  w[k] = nk[k] / sum_k nk[k];  mean[k][d] = (sum_n resp[n][k] x[n][d]) /
 *   nk[k];  cov[k][i][j] = (sum_n resp[n][k] (x[n][i] - mean[k][i]) (x[n][j] - mean[k][j])) / nk[k], + reg on the diagonal:
 *   two passes over centred values, the products on the f64 matrix cores.  The sums over n follow itcv_unsup_cov: slices
 *   whose length is a function of N alone, folded in ascending order; one triangle is computed and mirrored.  with_cov == 0
 *   stops after the means (cov may be null): the centre update of Lloyd's iteration.
 * Sampler.  z[r][i] = (float)(mean[c][i] + sum_{j <= i} chol[c][i][j] eps[r][j]), c = comp[r] (int32), eps[R][D] and
 *   z[R][D] fp32 dense, the sum in ascending j; a row whose c is outside [0, K) is not written and sets flags[1].
 * Supported: 1 <= K <= 64, 1 <= D <= 512, K <= N <= 2^24, 1 <= R <= 2^24, reg >= 0.  Anything unsupported, a null operand
 * or a short workspace returns non-zero before a launch; the workspace queries return 0 for it. */
int itcv_gmm_factor(double* chol, int K, int D, double* linv, double* logdet, int* info, void* stream);
size_t itcv_gmm_estep_workspace(int N, int D, int K);
int itcv_gmm_estep(const float* x, size_t ld, int N, int D, int K, const double* w, const double* mean, const double* linv,
                   const double* logdet, int hard, double* lp, double* resp, double* loglik, double* sum_loglik,
                   int* flags, void* ws, size_t ws_bytes, void* stream);
size_t itcv_gmm_mstep_workspace(int N, int D, int K, int with_cov);
int itcv_gmm_mstep(const float* x, size_t ld, const double* resp, int N, int D, int K, double reg, int with_cov,
                   double* nk, double* w, double* mean, double* cov, int* flags, void* ws, size_t ws_bytes,
                   void* stream);
int itcv_gmm_sample(const double* mean, const double* chol, const int* comp, const float* eps, int R, int D, int K,
                    float* z, int* flags, void* stream);

/* ---- reconstruction loss (ops.py:188-236) --------------------------------------------- */
#define ITCV_LOSS_MSE 0
#define ITCV_LOSS_L1 1
#define ITCV_LOSS_BCE 2
/* rows[b] = sum_p err(recon[b][p], x[b][p]) */
int itcv_recon_rows_fwd(const float* x, const float* recon, float* rows, int B, size_t P, int loss_type,
                        void* ws, size_t ws_bytes, void* stream);
size_t itcv_recon_workspace(int B, size_t P);
/* drecon[b][p] = g[b] * d err / d recon */
int itcv_recon_rows_bwd(const float* x, const float* recon, const float* g, float* drecon, int B, size_t P,
                        int loss_type, void* stream);

/* The whole of ops.reconstruction_loss plus the hook's `beta *` (ops.py:219-236, solvers/vae.py:79-87) in two launches:
 * reduction 0 none: out[B] = scale * rows; 1 sum / 2 mean: out[1] = scale * sum_b rows [/ B].  _bwd: drecon for the
 * gradient g of out ([B] for none, [1] else).  Workspace: itcv_recon_workspace. */
int itcv_recon_loss_fwd(const float* x, const float* recon, float* out, int B, size_t P, int loss_type, int reduction,
                        float scale, void* ws, size_t ws_bytes, void* stream);
int itcv_recon_loss_bwd(const float* x, const float* recon, const float* g, float* drecon, int B, size_t P,
                        int loss_type, int reduction, float scale, void* stream);
/* ---- structural similarity: a reconstruction loss and the PSNR / SSIM / MS-SSIM scores (not in the reference) ---- */
/* SSIM (Wang et al. 2004) of y (reconstruction) against x (target, a constant), both dense fp32 [B][C][H][W].  `window`
 * is K doubles in device memory, the 1-D taps g (made on the host in fp64, sum 1); the 2-D window is g (x) g, applied per
 * channel with valid filtering: H' x W' = (H - K + 1) x (W - K + 1) positions.  C1 = 0.01^2, C2 = 0.03^2 (L = 1).  With
 * w* the windowed sum, at every position
 *     mx = w*x, my = w*y, ex2 = w*x^2, ey2 = w*y^2, exy = w*xy;   sx = ex2 - mx^2, sy = ey2 - my^2, sxy = exy - mx my;
 *     A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = (mx^2 + my^2) + C1, B2 = (sx + sy) + C2;
 *     S = (A1 A2) / (B1 B2),  cs = A2 / B2            (no clamp anywhere)
 * and SSIM_b is the mean of S over the n = C H' W' positions of image b.  With P = C H W:
 *     rows[b] = (P alpha) (1 - SSIM_b) + (1 - alpha) sum_p |y_bp - x_bp|,     0 <= alpha <= 1,
 * the units of the other reconstruction losses (a sum over P elements).  reduction 0 (none): out[B] = scale * rows;
 * 1 (sum) / 2 (mean): out[1] = scale * sum_b rows [/ B]; the arithmetic is fp64 up to ONE rounding to fp32 at the end.
 * _bwd: for the gradient g of out ([B] for none, [1] else), gb = g scale [/ B],
 *     dy = -gb (P alpha / n) [ Wt(dS/dmy) + 2 y Wt(dS/dey2) + x Wt(dS/dexy) ] + gb (1 - alpha) sign(y - x),
 *     dS/dmy = 2 mx (A2 - A1) / (B1 B2) + 2 my S (1 / B2 - 1 / B1),  dS/dey2 = -S / B2,  dS/dexy = 2 A1 / (B1 B2),
 * Wt the full correlation of a map on H' x W' back onto H x W (the adjoint of valid filtering), sign(0) = 0.
 * _stats: stats[B][C][2] fp64 = the mean of S and the mean of cs over the H' W' positions of every plane.
 * Everything is fp64 from the widened inputs (x^2 and xy are exact there), every operation rounded on its own, every sum
 * in a fixed order that depends on the shapes alone (taps ascending, rows of the window outside columns), no atomic: same
 * inputs, same bits, and a plane's numbers do not depend on B or on where the plane sits in the batch.  The forward and
 * the statistics are two launches (16 x 16 tiles of positions with their halo in LDS, one fp64 partial per tile and sum;
 * a finish) and write nothing of image size; the backward is one launch that recomputes the moments.
 * itcv_ssim_workspace = 3 * B * C * ceil(H' / 16) * ceil(W' / 16) * sizeof(double).
 * Supported: K odd, 3 <= K <= 15; K <= H, W <= 4096; B * C <= 2^20; B * C * ceil(H / 16) * ceil(W / 16) <= 2^30;
 * 0 <= alpha <= 1.  Anything else, a null operand or a short workspace returns non-zero before a launch; the workspace
 * query returns 0 for it. */
size_t itcv_ssim_workspace(int B, int C, int H, int W, int K);
int itcv_ssim_loss_fwd(const float* x, const float* y, const double* window, float* out, int B, int C, int H, int W, int K,
                       double alpha, int reduction, float scale, void* ws, size_t ws_bytes, void* stream);
int itcv_ssim_loss_bwd(const float* x, const float* y, const double* window, const float* g, float* dy, int B, int C, int H,
                       int W, int K, double alpha, int reduction, float scale, void* stream);
int itcv_ssim_stats(const float* x, const float* y, const double* window, double* stats, int B, int C, int H, int W, int K,
                    void* ws, size_t ws_bytes, void* stream);

/* solvers/intro.py:102-103: out[0] = mean_j exp(c * (a[j] + b[j])) (c = -2 * scale); w[B] is kept for _bwd, which
 * writes da[j] = db[j] = g[0] * d out / d a[j] (db may be NULL). */
int itcv_exp_elbo_fwd(const float* a, const float* b, float* out, float* w, int B, float c, void* stream);
int itcv_exp_elbo_bwd(const float* g, const float* w, float* da, float* db, int B, void* stream);
/* out[0] = sum_k weights[k] * terms[k][0], n <= 8 device scalars (solvers/intro.py:105-108,149-151, solvers/vae.py:106:
 * the scalar arithmetic of a loss in one launch); _bwd: grads[k] = g[0] * weights[k].  `terms` / `weights` are HOST arrays. */
int itcv_lincomb_fwd(const float* const* terms, const float* weights, int n, float* out, void* stream);
int itcv_lincomb_bwd(const float* g, const float* weights, int n, float* grads, void* stream);

/* ---- optimiser (train.py:141-144, solvers/intro.py:109-116,153-160) --------------------- */
/* out[0] = sum x^2 (fp64, deterministic) */
size_t itcv_sumsq_workspace(size_t n);
int itcv_sumsq(const float* x, size_t n, double* out, void* ws, size_t ws_bytes, void* stream);
/* torch.nn.utils.clip_grad_norm_: total = sqrt(sum_k sumsq[k]); coef = min(1, clip/(total+1e-6));
 * writes norm_out[0] = total, coef_out[0] = coef (device scalars, no host sync) */
int itcv_clip_coef(const double* sumsq, int nparts, double clip, float* norm_out, float* coef_out,
                   void* stream);
int itcv_scale_by_dev(float* x, size_t n, const float* coef_dev, void* stream);
/* torch.optim.Adam defaults (no amsgrad / weight decay), one flat launch; step is 1-based */
int itcv_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                   float beta2, float eps, int step, void* stream);
/* same update with the 0-based count of completed steps read from (and incremented in) device
 * memory, so that a captured launch (hipGraph replay) advances the bias correction */
int itcv_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1,
                       float beta2, float eps, int* step_dev, void* stream);
/* Fused torch.optim updates (train.py:140-144 picks the class from the run config) over one flat fp32 buffer of n
 * elements (n % 4 == 0, every pointer 16-byte aligned): the single-tensor arithmetic of torch/optim/{adam,sgd,adagrad,
 * rmsprop}.py in torch's order.  Each reads the 0-based count of completed steps from step_dev (bias corrections,
 * Adagrad's lr decay, SGD's first-step momentum buffer) and increments it, so captured launches advance it.
 * `live` (may be NULL) holds one byte per 4 elements: 0 marks elements of a parameter that never receives a gradient
 * (torch skips such a parameter: no weight decay, no state); those elements of p and of every state buffer are left
 * untouched.  Hyper-parameters are the Python floats of the param group; flags are ITCV_OPT_* bits. */
#define ITCV_OPT_MAXIMIZE 0x1
#define ITCV_OPT_NESTEROV 0x2     /* SGD */
#define ITCV_OPT_AMSGRAD 0x4      /* Adam */
#define ITCV_OPT_DECOUPLED_WD 0x8 /* Adam: AdamW / decoupled_weight_decay=True */
#define ITCV_OPT_CENTERED 0x10    /* RMSprop */
/* Adam / AdamW with weight decay, amsgrad (max_exp_avg_sq, else may be NULL) and/or maximize */
int itcv_adamx_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                        const unsigned char* live, size_t n, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int flags, int* step_dev, void* stream);
/* SGD; momentum_buffer may be NULL when momentum == 0 (on the first step it becomes a copy of the gradient) */
int itcv_sgd_step_dev(float* p, const float* g, float* momentum_buffer, const unsigned char* live, size_t n, double lr,
                      double momentum, double dampening, double weight_decay, int flags, int* step_dev, void* stream);
/* Adagrad: clr = lr / (1 + (step - 1) * lr_decay); `sum` starts at initial_accumulator_value (set by the caller) */
int itcv_adagrad_step_dev(float* p, const float* g, float* sum, const unsigned char* live, size_t n, double lr,
                          double lr_decay, double weight_decay, double eps, int flags, int* step_dev, void* stream);
/* RMSprop; momentum_buffer only when momentum > 0, grad_avg only when ITCV_OPT_CENTERED (else may be NULL) */
int itcv_rmsprop_step_dev(float* p, const float* g, float* square_avg, float* momentum_buffer, float* grad_avg,
                          const unsigned char* live, size_t n, double lr, double alpha, double eps,
                          double weight_decay, double momentum, int flags, int* step_dev, void* stream);
int itcv_fill(float* x, size_t n, float value, void* stream);
/* Input pipeline (dataset.py:219-224 transforms.RandomHorizontalFlip, moved behind the host -> device copy):
 * y[b] = x[b] mirrored along W where flip[b] != 0, else x[b]; x, y are [B][rows_per_image][W] (rows = C*H), x != y. */
int itcv_hflip(const float* x, float* y, const unsigned char* flip, int B, int rows_per_image, int W, void* stream);
/* Device-resident image tables (dataset.py:75-81,141-147: Image.fromarray + ToTensor of one stored uint8 image, for n
 * images in one launch).  table is planar [num_images][rows_per_image = C*H][W] uint8; out is n dense fp32 images
 * [n][rows_per_image][W] (the caller offsets out itself to land inside a larger buffer).
 *   out[j][r][w] = (float)table[idx[j]][r][w'] / 255.0f,   w' = W-1-w where flip != NULL and flip[j] != 0, else w
 * with the IEEE correctly rounded fp32 division -- torchvision's ToTensor (.float().div(255)) bit for bit; a product with
 * 1/255.f differs from it for 126 of the 256 byte values and is not used.  An idx[j] outside [0, num_images) writes image
 * j of out as zeros, reads nothing from the table and ORs bit 0 into flags[0] (int, device memory, cleared by the caller).
 * Every address is formed in 64 bits (tables are several GB); one image holds fewer than 2^31 bytes.  W % 16 == 0 with
 * table and out 16-byte aligned takes 16-byte loads and stores, every other shape a scalar form with the same results.
 * Asynchronous on stream; allocates nothing. */
int itcv_gather_u8(const unsigned char* table, long long num_images, int rows_per_image, int W, const long long* idx,
                   int n, const unsigned char* flip, float* out, int* flags, void* stream);
/* Pillow's 8-bit bicubic resize (dataset.py:78-79,144-145 and load_image: Image.resize(..., Image.BICUBIC) per sample)
 * of n images of a planar uint8 table [num_images][planes][Hin][Win], bit for bit.  idx as in itcv_gather_u8, or NULL
 * for images 0..n-1 (n <= num_images).  out is planar [n][planes][Hout][Wout]: uint8, or fp32 byte / 255.0f (correctly
 * rounded, as itcv_gather_u8) when out_is_f32; image j is written with its columns reversed where flip != NULL and
 * flip[j] != 0 (the resize of the unmirrored source, mirrored afterwards).
 * An axis is described by its plan, made on the host in fp64 as Pillow makes it (hipvae/resize.py bicubic_plan):
 * bounds [out][2] = {first source index, tap count <= k}, coef [out][k] int32 in units of 2^-22, in device memory.  One
 * pass computes  clamp((2^21 + sum_t src[first + t] * coef[t]) >> 22, 0, 255)  in int32 (arithmetic shift); the
 * horizontal pass runs first and rounds to uint8, the vertical pass runs on its result.  An axis whose size does not
 * change has NULL bounds and coef (k ignored) and gets no pass -- Pillow skips it too.  Both NULL is a copy and is
 * legal for uint8 output only (the fp32 form of that is itcv_gather_u8).  sum |coef| of a row must stay below
 * (2^31 - 2^21) / 255 (the plan builder checks it), so int32 cannot overflow.
 * An idx[j] outside [0, num_images) writes image j as zeros and ORs bit 0 into flags[0], as itcv_gather_u8 does; a plan
 * whose row windows do not fit the image ORs bit 1, reads nothing and writes zeros.  Window starts and counts are
 * clamped to the source row, so no plan makes the kernel read outside the table.
 * Asynchronous on stream; allocates nothing. */
int itcv_resize_u8(const unsigned char* table, long long num_images, int planes, int Hin, int Win, const long long* idx,
                   int n, const unsigned char* flip, const int* xbounds, const int* xcoef, int kx, const int* ybounds,
                   const int* ycoef, int ky, int Hout, int Wout, void* out, int out_is_f32, int* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ITCV_HIP_H */
