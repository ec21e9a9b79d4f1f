// The label regulariser of the semi-supervised S2 objectives (Locatello et al. 2020, "Disentangling Factors of Variation
// Using Few Labels"; disentanglement_lib's `semi_supervised_vae`: supervised_regularizer_xent / _l2 / _cov) with its
// gradient.  The rules are in include/itcv_hip.h:
//   sup_rows     : forms xent and l2.  ONE wave per labelled row, four rows per 256-thread block, the blocks stride over the
//                  rows.  Lane f < F holds the one term of factor f in fp64 from the fp32 inputs; one wave reduction gives
//                  the row's partial.
//   sup_cov_tile : form cov.  C = X^T Y / B (X, Y = mu, y minus their column means) is [D, F] and tiled kSupTile x kSupTile
//                  over a 2-D grid.  A block first re-derives the fp64 column means of its strip of mu and its strip of y
//                  (four row classes per column, folded in a fixed order), then walks the rows in chunks of kSupRows: the
//                  centred values are staged in LDS as fp64 and every thread keeps a 2 x 2 patch of the tile in fp64
//                  registers.  The block writes its patch of W (C with W_ii = 0) TRANSPOSED, [F][D] fp64, so that the
//                  backward is a row-major product, the means of its y strip (the blocks of the first mu strip) and one
//                  fp64 partial, sum W_ij^2.
//   sup_finish   : ONE block adds the partials in index order (objective.h's ordered_sum), reads gamma -- from the device
//                  when a pointer is given -- and writes the scalar, the two logged terms and the gamma it used (the
//                  backward reads that copy, not the pointer again).
//   sup_rows_bwd / sup_cov_bwd : ONE launch.  xent and l2 need no reduction; cov is (2 / B) Y_c W^T in fp64 over LDS-staged
//                  chunks of kSupBwdK factors, a kSupBwdRows x kSupBwdCols tile of [B, D] per block.
// D up to 512 and F up to 64 are covered by the grid, never by one block's LDS.  Every sum has a fixed order, there is no
// atomic, and nothing depends on the grid or on timing: the same inputs give the same bits.  Nothing in this file may be
// contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kSupMaxD = 512;
constexpr int kSupMaxF = 64;              // one lane per factor
constexpr int kSupMaxB = 1 << 24;
constexpr int kSupThreads = 256;
constexpr int kSupRowsPerBlock = kSupThreads / kWave;
constexpr int kSupMaxBlocks = 256;        // 1024 rows a trip; the rest of the batch is walked by the stride
constexpr int kSupXent = 1, kSupL2 = 2, kSupCov = 3;
constexpr int kSupTile = 32;              // C is tiled 32 x 32: at most 16 x 2 tiles
constexpr int kSupRows = 64;              // rows of one staged chunk: 2 x 64 x 32 doubles = 32 KiB of LDS
constexpr int kSupBwdRows = 16;
constexpr int kSupBwdCols = 64;
constexpr int kSupBwdK = 32;

__global__ __launch_bounds__(kSupThreads) void sup_rows_kernel(const float* __restrict__ mu, size_t ldm,
                                                               const float* __restrict__ y, size_t ldy,
                                                               const int* __restrict__ sizes, int B, int F, int form,
                                                               double scale, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = blockIdx.x * kSupRowsPerBlock + w; b < B; b += gridDim.x * kSupRowsPerBlock) {   // wave-uniform
    double v = 0.0;
    if (lane < F) {
      const double m = mu[(size_t)b * ldm + lane], yy = y[(size_t)b * ldy + lane];
      if (form == kSupXent) {
        const double t = yy / (double)sizes[lane];
        v = ((m > 0.0 ? m : 0.0) - m * t) + log1p(exp(-fabs(m)));
      } else {
        const double d = scale * m - yy;
        v = d * d;
      }
    }
    v = wave_sum(v);
    if (lane == 0) part[b] = v;
  }
}

// out[0] = gamma * sup; terms[2] = {sup, gamma}; keep[0] = gamma, as read here
__global__ __launch_bounds__(kSupThreads) void sup_finish_kernel(const double* __restrict__ part, size_t n,
                                                                 const double* __restrict__ gamma_dev, double gamma,
                                                                 float* __restrict__ out, float* __restrict__ terms,
                                                                 double* __restrict__ keep) {
  __shared__ double red[kSupThreads];
  const double sup = ordered_sum<kSupThreads>(part, n, red);
  if (threadIdx.x == 0) {
    const double g = gamma_dev ? gamma_dev[0] : gamma;
    out[0] = (float)(g != 0.0 ? g * sup : 0.0);
    terms[0] = (float)sup;
    terms[1] = (float)g;
    keep[0] = g;
  }
}

__global__ __launch_bounds__(kSupThreads) void sup_rows_bwd_kernel(const float* __restrict__ g, const float* __restrict__ mu,
                                                                   size_t ldm, const float* __restrict__ y, size_t ldy,
                                                                   const int* __restrict__ sizes,
                                                                   const double* __restrict__ keep, int B, int D, int F,
                                                                   int form, double scale, float* __restrict__ dmu) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double gk = keep[0] != 0.0 ? (double)g[0] * keep[0] : 0.0;
  for (int b = blockIdx.x * kSupRowsPerBlock + w; b < B; b += gridDim.x * kSupRowsPerBlock) {
    for (int d = lane; d < D; d += 64) {
      float r = 0.f;                                   // columns >= F, and everything under gamma = 0: exactly zero
      if (d < F && gk != 0.0) {
        const double m = mu[(size_t)b * ldm + d], yy = y[(size_t)b * ldy + d];
        double dm;
        if (form == kSupXent) {
          const double e = exp(-fabs(m));
          const double sig = m >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
          dm = sig - yy / (double)sizes[d];
        } else {
          dm = 2.0 * scale * (scale * m - yy);
        }
        r = (float)(gk * dm);
      }
      dmu[(size_t)b * D + d] = r;
    }
  }
}

__global__ __launch_bounds__(kSupThreads) void sup_cov_tile_kernel(const float* __restrict__ mu, size_t ldm,
                                                                   const float* __restrict__ y, size_t ldy, int B, int D,
                                                                   int F, double* __restrict__ Wt,
                                                                   double* __restrict__ keep, double* __restrict__ part) {
  const int ti = blockIdx.y, tj = blockIdx.x;         // strip ti of mu's columns against strip tj of y's
  __shared__ double xa[kSupRows][kSupTile], yb[kSupRows][kSupTile];
  __shared__ double msum[4][2 * kSupTile];
  __shared__ double m[2 * kSupTile];                  // [0, 32): means of mu's strip; [32, 64): of y's strip
  __shared__ double red[kSupThreads / 64];
  const int tid = threadIdx.x;
  const double inv_b = 1.0 / (double)B;
  {
    // column sums over the row classes b = q, q + 4, ...
    const int c = tid & 63, q = tid >> 6;
    const bool second = c >= kSupTile;
    const int col = (second ? tj : ti) * kSupTile + (c & (kSupTile - 1));
    double s = 0.0;
    if (col < (second ? F : D)) {
      const float* src = (second ? y : mu) + col;
      const size_t ld = second ? ldy : ldm;
      for (int b = q; b < B; b += 4) s += (double)src[(size_t)b * ld];
    }
    msum[q][c] = s;
    __syncthreads();
    if (tid < 2 * kSupTile) {
      m[tid] = (((msum[0][tid] + msum[1][tid]) + msum[2][tid]) + msum[3][tid]) * inv_b;
      const int gc = tj * kSupTile + tid - kSupTile;
      if (ti == 0 && tid >= kSupTile && gc < F) keep[1 + gc] = m[tid];
    }
    __syncthreads();
  }
  // the 2 x 2 patch of this thread: columns 2 pi, 2 pi + 1 of mu's strip against columns 2 pj, 2 pj + 1 of y's strip
  const int pi = tid & 15, pj = tid >> 4;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int r0 = 0; r0 < B; r0 += kSupRows) {
    const int nr = min(kSupRows, B - r0);
#pragma unroll
    for (int u = 0; u < kSupRows * 2 * kSupTile / kSupThreads; ++u) {
      const int e = tid + u * kSupThreads;
      const int r = e >> 6, c = e & 63;
      const bool second = c >= kSupTile;
      const int col = (second ? tj : ti) * kSupTile + (c & (kSupTile - 1));
      double v = 0.0;
      if (r < nr && col < (second ? F : D))
        v = (double)(second ? y[(size_t)(r0 + r) * ldy + col] : mu[(size_t)(r0 + r) * ldm + col]) - m[c];
      if (second) yb[r][c - kSupTile] = v; else xa[r][c] = v;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const double a0 = xa[r][2 * pi], a1 = xa[r][2 * pi + 1];
      const double b0 = yb[r][2 * pj], b1 = yb[r][2 * pj + 1];
      acc[0][0] += a0 * b0;
      acc[0][1] += a0 * b1;
      acc[1][0] += a1 * b0;
      acc[1][1] += a1 * b1;
    }
    __syncthreads();
  }
  double sq = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gi = ti * kSupTile + 2 * pi + a, gj = tj * kSupTile + 2 * pj + b;
      if (gi < D && gj < F) {
        const double wv = gi == gj ? 0.0 : acc[a][b] * inv_b;
        sq += wv * wv;
        Wt[(size_t)gj * D + gi] = wv;
      }
    }
  }
  sq = block_sum(sq, red);
  if (tid == 0) part[ti * gridDim.x + tj] = sq;
}

__global__ __launch_bounds__(kSupThreads) void sup_cov_bwd_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                                  size_t ldy, const double* __restrict__ Wt,
                                                                  const double* __restrict__ keep, int B, int D, int F,
                                                                  float* __restrict__ dmu) {
  __shared__ double ys[kSupBwdRows][kSupBwdK];
  __shared__ double wsh[kSupBwdK][kSupBwdCols];
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
  const int r0 = blockIdx.x * kSupBwdRows, c0 = blockIdx.y * kSupBwdCols;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < F; k0 += kSupBwdK) {
    const int nk = min(kSupBwdK, F - k0);
#pragma unroll
    for (int u = 0; u < kSupBwdRows * kSupBwdK / kSupThreads; ++u) {
      const int e = tid + u * kSupThreads;
      const int r = e / kSupBwdK, k = e % kSupBwdK;
      const int row = r0 + r;
      ys[r][k] = (row < B && k < nk) ? (double)y[(size_t)row * ldy + k0 + k] - keep[1 + k0 + k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kSupBwdK * kSupBwdCols / kSupThreads; ++u) {
      const int e = tid + u * kSupThreads;
      const int k = e / kSupBwdCols, c = e % kSupBwdCols;
      wsh[k][c] = (k < nk && c0 + c < D) ? Wt[(size_t)(k0 + k) * D + c0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      const double wv = wsh[k][col];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] += ys[rg * 4 + a][k] * wv;
    }
    __syncthreads();
  }
  const int gj = c0 + col;
  if (gj >= D) return;
  const double gk = keep[0] != 0.0 ? (double)g[0] * keep[0] : 0.0;
  const double inv_b = 1.0 / (double)B;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = r0 + rg * 4 + a;
    if (row >= B) continue;
    dmu[(size_t)row * D + gj] = gk != 0.0 ? (float)(gk * (2.0 * inv_b * acc[a])) : 0.f;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline size_t sup_parts(int B, int D, int F, int form) {
  return form == kSupCov ? (size_t)cdiv(D, kSupTile) * cdiv(F, kSupTile) : (size_t)B;
}
static inline bool sup_shape_ok(int B, int D, int F, int form) {
  return B >= 1 && B <= kSupMaxB && D >= 1 && D <= kSupMaxD && F >= 1 && F <= kSupMaxF && F <= D && form >= kSupXent &&
         form <= kSupCov;
}

// nothing is launched on a failure
static int sup_check(const char* name, bool ptrs, int B, int D, int F, int form, int min_size, bool gamma_ok, double scale,
                     size_t ld_mu, size_t ld_y) {
  if (need_pointers(name, ptrs) || need_dim(name, "B_l = %lld labelled rows", B, 1, kSupMaxB, "1..2^24") ||
      need_dim(name, "D = %lld", D, 1, kSupMaxD, "1..512") || need_dim(name, "F = %lld factors", F, 1, kSupMaxF, "1..64"))
    return 1;
  if (F > D) return fail("%s: F = %lld factors exceed the D = %lld latent dimensions", name, F, D);
  if (form != kSupXent && form != kSupL2 && form != kSupCov) return fail("%s: form %lld is not 1 (xent), 2 (l2) or 3 (cov)", name, form);
  if (form == kSupXent && min_size < 1) return fail("%s: xent needs every factor size >= 1 (got %lld)", name, min_size);
  if (!gamma_ok) return fail("%s: gamma must be a finite number", name);
  if (!finite(scale)) return fail("%s: scale must be a finite number", name);
  return need_stride(name, "mu's", ld_mu, "D", D) || need_stride(name, "y's", ld_y, "F", F);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_sup_workspace(int B, int D, int F, int form) {
  return sup_shape_ok(B, D, F, form) ? sup_parts(B, D, F, form) * sizeof(double) : 0;
}

int itcv_sup_fwd(const float* mu, size_t ld_mu, const float* y, size_t ld_y, const int* sizes, int min_size,
                 const double* gamma_dev, double gamma, double scale, float* out, float* terms, double* Wt, double* keep,
                 void* ws, size_t ws_bytes, int B, int D, int F, int form, void* stream) {
  const char* name = "itcv_sup_fwd";
  const bool ptrs = mu && y && out && terms && keep && (form != kSupXent || sizes) && (form != kSupCov || Wt);
  if (int e = sup_check(name, ptrs, B, D, F, form, min_size, gamma_dev || itcv::finite(gamma), scale, ld_mu, ld_y))
    return e;
  const size_t n = sup_parts(B, D, F, form);
  ITCV_REQUIRE(ws && ws_bytes >= n * sizeof(double), "itcv_sup_fwd(workspace)");
  double* part = static_cast<double*>(ws);
  hipStream_t st = S(stream);
  if (form == kSupCov) {
    hipLaunchKernelGGL(sup_cov_tile_kernel, dim3(cdiv(F, kSupTile), cdiv(D, kSupTile)), dim3(kSupThreads), 0, st, mu, ld_mu,
                       y, ld_y, B, D, F, Wt, keep, part);
    ITCV_CHECK_LAUNCH("itcv_sup_fwd(tiles)");
  } else {
    const dim3 grid(row_grid(B, kSupRowsPerBlock, kSupMaxBlocks));
    hipLaunchKernelGGL(sup_rows_kernel, grid, dim3(kSupThreads), 0, st, mu, ld_mu, y, ld_y, sizes, B, F, form, scale, part);
    ITCV_CHECK_LAUNCH("itcv_sup_fwd(rows)");
  }
  hipLaunchKernelGGL(sup_finish_kernel, dim3(1), dim3(kSupThreads), 0, st, (const double*)part, n, gamma_dev, gamma, out,
                     terms, keep);
  ITCV_CHECK_LAUNCH("itcv_sup_fwd(finish)");
  return 0;
}

int itcv_sup_bwd(const float* g, const float* mu, size_t ld_mu, const float* y, size_t ld_y, const int* sizes, int min_size,
                 double scale, const double* Wt, const double* keep, float* dmu, int B, int D, int F, int form,
                 void* stream) {
  const char* name = "itcv_sup_bwd";
  const bool ptrs = g && mu && y && keep && dmu && (form != kSupXent || sizes) && (form != kSupCov || Wt);
  if (int e = sup_check(name, ptrs, B, D, F, form, min_size, true, scale, ld_mu, ld_y)) return e;
  hipStream_t st = S(stream);
  if (form == kSupCov)
    hipLaunchKernelGGL(sup_cov_bwd_kernel, dim3(cdiv(B, kSupBwdRows), cdiv(D, kSupBwdCols)), dim3(kSupThreads), 0, st, g, y,
                       ld_y, Wt, keep, B, D, F, dmu);
  else
    hipLaunchKernelGGL(sup_rows_bwd_kernel, dim3(row_grid(B, kSupRowsPerBlock, kSupMaxBlocks)), dim3(kSupThreads), 0, st, g,
                       mu, ld_mu, y, ld_y, sizes, keep, B, D, F, form, scale, dmu);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
