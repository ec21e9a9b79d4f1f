// Structural similarity (Wang et al. 2004) as a reconstruction loss, its gradient, and the per-channel means the
// PSNR / SSIM / MS-SSIM scores are built from.  The rules are in include/itcv_hip.h.  x (target) and y (reconstruction)
// are dense fp32 [B][C][H][W]; the window g has K taps (K doubles in device memory, made on the host); the map has
// H' x W' = (H - K + 1) x (W - K + 1) positions ("valid" filtering).  All arithmetic is fp64 from the widened inputs:
//   tile  : a block of 256 threads owns a 16 x 16 tile of positions of one plane.  It stages the (16 + K - 1)^2 halo of
//           x and y in LDS, runs the horizontal pass of the five moments (w*x, w*y, w*x^2, w*y^2, w*xy) into LDS, then
//           the vertical pass, one position a thread, evaluates S and cs there and leaves three fp64 partials: sum S,
//           sum cs, and sum |y - x| over the pixels the tile owns (every pixel belongs to exactly one tile: the last
//           tile of a row or column also owns the K - 1 pixels behind it);
//   finish: one wave per image (loss) or per plane (statistics) folds the partials in tile order;
//   bwd   : a block owns a 16 x 16 tile of PIXELS.  It stages the (16 + 2K - 2)^2 footprint, recomputes the moments on
//           the (16 + K - 1)^2 ring of positions that reach the tile, forms dS/d(mu_y), dS/d(ey2), dS/d(exy) there (zero
//           outside the map) and filters the three maps back with the same two passes: the adjoint of valid filtering.
// Every tap sum runs in ascending tap order, s = s + g[k] * v, each operation rounded on its own; block sums are the xor
// butterfly and the wave totals in wave order; there is no atomic.  A plane's numbers depend on that plane alone.
// Nothing in this file may be contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kSsimTile = 16;
constexpr int kSsimThreads = kSsimTile * kSsimTile;
constexpr int kSsimMinK = 3, kSsimMaxK = 15;
constexpr int kSsimMaxSide = 4096;
constexpr int kSsimMaxPlanes = 1 << 20;
constexpr long long kSsimMaxBlocks = 1LL << 30;
constexpr int kSsimHalo = kSsimTile + kSsimMaxK - 1;          // 30: the forward's LDS is sized for K = 15
constexpr double kSsimC1 = 0.01 * 0.01, kSsimC2 = 0.03 * 0.03;
constexpr int kSsimFinishThreads = 1024;

struct SsimPoint {
  double S, cs, A1, A2, B1, B2, mx, my;
};
// S and cs at one position from its five moments
__device__ __forceinline__ SsimPoint ssim_point(double mx, double my, double ex2, double ey2, double exy) {
  SsimPoint p;
  const double mxx = mx * mx, myy = my * my, mxy = mx * my;
  const double sx = ex2 - mxx, sy = ey2 - myy, sxy = exy - mxy;
  p.A1 = 2.0 * mxy + kSsimC1;
  p.A2 = 2.0 * sxy + kSsimC2;
  p.B1 = (mxx + myy) + kSsimC1;
  p.B2 = (sx + sy) + kSsimC2;
  p.S = (p.A1 * p.A2) / (p.B1 * p.B2);
  p.cs = p.A2 / p.B2;
  p.mx = mx, p.my = my;
  return p;
}

// the five tap sums along a row of LDS floats: out[m] = sum_k g[k] * moment_m(xs[k], ys[k]), ascending k
__device__ __forceinline__ void ssim_row_taps(const float* __restrict__ xs, const float* __restrict__ ys,
                                              const double* __restrict__ g, int K, double (&out)[5]) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
  for (int k = 0; k < K; ++k) {
    const double w = g[k], xv = (double)xs[k], yv = (double)ys[k];
    a0 = a0 + w * xv;
    a1 = a1 + w * yv;
    a2 = a2 + w * (xv * xv);
    a3 = a3 + w * (yv * yv);
    a4 = a4 + w * (xv * yv);
  }
  out[0] = a0, out[1] = a1, out[2] = a2, out[3] = a3, out[4] = a4;
}

// part[3][planes * nt]: plane-major, tile t = (tile row) * ntw + (tile column)
__global__ __launch_bounds__(kSsimThreads) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const double* __restrict__ win, double* __restrict__ part,
                                                                 int H, int W, int K, int nth, int ntw, size_t nparts) {
  __shared__ float sx[kSsimHalo][kSsimHalo];
  __shared__ float sy[kSsimHalo][kSsimHalo];
  __shared__ double sh[5][kSsimHalo][kSsimTile];
  __shared__ double sg[kSsimMaxK + 1];
  __shared__ double red[kSsimThreads / 64];
  const int tid = threadIdx.x, tx = tid & (kSsimTile - 1), ty = tid >> 4;
  const int nt = nth * ntw;
  const size_t blk = blockIdx.x;
  const size_t plane = blk / nt;
  const int t = (int)(blk - plane * nt), ti = t / ntw, tj = t - ti * ntw;
  const int r0 = ti * kSsimTile, c0 = tj * kSsimTile;
  const int HB = kSsimTile + K - 1;
  const int Hp = H - K + 1, Wp = W - K + 1;
  const float* xp = x + plane * ((size_t)H * W);
  const float* yp = y + plane * ((size_t)H * W);
  if (tid < K) sg[tid] = win[tid];
  // pixels this tile owns: its 16 rows / columns, and everything behind them for the last tile of the axis
  const int own_r = ti == nth - 1 ? H - r0 : kSsimTile, own_c = tj == ntw - 1 ? W - c0 : kSsimTile;
  double l1 = 0.0;
  for (int e = tid; e < HB * HB; e += kSsimThreads) {
    const int r = e / HB, c = e - r * HB;
    float xv = 0.f, yv = 0.f;
    if (r0 + r < H && c0 + c < W) {
      const size_t o = (size_t)(r0 + r) * W + (c0 + c);
      xv = xp[o], yv = yp[o];
      if (r < own_r && c < own_c) l1 = l1 + fabs((double)yv - (double)xv);
    }
    sx[r][c] = xv, sy[r][c] = yv;
  }
  __syncthreads();
  for (int e = tid; e < HB * kSsimTile; e += kSsimThreads) {
    const int r = e >> 4, j = e & (kSsimTile - 1);
    double m[5];
    ssim_row_taps(&sx[r][j], &sy[r][j], sg, K, m);
#pragma unroll
    for (int q = 0; q < 5; ++q) sh[q][r][j] = m[q];
  }
  __syncthreads();
  double S = 0.0, cs = 0.0;
  if (r0 + ty < Hp && c0 + tx < Wp) {
    double m[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s = s + sg[k] * sh[q][ty + k][tx];
      m[q] = s;
    }
    const SsimPoint p = ssim_point(m[0], m[1], m[2], m[3], m[4]);
    S = p.S, cs = p.cs;
  }
  S = block_sum(S, red);
  cs = block_sum(cs, red);
  l1 = block_sum(l1, red);
  if (tid == 0) part[blk] = S, part[nparts + blk] = cs, part[2 * nparts + blk] = l1;
}

// a[0] + ... + a[n - 1] by one wave: lane l folds the run [l * per, (l + 1) * per) in order, the xor butterfly the 64 runs
__device__ __forceinline__ double ssim_wave_fold(const double* __restrict__ a, int n) {
  const int lane = threadIdx.x & 63, per = (n + 63) / 64;
  const int lo = lane * per, hi = lo + per < n ? lo + per : n;
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s = s + a[i];
  return wave_sum(s);
}

// One block.  Wave w takes the images w, w + 16, ...: rows[b] = P alpha (1 - sum S / n) + (1 - alpha) sum |y - x| in
// fp64, then reduction 0: out[b] = (float)(scale rows[b]); 1 / 2: out[0] = (float)(scale sum_b rows[b] [/ B]), the rows
// of a wave added in ascending b, the 16 wave totals in wave order.  One rounding to fp32, at the end.
__global__ __launch_bounds__(kSsimFinishThreads) void ssim_loss_finish_kernel(const double* __restrict__ part, size_t nparts,
                                                                              float* __restrict__ out, int B, int per_image,
                                                                              double P, double n, double alpha,
                                                                              int reduction, float scale) {
  __shared__ double tot[kSsimFinishThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int b = w; b < B; b += kSsimFinishThreads / 64) {
    const double sS = ssim_wave_fold(part + (size_t)b * per_image, per_image);
    const double sL = ssim_wave_fold(part + 2 * nparts + (size_t)b * per_image, per_image);
    const double row = (P * alpha) * (1.0 - sS / n) + (1.0 - alpha) * sL;
    if (reduction == 0 && lane == 0) out[b] = (float)((double)scale * row);
    acc = acc + row;
  }
  if (reduction == 0) return;
  if (lane == 0) tot[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < kSsimFinishThreads / 64; ++k) s = s + tot[k];
    out[0] = (float)((double)scale * (reduction == 2 ? s / (double)B : s));
  }
}

// a wave per plane: stats[plane] = {sum S / n1, sum cs / n1}, n1 the positions of one plane
__global__ __launch_bounds__(256) void ssim_stats_finish_kernel(const double* __restrict__ part, size_t nparts,
                                                                double* __restrict__ stats, int planes, int nt, double n1) {
  const int lane = threadIdx.x & 63;
  const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (plane >= planes) return;
  const double sS = ssim_wave_fold(part + (size_t)plane * nt, nt);
  const double sC = ssim_wave_fold(part + nparts + (size_t)plane * nt, nt);
  if (lane == 0) stats[2 * (size_t)plane] = sS / n1, stats[2 * (size_t)plane + 1] = sC / n1;
}

// Dynamic LDS, for F = 16 + 2K - 2 and R = 16 + K - 1: floats fx[F][F], fy[F][F]; doubles h[5][F][R] (later hh[3][R][16]),
// coef[3][R][R], g[16].
__host__ __device__ inline size_t ssim_bwd_lds(int K) {
  const size_t F = kSsimTile + 2 * K - 2, R = kSsimTile + K - 1;
  const size_t fl = (2 * F * F * sizeof(float) + 7) & ~(size_t)7;
  return fl + (5 * F * R + 3 * R * R + 16) * sizeof(double);
}

// grid = planes * nth * ntw tiles of pixels.  coef_ssim[b] = -g P alpha / n, coef_l1 = g (1 - alpha), g the upstream
// gradient of image b's row times scale [/ B]
__global__ __launch_bounds__(kSsimThreads) void ssim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const double* __restrict__ win, const float* __restrict__ gup,
                                                                float* __restrict__ dy, int C, int H, int W, int K, int nth,
                                                                int ntw, double P, double n, double alpha, int reduction,
                                                                double coef) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ssim_lds[];
  const int F = kSsimTile + 2 * K - 2, R = kSsimTile + K - 1;
  float* fx = reinterpret_cast<float*>(ssim_lds);
  float* fy = fx + F * F;
  double* h = reinterpret_cast<double*>(ssim_lds + ((2 * (size_t)F * F * sizeof(float) + 7) & ~(size_t)7));
  double* cf = h + 5 * F * R;
  double* sg = cf + 3 * R * R;
  const int tid = threadIdx.x, tx = tid & (kSsimTile - 1), ty = tid >> 4;
  const int nt = nth * ntw;
  const size_t blk = blockIdx.x;
  const size_t plane = blk / nt;
  const int t = (int)(blk - plane * nt), ti = t / ntw, tj = t - ti * ntw;
  const int R0 = ti * kSsimTile, C0 = tj * kSsimTile;        // the tile's first pixel
  const int pr0 = R0 - (K - 1), pc0 = C0 - (K - 1);          // the ring's first position = the footprint's first pixel
  const int Hp = H - K + 1, Wp = W - K + 1;
  const float* xp = x + plane * ((size_t)H * W);
  const float* yp = y + plane * ((size_t)H * W);
  if (tid < K) sg[tid] = win[tid];
  for (int e = tid; e < F * F; e += kSsimThreads) {
    const int r = e / F, c = e - r * F;
    const int pr = pr0 + r, pc = pc0 + c;
    float xv = 0.f, yv = 0.f;
    if (pr >= 0 && pr < H && pc >= 0 && pc < W) {
      const size_t o = (size_t)pr * W + pc;
      xv = xp[o], yv = yp[o];
    }
    fx[e] = xv, fy[e] = yv;
  }
  __syncthreads();
  // horizontal pass: footprint rows x ring columns
  for (int e = tid; e < F * R; e += kSsimThreads) {
    const int r = e / R, j = e - r * R;
    double m[5];
    ssim_row_taps(fx + r * F + j, fy + r * F + j, sg, K, m);
#pragma unroll
    for (int q = 0; q < 5; ++q) h[(q * F + r) * R + j] = m[q];
  }
  __syncthreads();
  // vertical pass and the three coefficient maps on the ring
  for (int e = tid; e < R * R; e += kSsimThreads) {
    const int i = e / R, j = e - i * R;
    const int pr = pr0 + i, pc = pc0 + j;
    double ca = 0.0, cb = 0.0, cc = 0.0;
    if (pr >= 0 && pr < Hp && pc >= 0 && pc < Wp) {
      double m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s = s + sg[k] * h[(q * F + i + k) * R + j];
        m[q] = s;
      }
      const SsimPoint p = ssim_point(m[0], m[1], m[2], m[3], m[4]);
      const double b12 = p.B1 * p.B2;
      ca = (2.0 * p.mx) * (p.A2 - p.A1) / b12 + (2.0 * p.my) * p.S * (1.0 / p.B2 - 1.0 / p.B1);
      cb = -p.S / p.B2;
      cc = (2.0 * p.A1) / b12;
    }
    cf[e] = ca, cf[R * R + e] = cb, cf[2 * R * R + e] = cc;
  }
  __syncthreads();
  // the adjoint: pixel u receives g[u - p] coef[p]; ring row r, pixel column tx: taps at ring columns tx + K - 1 - k
  double* hh = h;
  for (int e = tid; e < R * kSsimTile; e += kSsimThreads) {
    const int r = e >> 4, j = e & (kSsimTile - 1);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double* row = cf + (q * R + r) * R + j + (K - 1);
      double s = 0.0;
      for (int k = 0; k < K; ++k) s = s + sg[k] * row[-k];
      hh[(q * R + r) * kSsimTile + j] = s;
    }
  }
  __syncthreads();
  const int ur = R0 + ty, uc = C0 + tx;
  if (ur >= H || uc >= W) return;
  double tq[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s = s + sg[k] * hh[(q * R + ty + (K - 1) - k) * kSsimTile + tx];
    tq[q] = s;
  }
  const size_t b = plane / C;
  const double g = (double)(reduction ? gup[0] : gup[b]) * coef;
  const int fo = (ty + K - 1) * F + (tx + K - 1);
  const double xv = (double)fx[fo], yv = (double)fy[fo];
  const double sgn = yv > xv ? 1.0 : (yv < xv ? -1.0 : 0.0);
  const double inner = (tq[0] + (2.0 * yv) * tq[1]) + xv * tq[2];
  const double ks = -(g * ((P * alpha) / n));
  dy[plane * ((size_t)H * W) + (size_t)ur * W + uc] = (float)(ks * inner + (g * (1.0 - alpha)) * sgn);
}

// ---- host side -------------------------------------------------------------------------------------------------------
struct SsimShape {
  int nth, ntw;          // tiles of positions (forward)
  int pth, ptw;          // tiles of pixels (backward)
  long long planes;
  size_t nparts;         // planes * nth * ntw
};
static int ssim_shape(const char* name, int B, int C, int H, int W, int K, SsimShape* s) {
  if (need_dim(name, "K = %lld taps", K, kSsimMinK, kSsimMaxK, "the odd numbers 3..15")) return 1;
  if (!(K & 1)) return fail("%s: K = %lld taps is outside the odd numbers 3..15", name, K);
  if (need_dim(name, "B = %lld images", B, 1, kSsimMaxPlanes, "1..2^20") ||
      need_dim(name, "C = %lld channels", C, 1, kSsimMaxPlanes, "1..2^20") ||
      need_dim(name, "B * C = %lld planes", (long long)B * C, 1, kSsimMaxPlanes, "1..2^20") ||
      need_dim(name, "H = %lld", H, K, kSsimMaxSide, "K..4096") || need_dim(name, "W = %lld", W, K, kSsimMaxSide, "K..4096"))
    return 1;
  s->planes = (long long)B * C;
  s->nth = cdiv(H - K + 1, kSsimTile), s->ntw = cdiv(W - K + 1, kSsimTile);
  s->pth = cdiv(H, kSsimTile), s->ptw = cdiv(W, kSsimTile);
  if (need_dim(name, "B * C * tiles = %lld blocks", s->planes * s->pth * s->ptw, 1, kSsimMaxBlocks, "1..2^30")) return 1;
  s->nparts = (size_t)s->planes * s->nth * s->ntw;
  return 0;
}
static int ssim_alpha(const char* name, double alpha) {
  return alpha >= 0.0 && alpha <= 1.0 ? 0 : fail("%s: alpha is outside 0..1", name);
}
static void ssim_launch_tiles(const float* x, const float* y, const double* window, double* part, int H, int W, int K,
                              const SsimShape& s, hipStream_t st) {
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)s.nparts), dim3(kSsimThreads), 0, st, x, y, window, part, H, W, K,
                     s.nth, s.ntw, s.nparts);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_ssim_workspace(int B, int C, int H, int W, int K) {
  if (K < kSsimMinK || K > kSsimMaxK || !(K & 1) || B < 1 || C < 1 || (long long)B * C > kSsimMaxPlanes || H < K ||
      W < K || H > kSsimMaxSide || W > kSsimMaxSide)
    return 0;
  const long long planes = (long long)B * C;
  if (planes * cdiv(H, kSsimTile) * cdiv(W, kSsimTile) > kSsimMaxBlocks) return 0;
  return (size_t)3 * planes * cdiv(H - K + 1, kSsimTile) * cdiv(W - K + 1, kSsimTile) * sizeof(double);
}

int itcv_ssim_loss_fwd(const float* x, const float* y, const double* window, float* out, int B, int C, int H, int W, int K,
                       double alpha, int reduction, float scale, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_ssim_loss_fwd";
  SsimShape s;
  if (ssim_shape(name, B, C, H, W, K, &s) || ssim_alpha(name, alpha) ||
      need_dim(name, "reduction = %lld", reduction, 0, 2, "0..2") || need_pointers(name, x && y && window && out))
    return 1;
  ITCV_REQUIRE(ws && ws_bytes >= 3 * s.nparts * sizeof(double), "itcv_ssim_loss_fwd(workspace)");
  double* part = static_cast<double*>(ws);
  hipStream_t st = S(stream);
  ssim_launch_tiles(x, y, window, part, H, W, K, s, st);
  ITCV_CHECK_LAUNCH(name);
  const double P = (double)C * H * W, n = (double)C * (H - K + 1) * (W - K + 1);
  hipLaunchKernelGGL(ssim_loss_finish_kernel, dim3(1), dim3(kSsimFinishThreads), 0, st, (const double*)part, s.nparts, out, B,
                     C * s.nth * s.ntw, P, n, alpha, reduction, scale);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_ssim_loss_bwd(const float* x, const float* y, const double* window, const float* g, float* dy, int B, int C, int H,
                       int W, int K, double alpha, int reduction, float scale, void* stream) {
  const char* name = "itcv_ssim_loss_bwd";
  SsimShape s;
  if (ssim_shape(name, B, C, H, W, K, &s) || ssim_alpha(name, alpha) ||
      need_dim(name, "reduction = %lld", reduction, 0, 2, "0..2") || need_pointers(name, x && y && window && g && dy))
    return 1;
  const double P = (double)C * H * W, n = (double)C * (H - K + 1) * (W - K + 1);
  const double coef = reduction == 2 ? (double)scale / (double)B : (double)scale;
  launch_lds<ssim_bwd_kernel>(dim3((unsigned)(s.planes * s.pth * s.ptw)), dim3(kSsimThreads), ssim_bwd_lds(K), S(stream), x, y,
                              window, g, dy, C, H, W, K, s.pth, s.ptw, P, n, alpha, reduction, coef);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_ssim_stats(const float* x, const float* y, const double* window, double* stats, int B, int C, int H, int W, int K,
                    void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_ssim_stats";
  SsimShape s;
  if (ssim_shape(name, B, C, H, W, K, &s) || need_pointers(name, x && y && window && stats)) return 1;
  ITCV_REQUIRE(ws && ws_bytes >= 3 * s.nparts * sizeof(double), "itcv_ssim_stats(workspace)");
  double* part = static_cast<double*>(ws);
  hipStream_t st = S(stream);
  ssim_launch_tiles(x, y, window, part, H, W, K, s, st);
  ITCV_CHECK_LAUNCH(name);
  const int planes = (int)s.planes;
  hipLaunchKernelGGL(ssim_stats_finish_kernel, dim3(cdiv(planes, 4)), dim3(256), 0, st, (const double*)part, s.nparts, stats,
                     planes, s.nth * s.ntw, (double)(H - K + 1) * (W - K + 1));
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
