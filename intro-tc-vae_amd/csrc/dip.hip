// The KL hook of DIP-VAE-I / II (Kumar et al. 2018; disentanglement_lib's `dip_vae`): coef_kl * mean KL + the covariance
// regulariser of the aggregate posterior, with its gradient.  The rules are in include/itcv_hip.h:
//   dip_tile   : C = X^T X / Bt (X = mu_all minus its column means) is tiled kDipTile x kDipTile over a 2-D grid; only the
//                tiles on and above the diagonal do work, the mirror image is written by the same block.  A block first
//                re-derives the fp64 column means of its own two column strips (four row classes per column, folded in a
//                fixed order), then walks the rows in chunks of kDipRows: the centred values are staged in LDS as fp64 and
//                every thread keeps a 2 x 2 patch of the tile in fp64 registers.  Kind II adds mean_b exp(logvar) to the
//                diagonal (the spare half of the means pass of a diagonal tile computes it).  The block writes its patch of
//                W = 2 lambda_od offdiag(C) + diag(2 lambda_d (C_ii - 1)) in fp32, the means of its strip (diagonal tiles)
//                and its two fp64 loss partials {sum C_ij^2 (i != j), sum (C_ii - 1)^2} into the workspace.
//   dip_finish : ONE block folds the tile partials (one per thread, fixed tree) and the KL of the local rows (objective.h's
//                mean_kl_rows) into the scalar and the three logged terms.
//   dip_bwd    : ONE launch, a kDipBwdRows x kDipBwdCols tile of [Bt, D] per block: (2 / Bt) X W in fp64 over LDS-staged
//                chunks of kDipBwdK, plus the diagonal term of logvar (kind II) and the KL gradient on the local rows.
// D up to 512 is covered by the grid, never by one block's LDS.  Every sum has a fixed order, there is no atomic, and
// nothing depends on the grid or on timing: the same inputs give the same bits.  Nothing in this file may be contracted into
// a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kDipMaxD = 512;
constexpr int kDipMaxBt = 1 << 24;
constexpr int kDipTile = 32;              // C is tiled 32 x 32: at most 16 x 16 tiles
constexpr int kDipRows = 64;              // rows of one staged chunk: 2 x 64 x 32 doubles = 32 KiB of LDS
constexpr int kDipThreads = 256;
constexpr int kDipBwdRows = 16;
constexpr int kDipBwdCols = 64;
constexpr int kDipBwdK = 32;

__global__ __launch_bounds__(kDipThreads) void dip_tile_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                               int ld, int Bt, int D, int kind, double lam_od, double lam_d,
                                                               float* __restrict__ W, double* __restrict__ mean,
                                                               double* __restrict__ part) {
  const int ti = blockIdx.y, tj = blockIdx.x, nt = gridDim.x;
  if (tj < ti) return;                                // block-uniform, before any barrier
  __shared__ double xa[kDipRows][kDipTile], xb[kDipRows][kDipTile];
  __shared__ double msum[4][2 * kDipTile];
  __shared__ double m[2 * kDipTile];                  // [0, 32): means of strip ti; [32, 64): of strip tj
  __shared__ double ev[kDipTile];                     // mean_b exp(logvar) of strip ti (diagonal tiles of kind II)
  __shared__ double red[kDipThreads / 64];
  const int tid = threadIdx.x;
  const bool diag_tile = ti == tj;
  const double inv_bt = 1.0 / (double)Bt;
  {
    // column sums over the row classes b = q, q + 4, ...; on a diagonal tile the second strip is the first one, and its
    // threads sum exp(logvar) instead
    const int c = tid & 63, q = tid >> 6;
    const bool second = c >= kDipTile;
    const int col = (second ? tj : ti) * kDipTile + (c & (kDipTile - 1));
    const bool want_ev = second && diag_tile;
    double s = 0.0;
    if (col < D && !(want_ev && kind != 2)) {
      const float* src = (want_ev ? lv : mu) + col;
      for (int b = q; b < Bt; b += 4) {
        const float v = src[(size_t)b * ld];
        s += want_ev ? exp((double)v) : (double)v;
      }
    }
    msum[q][c] = s;
    __syncthreads();
    if (tid < 2 * kDipTile) {
      const double tot = ((msum[0][tid] + msum[1][tid]) + msum[2][tid]) + msum[3][tid];
      if (tid >= kDipTile && diag_tile) {
        ev[tid - kDipTile] = tot * inv_bt;
        m[tid] = 0.0;                                 // set below
      } else {
        m[tid] = tot * inv_bt;
      }
    }
    __syncthreads();
    if (diag_tile && tid < kDipTile) {
      m[kDipTile + tid] = m[tid];
      const int gc = ti * kDipTile + tid;
      if (gc < D) mean[gc] = m[tid];
    }
    __syncthreads();
  }
  // the 2 x 2 patch of this thread: rows 2 pi, 2 pi + 1 of strip ti against columns 2 pj, 2 pj + 1 of strip tj
  const int pi = tid >> 4, pj = tid & 15;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int r0 = 0; r0 < Bt; r0 += kDipRows) {
    const int nr = min(kDipRows, Bt - r0);
#pragma unroll
    for (int u = 0; u < kDipRows * 2 * kDipTile / kDipThreads; ++u) {
      const int e = tid + u * kDipThreads;
      const int r = e >> 6, c = e & 63;
      const bool second = c >= kDipTile;
      const int col = (second ? tj : ti) * kDipTile + (c & (kDipTile - 1));
      double v = 0.0;
      if (r < nr && col < D) v = (double)mu[(size_t)(r0 + r) * ld + col] - m[c];
      if (second) xb[r][c - kDipTile] = v; else xa[r][c] = v;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const double a0 = xa[r][2 * pi], a1 = xa[r][2 * pi + 1];
      const double b0 = xb[r][2 * pj], b1 = xb[r][2 * pj + 1];
      acc[0][0] += a0 * b0;
      acc[0][1] += a0 * b1;
      acc[1][0] += a1 * b0;
      acc[1][1] += a1 * b1;
    }
    __syncthreads();
  }
  double od = 0.0, dg = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int gi = ti * kDipTile + 2 * pi + a, gj = tj * kDipTile + 2 * pj + b;
      if (gi < D && gj < D) {
        double c = acc[a][b] * inv_bt;
        double w;
        if (gi == gj) {
          if (kind == 2) c += ev[2 * pi + a];
          const double e = c - 1.0;
          dg += e * e;
          w = 2.0 * lam_d * e;
        } else {
          od += c * c;
          w = 2.0 * lam_od * c;
        }
        W[(size_t)gi * D + gj] = (float)w;
        if (!diag_tile) W[(size_t)gj * D + gi] = (float)w;
      }
    }
  }
  od = block_sum(od, red);
  dg = block_sum(dg, red);
  if (tid == 0) {
    double* p = part + 2 * (size_t)(ti * nt + tj);
    p[0] = diag_tile ? od : 2.0 * od;                 // the mirror tile holds the same squares
    p[1] = dg;
  }
}

// out[0] = coef_kl * mean_{local rows} KL + lam_od * sum_{i != j} C_ij^2 + lam_d * sum_i (C_ii - 1)^2;
// terms[3] = {mean KL, the off-diagonal term, the diagonal term}
__global__ __launch_bounds__(1024) void dip_finish_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int ld,
                                                          int Bl, int D, int nt, const double* __restrict__ part,
                                                          double lam_od, double lam_d, double coef_kl,
                                                          float* __restrict__ out, float* __restrict__ terms) {
  __shared__ double red[16];
  __shared__ double klw[16];
  const int tid = threadIdx.x;
  double od = 0.0, dg = 0.0;
  if (tid < nt * nt && (tid % nt) >= (tid / nt)) od = part[2 * tid], dg = part[2 * tid + 1];
  od = block_sum(od, red);
  dg = block_sum(dg, red);
  const double kl = mean_kl_rows(mu, lv, (size_t)ld, Bl, D, klw);
  if (tid == 0) {
    const double t_od = lam_od * od, t_dg = lam_d * dg;
    out[0] = (float)((coef_kl != 0.0 ? coef_kl * kl : 0.0) + (t_od + t_dg));
    terms[0] = (float)kl, terms[1] = (float)t_od, terms[2] = (float)t_dg;
  }
}

__global__ __launch_bounds__(kDipThreads) void dip_bwd_kernel(const float* __restrict__ g, const float* __restrict__ mu,
                                                              const float* __restrict__ lv, int ld,
                                                              const float* __restrict__ W, const double* __restrict__ mean,
                                                              int Bl, int Bt, int row_offset, int D, int kind, double coef_kl,
                                                              float* __restrict__ dmu, float* __restrict__ dlv) {
  __shared__ double xs[kDipBwdRows][kDipBwdK];
  __shared__ float wsh[kDipBwdK][kDipBwdCols];
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
  const int r0 = blockIdx.x * kDipBwdRows, c0 = blockIdx.y * kDipBwdCols;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < D; k0 += kDipBwdK) {
    const int nk = min(kDipBwdK, D - k0);
#pragma unroll
    for (int u = 0; u < kDipBwdRows * kDipBwdK / kDipThreads; ++u) {
      const int e = tid + u * kDipThreads;
      const int r = e / kDipBwdK, k = e % kDipBwdK;
      const int row = r0 + r;
      xs[r][k] = (row < Bt && k < nk) ? (double)mu[(size_t)row * ld + k0 + k] - mean[k0 + k] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kDipBwdK * kDipBwdCols / kDipThreads; ++u) {
      const int e = tid + u * kDipThreads;
      const int k = e / kDipBwdCols, c = e % kDipBwdCols;
      wsh[k][c] = (k < nk && c0 + c < D) ? W[(size_t)(k0 + k) * D + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      const double wv = (double)wsh[k][col];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] += xs[rg * 4 + a][k] * wv;
    }
    __syncthreads();
  }
  const int gj = c0 + col;
  if (gj >= D) return;
  const double g0 = (double)g[0], inv_bt = 1.0 / (double)Bt;
  const double wjj = (double)W[(size_t)gj * D + gj];
  const double ckl = coef_kl != 0.0 ? coef_kl / (double)Bl : 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = r0 + rg * 4 + a;
    if (row >= Bt) continue;
    const size_t at = (size_t)row * ld + gj;
    double dm = 2.0 * inv_bt * acc[a], dl = 0.0;
    const bool local = ckl != 0.0 && row >= row_offset && row < row_offset + Bl;
    if (kind == 2 || local) {
      const double e = (double)expf(lv[at]);
      if (kind == 2) dl = e * wjj * inv_bt;
      if (local) dl += ckl * (-0.5 * (1.0 - e));
    }
    if (local) dm += ckl * (double)mu[at];
    dmu[at] = (float)(g0 * dm);
    dlv[at] = (float)(g0 * dl);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline int dip_tiles(int D) { return cdiv(D, kDipTile); }
static inline size_t dip_ws(int D) { return (size_t)dip_tiles(D) * dip_tiles(D) * 2 * sizeof(double); }

// nothing is launched on a failure
static int dip_check(const char* name, bool ptrs, int ld, int Bl, int Bt, int row_offset, int D, int kind, double lam_od,
                     double lam_d, double coef_kl) {
  if (need_pointers(name, ptrs) || need_dim(name, "Bt = %lld rows", Bt, 2, kDipMaxBt, "2..2^24") ||
      need_dim(name, "D = %lld", D, 1, kDipMaxD, "1..512"))
    return 1;
  if (Bl < 1 || row_offset < 0 || (long long)row_offset + Bl > Bt)
    return fail("%s: rows must lie inside the global batch (row_offset = %lld, Bt = %lld)", name, row_offset, Bt);
  if (kind != 1 && kind != 2) return fail("%s: kind %lld is not 1 (DIP-VAE-I) or 2 (DIP-VAE-II)", name, kind);
  if (!(lam_od >= 0.0 && finite(lam_od) && lam_d >= 0.0 && finite(lam_d)))
    return fail("%s: lambda_od and lambda_d must be finite numbers >= 0", name);
  if (!finite(coef_kl)) return fail("%s: coef_kl must be a finite number", name);
  if (ld != D && ld != 2 * D)
    return fail("%s: row stride %lld of mu_all / logvar_all is neither D nor 2 D (D = %lld)", name, ld, D);
  return 0;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_dip_kl_workspace(int Bt, int D) { return (Bt >= 2 && D >= 1 && D <= kDipMaxD) ? dip_ws(D) : 0; }

int itcv_dip_kl_fwd(const float* mu_all, const float* logvar_all, int ld, float* out, float* terms, float* W, double* mean,
                    int Bl, int Bt, int row_offset, int D, int kind, double lambda_od, double lambda_d, double coef_kl,
                    void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_dip_kl_fwd";
  if (int e = dip_check(name, mu_all && logvar_all && out && terms && W && mean, ld, Bl, Bt, row_offset, D, kind, lambda_od,
                        lambda_d, coef_kl))
    return e;
  ITCV_REQUIRE(ws && ws_bytes >= dip_ws(D), "itcv_dip_kl_fwd(workspace)");
  double* part = static_cast<double*>(ws);
  const int nt = dip_tiles(D);
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(dip_tile_kernel, dim3(nt, nt), dim3(kDipThreads), 0, st, mu_all, logvar_all, ld, Bt, D, kind, lambda_od,
                     lambda_d, W, mean, part);
  ITCV_CHECK_LAUNCH("itcv_dip_kl_fwd(tiles)");
  const size_t off = (size_t)row_offset * ld;
  hipLaunchKernelGGL(dip_finish_kernel, dim3(1), dim3(1024), 0, st, mu_all + off, logvar_all + off, ld, Bl, D, nt,
                     (const double*)part, lambda_od, lambda_d, coef_kl, out, terms);
  ITCV_CHECK_LAUNCH("itcv_dip_kl_fwd(finish)");
  return 0;
}

int itcv_dip_kl_bwd(const float* g, const float* mu_all, const float* logvar_all, int ld, const float* W, const double* mean,
                    float* dmu_all, float* dlogvar_all, int Bl, int Bt, int row_offset, int D, int kind, double coef_kl,
                    void* stream) {
  const char* name = "itcv_dip_kl_bwd";
  if (int e = dip_check(name, g && mu_all && logvar_all && W && mean && dmu_all && dlogvar_all, ld, Bl, Bt, row_offset, D,
                        kind, 0.0, 0.0, coef_kl))
    return e;
  hipLaunchKernelGGL(dip_bwd_kernel, dim3(cdiv(Bt, kDipBwdRows), cdiv(D, kDipBwdCols)), dim3(kDipThreads), 0, S(stream), g,
                     mu_all, logvar_all, ld, W, mean, Bl, Bt, row_offset, D, kind, coef_kl, dmu_all, dlogvar_all);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
