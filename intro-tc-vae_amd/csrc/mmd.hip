// The KL hook of InfoVAE / MMD-VAE (Zhao et al. 2017) and WAE-MMD (Tolstikhin et al. 2018): coef_kl * mean KL + lambda_mmd *
// the unbiased kernel two-sample statistic MMD^2 between the batch's sampled latents and draws from the prior, with its
// gradient.  The rules are in include/itcv_hip.h:
//   mmd_tile   : the points X = [z_all ; prior] (Bt + P rows) are cut into strips of kMmdTile rows, z strips first, each
//                set padded to whole strips; the pair matrix of X is tiled over a 2-D grid of strips and only the tiles on
//                and above the diagonal do work.  That triangle IS the three blocks the statistic needs: zz tiles (upper
//                ones computed, their weights mirrored by the same block), every zp tile, and the upper pp tiles (sum
//                only).  A block stages its two strips in LDS as fp32 in chunks of kMmdChunk columns; every thread keeps
//                the d^2 of a 2 x 2 patch of pairs in fp64 registers, then evaluates k and k' in fp64.  It writes its
//                patch of Wt = (A | C) in fp32, ONE fp64 partial of its kernel sum, and the fp64 sums of its weights along
//                its rows (and, mirrored, along its columns) into the workspace: they are taken from the fp64 values in a
//                fixed order, never from the rounded fp32 ones.
//   mmd_finish : block 0 folds the tile partials (fixed per-thread order, fixed tree) and the KL of the local rows
//                (objective.h's mean_kl_rows) into the scalar and the five logged terms; the blocks behind it fold the
//                per-strip row sums into rs [Bt], one row a thread, strips ascending.
//   mmd_bwd    : ONE launch, a kMmdBwdRows x kMmdBwdCols tile of [Bt, D] per block: rs o z - Wt [z ; p] in fp64 over
//                LDS-staged chunks of kMmdBwdK points; the blocks behind those write the KL gradient of the local rows.
// Limits: Bt, P in 2..4096 and D in 1..512, covered by the grid, never by one block's LDS; they bound Wt at
// 4096 x 8192 x 4 bytes = 128 MiB and the workspace at 8.5 MiB.  Nothing of size Bt x Bt x D exists anywhere.  Every sum
// has a fixed order, there is no atomic, and nothing depends on the grid or on timing: the same inputs give the same bits.
// Nothing in this file may be contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kMmdMaxN = 4096;            // Bt and P
constexpr int kMmdMaxD = 512;
constexpr int kMmdMaxBl = 1 << 24;
constexpr int kMmdTile = 32;              // strips of 32 points: at most 256 x 256 tiles
constexpr int kMmdChunk = 64;             // columns of one staged chunk: 2 x 32 x 65 floats = 16.3 KiB of LDS
constexpr int kMmdThreads = 256;
constexpr int kMmdBwdRows = 16;
constexpr int kMmdBwdCols = 64;
constexpr int kMmdBwdK = 32;
constexpr int kMmdScales = 7;
__constant__ const double kMmdImqScale[kMmdScales] = {0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0};

// k(d2) and k'(d2): kind 1 = rbf exp(-d2 / h); kind 2 = imq sum_s C_s / (C_s + d2), C_s = s h
__device__ __forceinline__ void mmd_kernel_value(int kind, double h, double d2, double& k, double& kp) {
  if (kind == 1) {
    k = exp(-d2 / h);
    kp = -k / h;
  } else {
    k = 0.0, kp = 0.0;
#pragma unroll
    for (int s = 0; s < kMmdScales; ++s) {
      const double c = kMmdImqScale[s] * h, den = c + d2;
      k += c / den;
      kp -= c / (den * den);
    }
  }
}

__global__ __launch_bounds__(kMmdThreads) void mmd_tile_kernel(const float* __restrict__ z, const float* __restrict__ pr,
                                                               int Bt, int P, int D, int kind, double h,
                                                               float* __restrict__ Wt, double* __restrict__ part,
                                                               double* __restrict__ rowpart) {
  const int ti = blockIdx.y, tj = blockIdx.x, nt = gridDim.x;
  if (tj < ti) return;                                // block-uniform, before any barrier
  __shared__ float xa[kMmdTile][kMmdChunk + 1], xb[kMmdTile][kMmdChunk + 1];
  __shared__ double wsm[kMmdTile][kMmdTile + 1];
  __shared__ double red[kMmdThreads / 64];
  const int tid = threadIdx.x;
  const int nz = cdiv(Bt, kMmdTile);
  const bool a_is_z = ti < nz, b_is_z = tj < nz;
  const float* __restrict__ srca = a_is_z ? z : pr;
  const float* __restrict__ srcb = b_is_z ? z : pr;
  const int na = a_is_z ? Bt : P, nb = b_is_z ? Bt : P;                  // points of the sets the strips belong to
  const int a0 = (a_is_z ? ti : ti - nz) * kMmdTile, b0 = (b_is_z ? tj : tj - nz) * kMmdTile;
  const bool diag_tile = ti == tj;
  // the 2 x 2 patch of this thread: points pi, pi + 16 of strip ti against points pj, pj + 16 of strip tj
  const int pi = tid >> 4, pj = tid & 15;
  double d2[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int l0 = 0; l0 < D; l0 += kMmdChunk) {
    const int nl = min(kMmdChunk, D - l0);
#pragma unroll
    for (int u = 0; u < kMmdTile * kMmdChunk / kMmdThreads; ++u) {
      const int e = tid + u * kMmdThreads;
      const int r = e >> 6, l = e & 63;
      float va = 0.f, vb = 0.f;
      if (l < nl) {
        if (a0 + r < na) va = srca[(size_t)(a0 + r) * D + l0 + l];
        if (b0 + r < nb) vb = srcb[(size_t)(b0 + r) * D + l0 + l];
      }
      xa[r][l] = va, xb[r][l] = vb;
    }
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const double p0 = (double)xa[pi][l], p1 = (double)xa[pi + 16][l];
      const double q0 = (double)xb[pj][l], q1 = (double)xb[pj + 16][l];
      const double e00 = p0 - q0, e01 = p0 - q1, e10 = p1 - q0, e11 = p1 - q1;
      d2[0][0] += e00 * e00;
      d2[0][1] += e01 * e01;
      d2[1][0] += e10 * e10;
      d2[1][1] += e11 * e11;
    }
    __syncthreads();
  }
  // weights: A = k' 2 / (Bt (Bt - 1)) against z, C = k' (-2) / (Bt P) against the prior; the pp tiles carry none
  const double wscale = !a_is_z ? 0.0 : (b_is_z ? 2.0 / ((double)Bt * (double)(Bt - 1)) : -2.0 / ((double)Bt * (double)P));
  const int ldw = Bt + P;
  double ksum = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ri = pi + 16 * a, rj = pj + 16 * b;
      const int gi = a0 + ri, gj = b0 + rj;
      double w = 0.0;
      if (gi < na && gj < nb && !(diag_tile && gi == gj)) {
        double k, kp;
        mmd_kernel_value(kind, h, d2[a][b], k, kp);
        ksum += k;
        w = kp * wscale;
      }
      wsm[ri][rj] = w;
      if (a_is_z && gi < na && gj < nb) {
        const float wf = (float)w;
        Wt[(size_t)gi * ldw + (b_is_z ? gj : Bt + gj)] = wf;
        if (b_is_z && !diag_tile) Wt[(size_t)gj * ldw + gi] = wf;       // the mirror tile of the zz block
      }
    }
  }
  ksum = block_sum(ksum, red);                        // its barriers also publish wsm
  if (tid == 0) part[(size_t)ti * nt + tj] = (diag_tile || a_is_z != b_is_z) ? ksum : 2.0 * ksum;
  if (!a_is_z) return;
  if (tid < kMmdTile) {
    // sum over the strip tj of the weights of row a0 + tid
    if (a0 + tid < Bt) {
      double s = 0.0;
      for (int c = 0; c < kMmdTile; ++c) s += wsm[tid][c];
      rowpart[(size_t)tj * Bt + a0 + tid] = s;
    }
  } else if (tid < 2 * kMmdTile && b_is_z && !diag_tile) {
    // the mirror tile: sum over the strip ti of the weights of row b0 + c
    const int c = tid - kMmdTile;
    if (b0 + c < Bt) {
      double s = 0.0;
      for (int r = 0; r < kMmdTile; ++r) s += wsm[r][c];
      rowpart[(size_t)ti * Bt + b0 + c] = s;
    }
  }
}

// block 0: out[0] = coef_kl * mean_{local rows} KL + lambda * MMD^2, terms[5] = {mean KL, MMD^2, S_zz, S_pp, S_zp};
// blocks 1..: rs[i] = sum over the strips of rowpart, strips ascending
__global__ __launch_bounds__(1024) void mmd_finish_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int Bl,
                                                          int Bt, int P, int D, int nt, const double* __restrict__ part,
                                                          const double* __restrict__ rowpart, double lambda, double coef_kl,
                                                          float* __restrict__ out, float* __restrict__ terms,
                                                          double* __restrict__ rs) {
  const int tid = threadIdx.x;
  if (blockIdx.x > 0) {
    const int i = (blockIdx.x - 1) * 1024 + tid;
    if (i < Bt) rs[i] = fold_strided(0.0, rowpart + i, (size_t)Bt, nt);
    return;
  }
  __shared__ double red[16];
  __shared__ double klw[16];
  const int nz = cdiv(Bt, kMmdTile);
  double zz = 0.0, pp = 0.0, zp = 0.0;
  for (int e = tid; e < nt * nt; e += 1024) {
    const int ti = e / nt, tj = e - ti * nt;
    if (tj < ti) continue;
    const double v = part[e];
    if (tj < nz) zz += v;
    else if (ti < nz) zp += v;
    else pp += v;
  }
  zz = block_sum(zz, red);
  pp = block_sum(pp, red);
  zp = block_sum(zp, red);
  const double kl = mean_kl_rows(mu, lv, (size_t)D, Bl, D, klw);
  if (tid == 0) {
    const double s_zz = zz / ((double)Bt * (double)(Bt - 1)), s_pp = pp / ((double)P * (double)(P - 1));
    const double s_zp = zp / ((double)Bt * (double)P);
    const double mmd2 = (s_zz + s_pp) - 2.0 * s_zp;
    out[0] = (float)((coef_kl != 0.0 ? coef_kl * kl : 0.0) + lambda * mmd2);
    terms[0] = (float)kl, terms[1] = (float)mmd2, terms[2] = (float)s_zz, terms[3] = (float)s_pp, terms[4] = (float)s_zp;
  }
}

// blocks x < cdiv(Bt, 16): dz_all = g lambda 2 (rs o z - Wt [z ; p]); the blocks behind them: dmu / dlogvar of the local rows
__global__ __launch_bounds__(kMmdThreads) void mmd_bwd_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                              const float* __restrict__ pr, const float* __restrict__ mu,
                                                              const float* __restrict__ lv, const float* __restrict__ Wt,
                                                              const double* __restrict__ rs, int Bl, int Bt, int P, int D,
                                                              double lambda, double coef_kl, float* __restrict__ dz,
                                                              float* __restrict__ dmu, float* __restrict__ dlv) {
  __shared__ float wsh[kMmdBwdRows][kMmdBwdK];
  __shared__ float xs[kMmdBwdK][kMmdBwdCols];
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
  const int nbz = cdiv(Bt, kMmdBwdRows);
  const int c0 = blockIdx.y * kMmdBwdCols, gj = c0 + col;
  const double g0 = (double)g[0];
  if ((int)blockIdx.x >= nbz) {                       // block-uniform, before any barrier
    if (gj >= D) return;
    const double ckl = coef_kl != 0.0 ? coef_kl / (double)Bl : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = ((int)blockIdx.x - nbz) * kMmdBwdRows + rg * 4 + a;
      if (row >= Bl) continue;
      const size_t at = (size_t)row * D + gj;
      double dm = 0.0, dl = 0.0;
      if (ckl != 0.0) {
        dm = ckl * (double)mu[at];
        dl = ckl * (-0.5 * (1.0 - (double)expf(lv[at])));
      }
      dmu[at] = (float)(g0 * dm);
      dlv[at] = (float)(g0 * dl);
    }
    return;
  }
  const int r0 = blockIdx.x * kMmdBwdRows, N = Bt + P;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < N; k0 += kMmdBwdK) {
    const int nk = min(kMmdBwdK, N - k0);
#pragma unroll
    for (int u = 0; u < kMmdBwdRows * kMmdBwdK / kMmdThreads; ++u) {
      const int e = tid + u * kMmdThreads;
      const int r = e / kMmdBwdK, k = e % kMmdBwdK;
      wsh[r][k] = (r0 + r < Bt && k < nk) ? Wt[(size_t)(r0 + r) * N + k0 + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kMmdBwdK * kMmdBwdCols / kMmdThreads; ++u) {
      const int e = tid + u * kMmdThreads;
      const int k = e / kMmdBwdCols, c = e % kMmdBwdCols;
      const int pt = k0 + k;
      float v = 0.f;
      if (k < nk && c0 + c < D) v = pt < Bt ? z[(size_t)pt * D + c0 + c] : pr[(size_t)(pt - Bt) * D + c0 + c];
      xs[k][c] = v;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      const double xv = (double)xs[k][col];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] += (double)wsh[rg * 4 + a][k] * xv;
    }
    __syncthreads();
  }
  if (gj >= D) return;
  const double f = g0 * lambda * 2.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = r0 + rg * 4 + a;
    if (row >= Bt) continue;
    const size_t at = (size_t)row * D + gj;
    dz[at] = (float)(f * (rs[row] * (double)z[at] - acc[a]));
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline int mmd_tiles(int Bt, int P) { return cdiv(Bt, kMmdTile) + cdiv(P, kMmdTile); }
static inline size_t mmd_ws(int Bt, int P) {
  const size_t nt = (size_t)mmd_tiles(Bt, P);
  return (nt * nt + nt * (size_t)Bt) * sizeof(double);
}

// nothing is launched on a failure
static int mmd_check(const char* name, bool ptrs, int Bl, int Bt, int P, int D, int kind, double h, double lambda,
                     double coef_kl) {
  if (need_pointers(name, ptrs) || need_dim(name, "Bt = %lld rows", Bt, 2, kMmdMaxN, "2..4096") ||
      need_dim(name, "P = %lld prior rows", P, 2, kMmdMaxN, "2..4096") ||
      need_dim(name, "Bl = %lld local rows", Bl, 1, kMmdMaxBl, "1..2^24") ||
      need_dim(name, "D = %lld", D, 1, kMmdMaxD, "1..512"))
    return 1;
  if (kind != 1 && kind != 2) return fail("%s: kernel %lld is not 1 (rbf) or 2 (imq)", name, kind);
  if (!(h > 0.0 && finite(h))) return fail("%s: the bandwidth h must be a finite number > 0", name);
  if (!(lambda >= 0.0 && finite(lambda))) return fail("%s: lambda_mmd must be a finite number >= 0", name);
  if (!finite(coef_kl)) return fail("%s: coef_kl must be a finite number", name);
  return 0;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_mmd_kl_workspace(int Bt, int P) {
  return (Bt >= 2 && Bt <= kMmdMaxN && P >= 2 && P <= kMmdMaxN) ? mmd_ws(Bt, P) : 0;
}

int itcv_mmd_kl_fwd(const float* z_all, const float* prior, const float* mu, const float* logvar, float* out, float* terms,
                    float* Wt, double* rs, int Bl, int Bt, int P, int D, int kernel, double h, double lambda_mmd,
                    double coef_kl, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_mmd_kl_fwd";
  if (int e = mmd_check(name, z_all && prior && mu && logvar && out && terms && Wt && rs, Bl, Bt, P, D, kernel, h,
                        lambda_mmd, coef_kl))
    return e;
  ITCV_REQUIRE(ws && ws_bytes >= mmd_ws(Bt, P), "itcv_mmd_kl_fwd(workspace)");
  const int nt = mmd_tiles(Bt, P);
  double* part = static_cast<double*>(ws);
  double* rowpart = part + (size_t)nt * nt;
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(mmd_tile_kernel, dim3(nt, nt), dim3(kMmdThreads), 0, st, z_all, prior, Bt, P, D, kernel, h, Wt, part,
                     rowpart);
  ITCV_CHECK_LAUNCH("itcv_mmd_kl_fwd(tiles)");
  hipLaunchKernelGGL(mmd_finish_kernel, dim3(1 + cdiv(Bt, 1024)), dim3(1024), 0, st, mu, logvar, Bl, Bt, P, D, nt,
                     (const double*)part, (const double*)rowpart, lambda_mmd, coef_kl, out, terms, rs);
  ITCV_CHECK_LAUNCH("itcv_mmd_kl_fwd(finish)");
  return 0;
}

int itcv_mmd_kl_bwd(const float* g, const float* z_all, const float* prior, const float* mu, const float* logvar,
                    const float* Wt, const double* rs, float* dz_all, float* dmu, float* dlogvar, int Bl, int Bt, int P,
                    int D, double lambda_mmd, double coef_kl, void* stream) {
  const char* name = "itcv_mmd_kl_bwd";
  if (int e = mmd_check(name, g && z_all && prior && mu && logvar && Wt && rs && dz_all && dmu && dlogvar, Bl, Bt, P, D, 1,
                        1.0, lambda_mmd, coef_kl))
    return e;
  hipLaunchKernelGGL(mmd_bwd_kernel, dim3(cdiv(Bt, kMmdBwdRows) + cdiv(Bl, kMmdBwdRows), cdiv(D, kMmdBwdCols)),
                     dim3(kMmdThreads), 0, S(stream), g, z_all, prior, mu, logvar, Wt, rs, Bl, Bt, P, D, lambda_mmd, coef_kl,
                     dz_all, dmu, dlogvar);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
