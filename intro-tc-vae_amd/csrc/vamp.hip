// The KL term of a VAE with a VampPrior (Tomczak & Welling 2018): beta * (log q(z | x) - log p(z)) of one sample per row
// against the uniform mixture p(z) = (1 / K) sum_k N(z; p_mu_k, diag exp(p_logvar_k)) of K diagonal components, with its
// gradient to the rows and to the components.  The rules are in include/itcv_hip.h:
//   vamp_pair   : the pair matrix L [B, K] is cut into kVampTile x kVampTile tiles over a 2-D grid.  A block stages its
//                 32 rows (the fp32 sample z = mu + eps exp(logvar / 2), formed in fp64) and its 32 components (p_mu,
//                 p_logvar and iv = exp(-p_logvar), ONE exp per staged element) in LDS in chunks of kVampChunk columns;
//                 every thread keeps a 2 x 2 patch of pairs in fp64 registers.  It writes its patch of L in fp64 and, per
//                 row, the max and the sum of exp(L - max) over its 32 components, in component order.  The blocks of the
//                 first component tile also write z and log q of their rows (a wave per row, a fixed lane order).
//   vamp_finish : block 0 folds the tile partials of every row in tile order into logp and rows, then the scalar and the
//                 three logged terms with objective.h's ordered_sum; the blocks behind it take kVampFinishRows rows each,
//                 fold the same partials in the same order (the same bits) and overwrite L with r = exp(L - logsumexp).
//   vamp_bwd    : ONE launch.  Blocks x < cdiv(B, 16): a 16 x 64 tile of [B, D], A = sum_k r (z - p_mu) iv over LDS-staged
//                 chunks of 32 components -> dmu, dlogvar.  The blocks behind them: a 16 x 64 tile of [K, D], the sums over
//                 b of G r (z - p_mu) iv and G r (1 - (z - p_mu)^2 iv) over staged chunks of 32 rows -> dp_mu, dp_logvar.
//   vamp_logprob: the pair pass on given rows (no sample, no log q, L not kept) and a one-thread-a-row finish.
// L is formed from the fp32 z that the op returns, so vamp_logprob on that z gives the same bits.  Limits: B, K in 1..4096,
// B K <= 2^22 (L is at most 32 MiB), D in 1..512, covered by the grid, never by one block's LDS.  Every sum has a fixed
// order, there is no atomic, and nothing depends on the grid or on timing: the same inputs give the same bits.  Nothing in
// this file may be contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kVampMaxB = 4096;
constexpr int kVampMaxK = 4096;
constexpr int kVampMaxD = 512;
constexpr long long kVampMaxPairs = 1ll << 22;
constexpr int kVampTile = 32;             // rows and components of one tile of L
constexpr int kVampChunk = 32;            // staged columns: 3 x 32 x 33 floats + 32 x 33 doubles = 20.6 KiB, + the L patch
constexpr int kVampThreads = 256;
constexpr int kVampFinishRows = 16;       // rows of L one finish block turns into r a trip: four a wave
constexpr int kVampFinishBlocks = 128;    // of those blocks at most; above 2048 rows they walk the rest by the stride
constexpr int kVampBwdRows = 16;          // rows (or components) of one backward tile
constexpr int kVampBwdCols = 64;
constexpr int kVampBwdK = 32;             // components (or rows) of one staged chunk of the backward
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

template <bool SAMPLE>
__global__ __launch_bounds__(kVampThreads) void vamp_pair_kernel(
    const float* __restrict__ mu, size_t ldm, const float* __restrict__ lv, size_t ldl, const float* __restrict__ eps,
    size_t lde, const float* __restrict__ pmu, size_t ldpm, const float* __restrict__ plv, size_t ldpl, int B, int K, int D,
    float* __restrict__ z, double* __restrict__ L, double* __restrict__ pmax, double* __restrict__ psum,
    double* __restrict__ logq) {
  __shared__ float zs[kVampTile][kVampChunk + 1], pms[kVampTile][kVampChunk + 1], pls[kVampTile][kVampChunk + 1];
  __shared__ double ivs[kVampTile][kVampChunk + 1];
  __shared__ double lsm[kVampTile][kVampTile + 1];
  const int tid = threadIdx.x, tj = blockIdx.x, ti = blockIdx.y;
  const int r0 = ti * kVampTile, k0 = tj * kVampTile;
  // the 2 x 2 patch of this thread: rows pi, pi + 16 of the tile against components pj, pj + 16
  const int pi = tid >> 4, pj = tid & 15;
  double s[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, ls[2] = {0.0, 0.0};
  for (int l0 = 0; l0 < D; l0 += kVampChunk) {
    const int nl = min(kVampChunk, D - l0);
#pragma unroll
    for (int u = 0; u < kVampTile * kVampChunk / kVampThreads; ++u) {
      const int e = tid + u * kVampThreads;
      const int r = e / kVampChunk, l = e % kVampChunk;
      float zv = 0.f, pv = 0.f, pl = 0.f;
      double iv = 0.0;
      if (l < nl) {
        if (r0 + r < B) {
          const size_t row = (size_t)(r0 + r);
          if constexpr (SAMPLE) {
            zv = (float)posterior_sample((double)mu[row * ldm + l0 + l], (double)lv[row * ldl + l0 + l],
                                         (double)eps[row * lde + l0 + l]);
            if (tj == 0) z[row * D + l0 + l] = zv;
          } else {
            zv = mu[row * ldm + l0 + l];
          }
        }
        if (k0 + r < K) {
          const size_t row = (size_t)(k0 + r);
          pv = pmu[row * ldpm + l0 + l];
          pl = plv[row * ldpl + l0 + l];
          iv = exp(-(double)pl);
        }
      }
      zs[r][l] = zv, pms[r][l] = pv, pls[r][l] = pl, ivs[r][l] = iv;
    }
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const double p0 = (double)zs[pi][l], p1 = (double)zs[pi + 16][l];
      const double q0 = (double)pms[pj][l], q1 = (double)pms[pj + 16][l];
      const double i0 = ivs[pj][l], i1 = ivs[pj + 16][l];
      const double e00 = p0 - q0, e01 = p0 - q1, e10 = p1 - q0, e11 = p1 - q1;
      s[0][0] += e00 * e00 * i0;
      s[0][1] += e01 * e01 * i1;
      s[1][0] += e10 * e10 * i0;
      s[1][1] += e11 * e11 * i1;
      ls[0] += (double)pls[pj][l];
      ls[1] += (double)pls[pj + 16][l];
    }
    __syncthreads();
  }
  const double dc = (double)D * kLog2Pi;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ri = pi + 16 * a, rj = pj + 16 * b;
      const int gi = r0 + ri, gj = k0 + rj;
      const double v = -0.5 * (dc + ls[b] + s[a][b]);
      lsm[ri][rj] = v;
      if (L && gi < B && gj < K) L[(size_t)gi * K + gj] = v;
    }
  }
  __syncthreads();
  if (tid < kVampTile && r0 + tid < B) {
    // max and sum of exp over the components of this tile, in component order; a tile holds at least one component
    const int nk = min(kVampTile, K - k0);
    double m = lsm[tid][0];
    for (int c = 1; c < nk; ++c) m = lsm[tid][c] > m ? lsm[tid][c] : m;
    double t = 0.0;
    for (int c = 0; c < nk; ++c) t += exp(lsm[tid][c] - m);
    pmax[(size_t)tj * B + r0 + tid] = m;
    psum[(size_t)tj * B + r0 + tid] = t;
  }
  if constexpr (SAMPLE) {
    if (tj != 0) return;
    // log q(z | x) = -1/2 sum_d (log 2 pi + logvar + eps^2): a wave per row, lane l takes columns l, l + 64, ...
    const int lane = tid & 63, w = tid >> 6;
    for (int r = w; r < kVampTile; r += kVampThreads / kWave) {
      if (r0 + r >= B) break;                         // wave-uniform
      const size_t row = (size_t)(r0 + r);
      double a = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double n = (double)eps[row * lde + d];
        a += kLog2Pi + (double)lv[row * ldl + d] + n * n;
      }
      a = wave_sum(a);
      if (lane == 0) logq[row] = -0.5 * a;
    }
  }
}

// logsumexp of row b of L from the partials of its ntk tiles, tiles ascending: the same bits wherever it is called
__device__ __forceinline__ double vamp_row_lse(const double* __restrict__ pmax, const double* __restrict__ psum, int b,
                                               int B, int ntk) {
  double m = pmax[b];
  for (int t = 1; t < ntk; ++t) {
    const double v = pmax[(size_t)t * B + b];
    m = v > m ? v : m;
  }
  double sum = 0.0;
  for (int t = 0; t < ntk; ++t) sum += psum[(size_t)t * B + b] * exp(pmax[(size_t)t * B + b] - m);
  return m + log(sum);
}

// block 0: logp, rows, out[0] = beta * (mean or sum of) (logq - logp), terms[3] = {mean KL, mean logq, mean logp};
// blocks 1..: L <- r, kVampFinishRows rows a trip (objective.h's row_grid)
__global__ __launch_bounds__(kVampThreads) void vamp_finish_kernel(double* __restrict__ L, const double* __restrict__ pmax,
                                                                   const double* __restrict__ psum,
                                                                   const double* __restrict__ logq, int B, int K, int ntk,
                                                                   double beta, int reduce, double* logp, double* klrow,
                                                                   float* __restrict__ rows, float* __restrict__ out,
                                                                   float* __restrict__ terms) {
  const int tid = threadIdx.x;
  if (blockIdx.x > 0) {
    const int lane = tid & 63, w = tid >> 6;
    for (int base = ((int)blockIdx.x - 1) * kVampFinishRows; base < B; base += ((int)gridDim.x - 1) * kVampFinishRows) {
      for (int rr = w; rr < kVampFinishRows; rr += kVampThreads / kWave) {
        const int b = base + rr;
        if (b >= B) break;                            // wave-uniform
        const double lse = vamp_row_lse(pmax, psum, b, B, ntk);
        double* __restrict__ row = L + (size_t)b * K;
        for (int k = lane; k < K; k += 64) row[k] = exp(row[k] - lse);
      }
    }
    return;
  }
  __shared__ double red[kVampThreads];
  const double logk = log((double)K);
  for (int b = tid; b < B; b += kVampThreads) {
    const double lp = vamp_row_lse(pmax, psum, b, B, ntk) - logk;
    const double kl = logq[b] - lp;
    logp[b] = lp;
    klrow[b] = kl;
    rows[b] = (float)(beta != 0.0 ? beta * kl : 0.0);
  }
  __syncthreads();                                    // ordered_sum reads what other threads of this block wrote
  const double skl = ordered_sum<kVampThreads>(klrow, (size_t)B, red);
  const double slq = ordered_sum<kVampThreads>(logq, (size_t)B, red);
  const double slp = ordered_sum<kVampThreads>(logp, (size_t)B, red);
  if (tid == 0) {
    const double mean = skl / (double)B;
    out[0] = (float)(beta != 0.0 ? beta * (reduce == 2 ? skl : mean) : 0.0);
    terms[0] = (float)mean, terms[1] = (float)(slq / (double)B), terms[2] = (float)(slp / (double)B);
  }
}

__global__ __launch_bounds__(kVampThreads) void vamp_logprob_finish_kernel(const double* __restrict__ pmax,
                                                                           const double* __restrict__ psum, int N, int K,
                                                                           int ntk, double* __restrict__ logp) {
  for (int b = blockIdx.x * kVampThreads + threadIdx.x; b < N; b += gridDim.x * kVampThreads)
    logp[b] = vamp_row_lse(pmax, psum, b, N, ntk) - log((double)K);
}

// G_b = gscale * g[b] (g_rows) or gscale * g[0]; a NULL g or gz is a zero gradient.
__global__ __launch_bounds__(kVampThreads) void vamp_bwd_kernel(
    const float* __restrict__ gz, size_t ldgz, const float* __restrict__ g, int g_rows, double gscale,
    const float* __restrict__ lv, size_t ldl, const float* __restrict__ eps, size_t lde, const float* __restrict__ z,
    const float* __restrict__ pmu, size_t ldpm, const float* __restrict__ plv, size_t ldpl, const double* __restrict__ r,
    int B, int K, int D, double beta, float* __restrict__ dmu, float* __restrict__ dlv, float* __restrict__ dpmu,
    float* __restrict__ dplv) {
  // one buffer, carved by the two parts: rows 512 + 2048 doubles and 2048 floats, components 512 doubles and 2048 floats
  __shared__ double smem[kVampBwdRows * kVampBwdK + kVampBwdK * kVampBwdCols + kVampBwdK * kVampBwdCols / 2];
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
  const int nbr = cdiv(B, kVampBwdRows);
  const int c0 = blockIdx.y * kVampBwdCols, gj = c0 + col;
  if ((int)blockIdx.x < nbr) {                        // block-uniform
    double (*rs)[kVampBwdK] = reinterpret_cast<double (*)[kVampBwdK]>(smem);
    double (*ivs)[kVampBwdCols] = reinterpret_cast<double (*)[kVampBwdCols]>(smem + kVampBwdRows * kVampBwdK);
    float (*pms)[kVampBwdCols] =
        reinterpret_cast<float (*)[kVampBwdCols]>(smem + kVampBwdRows * kVampBwdK + kVampBwdK * kVampBwdCols);
    const int r0 = blockIdx.x * kVampBwdRows;
    double zr[4], acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = r0 + rg * 4 + a;
      zr[a] = (row < B && gj < D) ? (double)z[(size_t)row * D + gj] : 0.0;
    }
    for (int k0 = 0; k0 < K; k0 += kVampBwdK) {
      const int nk = min(kVampBwdK, K - k0);
#pragma unroll
      for (int u = 0; u < kVampBwdRows * kVampBwdK / kVampThreads; ++u) {
        const int e = tid + u * kVampThreads;
        const int rr = e / kVampBwdK, k = e % kVampBwdK;
        rs[rr][k] = (r0 + rr < B && k < nk) ? r[(size_t)(r0 + rr) * K + k0 + k] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kVampBwdK * kVampBwdCols / kVampThreads; ++u) {
        const int e = tid + u * kVampThreads;
        const int k = e / kVampBwdCols, c = e % kVampBwdCols;
        float pv = 0.f;
        double iv = 0.0;
        if (k < nk && c0 + c < D) {
          pv = pmu[(size_t)(k0 + k) * ldpm + c0 + c];
          iv = exp(-(double)plv[(size_t)(k0 + k) * ldpl + c0 + c]);
        }
        pms[k][c] = pv, ivs[k][c] = iv;
      }
      __syncthreads();
      for (int k = 0; k < nk; ++k) {
        const double pv = (double)pms[k][col], iv = ivs[k][col];
#pragma unroll
        for (int a = 0; a < 4; ++a) acc[a] += rs[rg * 4 + a][k] * ((zr[a] - pv) * iv);
      }
      __syncthreads();
    }
    if (gj >= D) return;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int row = r0 + rg * 4 + a;
      if (row >= B) continue;
      const double G = g ? gscale * (double)g[g_rows ? row : 0] : 0.0;
      const double gb = beta != 0.0 ? G * beta : 0.0;
      const double t = (gz ? (double)gz[(size_t)row * ldgz + gj] : 0.0) + gb * acc[a];
      const double l = (double)lv[(size_t)row * ldl + gj], n = (double)eps[(size_t)row * lde + gj];
      dmu[(size_t)row * D + gj] = (float)t;
      dlv[(size_t)row * D + gj] = (float)(0.5 * exp(0.5 * l) * (n * t) - 0.5 * gb);
    }
    return;
  }
  double (*gs)[kVampBwdRows] = reinterpret_cast<double (*)[kVampBwdRows]>(smem);
  float (*zs)[kVampBwdCols] = reinterpret_cast<float (*)[kVampBwdCols]>(smem + kVampBwdK * kVampBwdRows);
  const int q0 = ((int)blockIdx.x - nbr) * kVampBwdRows;
  double pm[4], iv[4], am[4] = {0.0, 0.0, 0.0, 0.0}, al[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int k = q0 + rg * 4 + a;
    const bool ok = k < K && gj < D;
    pm[a] = ok ? (double)pmu[(size_t)k * ldpm + gj] : 0.0;
    iv[a] = ok ? exp(-(double)plv[(size_t)k * ldpl + gj]) : 0.0;
  }
  for (int b0 = 0; b0 < B; b0 += kVampBwdK) {
    const int nb = min(kVampBwdK, B - b0);
#pragma unroll
    for (int u = 0; u < kVampBwdK * kVampBwdRows / kVampThreads; ++u) {
      const int e = tid + u * kVampThreads;
      const int b = e / kVampBwdRows, k = e % kVampBwdRows;
      double v = 0.0;
      if (b < nb && q0 + k < K && g) v = gscale * (double)g[g_rows ? b0 + b : 0] * r[(size_t)(b0 + b) * K + q0 + k];
      gs[b][k] = v;
    }
#pragma unroll
    for (int u = 0; u < kVampBwdK * kVampBwdCols / kVampThreads; ++u) {
      const int e = tid + u * kVampThreads;
      const int b = e / kVampBwdCols, c = e % kVampBwdCols;
      zs[b][c] = (b < nb && c0 + c < D) ? z[(size_t)(b0 + b) * D + c0 + c] : 0.f;
    }
    __syncthreads();
    for (int b = 0; b < nb; ++b) {
      const double zv = (double)zs[b][col];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const double w = gs[b][rg * 4 + a], d = zv - pm[a], u = d * iv[a];
        am[a] += w * u;
        al[a] += w * (1.0 - d * u);
      }
    }
    __syncthreads();
  }
  if (gj >= D) return;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int k = q0 + rg * 4 + a;
    if (k >= K) continue;
    dpmu[(size_t)k * D + gj] = (float)(beta != 0.0 ? -(beta * am[a]) : 0.0);
    dplv[(size_t)k * D + gj] = (float)(beta != 0.0 ? 0.5 * beta * al[a] : 0.0);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline int vamp_tiles(int n) { return cdiv(n, kVampTile); }
static inline bool vamp_shape_ok(int B, int K, int D) {
  return B >= 1 && B <= kVampMaxB && K >= 1 && K <= kVampMaxK && D >= 1 && D <= kVampMaxD &&
         (long long)B * K <= kVampMaxPairs;
}
// the max and sum partials of every component tile and row, and the KL of every row
static inline size_t vamp_ws(int B, int K) { return (2 * (size_t)vamp_tiles(K) + 1) * (size_t)B * sizeof(double); }
static inline size_t min_ld(size_t a, size_t b) { return a < b ? a : b; }

// nothing is launched on a failure
static int vamp_check(const char* name, bool ptrs, int B, int K, int D, double beta, size_t ld_min, size_t pld_min) {
  if (need_pointers(name, ptrs) || need_dim(name, "B = %lld rows", B, 1, kVampMaxB, "1..4096") ||
      need_dim(name, "K = %lld components", K, 1, kVampMaxK, "1..4096") ||
      need_dim(name, "D = %lld", D, 1, kVampMaxD, "1..512") ||
      need_dim(name, "B K = %lld pairs", (long long)B * K, 1, kVampMaxPairs, "1..2^22"))
    return 1;
  if (!finite(beta)) return fail("%s: beta must be a finite number", name);
  return need_stride(name, "a", ld_min, "D", D) || need_stride(name, "a component", pld_min, "D", D);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_vamp_workspace(int B, int K, int D) { return vamp_shape_ok(B, K, D) ? vamp_ws(B, K) : 0; }

int itcv_vamp_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps, size_t ld_eps,
                  const float* p_mu, size_t ld_pmu, const float* p_logvar, size_t ld_plogvar, float* z, double* L,
                  double* logq, double* logp, float* rows, float* out, float* terms, int B, int K, int D, double beta,
                  int reduce, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_vamp_fwd";
  if (int e = vamp_check(name, mu && logvar && eps && p_mu && p_logvar && z && L && logq && logp && rows && out && terms,
                         B, K, D, beta, min_ld(min_ld(ld_mu, ld_logvar), ld_eps), min_ld(ld_pmu, ld_plogvar)))
    return e;
  if (reduce < 0 || reduce > 2) return fail("%s: reduce %lld is not 0 (none), 1 (mean) or 2 (sum)", name, reduce);
  ITCV_REQUIRE(ws && ws_bytes >= vamp_ws(B, K), "itcv_vamp_fwd(workspace)");
  const int ntk = vamp_tiles(K);
  double* pmax = static_cast<double*>(ws);
  double* psum = pmax + (size_t)ntk * B;
  double* klrow = psum + (size_t)ntk * B;
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(vamp_pair_kernel<true>, dim3(ntk, vamp_tiles(B)), dim3(kVampThreads), 0, st, mu, ld_mu, logvar,
                     ld_logvar, eps, ld_eps, p_mu, ld_pmu, p_logvar, ld_plogvar, B, K, D, z, L, pmax, psum, logq);
  ITCV_CHECK_LAUNCH("itcv_vamp_fwd(pairs)");
  hipLaunchKernelGGL(vamp_finish_kernel, dim3(1 + row_grid(B, kVampFinishRows, kVampFinishBlocks)), dim3(kVampThreads), 0, st, L,
                     (const double*)pmax, (const double*)psum, (const double*)logq, B, K, ntk, beta, reduce, logp, klrow,
                     rows, out, terms);
  ITCV_CHECK_LAUNCH("itcv_vamp_fwd(finish)");
  return 0;
}

int itcv_vamp_bwd(const float* gz, size_t ld_gz, const float* g, int g_rows, double g_scale, const float* logvar,
                  size_t ld_logvar, const float* eps, size_t ld_eps, const float* z, const float* p_mu, size_t ld_pmu,
                  const float* p_logvar, size_t ld_plogvar, const double* r, float* dmu, float* dlogvar, float* dp_mu,
                  float* dp_logvar, int B, int K, int D, double beta, void* stream) {
  const char* name = "itcv_vamp_bwd";
  const size_t ld_min = min_ld(min_ld(ld_logvar, ld_eps), gz ? ld_gz : ld_eps);
  if (int e = vamp_check(name, logvar && eps && z && p_mu && p_logvar && r && dmu && dlogvar && dp_mu && dp_logvar, B, K,
                         D, beta, ld_min, min_ld(ld_pmu, ld_plogvar)))
    return e;
  if (!itcv::finite(g_scale)) return fail("%s: g_scale must be a finite number", name);
  hipLaunchKernelGGL(vamp_bwd_kernel, dim3(cdiv(B, kVampBwdRows) + cdiv(K, kVampBwdRows), cdiv(D, kVampBwdCols)),
                     dim3(kVampThreads), 0, S(stream), gz, ld_gz, g, g_rows, g_scale, logvar, ld_logvar, eps, ld_eps, z,
                     p_mu, ld_pmu, p_logvar, ld_plogvar, r, B, K, D, beta, dmu, dlogvar, dp_mu, dp_logvar);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_vamp_logprob(const float* x, size_t ld_x, const float* p_mu, size_t ld_pmu, const float* p_logvar,
                      size_t ld_plogvar, double* logp, int N, int K, int D, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_vamp_logprob";
  if (int e = vamp_check(name, x && p_mu && p_logvar && logp, N, K, D, 0.0, ld_x, min_ld(ld_pmu, ld_plogvar)))
    return e;
  ITCV_REQUIRE(ws && ws_bytes >= vamp_ws(N, K), "itcv_vamp_logprob(workspace)");
  const int ntk = vamp_tiles(K);
  double* pmax = static_cast<double*>(ws);
  double* psum = pmax + (size_t)ntk * N;
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(vamp_pair_kernel<false>, dim3(ntk, vamp_tiles(N)), dim3(kVampThreads), 0, st, x, ld_x,
                     (const float*)nullptr, (size_t)0, (const float*)nullptr, (size_t)0, p_mu, ld_pmu, p_logvar, ld_plogvar,
                     N, K, D, (float*)nullptr, (double*)nullptr, pmax, psum, (double*)nullptr);
  ITCV_CHECK_LAUNCH("itcv_vamp_logprob(pairs)");
  hipLaunchKernelGGL(vamp_logprob_finish_kernel, dim3(row_grid(N, kVampThreads, 8)), dim3(kVampThreads), 0, st,
                     (const double*)pmax, (const double*)psum, N, K, ntk, logp);
  ITCV_CHECK_LAUNCH("itcv_vamp_logprob(finish)");
  return 0;
}

}  // extern "C"
