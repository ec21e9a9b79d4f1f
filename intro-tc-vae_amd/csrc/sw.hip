// The KL hook of the sliced-Wasserstein autoencoder (Kolouri et al. 2018) and the sliced-Wasserstein distance as a score
// (Deshpande et al. 2018): coef_kl * mean KL + lambda_sw * SW^2 between the batch's sampled latents and as many draws from
// the prior, over L random directions, with its gradient.  The rules are in include/itcv_hip.h:
//   sw_project_sort : ONE block per projection l (the grid is capped; a block walks l by the grid stride).  The block
//                normalises its direction in fp64, projects every row of z_all and of the prior onto it (a wave per row,
//                lanes over d: per-lane partial sums in ascending d, then the xor butterfly -- an order that depends on D
//                alone, so equal rows get equal bits wherever they stand), turns the projections into monotone uint64
//                keys (sign-flip map, -0 canonicalised) and sorts (key, row) pairs of z and the keys of the prior with
//                udr.hip's upward-pointing bitonic network: a pair whose upper index is past Bt is skipped, so any Bt
//                works without padding.  The pair (key, row) is compared as a pair, which makes the order the stable one
//                and total for any keys.  It then writes the differences of the sorted projections back to the rows they
//                came from (G[l][row]: the backward needs no permutation), folds their squares in index order into
//                per[l], and writes Theta[l].  The keys sit in LDS up to kSwLdsRows rows (20 B a row), above that in one
//                slice of the caller's workspace per resident block.  The step of the network is one function for both;
//                on the workspace path the steps that stay inside an aligned chunk of 4096 rows run on the chunk staged
//                in LDS and only the few that cross chunks run on the workspace in place.
//   sw_finish  : block 0 folds per[L] (objective.h's ordered_sum) and the KL of the local rows (mean_kl_rows) into the
//                scalar and the three logged terms.
//   sw_bwd     : ONE launch, a kSwBwdRows x kSwBwdCols tile of [Bt, D] per block: sum_l G[l][i] Theta[l][d] in fp64, l
//                ascending, over LDS-staged chunks of kSwBwdK projections; the blocks behind those write the KL gradient
//                of the local rows.
// Every sum has a fixed order, there is no atomic, and nothing depends on the grid, on where the keys sit or on timing:
// the same inputs give the same bits.  Nothing in this file may be contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kSwMaxBt = 1 << 20;
constexpr int kSwMaxL = 4096;
constexpr int kSwMaxD = 2048;
constexpr int kSwMaxBl = 1 << 24;
constexpr long long kSwMaxG = 1ll << 26;  // L * Bt doubles of G: 512 MiB
constexpr int kSwThreads = 1024;
constexpr int kSwLdsRows = 4096;          // 80 KiB of keys next to 24 KiB of direction and fold scratch: of the CU's 160 KiB
constexpr int kSwRowBytes = 20;           // uint64 key + int32 row of z, uint64 key of the prior
constexpr int kSwMaxBlocks = 256;         // one block per CU
constexpr int kSwBwdRows = 16;
constexpr int kSwBwdCols = 64;
constexpr int kSwBwdK = 32;
constexpr int kSwBwdThreads = 256;

// the test options "sw_lds_rows" / "sw_max_blocks" (itcv_set_option in abi.hip): 0 = the constants above
int g_sw_lds_rows = 0;
int g_sw_max_blocks = 0;

// ascending in the numeric order of doubles; +0 and -0 share one key, denormals are ordinary values, and the map is total
// (a NaN sorts behind +inf or before -inf by its sign bit)
__device__ __forceinline__ uint64_t sw_key(double v) {
  uint64_t u = (uint64_t)__double_as_longlong(v);
  if ((u << 1) == 0) u = 0;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double sw_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// sum_d theta[d] x[d] by one wave: lane partial sums over d = lane, lane + 64, ... ascending, then the xor butterfly,
// which leaves the same bits in every lane
__device__ __forceinline__ double sw_dot(const double* __restrict__ theta, const float* __restrict__ x, int D, int lane) {
  double s = 0.0;
  for (int d = lane; d < D; d += 64) s += theta[d] * (double)x[d];
  return wave_sum(s);
}

// One step of the bitonic network of udr_rank_kernel on n (key, row) pairs of z and n keys of the prior: merging runs of
// k / 2 into runs of k, the first step (s == k / 2) pairs i with its mirror image in the run of k, the following steps
// pair i with i + s; the smaller always goes to the lower index, and a pair whose upper index is past n is skipped (the
// missing tail behaves as +infinity and never moves).  (key, row) is compared as a pair: the stable order, total for any
// keys.  p numbers the pairs of a step: `half` of them.  No barrier inside.
__device__ __forceinline__ void sw_sort_step(uint64_t* uk, uint64_t* vk, int* row, int n, int half, int k, int s, int tid) {
  const bool mirror = s == (k >> 1);
  for (int p = tid; p < half; p += kSwThreads) {
    const int i = ((p & ~(s - 1)) << 1) | (p & (s - 1));
    const int j = mirror ? (i ^ (k - 1)) : (i | s);
    if (j < n) {                                        // i < j always
      const uint64_t a = uk[i], b = uk[j];
      const int ra = row[i], rb = row[j];
      if (a > b || (a == b && ra > rb)) uk[i] = b, uk[j] = a, row[i] = rb, row[j] = ra;
      const uint64_t c = vk[i], e = vk[j];
      if (c > e) vk[i] = e, vk[j] = c;
    }
  }
}

// the whole network on n entries, a barrier behind every step
__device__ __forceinline__ void sw_sort_all(uint64_t* uk, uint64_t* vk, int* row, int n, int tid) {
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int s = k >> 1; s >= 1; s >>= 1) {
      sw_sort_step(uk, vk, row, n, np2 >> 1, k, s, tid);
      __syncthreads();
    }
  }
}

__device__ __forceinline__ void sw_copy_rows(uint64_t* __restrict__ duk, uint64_t* __restrict__ dvk, int* __restrict__ drow,
                                             const uint64_t* __restrict__ suk, const uint64_t* __restrict__ svk,
                                             const int* __restrict__ srow, int n, int tid) {
  for (int i = tid; i < n; i += kSwThreads) duk[i] = suk[i], dvk[i] = svk[i], drow[i] = srow[i];
  __syncthreads();
}

// dynamic LDS: theta [D rounded up to even] | red [kSwThreads] | ukey [R] | vkey [R] | row [R], R = Bt (IN_LDS) or chunk.
// !IN_LDS: the keys sit in this block's slice of the workspace, and the LDS arrays stage one aligned chunk of `chunk` rows
// (a power of two) at a time: every step of the network whose pairs lie inside a chunk (s < chunk) runs on the staged
// chunk, the others (s >= chunk) on the workspace in place.  The steps and their order are those of the LDS path; the
// sorted sequence -- unique, because (key, row) is a total order -- is the same.
template <bool IN_LDS>
__global__ __launch_bounds__(kSwThreads) void sw_project_sort_kernel(const float* __restrict__ z, size_t ldz,
                                                                     const float* __restrict__ pr, size_t ldp,
                                                                     const float* __restrict__ t, int Bt, int L, int D,
                                                                     char* __restrict__ ws, size_t slice, int chunk,
                                                                     double* __restrict__ per, double* __restrict__ Theta,
                                                                     double* __restrict__ G) {
  extern __shared__ double sw_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, T = kSwThreads;
  double* theta = sw_lds;
  double* red = theta + ((D + 1) & ~1);
  const int R = IN_LDS ? Bt : chunk;
  uint64_t* luk = reinterpret_cast<uint64_t*>(red + T);
  uint64_t* lvk = luk + R;
  int* lrow = reinterpret_cast<int*>(lvk + R);
  uint64_t* uk = IN_LDS ? luk : reinterpret_cast<uint64_t*>(ws + (size_t)blockIdx.x * slice);
  uint64_t* vk = IN_LDS ? lvk : uk + Bt;
  int* row = IN_LDS ? lrow : reinterpret_cast<int*>(vk + Bt);
  for (int l = blockIdx.x; l < L; l += gridDim.x) {   // block-uniform
    // the direction: theta = t_l / |t_l|, the norm in fp64 (thread partial sums over d = tid, tid + 1024, then the wave
    // butterflies and the wave totals in wave order: an order that depends on D alone); a zero row stays zero
    double n2 = 0.0;
    for (int d = tid; d < D; d += T) {
      const double v = (double)t[(size_t)l * D + d];
      n2 += v * v;
    }
    n2 = block_sum(n2, red);
    const double nrm = sqrt(n2);
    for (int d = tid; d < D; d += T) {
      const double v = (double)t[(size_t)l * D + d];
      const double th = nrm > 0.0 ? v / nrm : 0.0;
      theta[d] = th;
      Theta[(size_t)l * D + d] = th;
    }
    __syncthreads();
    // four rows of a wave at a time: their loads are in flight together (a row at a time is one exposed memory round
    // trip per row); the sum of a row is sw_dot's whichever way it is reached
    constexpr int kRows = 4, kWaves = kSwThreads / 64;
    int i0 = wid;
    for (; i0 + (kRows - 1) * kWaves < Bt; i0 += kRows * kWaves) {
      double su[kRows], sv[kRows];
#pragma unroll
      for (int a = 0; a < kRows; ++a) su[a] = 0.0, sv[a] = 0.0;
      for (int d = lane; d < D; d += 64) {
        const double th = theta[d];
        float zv[kRows], pv[kRows];
#pragma unroll
        for (int a = 0; a < kRows; ++a) {
          zv[a] = z[(size_t)(i0 + a * kWaves) * ldz + d];
          pv[a] = pr[(size_t)(i0 + a * kWaves) * ldp + d];
        }
#pragma unroll
        for (int a = 0; a < kRows; ++a) su[a] += th * (double)zv[a], sv[a] += th * (double)pv[a];
      }
#pragma unroll
      for (int a = 0; a < kRows; ++a) {
        const double u = wave_sum(su[a]), v = wave_sum(sv[a]);
        const int i = i0 + a * kWaves;
        if (lane == 0) uk[i] = sw_key(u), vk[i] = sw_key(v), row[i] = i;
      }
    }
    for (int i = i0; i < Bt; i += kWaves) {
      const double u = sw_dot(theta, z + (size_t)i * ldz, D, lane);
      const double v = sw_dot(theta, pr + (size_t)i * ldp, D, lane);
      if (lane == 0) uk[i] = sw_key(u), vk[i] = sw_key(v), row[i] = i;
    }
    __syncthreads();
    if (IN_LDS) {
      sw_sort_all(uk, vk, row, Bt, tid);
    } else {
      int np2 = 1;
      while (np2 < Bt) np2 <<= 1;
      // runs up to `chunk`: the whole network of every chunk, staged
      if (chunk >= 2) {
        for (int c0 = 0; c0 < Bt; c0 += chunk) {
          const int n = min(chunk, Bt - c0);
          sw_copy_rows(luk, lvk, lrow, uk + c0, vk + c0, row + c0, n, tid);
          sw_sort_all(luk, lvk, lrow, n, tid);
          sw_copy_rows(uk + c0, vk + c0, row + c0, luk, lvk, lrow, n, tid);
        }
      }
      // longer runs: the steps across chunks in place, then the steps inside every chunk, staged
      for (int k = 2 * chunk; k <= np2; k <<= 1) {
        for (int s = k >> 1; s >= chunk; s >>= 1) {
          sw_sort_step(uk, vk, row, Bt, np2 >> 1, k, s, tid);
          __syncthreads();
        }
        if (chunk >= 2) {
          for (int c0 = 0; c0 < Bt; c0 += chunk) {
            const int n = min(chunk, Bt - c0);
            sw_copy_rows(luk, lvk, lrow, uk + c0, vk + c0, row + c0, n, tid);
            for (int s = chunk >> 1; s >= 1; s >>= 1) {
              sw_sort_step(luk, lvk, lrow, n, chunk >> 1, k, s, tid);
              __syncthreads();
            }
            sw_copy_rows(uk + c0, vk + c0, row + c0, luk, lvk, lrow, n, tid);
          }
        }
      }
    }
    // the differences go back to the rows they came from; their squares take the place of the prior's keys
    double* sq = reinterpret_cast<double*>(vk);
    for (int i = tid; i < Bt; i += T) {
      const double dlt = sw_value(uk[i]) - sw_value(vk[i]);
      if (G) G[(size_t)l * Bt + row[i]] = dlt;
      sq[i] = dlt * dlt;
    }
    __syncthreads();
    const double s2 = ordered_sum<kSwThreads>(sq, (size_t)Bt, red);
    if (tid == 0) per[l] = s2 / (double)Bt;
    __syncthreads();                                    // the next trip overwrites theta, red and the keys
  }
}

// out[0] = coef_kl * mean_{local rows} KL + lambda * SW^2, terms[3] = {mean KL, SW^2, max_l SW_l^2}
__global__ __launch_bounds__(1024) void sw_finish_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int Bl,
                                                         int D, int L, const double* __restrict__ per, double lambda,
                                                         double coef_kl, float* __restrict__ out,
                                                         float* __restrict__ terms) {
  __shared__ double red[1024];
  __shared__ double klw[16];
  const int tid = threadIdx.x;
  const double total = ordered_sum<1024>(per, (size_t)L, red);
  double m = 0.0;
  for (int l = tid; l < L; l += 1024) m = per[l] > m ? per[l] : m;
  __syncthreads();
  red[tid] = m;
  __syncthreads();
  const double kl = mu ? mean_kl_rows(mu, lv, (size_t)D, Bl, D, klw) : 0.0;
  if (tid == 0) {
    for (int k = 1; k < 1024; ++k) m = red[k] > m ? red[k] : m;
    const double sw2 = total / (double)L;
    out[0] = (float)((coef_kl != 0.0 ? coef_kl * kl : 0.0) + lambda * sw2);
    terms[0] = (float)kl, terms[1] = (float)sw2, terms[2] = (float)m;
  }
}

// blocks x < cdiv(Bt, 16): dz_all = g lambda 2 / (L Bt) sum_l G[l][i] Theta[l][d]; the blocks behind them: dmu / dlogvar
// of the local rows
__global__ __launch_bounds__(kSwBwdThreads) void sw_bwd_kernel(const float* __restrict__ g, const float* __restrict__ mu,
                                                               const float* __restrict__ lv, const double* __restrict__ G,
                                                               const double* __restrict__ Theta, int Bl, int Bt, int L,
                                                               int D, double lambda, double coef_kl,
                                                               float* __restrict__ dz, float* __restrict__ dmu,
                                                               float* __restrict__ dlv) {
  __shared__ double gsh[kSwBwdK][kSwBwdRows];
  __shared__ double ths[kSwBwdK][kSwBwdCols];
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
  const int nbz = cdiv(Bt, kSwBwdRows);
  const int c0 = blockIdx.y * kSwBwdCols, gj = c0 + col;
  const double g0 = (double)g[0];
  if ((int)blockIdx.x >= nbz) {                       // block-uniform, before any barrier
    if (gj >= D) return;
    const double ckl = coef_kl != 0.0 ? coef_kl / (double)Bl : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int r = ((int)blockIdx.x - nbz) * kSwBwdRows + rg * 4 + a;
      if (r >= Bl) continue;
      const size_t at = (size_t)r * D + gj;
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
  const int r0 = blockIdx.x * kSwBwdRows;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int l0 = 0; l0 < L; l0 += kSwBwdK) {
    const int nl = min(kSwBwdK, L - l0);
#pragma unroll
    for (int u = 0; u < kSwBwdK * kSwBwdRows / kSwBwdThreads; ++u) {
      const int e = tid + u * kSwBwdThreads;
      const int k = e / kSwBwdRows, r = e % kSwBwdRows;
      gsh[k][r] = (k < nl && r0 + r < Bt) ? G[(size_t)(l0 + k) * Bt + r0 + r] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kSwBwdK * kSwBwdCols / kSwBwdThreads; ++u) {
      const int e = tid + u * kSwBwdThreads;
      const int k = e / kSwBwdCols, c = e % kSwBwdCols;
      ths[k][c] = (k < nl && c0 + c < D) ? Theta[(size_t)(l0 + k) * D + c0 + c] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nl; ++k) {
      const double th = ths[k][col];
#pragma unroll
      for (int a = 0; a < 4; ++a) acc[a] += gsh[k][rg * 4 + a] * th;
    }
    __syncthreads();
  }
  if (gj >= D) return;
  const double f = g0 * lambda * (2.0 / ((double)L * (double)Bt));
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int r = r0 + rg * 4 + a;
    if (r >= Bt) continue;
    dz[(size_t)r * D + gj] = (float)(f * acc[a]);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline int sw_lds_rows() { return g_sw_lds_rows > 0 && g_sw_lds_rows < kSwLdsRows ? g_sw_lds_rows : kSwLdsRows; }
static inline int sw_blocks(int L) { return row_grid(L, 1, g_sw_max_blocks > 0 ? g_sw_max_blocks : kSwMaxBlocks); }
static inline size_t sw_slice(int Bt) { return align_up((size_t)Bt * kSwRowBytes, 16); }
static inline size_t sw_ws(int Bt, int L) {
  return Bt > sw_lds_rows() ? (size_t)sw_blocks(L) * sw_slice(Bt) : 0;
}
// rows of the staged chunk of the workspace path: the largest power of two that the rows kept in LDS allow
static inline int sw_chunk() {
  int c = 1;
  while (2 * c <= sw_lds_rows()) c <<= 1;
  return c;
}
static inline size_t sw_lds_bytes(int rows, int D) {
  return ((size_t)((D + 1) & ~1) + kSwThreads) * sizeof(double) + sw_slice(rows);
}

// nothing is launched on a failure
static int sw_check(const char* name, bool ptrs, int Bl, int Bt, int L, int D, bool with_g, double lambda, double coef_kl) {
  if (need_pointers(name, ptrs) || need_dim(name, "Bt = %lld rows", Bt, 1, kSwMaxBt, "1..2^20") ||
      need_dim(name, "L = %lld projections", L, 1, kSwMaxL, "1..4096") ||
      need_dim(name, "D = %lld", D, 1, kSwMaxD, "1..2048") ||
      need_dim(name, "Bl = %lld local rows", Bl, 1, kSwMaxBl, "1..2^24"))
    return 1;
  if (with_g && (long long)L * Bt > kSwMaxG) return fail("%s: L * Bt = %lld is above 2^26", name, (long long)L * Bt);
  if (!(lambda >= 0.0 && finite(lambda))) return fail("%s: lambda_sw must be a finite number >= 0", name);
  if (!finite(coef_kl)) return fail("%s: coef_kl must be a finite number", name);
  return 0;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_sw_lds_rows(void) { return sw_lds_rows(); }

size_t itcv_sw_workspace(int Bt, int L, int D) {
  return (Bt >= 1 && Bt <= kSwMaxBt && L >= 1 && L <= kSwMaxL && D >= 1 && D <= kSwMaxD) ? sw_ws(Bt, L) : 0;
}

int itcv_sw_kl_fwd(const float* z_all, size_t ldz, const float* prior, size_t ldp, const float* t, const float* mu,
                   const float* logvar, float* out, float* terms, double* per, double* Theta, double* G, int Bl, int Bt,
                   int L, int D, double lambda_sw, double coef_kl, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_sw_kl_fwd";
  // mu and logvar may both be NULL when coef_kl == 0 (the score): no KL is read and terms[0] is 0
  const bool kl_ptrs = (mu && logvar) || (!mu && !logvar && coef_kl == 0.0);
  if (int e = sw_check(name, z_all && prior && t && kl_ptrs && out && terms && per && Theta, Bl, Bt, L, D, G != nullptr,
                       lambda_sw, coef_kl))
    return e;
  if (need_stride(name, "z_all's", ldz, "D", D) || need_stride(name, "prior's", ldp, "D", D)) return 1;
  const size_t need = sw_ws(Bt, L);
  ITCV_REQUIRE(ws_bytes >= need && (need == 0 || ws), "itcv_sw_kl_fwd(workspace)");
  const bool in_lds = Bt <= sw_lds_rows();
  const int blocks = sw_blocks(L);
  hipStream_t st = S(stream);
  if (in_lds)
    launch_lds<sw_project_sort_kernel<true>>(dim3(blocks), dim3(kSwThreads), sw_lds_bytes(Bt, D), st, z_all, ldz, prior, ldp,
                                             t, Bt, L, D, (char*)nullptr, (size_t)0, 0, per, Theta, G);
  else
    launch_lds<sw_project_sort_kernel<false>>(dim3(blocks), dim3(kSwThreads), sw_lds_bytes(sw_chunk(), D), st, z_all, ldz,
                                              prior, ldp, t, Bt, L, D, static_cast<char*>(ws), sw_slice(Bt), sw_chunk(), per,
                                              Theta, G);
  ITCV_CHECK_LAUNCH("itcv_sw_kl_fwd(project and sort)");
  hipLaunchKernelGGL(sw_finish_kernel, dim3(1), dim3(1024), 0, st, mu, logvar, Bl, D, L, (const double*)per, lambda_sw,
                     coef_kl, out, terms);
  ITCV_CHECK_LAUNCH("itcv_sw_kl_fwd(finish)");
  return 0;
}

int itcv_sw_kl_bwd(const float* g, const float* mu, const float* logvar, const double* G, const double* Theta,
                   float* dz_all, float* dmu, float* dlogvar, int Bl, int Bt, int L, int D, double lambda_sw,
                   double coef_kl, void* stream) {
  const char* name = "itcv_sw_kl_bwd";
  if (int e = sw_check(name, g && mu && logvar && G && Theta && dz_all && dmu && dlogvar, Bl, Bt, L, D, true, lambda_sw,
                       coef_kl))
    return e;
  hipLaunchKernelGGL(sw_bwd_kernel, dim3(cdiv(Bt, kSwBwdRows) + cdiv(Bl, kSwBwdRows), cdiv(D, kSwBwdCols)),
                     dim3(kSwBwdThreads), 0, S(stream), g, mu, logvar, G, Theta, Bl, Bt, L, D, lambda_sw, coef_kl, dz_all,
                     dmu, dlogvar);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
