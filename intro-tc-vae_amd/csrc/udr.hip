// The two device primitives of the Unsupervised Disentanglement Ranking (Duan et al. 2020; disentanglement_lib's `udr`).
// The rules are in include/itcv_hip.h:
//   udr_ranks : ONE block per column.  Every value becomes a monotone uint32 key (sign-flip map, -0 canonicalised); the keys
//               of the column are sorted in place by a bitonic network whose compare-exchanges all point upwards, so that
//               a pair whose upper index is past N is simply skipped (the missing tail behaves as +infinity and never
//               moves): any N, no padding, no second buffer.  Every row then finds L = #{keys < its key} and H = #{keys <=
//               its key} by two binary searches and writes L + H + 1, twice scipy's tie-averaged rank, an exact integer.
//               The sorted keys sit in LDS up to kRankLdsRows rows, above that in the caller's workspace; the code is the
//               same (a __syncthreads orders the block's own global writes).
//   udr_lasso : the covariance is normalised to the correlation R once (its own launch, into the workspace), then ONE WAVE
//               per target column runs cyclic coordinate descent in fp64: lane l holds w[l], w[l + 64], ... and the
//               matching entries of c in registers; the sum of coordinate k is a per-lane partial sum in ascending index
//               followed by the xor butterfly, and only the lane that owns w[k] applies the update, so nothing is
//               broadcast.  Eight waves (targets) share a block; G = R[:Da, :Da] sits in LDS up to kLassoLdsDim, above
//               that its rows are read from the workspace.  A last one-thread launch folds the per-target records into
//               info[3].
// Nothing depends on the grid or on timing: the same inputs give the same bits.  The only atomic is the integer OR that
// raises the sticky non-finite flag.  Nothing in this file may be contracted into a fused multiply-add.
#include "dense.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kUdrMaxD = kMatrixMaxDim;   // the limits of itcv_unsup_cov
constexpr int kUdrMaxN = 1 << 24;
constexpr int kRankThreads = 1024;
constexpr int kRankLdsRows = 32768;       // 128 KiB of keys; the in-place sort needs nothing else of the CU's 160 KiB
constexpr int kLassoLdsDim = 128;         // 128 x 129 doubles = 129 KiB
constexpr int kLassoWaves = 8;            // targets per block
constexpr int kLassoRegs = kUdrMaxD / 64; // coordinates per lane

// ---- ranks -----------------------------------------------------------------------------------------------------------
// ascending in the numeric order of finite floats; +0 and -0 share one key, denormals are ordinary values
__device__ __forceinline__ uint32_t rank_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool IN_LDS>
__global__ __launch_bounds__(kRankThreads) void udr_rank_kernel(const float* __restrict__ x, size_t ld, int N, int D,
                                                                uint32_t* __restrict__ wsk, float* __restrict__ r2,
                                                                int* __restrict__ flags) {
  extern __shared__ uint32_t udr_keys[];
  const int d = blockIdx.x, tid = threadIdx.x, T = kRankThreads;
  uint32_t* keys = IN_LDS ? udr_keys : wsk + (size_t)d * N;
  bool bad = false;
  for (int n = tid; n < N; n += T) {
    const float v = x[(size_t)n * ld + d];
    bad |= !finite_f(v);
    keys[n] = rank_key(v);
  }
  if (bad) atomicOr(&flags[0], 1);
  __syncthreads();
  // Bitonic sort of keys[0, N).  Merging runs of k / 2 into runs of k: the first step pairs i with its mirror image in
  // the run of k (i ^ (k - 1)), the following steps pair i with i + s, s = k / 4 .. 1; the smaller key always goes to the
  // lower index.  p numbers the pairs of a step; the number of pairs is half of N rounded up to a power of two.
  int np2 = 1;
  while (np2 < N) np2 <<= 1;
  const int half = np2 >> 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int s = k >> 1; s >= 1; s >>= 1) {
      const bool mirror = s == (k >> 1);
      for (int p = tid; p < half; p += T) {
        const int i = ((p & ~(s - 1)) << 1) | (p & (s - 1));
        const int j = mirror ? (i ^ (k - 1)) : (i | s);
        if (j < N) {                                  // i < j always
          const uint32_t a = keys[i], b = keys[j];
          if (a > b) keys[i] = b, keys[j] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int n = tid; n < N; n += T) {
    const uint32_t key = rank_key(x[(size_t)n * ld + d]);
    int lo = 0, hi = N;
    while (lo < hi) {                                 // L = #{keys < key}
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int L = lo;
    hi = N;
    while (lo < hi) {                                 // H = #{keys <= key}
      const int mid = (lo + hi) >> 1;
      if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    r2[(size_t)n * D + d] = (float)(L + lo + 1);
  }
}

// ---- Lasso -----------------------------------------------------------------------------------------------------------
// R[k][l] = C[k][l] / sqrt(C[k][k] C[l][l]); a column of variance exactly 0 has its row and column 0, the diagonal too
__global__ __launch_bounds__(256) void udr_corr_kernel(const double* __restrict__ C, int Dt, double* __restrict__ R) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Dt * Dt) return;
  const int k = e / Dt, l = e - k * Dt;
  const double ckk = C[(size_t)k * Dt + k], cll = C[(size_t)l * Dt + l];
  R[e] = (ckk == 0.0 || cll == 0.0) ? 0.0 : C[e] / sqrt(ckk * cll);
}

// sum_l G[k][l] w[l] over l < Da (without l == skip): lane partial sums in ascending l, then the xor butterfly, which
// leaves the same bits in every lane
__device__ __forceinline__ double lasso_row_dot(const double* __restrict__ row, const double (&w)[kLassoRegs], int Da,
                                                int lane, int skip) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kLassoRegs; ++j) {
    const int l = j * 64 + lane;
    if (j * 64 < Da && l < Da && l != skip) s += row[l] * w[j];
  }
  return wave_sum(s);
}

// rec[t] = {not converged, sweeps}
template <bool IN_LDS>
__global__ __launch_bounds__(kLassoWaves * 64) void udr_lasso_kernel(const double* __restrict__ R, int Da, int Db,
                                                                     double alpha, double gtol, int max_sweeps,
                                                                     double* __restrict__ W, int* __restrict__ rec) {
  extern __shared__ double udr_g[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int Dt = Da + Db;
  const int lda = IN_LDS ? (Da | 1) : Dt;
  if (IN_LDS) {
    for (int e = tid; e < Da * Da; e += kLassoWaves * 64) {
      const int i = e / Da, j = e - i * Da;
      udr_g[i * lda + j] = R[(size_t)i * Dt + j];
    }
    __syncthreads();
  }
  const double* G = IN_LDS ? udr_g : R;
  const int t = blockIdx.x * kLassoWaves + wid;
  if (t >= Db) return;                                // wave-uniform, after the only barrier
  double w[kLassoRegs], c[kLassoRegs];
#pragma unroll
  for (int j = 0; j < kLassoRegs; ++j) {
    const int l = j * 64 + lane;
    w[j] = 0.0;
    c[j] = l < Da ? R[(size_t)l * Dt + Da + t] : 0.0;
  }
  int sweeps = 0;
  bool conv = false;
  for (;;) {
#pragma unroll
    for (int j = 0; j < kLassoRegs; ++j) {
      if (j * 64 < Da) {
        const int kend = min(64, Da - j * 64);
        for (int kk = 0; kk < kend; ++kk) {
          const int k = j * 64 + kk;
          const double* row = G + (size_t)k * lda;
          const double s = lasso_row_dot(row, w, Da, lane, k);
          if (lane == kk) {
            const double gkk = row[k];
            const double rho = c[j] - s;
            const double st = rho > alpha ? rho - alpha : (rho < -alpha ? rho + alpha : 0.0);
            w[j] = gkk != 0.0 ? st / gkk : 0.0;
          }
        }
      }
    }
    ++sweeps;
    // the stop test: v = max_k of the distance of the gradient from the subdifferential; a nan anywhere keeps going
    double v = 0.0;
    bool sawnan = false;
#pragma unroll
    for (int j = 0; j < kLassoRegs; ++j) {
      if (j * 64 < Da) {
        const int kend = min(64, Da - j * 64);
        for (int kk = 0; kk < kend; ++kk) {
          const int k = j * 64 + kk;
          const double s = lasso_row_dot(G + (size_t)k * lda, w, Da, lane, -1);
          if (lane == kk) {
            const double g = s - c[j], wk = w[j];
            const double val = wk != 0.0 ? fabs(g + (wk > 0.0 ? alpha : -alpha)) : fmax(fabs(g) - alpha, 0.0);
            sawnan |= !(g == g);
            if (val > v) v = val;
          }
        }
      }
    }
    v = wave_max(v);
    if (__ballot(sawnan) == 0ull && v <= gtol) {
      conv = true;
      break;
    }
    if (sweeps >= max_sweeps) break;
  }
#pragma unroll
  for (int j = 0; j < kLassoRegs; ++j) {
    const int l = j * 64 + lane;
    if (l < Da) W[(size_t)l * Db + t] = fabs(w[j]);
  }
  if (lane == 0) rec[2 * t] = conv ? 0 : 1, rec[2 * t + 1] = sweeps;
}

// info[3] = {any target not converged, how many, the largest sweep count}
__global__ __launch_bounds__(64) void udr_lasso_info_kernel(const int* __restrict__ rec, int Db, int* __restrict__ info) {
  if (threadIdx.x != 0) return;
  int bad = 0, most = 0;
  for (int t = 0; t < Db; ++t) bad += rec[2 * t], most = max(most, rec[2 * t + 1]);
  info[0] = bad ? 1 : 0, info[1] = bad, info[2] = most;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline bool rank_shape_ok(int N, int D) { return N >= 2 && N <= kUdrMaxN && D >= 1 && D <= kUdrMaxD; }
static inline size_t rank_ws(int N, int D) { return N > kRankLdsRows ? (size_t)N * D * sizeof(uint32_t) : 0; }
static inline bool lasso_shape_ok(int Da, int Db) { return Da >= 1 && Db >= 1 && Da + Db <= kUdrMaxD; }
struct LassoWs {
  size_t corr, rec, total;
};
static inline LassoWs lasso_ws(int Da, int Db) {
  LassoWs w;
  w.corr = 0;
  w.rec = w.corr + (size_t)(Da + Db) * (Da + Db) * sizeof(double);
  w.total = w.rec + (size_t)Db * 2 * sizeof(int);
  return w;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_udr_rank_lds_rows(void) { return kRankLdsRows; }

size_t itcv_udr_ranks_workspace(int N, int D) { return rank_shape_ok(N, D) ? rank_ws(N, D) : 0; }

int itcv_udr_ranks(const float* x, size_t ld, int N, int D, float* r2, int* flags, void* ws, size_t ws_bytes,
                   void* stream) {
  const char* name = "itcv_udr_ranks";
  if (need_dim(name, "N = %lld rows", N, 2, kUdrMaxN, "2..2^24") || need_dim(name, "D = %lld", D, 1, kUdrMaxD, "1..512"))
    return 1;
  const size_t need = rank_ws(N, D);
  ITCV_REQUIRE(ws_bytes >= need && (need == 0 || ws), "itcv_udr_ranks(workspace)");
  ITCV_REQUIRE(x && r2 && flags && ld >= (size_t)D, name);
  hipStream_t st = S(stream);
  if (N <= kRankLdsRows)
    launch_lds<udr_rank_kernel<true>>(dim3(D), dim3(kRankThreads), (size_t)N * sizeof(uint32_t), st, x, ld, N, D,
                                      (uint32_t*)nullptr, r2, flags);
  else
    hipLaunchKernelGGL(udr_rank_kernel<false>, dim3(D), dim3(kRankThreads), 0, st, x, ld, N, D, static_cast<uint32_t*>(ws),
                       r2, flags);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_udr_lasso_workspace(int Da, int Db) { return lasso_shape_ok(Da, Db) ? lasso_ws(Da, Db).total : 0; }

int itcv_udr_lasso(const double* cov, int Da, int Db, double alpha, double gtol, int max_sweeps, double* W, int* info,
                   void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_udr_lasso";
  if (Da < 1 || Db < 1) return fail("%s: Da = %lld, Db = %lld: both must be at least 1", name, Da, Db);
  if (Da + Db > kUdrMaxD) return fail("%s: Da + Db = %lld is above 512", name, (long long)Da + Db);
  if (!(alpha >= 0.0) || !(alpha <= DBL_MAX)) return fail("%s: alpha must be a finite number >= 0", name);
  if (!(gtol >= 0.0)) return fail("%s: gtol must be >= 0", name);
  if (max_sweeps < 1) return fail("%s: max_sweeps = %lld is below 1", name, max_sweeps);
  const LassoWs w = lasso_ws(Da, Db);
  ITCV_REQUIRE(ws && ws_bytes >= w.total, "itcv_udr_lasso(workspace)");
  ITCV_REQUIRE(cov && W && info, name);
  char* base = static_cast<char*>(ws);
  double* R = reinterpret_cast<double*>(base + w.corr);
  int* rec = reinterpret_cast<int*>(base + w.rec);
  const int Dt = Da + Db;
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(udr_corr_kernel, dim3(cdiv(Dt * Dt, 256)), dim3(256), 0, st, cov, Dt, R);
  ITCV_CHECK_LAUNCH(name);
  const dim3 grid(cdiv(Db, kLassoWaves)), block(kLassoWaves * 64);
  if (Da <= kLassoLdsDim)
    launch_lds<udr_lasso_kernel<true>>(grid, block, (size_t)Da * (Da | 1) * sizeof(double), st, (const double*)R, Da, Db,
                                       alpha, gtol, max_sweeps, W, rec);
  else
    hipLaunchKernelGGL(udr_lasso_kernel<false>, grid, block, 0, st, (const double*)R, Da, Db, alpha, gtol, max_sweeps, W,
                       rec);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(udr_lasso_info_kernel, dim3(1), dim3(64), 0, st, (const int*)rec, Db, info);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
