// Ex-post latent density: a full-covariance Gaussian mixture on the device (Ghosh et al. 2020, section 4; the EM rules of
// sklearn.mixture.GaussianMixture(covariance_type="full")).  The rules are in include/itcv_hip.h; all arithmetic is fp64
// on fp32 rows x[N][D] (row stride ld):
//   gmm_factor : one block per component: the Cholesky factor L_k of C_k in place (block_cholesky of csrc/dense.h), its
//                inverse by a right-looking forward substitution, the log-determinant; the matrix sits in LDS up to
//                kLdsMatrixDim, above that the block works in the caller's buffer itself;
//   gmm_estep  : y = Linv_k (x - m_k) on v_mfma_f64_16x16x4_f64, one wave per 16 rows and one component, the tiles above
//                the diagonal of Linv_k skipped, |y|^2 folded in ascending column order; then one thread per row takes
//                the max-shifted log-sum-exp over ascending k and the last block folds the block sums in block order;
//   gmm_mstep  : the weighted column sums, the means, then the weighted covariance of the centred values on the f64 matrix
//                cores, one tile pair, row slice and component per wave: the covariance pass of csrc/dense.h, which
//                itcv_unsup_cov runs unweighted, so with K = 1 and unit responsibilities the M-step adds what that call
//                adds, in its order (tests/test_hip_score_bits.py holds it to that);
//   gmm_sample : z = (float)(m_k + L_k eps), one wave per row.
// Every floating-point reduction has a fixed order that depends on the shapes alone, never on the grid; the only atomics
// are integer ones (the flags, the counter that finds the last block).  Nothing in this file may be contracted into a
// fused multiply-add.
#include "dense.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kGmmMaxD = kMatrixMaxDim;
constexpr int kGmmMaxN = 1 << 24;
constexpr int kGmmMaxK = 64;
constexpr double kLog2Pi = 1.8378770664093453;

// ---- factor ------------------------------------------------------------------------------------------------------------
// grid (component), 1024 threads.  A[D][lda] is the working matrix: LDS, or the component's own [D][D] of `chol` (a
// __syncthreads orders the block's own global writes).  X = Linv is built in its output: X = I, then for k ascending row k
// is divided by L[k][k] and L[i][k] X[k][j] is taken off X[i][j] for every i > k, j <= k.
template <bool IN_LDS>
__global__ __launch_bounds__(kMatrixThreads) void gmm_factor_kernel(double* __restrict__ chol, int D,
                                                                    double* __restrict__ linv,
                                                                    double* __restrict__ logdet, int* __restrict__ info) {
  extern __shared__ double gm_lds[];
  const int tid = threadIdx.x, T = kMatrixThreads;
  const int comp = blockIdx.x;
  double* G = chol + (size_t)comp * D * D;
  double* X = linv + (size_t)comp * D * D;
  const int lda = IN_LDS ? (D | 1) : D;
  double* A = IN_LDS ? gm_lds : G;
  const double nan = __builtin_nan("");

  if (IN_LDS) {
    for (int e = tid; e < D * D; e += T) {
      const int i = e / D, j = e - i * D;
      A[(size_t)i * lda + j] = G[e];
    }
  }
  __syncthreads();
  const int fail_dim = block_cholesky<kMatrixThreads>(A, lda, D);
  if (fail_dim >= 0) {
    __syncthreads();
    for (int e = tid; e < D * D; e += T) G[e] = nan, X[e] = nan;
    if (tid == 0) info[comp] = 1 + fail_dim, logdet[comp] = nan;
    return;
  }
  // L with a zero upper triangle, X = I
  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    if (IN_LDS)
      G[e] = j <= i ? A[(size_t)i * lda + j] : 0.0;
    else if (j > i)
      G[e] = 0.0;
    X[e] = i == j ? 1.0 : 0.0;
  }
  if (tid == 0) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += log(A[(size_t)d * lda + d]);
    logdet[comp] = 2.0 * s;
    info[comp] = 0;
  }
  __syncthreads();
  for (int k = 0; k < D; ++k) {
    const double lkk = A[(size_t)k * lda + k];
    for (int j = tid; j <= k; j += T) X[(size_t)k * D + j] = X[(size_t)k * D + j] / lkk;
    __syncthreads();
    const int w = k + 1, cnt = (D - k - 1) * w;
    for (int e = tid; e < cnt; e += T) {
      const int a = e / w, j = e - a * w, i = k + 1 + a;
      X[(size_t)i * D + j] = X[(size_t)i * D + j] - A[(size_t)i * lda + k] * X[(size_t)k * D + j];
    }
    __syncthreads();
  }
}

// ---- E-step ------------------------------------------------------------------------------------------------------------
// grid (64-row tile, component), four waves of 16 rows.  The f64 MFMA operand maps are at f64x4 in csrc/dense.h.
// Here A is the tile of centred rows (k runs over four columns j of x), B[j][i] = Linv[i][j] for the 16 outputs i of tile
// ti, zero for j > i; the products run over j < min(D, 16 ti + 16) only.  The 16 x 16 results go through LDS so that one
// lane per row adds y^2 in ascending column order.
__global__ __launch_bounds__(256) void gmm_logp_kernel(const float* __restrict__ x, size_t ld, int N, int D, int K,
                                                       const double* __restrict__ w, const double* __restrict__ mean,
                                                       const double* __restrict__ linv,
                                                       const double* __restrict__ logdet, double* __restrict__ lp,
                                                       int* __restrict__ flags, unsigned* __restrict__ counter) {
  __shared__ double ys[4][16][17];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  const int comp = blockIdx.y;
  if (blockIdx.x == 0 && comp == 0 && threadIdx.x == 0) *counter = 0u;      // for the second launch
  const double* mu = mean + (size_t)comp * D;
  const double* Li = linv + (size_t)comp * D * D;
  const int n0 = blockIdx.x * 64 + wid * 16;
  const int n = n0 + lr;
  const bool rok = n < N;
  const int nt = cdiv(D, 16);
  double q = 0.0;
  bool bad = false;
  for (int ti = 0; ti < nt; ++ti) {
    const int ci = ti * 16 + lr;
    const bool iok = ci < D;
    const int jend = min(D, ti * 16 + 16);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < jend; j0 += 4) {
      const int j = j0 + lk;
      double a = 0.0, b = 0.0;
      if (rok && j < D) {
        const float v = x[(size_t)n * ld + j];
        bad |= !finite_f(v);
        a = (double)v - mu[j];
      }
      if (iok && j <= ci) b = Li[(size_t)ci * D + j];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) ys[wid][lk + 4 * i][lr] = acc[i];
    __syncthreads();
    if (lane < 16) {
      const int cmax = min(16, D - ti * 16);
      for (int c = 0; c < cmax; ++c) {
        const double y = ys[wid][lane][c];
        q += y * y;
      }
    }
    __syncthreads();
  }
  if (lane < 16 && n0 + lane < N)
    lp[(size_t)(n0 + lane) * K + comp] = log(w[comp]) - 0.5 * (((double)D * kLog2Pi + logdet[comp]) + q);
  if (bad) atomicOr(&flags[0], 1);
}

// grid (256-row block), one thread per row.  The block sums of lse go to part[]; the block that finds itself last adds them
// in block order.
__global__ __launch_bounds__(256) void gmm_resp_kernel(const double* __restrict__ lp, int N, int K, int hard,
                                                       double* __restrict__ resp, double* __restrict__ loglik,
                                                       double* part, unsigned* counter, double* __restrict__ sum_loglik) {
  __shared__ double red[4];
  __shared__ int last;
  const int n = blockIdx.x * 256 + threadIdx.x;
  double lse = 0.0;
  if (n < N) {
    const double* p = lp + (size_t)n * K;
    double* r = resp + (size_t)n * K;
    double m = p[0];
    int am = 0;
    for (int k = 1; k < K; ++k)
      if (p[k] > m) m = p[k], am = k;
    if (hard) {
      for (int k = 0; k < K; ++k) r[k] = k == am ? 1.0 : 0.0;
      lse = m;
    } else {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += exp(p[k] - m);
      lse = m + log(s);
      for (int k = 0; k < K; ++k) r[k] = exp(p[k] - lse);
    }
    loglik[n] = lse;
  }
  const double bs = block_sum(lse, red);
  if (threadIdx.x == 0) {
    __hip_atomic_store(&part[blockIdx.x], bs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    double s = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) s += __hip_atomic_load(&part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *sum_loglik = s;
  }
}

// ---- M-step ------------------------------------------------------------------------------------------------------------
// grid (64-column tile of D + 1, row slice, component): the weighted block_colsum of the slice's rows; column d < D adds
// resp x, column D adds resp.
__global__ __launch_bounds__(256) void gmm_colsum_kernel(const float* __restrict__ x, size_t ld,
                                                         const double* __restrict__ resp, int N, int D, int K, int rows,
                                                         double* __restrict__ part, int* __restrict__ flags) {
  __shared__ double sm[4][64];
  const int d = blockIdx.x * 64 + (threadIdx.x & 63), comp = blockIdx.z;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  bool bad = false;
  const double s = block_colsum<true>(x, ld, d, D, r0, r1, resp + comp, (size_t)K, sm, &bad);
  if (bad) atomicOr(&flags[0], 1);
  if (threadIdx.x < 64 && d <= D) part[((size_t)comp * gridDim.y + blockIdx.y) * (D + 1) + d] = s;
}
// grid (256-column tile of D + 1, component): Nk = the slices in ascending order + 10 DBL_EPSILON, m = the slices / Nk; the
// thread of column D writes Nk and w = Nk / (sum of every Nk, ascending).
__global__ __launch_bounds__(256) void gmm_mean_kernel(const double* __restrict__ part, int ns, int D, int K,
                                                       double* __restrict__ nk, double* __restrict__ w,
                                                       double* __restrict__ mean) {
  const int d = blockIdx.x * 256 + threadIdx.x, comp = blockIdx.y;
  if (d > D) return;
  const size_t cs = (size_t)ns * (D + 1);
  const double tot = fold_strided(0.0, part + comp * cs + D, (size_t)(D + 1), ns) + 10.0 * DBL_EPSILON;
  if (d < D) {
    mean[(size_t)comp * D + d] = fold_strided(0.0, part + comp * cs + d, (size_t)(D + 1), ns) / tot;
  } else {
    double all = 0.0;
    for (int c = 0; c < K; ++c) all += fold_strided(0.0, part + c * cs + D, (size_t)(D + 1), ns) + 10.0 * DBL_EPSILON;
    nk[comp] = tot;
    w[comp] = tot / all;
  }
}
// grid (tile pair ti <= tj, row slice, component), one wave: the weighted cov_tile_rows, A = resp (x_i - m_i).
__global__ __launch_bounds__(64) void gmm_cov_tile_kernel(const float* __restrict__ x, size_t ld,
                                                          const double* __restrict__ resp, int N, int D, int K, int rows,
                                                          int nt, const double* __restrict__ mean,
                                                          double* __restrict__ part) {
  const int comp = blockIdx.z;
  int ti, tj;
  tile_pair(blockIdx.x, nt, &ti, &tj);
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  const f64x4 acc = cov_tile_rows<true>(x, ld, D, ti, tj, r0, r1, mean + (size_t)comp * D, resp + comp, (size_t)K);
  cov_tile_store(part + (((size_t)comp * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 256, acc);
}
// grid (tile pair, component): the slices in ascending order, divided by Nk, reg added on the diagonal; the upper triangle
// is written and mirrored.
__global__ __launch_bounds__(256) void gmm_cov_fold_kernel(const double* __restrict__ part, int ns, int npairs, int nt,
                                                           int D, double reg, const double* __restrict__ nk,
                                                           double* __restrict__ cov) {
  const int comp = blockIdx.y;
  int i, j;
  if (!cov_fold_element(blockIdx.x, nt, D, &i, &j)) return;
  const double s = fold_strided(0.0, part + ((size_t)comp * ns * npairs + blockIdx.x) * 256 + threadIdx.x,
                                (size_t)npairs * 256, ns);
  double c = s / nk[comp];
  if (i == j) c = c + reg;
  double* C = cov + (size_t)comp * D * D;
  C[(size_t)i * D + j] = c;
  C[(size_t)j * D + i] = c;
}

// ---- sampler -----------------------------------------------------------------------------------------------------------
// grid (4 rows), one wave per row: lane i adds L[i][j] eps[j] over ascending j <= i, then the mean.
__global__ __launch_bounds__(256) void gmm_sample_kernel(const double* __restrict__ mean, const double* __restrict__ chol,
                                                         const int* __restrict__ comp, const float* __restrict__ eps,
                                                         int R, int D, int K, float* __restrict__ z,
                                                         int* __restrict__ flags) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wid;
  if (r >= R) return;
  const int c = comp[r];
  if (c < 0 || c >= K) {
    if (lane == 0) atomicOr(&flags[1], 1);
    return;
  }
  const double* mu = mean + (size_t)c * D;
  const double* L = chol + (size_t)c * D * D;
  const float* e = eps + (size_t)r * D;
  for (int i = lane; i < D; i += 64) {
    double s = 0.0;
    for (int j = 0; j <= i; ++j) s += L[(size_t)i * D + j] * (double)e[j];
    z[(size_t)r * D + i] = (float)(mu[i] + s);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static int gmm_kd(const char* name, int D, int K) {
  return need_dim(name, "K = %lld components", K, 1, kGmmMaxK, "1..64") || need_dim(name, "D = %lld", D, 1, kGmmMaxD, "1..512");
}
static int gmm_shape(const char* name, int N, int D, int K) {
  if (gmm_kd(name, D, K)) return 1;
  if (N < K || N > kGmmMaxN) return fail("%s: N = %lld rows is outside K = %lld..2^24", name, N, K);
  return 0;
}
static inline bool gmm_ok(int N, int D, int K) {
  return K >= 1 && K <= kGmmMaxK && D >= 1 && D <= kGmmMaxD && N >= K && N <= kGmmMaxN;
}
struct MstepWs {
  int rows, ns, nt, npairs;
  size_t sums, part, total;
};
static inline MstepWs mstep_ws(int N, int D, int K, bool with_cov) {
  MstepWs w;
  w.rows = cov_slice_rows(N), w.ns = cdiv(N, w.rows);
  w.nt = cdiv(D, 16), w.npairs = w.nt * (w.nt + 1) / 2;
  w.sums = 0;
  w.part = w.sums + (size_t)K * w.ns * (D + 1) * sizeof(double);
  w.total = w.part + (with_cov ? (size_t)K * w.ns * w.npairs * 256 * sizeof(double) : 0);
  return w;
}
static inline size_t estep_ws(int N) { return 256 + (size_t)cdiv(N, 256) * sizeof(double); }

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_gmm_factor(double* chol, int K, int D, double* linv, double* logdet, int* info, void* stream) {
  const char* name = "itcv_gmm_factor";
  if (gmm_kd(name, D, K)) return 1;
  ITCV_REQUIRE(chol && linv && logdet && info, name);
  hipStream_t st = S(stream);
  if (D <= kLdsMatrixDim)
    launch_lds<gmm_factor_kernel<true>>(dim3(K), dim3(kMatrixThreads), (size_t)D * (D | 1) * sizeof(double), st, chol, D,
                                        linv, logdet, info);
  else
    hipLaunchKernelGGL(gmm_factor_kernel<false>, dim3(K), dim3(kMatrixThreads), 0, st, chol, D, linv, logdet, info);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_gmm_estep_workspace(int N, int D, int K) { return gmm_ok(N, D, K) ? estep_ws(N) : 0; }

int itcv_gmm_estep(const float* x, size_t ld, int N, int D, int K, const double* w, const double* mean, const double* linv,
                   const double* logdet, int hard, double* lp, double* resp, double* loglik, double* sum_loglik,
                   int* flags, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_gmm_estep";
  if (int e = gmm_shape(name, N, D, K)) return e;
  ITCV_REQUIRE(x && w && mean && linv && logdet && lp && resp && loglik && sum_loglik && flags && ld >= (size_t)D, name);
  ITCV_REQUIRE(ws && ws_bytes >= estep_ws(N), "itcv_gmm_estep(workspace)");
  unsigned* counter = static_cast<unsigned*>(ws);
  double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + 256);
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(gmm_logp_kernel, dim3(cdiv(N, 64), K), dim3(256), 0, st, x, ld, N, D, K, w, mean, linv, logdet, lp,
                     flags, counter);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(gmm_resp_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, (const double*)lp, N, K, hard ? 1 : 0, resp,
                     loglik, part, counter, sum_loglik);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_gmm_mstep_workspace(int N, int D, int K, int with_cov) {
  return gmm_ok(N, D, K) ? mstep_ws(N, D, K, with_cov != 0).total : 0;
}

int itcv_gmm_mstep(const float* x, size_t ld, const double* resp, int N, int D, int K, double reg, int with_cov,
                   double* nk, double* w, double* mean, double* cov, int* flags, void* ws, size_t ws_bytes,
                   void* stream) {
  const char* name = "itcv_gmm_mstep";
  if (int e = gmm_shape(name, N, D, K)) return e;
  if (!(reg >= 0.0) || !(reg <= DBL_MAX)) return fail("%s: reg must be finite and >= 0", name);
  ITCV_REQUIRE(x && resp && nk && w && mean && flags && (cov || !with_cov) && ld >= (size_t)D, name);
  const MstepWs m = mstep_ws(N, D, K, with_cov != 0);
  ITCV_REQUIRE(ws && ws_bytes >= m.total, "itcv_gmm_mstep(workspace)");
  char* base = static_cast<char*>(ws);
  double* sums = reinterpret_cast<double*>(base + m.sums);
  double* part = reinterpret_cast<double*>(base + m.part);
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(gmm_colsum_kernel, dim3(cdiv(D + 1, 64), m.ns, K), dim3(256), 0, st, x, ld, resp, N, D, K, m.rows,
                     sums, flags);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(gmm_mean_kernel, dim3(cdiv(D + 1, 256), K), dim3(256), 0, st, (const double*)sums, m.ns, D, K, nk, w,
                     mean);
  ITCV_CHECK_LAUNCH(name);
  if (!with_cov) return 0;
  hipLaunchKernelGGL(gmm_cov_tile_kernel, dim3(m.npairs, m.ns, K), dim3(64), 0, st, x, ld, resp, N, D, K, m.rows, m.nt,
                     (const double*)mean, part);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(gmm_cov_fold_kernel, dim3(m.npairs, K), dim3(256), 0, st, (const double*)part, m.ns, m.npairs, m.nt,
                     D, reg, (const double*)nk, cov);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_gmm_sample(const double* mean, const double* chol, const int* comp, const float* eps, int R, int D, int K,
                    float* z, int* flags, void* stream) {
  const char* name = "itcv_gmm_sample";
  if (gmm_kd(name, D, K) || need_dim(name, "R = %lld rows", R, 1, kGmmMaxN, "1..2^24")) return 1;
  ITCV_REQUIRE(mean && chol && comp && eps && z && flags, name);
  hipLaunchKernelGGL(gmm_sample_kernel, dim3(cdiv(R, 4)), dim3(256), 0, S(stream), mean, chol, comp, eps, R, D, K, z,
                     flags);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
