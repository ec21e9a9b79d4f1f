// The unsupervised scores (Gaussian total correlation, Gaussian Wasserstein correlation) and the interventional
// robustness score IRS (Suter et al. 2019) on the device.  The rules are in include/itcv_hip.h; all arithmetic is fp64 on
// fp32 representations x[N][D] (row stride ld):
//   unsup_cov   : the column means, then the ddof = 1 covariance of the centred values on v_mfma_f64_16x16x4_f64, one
//                 16 x 16 tile pair and one row slice per wave; the slices are folded in ascending order and the lower
//                 triangle is the mirror of the upper one;
//   unsup_gauss : ONE block: Cholesky log-determinant of C, then the eigenvalues of S = D^1/2 C D^1/2 by a cyclic Jacobi
//                 iteration with a round-robin rotation order; the matrix sits in LDS up to kLdsMatrixDim, above that in a
//                 global workspace;
//   irs         : column means and largest deviations, the class counts, then one block per (factor value, 64 dimensions)
//                 that finds the two order statistics of |x - e| EXACTLY by a radix select on the bit patterns of the
//                 non-negative fp64 values, and one block that folds the quantiles into the score.
// Every floating-point reduction has a fixed order that depends on the shapes alone, never on the grid; counts and maxima
// go through integer atomics (order-free); there is no floating-point atomic.  Nothing in this file may be contracted
// into a fused multiply-add.
#include "dense.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kUsMaxD = kMatrixMaxDim;
constexpr int kUsMaxN = 1 << 24;
constexpr int kUsMaxCsize = 256;
constexpr int kIrsThreads = 1024;         // 16 row lanes x 64 dimensions
constexpr int kIrsRowLanes = kIrsThreads / 64;

// ---- column means ----------------------------------------------------------------------------------------------------
// grid (64-column tile, row slice): block_colsum of the slice's rows
__global__ __launch_bounds__(256) void us_colsum_kernel(const float* __restrict__ x, size_t ld, int N, int D, int rows,
                                                        double* __restrict__ part, int* __restrict__ flags) {
  __shared__ double sm[4][64];
  const int d = blockIdx.x * 64 + (threadIdx.x & 63);
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  bool bad = false;
  const double s = block_colsum<false>(x, ld, d, D, r0, r1, nullptr, 0, sm, &bad);
  if (bad && flags) atomicOr(&flags[0], 1);
  if (threadIdx.x < 64 && d < D) part[(size_t)blockIdx.y * D + d] = s;
}
__global__ __launch_bounds__(256) void us_mean_kernel(const double* __restrict__ part, int ns, int D, int N,
                                                      double* __restrict__ mean) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < D) mean[d] = fold_strided(0.0, part + d, (size_t)D, ns) / (double)N;
}

// ---- covariance ------------------------------------------------------------------------------------------------------
// grid (tile pair ti <= tj, row slice), one wave: cov_tile_rows of the slice's rows (csrc/dense.h)
__global__ __launch_bounds__(64) void us_cov_tile_kernel(const float* __restrict__ x, size_t ld, int N, int D, int rows,
                                                         int nt, const double* __restrict__ mean,
                                                         double* __restrict__ part) {
  int ti, tj;
  tile_pair(blockIdx.x, nt, &ti, &tj);
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  const f64x4 acc = cov_tile_rows<false>(x, ld, D, ti, tj, r0, r1, mean, nullptr, 0);
  cov_tile_store(part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256, acc);
}
// grid (tile pair): the slices in ascending order, divided by N - 1; the upper triangle is written and mirrored.
__global__ __launch_bounds__(256) void us_cov_fold_kernel(const double* __restrict__ part, int ns, int npairs, int nt, int N,
                                                          int D, double* __restrict__ cov) {
  int i, j;
  if (!cov_fold_element(blockIdx.x, nt, D, &i, &j)) return;
  const double s = fold_strided(0.0, part + (size_t)blockIdx.x * 256 + threadIdx.x, (size_t)npairs * 256, ns);
  const double c = s / (double)(N - 1);
  cov[(size_t)i * D + j] = c;
  cov[(size_t)j * D + i] = c;
}

// ---- Cholesky log-determinant and Jacobi eigenvalues -----------------------------------------------------------------
// One block of 1024 threads.  A[D][lda] is the working matrix (LDS or the global workspace; a __syncthreads orders the
// block's own global writes).  res[5] = {tc, w, w / tr C, tr C, logdet C}; eig[D] = the diagonal of S after the last
// sweep; info[4] = {pivot failed, its dimension, Jacobi not converged, sweeps taken}.
template <bool IN_LDS>
__global__ __launch_bounds__(kMatrixThreads) void us_gauss_kernel(const double* __restrict__ cov, int D,
                                                                  double* __restrict__ wsA, double* __restrict__ res,
                                                                  double* __restrict__ eig, int* __restrict__ info) {
  extern __shared__ double us_lds[];
  __shared__ double sd[kUsMaxD];
  __shared__ JacobiScratch js;
  const int tid = threadIdx.x, T = kMatrixThreads;
  const int lda = IN_LDS ? (D | 1) : D;
  double* A = IN_LDS ? us_lds : wsA;
  const double nan = __builtin_nan("");

  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    A[(size_t)i * lda + j] = cov[e];
  }
  __syncthreads();
  const int fail_dim = block_cholesky<kMatrixThreads>(A, lda, D);
  if (fail_dim >= 0) {
    if (tid == 0) {
      info[0] = 1, info[1] = fail_dim, info[2] = 0, info[3] = 0;
      for (int i = 0; i < 5; ++i) res[i] = nan;
    }
    for (int d = tid; d < D; d += T) eig[d] = nan;
    return;
  }
  double logdet = 0.0, sumlog = 0.0, tr = 0.0;
  if (tid == 0) {
    for (int d = 0; d < D; ++d) {
      logdet += log(A[(size_t)d * lda + d]);
      const double c = cov[(size_t)d * D + d];
      sumlog += log(c);
      tr += c;
    }
    logdet = 2.0 * logdet;
  }
  for (int d = tid; d < D; d += T) sd[d] = sqrt(cov[(size_t)d * D + d]);
  __syncthreads();
  // S = D^1/2 C D^1/2: the lower triangle, mirrored
  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    if (j <= i) {
      const double v = (sd[i] * cov[e]) * sd[j];
      A[(size_t)i * lda + j] = v;
      A[(size_t)j * lda + i] = v;
    }
  }
  __syncthreads();
  int sweeps;
  const bool conv = block_jacobi<kMatrixThreads>(A, lda, D, &js, &sweeps);
  for (int d = tid; d < D; d += T) eig[d] = A[(size_t)d * lda + d];
  if (tid == 0) {
    double ws = 0.0;
    for (int d = 0; d < D; ++d) ws += sqrt(fmax(A[(size_t)d * lda + d], 0.0));
    const double w = 2.0 * tr - 2.0 * ws;
    res[0] = 0.5 * (sumlog - logdet);
    res[1] = w;
    res[2] = w / tr;
    res[3] = tr;
    res[4] = logdet;
    info[0] = 0, info[1] = -1, info[2] = conv ? 0 : 1, info[3] = sweeps;
  }
}

// ---- IRS -------------------------------------------------------------------------------------------------------------
// class counts of every factor (integer atomics; cleared by the host) and the range check of the factor values
__global__ __launch_bounds__(256) void irs_count_kernel(const int* __restrict__ v, int N, SegPlan pl, int* __restrict__ cnt,
                                                        int* __restrict__ flags) {
  const int K = pl.K;
  const size_t total = (size_t)N * K;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e % K);
    const int val = v[e];
    if ((unsigned)val < (unsigned)(pl.off[k + 1] - pl.off[k]))
      atomicAdd(&cnt[pl.off[k] + val], 1);
    else
      atomicOr(&flags[1], 1);
  }
}
// maxdev[d] = max_n |x[n][d] - mean[d]|: a maximum of non-negative doubles is the maximum of their bit patterns
__global__ __launch_bounds__(256) void irs_maxdev_kernel(const float* __restrict__ x, size_t ld, int N, int D, int rows,
                                                         const double* __restrict__ mean,
                                                         unsigned long long* __restrict__ maxdev) {
  __shared__ double sm[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  double m = 0.0;
  if (d < D) {
    const double c = mean[d];
    for (int r = r0 + wid; r < r1; r += 4) {
      const double a = fabs((double)x[(size_t)r * ld + d] - c);
      if (a > m) m = a;
    }
  }
  sm[wid][lane] = m;
  __syncthreads();
  if (wid == 0 && d < D) {
    m = fmax(fmax(sm[0][lane], sm[1][lane]), fmax(sm[2][lane], sm[3][lane]));
    atomicMax(&maxdev[d], (unsigned long long)__double_as_longlong(m));
  }
}

// grid (factor value slot, 64-dimension tile), 16 row lanes x 64 dimensions.  order[k][N] lists the rows sorted by factor
// k (stable), so the rows of slot (k, v) are order[k][start .. start + n).  Per dimension: the mean e (row lane rl sums the
// group's rows rl, rl + 16, ... in ascending position; the 16 partial sums are added in lane order), then the lo-th
// smallest of a = |x - e| by a radix select on the 64-bit pattern, two bits a pass from the top: the kept prefix is the
// largest P with #{a < P} <= lo, which is a[lo] itself; one more pass gives a[hi].
__global__ __launch_bounds__(kIrsThreads) void irs_group_kernel(const float* __restrict__ x, size_t ld,
                                                                const int* __restrict__ order,
                                                                const int* __restrict__ cnt, int N, int D, SegPlan pl,
                                                                double q, double* __restrict__ Qs,
                                                                int* __restrict__ flags) {
  __shared__ double part[kIrsRowLanes][64];
  __shared__ int c3[3][3][64];
  __shared__ int cle[64];
  __shared__ unsigned long long mgt[64];
  const int tid = threadIdx.x, dl = tid & 63, rl = tid >> 6;
  const int slot = blockIdx.x;
  int k = 0;
  while (pl.off[k + 1] <= slot) ++k;
  const int d = blockIdx.y * 64 + dl;
  const bool live = d < D;
  const int n = cnt[slot];
  if (n <= 0) {                                       // block-uniform
    if (rl == 0 && live) Qs[(size_t)slot * D + d] = 0.0;
    return;
  }
  int start = 0;
  for (int u = pl.off[k]; u < slot; ++u) start += cnt[u];
  if (start + n > N) {                                // cannot happen with counts of this call; keeps every read inside
    if (tid == 0) atomicOr(&flags[1], 1);
    return;
  }
  const int* ord = order + (size_t)k * N + start;
  if (tid < 3 * 3 * 64) (&c3[0][0][0])[tid] = 0;
  if (tid < 64) cle[tid] = 0, mgt[tid] = ~0ull;
  bool bad = false;
  double s = 0.0;
  for (int r = rl; r < n; r += kIrsRowLanes) {
    int row = ord[r];
    if ((unsigned)row >= (unsigned)N) bad = true, row = 0;
    if (live) s += (double)x[(size_t)row * ld + d];
  }
  if (bad) atomicOr(&flags[1], 1);
  part[rl][dl] = s;
  __syncthreads();
  double e = part[0][dl];
#pragma unroll
  for (int u = 1; u < kIrsRowLanes; ++u) e += part[u][dl];
  e = e / (double)n;

  const double h = (double)(n - 1) * q;
  const int lo = (int)floor(h);
  const double t = h - (double)lo;
  const int hi = min(lo + 1, n - 1);
  unsigned long long prefix = 0;
  for (int pass = 0; pass < 32; ++pass) {
    const int shift = 62 - 2 * pass, buf = pass % 3;
    const unsigned long long p1 = prefix | (1ull << shift), p2 = prefix | (2ull << shift), p3 = prefix | (3ull << shift);
    int n1 = 0, n2 = 0, n3 = 0;
    if (live)
      for (int r = rl; r < n; r += kIrsRowLanes) {
        const unsigned row = min((unsigned)ord[r], (unsigned)(N - 1));
        const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs((double)x[(size_t)row * ld + d] - e));
        n1 += bits < p1, n2 += bits < p2, n3 += bits < p3;
      }
    if (n1) atomicAdd(&c3[buf][0][dl], n1);
    if (n2) atomicAdd(&c3[buf][1][dl], n2);
    if (n3) atomicAdd(&c3[buf][2][dl], n3);
    __syncthreads();
    const int t1 = c3[buf][0][dl], t2 = c3[buf][1][dl], t3 = c3[buf][2][dl];
    prefix = t3 <= lo ? p3 : (t2 <= lo ? p2 : (t1 <= lo ? p1 : prefix));
    // the buffer of pass - 1 was last read before this pass's barrier and is next added to after the next one
    if (rl < 3) c3[(pass + 2) % 3][rl][dl] = 0;
  }
  const double alo = __longlong_as_double((long long)prefix);
  double ahi = alo;
  if (hi != lo) {                                     // block-uniform
    int nle = 0;
    unsigned long long mn = ~0ull;
    if (live)
      for (int r = rl; r < n; r += kIrsRowLanes) {
        const unsigned row = min((unsigned)ord[r], (unsigned)(N - 1));
        const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs((double)x[(size_t)row * ld + d] - e));
        if (bits <= prefix)
          ++nle;
        else if (bits < mn)
          mn = bits;
      }
    if (nle) atomicAdd(&cle[dl], nle);
    if (mn != ~0ull) atomicMin(&mgt[dl], mn);
    __syncthreads();
    if (cle[dl] < lo + 2) ahi = __longlong_as_double((long long)mgt[dl]);
  }
  if (rl == 0 && live) {
    const double diff = ahi - alo;
    Qs[(size_t)slot * D + d] = t < 0.5 ? alo + diff * t : ahi - diff * (1.0 - t);
  }
}

// One block, a thread per dimension: cum, M = 1 - cum / maxdev, the row maxima and their first arg-max; thread 0 then adds
// the weighted scores of the active dimensions in ascending d.  res = {IRS, number of active dimensions}.
__global__ __launch_bounds__(kUsMaxD) void irs_final_kernel(const double* __restrict__ Qs, const int* __restrict__ cnt,
                                                            SegPlan pl, int D, const float* __restrict__ mn,
                                                            const float* __restrict__ mx,
                                                            const double* __restrict__ maxdev, double* __restrict__ cum,
                                                            double* __restrict__ Mo, double* __restrict__ score,
                                                            int* __restrict__ parent, int* __restrict__ active,
                                                            double* __restrict__ res) {
  __shared__ double sc[kUsMaxD], mdv[kUsMaxD];
  __shared__ int act[kUsMaxD];
  const int d = threadIdx.x, K = pl.K;
  if (d < D) {
    const bool on = mn[d] < mx[d];
    const double md = maxdev[d];
    double best = 0.0;
    int arg = 0;
    for (int k = 0; k < K; ++k) {
      double sq = 0.0;
      int present = 0;
      for (int u = pl.off[k]; u < pl.off[k + 1]; ++u)
        if (cnt[u] > 0) sq += Qs[(size_t)u * D + d], ++present;
      const double c = sq / (double)present;
      const double m = on ? 1.0 - c / md : 0.0;
      cum[(size_t)d * K + k] = c;
      Mo[(size_t)d * K + k] = m;
      if (k == 0 || m > best) best = m, arg = k;
    }
    score[d] = on ? best : 0.0, parent[d] = arg, active[d] = on;
    sc[d] = best, mdv[d] = md, act[d] = on;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double num = 0.0, den = 0.0;
    int na = 0;
    for (int u = 0; u < D; ++u)
      if (act[u]) num += sc[u] * mdv[u], den += mdv[u], ++na;
    res[0] = na ? num / den : 0.0;
    res[1] = (double)na;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int us_shape(const char* name, int N, int D, int minN) {
  return need_dim(name, "N = %lld rows", N, minN, kUsMaxN, minN == 2 ? "2..2^24" : "1..2^24") ||
         need_dim(name, "D = %lld", D, 1, kUsMaxD, "1..512");
}
struct CovWs {
  int rows, ns, nt, npairs;
  size_t sums, mean, part, total;
};
static inline CovWs cov_ws(int N, int D) {
  CovWs w;
  w.rows = cov_slice_rows(N), w.ns = cdiv(N, w.rows);
  w.nt = cdiv(D, 16), w.npairs = w.nt * (w.nt + 1) / 2;
  w.sums = 0;
  w.mean = w.sums + (size_t)w.ns * D * sizeof(double);
  w.part = w.mean + (size_t)D * sizeof(double);
  w.total = w.part + (size_t)w.ns * w.npairs * 256 * sizeof(double);
  return w;
}
static int launch_mean(const char* name, const float* x, size_t ld, int N, int D, const CovWs& w, double* sums,
                       double* mean, int* flags, hipStream_t st) {
  hipLaunchKernelGGL(us_colsum_kernel, dim3(cdiv(D, 64), w.ns), dim3(256), 0, st, x, ld, N, D, w.rows, sums, flags);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(us_mean_kernel, dim3(cdiv(D, 256)), dim3(256), 0, st, (const double*)sums, w.ns, D, N, mean);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}
struct IrsWs {
  size_t sums, mean, cnt, qs, total;
};
static inline IrsWs irs_ws(int N, int D, int fsum) {
  const CovWs c = cov_ws(N, D);
  IrsWs w;
  w.sums = 0;
  w.mean = w.sums + (size_t)c.ns * D * sizeof(double);
  w.qs = w.mean + (size_t)D * sizeof(double);
  w.cnt = w.qs + (size_t)fsum * D * sizeof(double);
  w.total = w.cnt + (size_t)fsum * sizeof(int);
  return w;
}
constexpr SegWords kUsWords = {"K = %lld factors", "no factor sizes", "factor %lld has %lld values"};

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_unsup_cov_workspace(int N, int D) {
  if (N < 2 || N > kUsMaxN || D < 1 || D > kUsMaxD) return 0;
  return cov_ws(N, D).total;
}

int itcv_unsup_cov(const float* x, size_t ld, int N, int D, double* mean, double* cov, int* flags, void* ws,
                   size_t ws_bytes, void* stream) {
  const char* name = "itcv_unsup_cov";
  if (int e = us_shape(name, N, D, 2)) return e;
  ITCV_REQUIRE(x && mean && cov && flags && ld >= (size_t)D, name);
  const CovWs w = cov_ws(N, D);
  ITCV_REQUIRE(ws && ws_bytes >= w.total, "itcv_unsup_cov(workspace)");
  char* base = static_cast<char*>(ws);
  double* sums = reinterpret_cast<double*>(base + w.sums);
  double* part = reinterpret_cast<double*>(base + w.part);
  hipStream_t st = S(stream);
  if (int e = launch_mean(name, x, ld, N, D, w, sums, mean, flags, st)) return e;
  hipLaunchKernelGGL(us_cov_tile_kernel, dim3(w.npairs, w.ns), dim3(64), 0, st, x, ld, N, D, w.rows, w.nt,
                     (const double*)mean, part);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(us_cov_fold_kernel, dim3(w.npairs), dim3(256), 0, st, (const double*)part, w.ns, w.npairs, w.nt, N, D,
                     cov);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_unsup_gauss_lds_dim(void) { return kLdsMatrixDim; }

size_t itcv_unsup_gauss_workspace(int D) {
  if (D < 1 || D > kUsMaxD) return 0;
  return (size_t)D * D * sizeof(double);
}

int itcv_unsup_gauss(const double* cov, int D, double* res, double* eig, int* info, void* ws, size_t ws_bytes,
                     void* stream) {
  const char* name = "itcv_unsup_gauss";
  if (need_dim(name, "D = %lld", D, 1, kUsMaxD, "1..512")) return 1;
  ITCV_REQUIRE(cov && res && eig && info, name);
  hipStream_t st = S(stream);
  if (D <= kLdsMatrixDim) {
    launch_lds<us_gauss_kernel<true>>(dim3(1), dim3(kMatrixThreads), (size_t)D * (D | 1) * sizeof(double), st, cov, D,
                                      (double*)nullptr, res, eig, info);
  } else {
    ITCV_REQUIRE(ws && ws_bytes >= (size_t)D * D * sizeof(double), "itcv_unsup_gauss(workspace)");
    hipLaunchKernelGGL(us_gauss_kernel<false>, dim3(1), dim3(kMatrixThreads), 0, st, cov, D, static_cast<double*>(ws), res,
                       eig, info);
  }
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_irs_workspace(int N, int D, int K, int fsum) {
  if (N < 1 || N > kUsMaxN || D < 1 || D > kUsMaxD || K < 1 || K > kSegMaxK || fsum < K || fsum > K * kUsMaxCsize) return 0;
  return irs_ws(N, D, fsum).total;
}

int itcv_irs(const float* x, size_t ld, const int* v, const int* order, int N, int D, int K, const int* fsize, double q,
             const float* mn, const float* mx, double* maxdev, double* cum, double* M, double* score, int* parent,
             int* active, double* res, int* flags, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_irs";
  if (int e = us_shape(name, N, D, 1)) return e;
  SegPlan pl;
  if (int e = seg_plan(name, K, fsize, kUsMaxCsize, kUsWords, &pl)) return e;
  if (!(q >= 0.0 && q <= 1.0)) return fail("%s: the quantile lies outside [0, 1]", name);
  ITCV_REQUIRE(x && v && order && mn && mx && maxdev && cum && M && score && parent && active && res && flags &&
                   ld >= (size_t)D,
               name);
  const int fsum = pl.off[K];
  const IrsWs w = irs_ws(N, D, fsum);
  ITCV_REQUIRE(ws && ws_bytes >= w.total, "itcv_irs(workspace)");
  const CovWs c = cov_ws(N, D);
  char* base = static_cast<char*>(ws);
  double* sums = reinterpret_cast<double*>(base + w.sums);
  double* mean = reinterpret_cast<double*>(base + w.mean);
  double* Qs = reinterpret_cast<double*>(base + w.qs);
  int* cnt = reinterpret_cast<int*>(base + w.cnt);
  hipStream_t st = S(stream);
  if (hipMemsetAsync(cnt, 0, (size_t)fsum * sizeof(int), st) != hipSuccess ||
      hipMemsetAsync(maxdev, 0, (size_t)D * sizeof(double), st) != hipSuccess)
    return fail("%s: clearing the counts failed", name);
  if (int e = launch_mean(name, x, ld, N, D, c, sums, mean, nullptr, st)) return e;
  hipLaunchKernelGGL(irs_count_kernel, dim3(stream_grid((size_t)N * K, 1)), dim3(256), 0, st, v, N, pl, cnt, flags);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(irs_maxdev_kernel, dim3(cdiv(D, 64), c.ns), dim3(256), 0, st, x, ld, N, D, c.rows, (const double*)mean,
                     reinterpret_cast<unsigned long long*>(maxdev));
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(irs_group_kernel, dim3(fsum, cdiv(D, 64)), dim3(kIrsThreads), 0, st, x, ld, order, (const int*)cnt, N, D,
                     pl, q, Qs, flags);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(irs_final_kernel, dim3(1), dim3(kUsMaxD), 0, st, (const double*)Qs, (const int*)cnt, pl, D, mn, mx,
                     (const double*)maxdev, cum, M, score, parent, active, res);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
