// The unsupervised scores (Gaussian total correlation, Gaussian Wasserstein correlation) and the interventional
// robustness score IRS (Suter et al. 2019) on the device.  The rules are in include/itcv_hip.h; all arithmetic is fp64 on
// fp32 representations x[N][D] (row stride ld):
//   unsup_cov   : the column means, then the ddof = 1 covariance of the centred values on v_mfma_f64_16x16x4_f64, one
//                 16 x 16 tile pair and one row slice per wave; the slices are folded in ascending order and the lower
//                 triangle is the mirror of the upper one;
//   unsup_gauss : ONE block: Cholesky log-determinant of C, then the eigenvalues of S = D^1/2 C D^1/2 by a cyclic Jacobi
//                 iteration with a round-robin rotation order; the matrix sits in LDS up to kGaussLdsDim, above that in a
//                 global workspace;
//   irs         : column means and largest deviations, the class counts, then one block per (factor value, 64 dimensions)
//                 that finds the two order statistics of |x - e| EXACTLY by a radix select on the bit patterns of the
//                 non-negative fp64 values, and one block that folds the quantiles into the score.
// Every floating-point reduction has a fixed order that depends on the shapes alone, never on the grid; counts and maxima
// go through integer atomics (order-free); there is no floating-point atomic.  Nothing in this file may be contracted
// into a fused multiply-add.
#include <float.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kUsMaxD = 512;
constexpr int kUsMaxN = 1 << 24;
constexpr int kUsMaxK = 16;
constexpr int kUsMaxCsize = 256;
constexpr int kCovSliceRows = 512;        // rows per slice while that gives at most kCovMaxSlices slices
constexpr int kCovMaxSlices = 64;
constexpr int kGaussLdsDim = 128;         // 128 x 129 doubles = 129 KiB of the CU's 160 KiB
constexpr int kGaussThreads = 1024;
constexpr int kJacobiMaxSweeps = 60;
constexpr double kJacobiTol = 1e-14;
constexpr int kIrsThreads = 1024;         // 16 row lanes x 64 dimensions
constexpr int kIrsRowLanes = kIrsThreads / 64;

typedef double us_f64x4 __attribute__((ext_vector_type(4)));

struct UsPlan {
  int K;
  int coff[kUsMaxK + 1];   // prefix sums of the factor sizes; fsum = coff[K]
};

// rows per slice and number of slices: a function of N alone
static inline int cov_slice_rows(int N) {
  int ns = cdiv(N, kCovSliceRows);
  if (ns > kCovMaxSlices) ns = kCovMaxSlices;
  return cdiv(cdiv(N, ns), 4) * 4;
}

__device__ __forceinline__ bool us_finite(float v) { return fabsf(v) <= FLT_MAX; }

// ---- column means ----------------------------------------------------------------------------------------------------
// grid (64-column tile, row slice): wave w sums rows r0 + w, r0 + w + 4, ... in ascending order; the four are added in
// wave order.
__global__ __launch_bounds__(256) void us_colsum_kernel(const float* __restrict__ x, size_t ld, int N, int D, int rows,
                                                        double* __restrict__ part, int* __restrict__ flags) {
  __shared__ double sm[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  double s = 0.0;
  bool bad = false;
  if (d < D)
    for (int r = r0 + wid; r < r1; r += 4) {
      const float v = x[(size_t)r * ld + d];
      bad |= !us_finite(v);
      s += (double)v;
    }
  sm[wid][lane] = s;
  if (bad && flags) atomicOr(&flags[0], 1);
  __syncthreads();
  if (wid == 0 && d < D) part[(size_t)blockIdx.y * D + d] = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}
__global__ __launch_bounds__(256) void us_mean_kernel(const double* __restrict__ part, int ns, int D, int N,
                                                      double* __restrict__ mean) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < D) mean[d] = fold_strided(0.0, part + d, (size_t)D, ns) / (double)N;
}

// ---- covariance ------------------------------------------------------------------------------------------------------
// grid (tile pair ti <= tj, row slice), one wave.  f64 MFMA operand maps (csrc/logreg.hip): lane l holds A[row l & 15]
// [k = l >> 4] and B[k = l >> 4][col l & 15]; result register i of lane l is C[row (l >> 4) + 4 i][col l & 15].  Here A
// is the transposed tile of centred columns ti, B the tile of centred columns tj, k runs over four rows of x per product;
// rows past the slice and columns past D enter as zeros.
__global__ __launch_bounds__(64) void us_cov_tile_kernel(const float* __restrict__ x, size_t ld, int N, int D, int rows,
                                                         int nt, const double* __restrict__ mean,
                                                         double* __restrict__ part) {
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  int p = blockIdx.x, ti = 0;
  while (p >= nt - ti) p -= nt - ti, ++ti;
  const int tj = ti + p;
  const int ci = ti * 16 + lr, cj = tj * 16 + lr;
  const bool iok = ci < D, jok = cj < D;
  const double mi = iok ? mean[ci] : 0.0, mj = jok ? mean[cj] : 0.0;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  us_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r += 4) {
    const int n = r + lk;
    const bool rok = n < r1;
    const double a = (rok && iok) ? (double)x[(size_t)n * ld + ci] - mi : 0.0;
    const double b = (rok && jok) ? (double)x[(size_t)n * ld + cj] - mj : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  double* out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[(lk + 4 * i) * 16 + lr] = acc[i];
}
// grid (tile pair): the slices in ascending order, divided by N - 1; the upper triangle is written and mirrored.
__global__ __launch_bounds__(256) void us_cov_fold_kernel(const double* __restrict__ part, int ns, int npairs, int nt, int N,
                                                          int D, double* __restrict__ cov) {
  int p = blockIdx.x, ti = 0;
  while (p >= nt - ti) p -= nt - ti, ++ti;
  const int tj = ti + p;
  const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
  const int i = ti * 16 + a, j = tj * 16 + b;
  if (i >= D || j >= D || (ti == tj && a > b)) return;
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
__global__ __launch_bounds__(kGaussThreads) void us_gauss_kernel(const double* __restrict__ cov, int D,
                                                                 double* __restrict__ wsA, double* __restrict__ res,
                                                                 double* __restrict__ eig, int* __restrict__ info) {
  extern __shared__ double us_lds[];
  __shared__ double sd[kUsMaxD];
  __shared__ double rc[kUsMaxD / 2], rs[kUsMaxD / 2], npp[kUsMaxD / 2], nqq[kUsMaxD / 2];
  __shared__ int pp[kUsMaxD / 2], qq[kUsMaxD / 2];
  __shared__ double red[kGaussThreads / 64];
  const int tid = threadIdx.x, T = kGaussThreads;
  const int lda = IN_LDS ? (D | 1) : D;
  double* A = IN_LDS ? us_lds : wsA;
  const double nan = __builtin_nan("");

  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    A[(size_t)i * lda + j] = cov[e];
  }
  __syncthreads();
  // Cholesky, right-looking, lower triangle in place
  int fail_dim = -1;
  const int tx = tid & 31, ty = tid >> 5;
  for (int j = 0; j < D; ++j) {
    const double piv = A[(size_t)j * lda + j];
    if (!(piv > 0.0) || !(piv <= DBL_MAX)) {          // block-uniform: every thread reads the same value
      fail_dim = j;
      break;
    }
    const double l = sqrt(piv);
    __syncthreads();
    if (tid == 0) A[(size_t)j * lda + j] = l;
    for (int i = j + 1 + tid; i < D; i += T) A[(size_t)i * lda + j] = A[(size_t)i * lda + j] / l;
    __syncthreads();
    for (int i = j + 1 + ty; i < D; i += 32) {
      const double lij = A[(size_t)i * lda + j];
      for (int k = j + 1 + tx; k <= i; k += 32) A[(size_t)i * lda + k] = A[(size_t)i * lda + k] - lij * A[(size_t)k * lda + j];
    }
    __syncthreads();
  }
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
  // cyclic Jacobi; round r of a sweep rotates the disjoint pairs of the round-robin schedule on Dp = D rounded up to even:
  // (r, Dp - 1) and ((r + k) mod (Dp - 1), (r - k) mod (Dp - 1)), k = 1 .. Dp / 2 - 1; a pair that touches index D (odd D)
  // or whose off-diagonal element is exactly 0 is skipped
  const int Dp = (D + 1) & ~1, np = Dp / 2, M = Dp - 1;
  int sweeps = 0;
  bool conv = false;
  for (;;) {
    double off = 0.0, tot = 0.0;
    for (int e = tid; e < D * D; e += T) {
      const int i = e / D, j = e - i * D;
      const double v = A[(size_t)i * lda + j];
      const double sq = v * v;
      tot += sq;
      if (i != j) off += sq;
    }
    off = block_sum(off, red);
    tot = block_sum(tot, red);
    if (sqrt(off) <= kJacobiTol * sqrt(tot)) {
      conv = true;
      break;
    }
    if (sweeps == kJacobiMaxSweeps) break;
    for (int r = 0; r < M; ++r) {
      if (tid < np) {
        const int k = tid;
        const int a = k == 0 ? r : (r + k) % M, b = k == 0 ? M : (r + M - k) % M;
        const int p = min(a, b), q = max(a, b);
        int po = -1;
        if (q < D) {
          const double apq = A[(size_t)p * lda + q];
          if (apq != 0.0) {
            const double app = A[(size_t)p * lda + p], aqq = A[(size_t)q * lda + q];
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            const double c = 1.0 / sqrt(1.0 + t * t);
            rc[k] = c, rs[k] = t * c;
            npp[k] = app - t * apq, nqq[k] = aqq + t * apq;
            po = p;
          }
        }
        pp[k] = po, qq[k] = q;
      }
      __syncthreads();
      for (int e = tid; e < np * D; e += T) {          // rows p, q of J^T A
        const int k = e / D, j = e - k * D;
        const int p = pp[k];
        if (p < 0) continue;
        const int q = qq[k];
        const double c = rc[k], s = rs[k];
        const double ap = A[(size_t)p * lda + j], aq = A[(size_t)q * lda + j];
        A[(size_t)p * lda + j] = c * ap - s * aq;
        A[(size_t)q * lda + j] = s * ap + c * aq;
      }
      __syncthreads();
      for (int e = tid; e < np * D; e += T) {          // columns p, q of (J^T A) J; the 2 x 2 block takes its closed form
        const int i = e / np, k = e - i * np;
        const int p = pp[k];
        if (p < 0) continue;
        const int q = qq[k];
        const double c = rc[k], s = rs[k];
        const double ap = A[(size_t)i * lda + p], aq = A[(size_t)i * lda + q];
        double vp = c * ap - s * aq, vq = s * ap + c * aq;
        if (i == p) vp = npp[k], vq = 0.0;
        if (i == q) vp = 0.0, vq = nqq[k];
        A[(size_t)i * lda + p] = vp;
        A[(size_t)i * lda + q] = vq;
      }
      __syncthreads();
    }
    ++sweeps;
  }
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
__global__ __launch_bounds__(256) void irs_count_kernel(const int* __restrict__ v, int N, UsPlan pl, int* __restrict__ cnt,
                                                        int* __restrict__ flags) {
  const int K = pl.K;
  const size_t total = (size_t)N * K;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e % K);
    const int val = v[e];
    if ((unsigned)val < (unsigned)(pl.coff[k + 1] - pl.coff[k]))
      atomicAdd(&cnt[pl.coff[k] + val], 1);
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
                                                                const int* __restrict__ cnt, int N, int D, UsPlan pl,
                                                                double q, double* __restrict__ Qs,
                                                                int* __restrict__ flags) {
  __shared__ double part[kIrsRowLanes][64];
  __shared__ int c3[3][3][64];
  __shared__ int cle[64];
  __shared__ unsigned long long mgt[64];
  const int tid = threadIdx.x, dl = tid & 63, rl = tid >> 6;
  const int slot = blockIdx.x;
  int k = 0;
  while (pl.coff[k + 1] <= slot) ++k;
  const int d = blockIdx.y * 64 + dl;
  const bool live = d < D;
  const int n = cnt[slot];
  if (n <= 0) {                                       // block-uniform
    if (rl == 0 && live) Qs[(size_t)slot * D + d] = 0.0;
    return;
  }
  int start = 0;
  for (int u = pl.coff[k]; u < slot; ++u) start += cnt[u];
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
                                                            UsPlan pl, int D, const float* __restrict__ mn,
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
      for (int u = pl.coff[k]; u < pl.coff[k + 1]; ++u)
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
  if (N < minN || N > kUsMaxN) return fail(minN == 2 ? "%s: N = %lld rows is outside 2..2^24" : "%s: N = %lld rows is outside 1..2^24", name, N);
  if (D < 1 || D > kUsMaxD) return fail("%s: D = %lld is outside 1..512", name, D);
  return 0;
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
static int us_plan(const char* name, int K, const int* fsize, UsPlan* pl) {
  if (K < 1 || K > kUsMaxK) return fail("%s: K = %lld factors is outside 1..16", name, K);
  if (!fsize) return fail("%s: no factor sizes", name);
  pl->K = K, pl->coff[0] = 0;
  for (int k = 0; k < K; ++k) {
    if (fsize[k] < 1 || fsize[k] > kUsMaxCsize)
      return fail("%s: factor %lld has %lld values, outside 1..256", name, k, fsize[k]);
    pl->coff[k + 1] = pl->coff[k] + fsize[k];
  }
  return 0;
}

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

int itcv_unsup_gauss_lds_dim(void) { return kGaussLdsDim; }

size_t itcv_unsup_gauss_workspace(int D) {
  if (D < 1 || D > kUsMaxD) return 0;
  return (size_t)D * D * sizeof(double);
}

int itcv_unsup_gauss(const double* cov, int D, double* res, double* eig, int* info, void* ws, size_t ws_bytes,
                     void* stream) {
  const char* name = "itcv_unsup_gauss";
  if (D < 1 || D > kUsMaxD) return fail("%s: D = %lld is outside 1..512", name, D);
  ITCV_REQUIRE(cov && res && eig && info, name);
  hipStream_t st = S(stream);
  if (D <= kGaussLdsDim) {
    launch_lds<us_gauss_kernel<true>>(dim3(1), dim3(kGaussThreads), (size_t)D * (D | 1) * sizeof(double), st, cov, D,
                                      (double*)nullptr, res, eig, info);
  } else {
    ITCV_REQUIRE(ws && ws_bytes >= (size_t)D * D * sizeof(double), "itcv_unsup_gauss(workspace)");
    hipLaunchKernelGGL(us_gauss_kernel<false>, dim3(1), dim3(kGaussThreads), 0, st, cov, D, static_cast<double*>(ws), res,
                       eig, info);
  }
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_irs_workspace(int N, int D, int K, int fsum) {
  if (N < 1 || N > kUsMaxN || D < 1 || D > kUsMaxD || K < 1 || K > kUsMaxK || fsum < K || fsum > K * kUsMaxCsize) return 0;
  return irs_ws(N, D, fsum).total;
}

int itcv_irs(const float* x, size_t ld, const int* v, const int* order, int N, int D, int K, const int* fsize, double q,
             const float* mn, const float* mx, double* maxdev, double* cum, double* M, double* score, int* parent,
             int* active, double* res, int* flags, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_irs";
  if (int e = us_shape(name, N, D, 1)) return e;
  UsPlan pl;
  if (int e = us_plan(name, K, fsize, &pl)) return e;
  if (!(q >= 0.0 && q <= 1.0)) return fail("%s: the quantile lies outside [0, 1]", name);
  ITCV_REQUIRE(x && v && order && mn && mx && maxdev && cum && M && score && parent && active && res && flags &&
                   ld >= (size_t)D,
               name);
  const int fsum = pl.coff[K];
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
