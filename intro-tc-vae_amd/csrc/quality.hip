// Sample-quality scores on the device: k-th-neighbour radii and the precision / recall / density / coverage counts
// (Kynkaanniemi et al. 2019, Naeem et al. 2020), the three sums of the polynomial-kernel MMD (KID, Binkowski et al. 2018)
// and the Frechet distance of two Gaussians.  The rules are in include/itcv_hip.h; the inputs are fp32 feature rows
// x[N][D] (row stride ld), read in place, and all arithmetic is fp64:
//   pairs     : a block owns 32 query rows and streams 64 candidate rows a tile through LDS, 32 columns a chunk; thread
//               (query tq, lane tc) accumulates d^2 = sum_d (a_d - b_d)^2 in ascending d for the candidates tc, tc + 8, ..
//               and then either keeps the k + 1 smallest values it has seen (radii; the 8 lists of a query are merged at
//               the end of the block, the lists of the candidate slices by a second kernel) or compares against the two
//               radii (counts; integer atomics and a minimum over bit patterns, both order-free);
//   poly_mmd  : a 64 x 64 tile of dot products a block on v_mfma_f64_16x16x4_f64 from the widened fp32 values, the kernel
//               value and the tile's sum in the epilogue; a block walks the tiles b, b + G, ... (G a function of the
//               shapes) and leaves one partial, one thread folds each sum's partials in ascending order;
//   frechet   : ONE block: Cholesky of C1 + eps I, M = L^T (C2 + eps I) L, then the cyclic Jacobi iteration on M itself
//               (block_cholesky and block_jacobi of csrc/dense.h, which itcv_unsup_gauss runs too).
// A selection does not depend on the visiting order and every floating-point sum has a fixed order that depends on the
// shapes alone; there is no floating-point atomic.  Nothing in this file may be contracted into a fused multiply-add.
#include "dense.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kQMaxN = 1 << 20;
constexpr int kQMaxD = 2048;
constexpr int kQMaxK = 16;
constexpr int kQLists = kQMaxK + 1;       // entries of a list: the k + 1 smallest
constexpr int kQRows = 32;                // query rows of a block
constexpr int kQCand = 64;                // candidate rows of a tile
constexpr int kQChunk = 32;               // columns of a chunk
constexpr int kQLd = kQChunk + 4;         // LDS row stride in floats: 16-byte rows, 8 rows of a wave on 32 different banks
constexpr int kQThreads = 256;            // 32 queries x 8 candidate lanes
constexpr int kQPer = kQCand / 8;         // candidates of a thread in a tile
constexpr int kQMaxSplits = 256;
constexpr int kQFillBlocks = 1024;        // splits = 0: slices until the grid has this many blocks
constexpr int kPolyTile = 64;
constexpr int kPolyParts = 1024;          // partial sums of one of the three sums
constexpr int kFrMaxD = kMatrixMaxDim;

// rows [r0, r0 + R) x columns [d0, d0 + kQChunk) of src into s[R][kQLd]; rows from rend on and columns from D on are 0
template <int R, int THREADS>
__device__ __forceinline__ bool q_load_rows(float (*s)[kQLd], const float* __restrict__ src, size_t ld, int r0, int rend,
                                            int d0, int D) {
  bool bad = false;
  for (int e = threadIdx.x; e < R * kQChunk; e += THREADS) {
    const int r = e / kQChunk, dd = e - r * kQChunk;
    const int row = r0 + r, d = d0 + dd;
    float v = 0.f;
    if (row < rend && d < D) {
      v = src[(size_t)row * ld + d];
      bad |= !finite_f(v);
    }
    s[r][dd] = v;
  }
  return bad;
}

// v into the ascending list l[0 .. K1)[tid] if it is below the list's largest entry
__device__ __forceinline__ void q_insert(double (*l)[kQThreads], int K1, int tid, double v) {
  if (!(v < l[K1 - 1][tid])) return;
  int p = K1 - 1;
  while (p > 0 && l[p - 1][tid] > v) {
    l[p][tid] = l[p - 1][tid];
    --p;
  }
  l[p][tid] = v;
}

// grid (query tile, candidate slice).  COUNTS false: lists[slice][NQ][K1], the K1 smallest d^2 of every query row over the
// slice's candidates, ascending (+inf where the slice has fewer).  COUNTS true: chits[c] += #{q : d^2 < r2q[q]},
// qcov[q] |= exists c : d^2 < r2c[c], qmin[q] = min(qmin[q], min_c d^2) as the bit pattern of a non-negative double.
template <bool COUNTS>
__global__ __launch_bounds__(kQThreads) void q_pairs_kernel(const float* __restrict__ q, size_t ldq, int NQ,
                                                            const float* __restrict__ c, size_t ldc, int NC, int D,
                                                            int slice, int K1, double* __restrict__ lists,
                                                            const double* __restrict__ r2q,
                                                            const double* __restrict__ r2c, int* __restrict__ chits,
                                                            int* __restrict__ qcov,
                                                            unsigned long long* __restrict__ qmin,
                                                            int* __restrict__ flags) {
  __shared__ __attribute__((aligned(16))) float sq[kQRows][kQLd];
  __shared__ __attribute__((aligned(16))) float sc[kQCand][kQLd];
  __shared__ double sl[COUNTS ? 1 : kQLists][kQThreads];
  __shared__ double sr2[kQCand];
  const int tid = threadIdx.x, tq = tid >> 3, tc = tid & 7;
  const int q0 = blockIdx.x * kQRows, qi = q0 + tq;
  const bool qok = qi < NQ;
  const int c_lo = blockIdx.y * slice, c_hi = min(NC, c_lo + slice);
  const double inf = __builtin_inf();
  bool bad = false, covered = false;
  double mn = inf, myr2 = 0.0;
  if constexpr (COUNTS) {
    if (qok) myr2 = r2q[qi];
  } else {
    for (int j = 0; j < K1; ++j) sl[j][tid] = inf;
  }
  const bool one_chunk = D <= kQChunk;
  if (one_chunk) bad |= q_load_rows<kQRows, kQThreads>(sq, q, ldq, q0, NQ, 0, D);
  for (int c0 = c_lo; c0 < c_hi; c0 += kQCand) {
    double acc[kQPer];
#pragma unroll
    for (int j = 0; j < kQPer; ++j) acc[j] = 0.0;
    for (int d0 = 0; d0 < D; d0 += kQChunk) {
      __syncthreads();
      if (!one_chunk) bad |= q_load_rows<kQRows, kQThreads>(sq, q, ldq, q0, NQ, d0, D);
      bad |= q_load_rows<kQCand, kQThreads>(sc, c, ldc, c0, c_hi, d0, D);
      if constexpr (COUNTS)
        if (d0 == 0 && tid < kQCand) sr2[tid] = c0 + tid < c_hi ? r2c[c0 + tid] : 0.0;
      __syncthreads();
      // the columns past D are zeros on both sides: they add +0.0 to a non-negative sum, which changes no bit
      const int dn = min(kQChunk, (D - d0 + 3) & ~3);
      for (int d = 0; d < dn; d += 4) {
        const float4 a = *reinterpret_cast<const float4*>(&sq[tq][d]);
#pragma unroll
        for (int j = 0; j < kQPer; ++j) {
          const float4 b = *reinterpret_cast<const float4*>(&sc[tc + 8 * j][d]);
          const double t0 = (double)a.x - (double)b.x, t1 = (double)a.y - (double)b.y;
          const double t2 = (double)a.z - (double)b.z, t3 = (double)a.w - (double)b.w;
          double s = acc[j];
          s = s + t0 * t0;
          s = s + t1 * t1;
          s = s + t2 * t2;
          s = s + t3 * t3;
          acc[j] = s;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kQPer; ++j) {
      const int ci = c0 + tc + 8 * j;
      if (ci >= c_hi || !qok) continue;
      const double v = acc[j];
      if constexpr (COUNTS) {
        if (v < myr2) atomicAdd(&chits[ci], 1);
        if (v < sr2[tc + 8 * j]) covered = true;
        if (v < mn) mn = v;
      } else {
        q_insert(sl, K1, tid, v);
      }
    }
  }
  if (bad) atomicOr(&flags[0], 1);
  if constexpr (COUNTS) {
    if (qok) {
      if (covered) atomicOr(&qcov[qi], 1);
      if (mn < inf) atomicMin(&qmin[qi], (unsigned long long)__double_as_longlong(mn));
    }
  } else {
    __syncthreads();
    if (tc == 0 && qok) {
      for (int t = 1; t < 8; ++t)
        for (int j = 0; j < K1; ++j) {
          const double v = sl[j][tid + t];
          if (!(v < sl[K1 - 1][tid])) break;          // ascending: the rest is no smaller
          q_insert(sl, K1, tid, v);
        }
      double* out = lists + ((size_t)blockIdx.y * NQ + qi) * K1;
      for (int j = 0; j < K1; ++j) out[j] = sl[j][tid];
    }
  }
}

// a thread per row: the K1-th smallest of the union of the ns lists
__global__ __launch_bounds__(kQThreads) void q_merge_kernel(const double* __restrict__ lists, int ns, int N, int K1,
                                                            double* __restrict__ r2) {
  __shared__ double sl[kQLists][kQThreads];
  const int tid = threadIdx.x, i = blockIdx.x * kQThreads + tid;
  if (i >= N) return;
  for (int j = 0; j < K1; ++j) sl[j][tid] = lists[(size_t)i * K1 + j];
  for (int s = 1; s < ns; ++s) {
    const double* l = lists + ((size_t)s * N + i) * K1;
    for (int j = 0; j < K1; ++j) {
      const double v = l[j];
      if (!(v < sl[K1 - 1][tid])) break;
      q_insert(sl, K1, tid, v);
    }
  }
  r2[i] = sl[K1 - 1][tid];
}

__global__ __launch_bounds__(256) void q_counts_init_kernel(int* __restrict__ chits, int M, int* __restrict__ qcov,
                                                            unsigned long long* __restrict__ qmin, int N) {
  const unsigned long long inf = (unsigned long long)__double_as_longlong(__builtin_inf());
  for (int e = blockIdx.x * 256 + threadIdx.x; e < max(N, M); e += gridDim.x * 256) {
    if (e < M) chits[e] = 0;
    if (e < N) qcov[e] = 0, qmin[e] = inf;
  }
}

// ---- polynomial-kernel sums --------------------------------------------------------------------------------------------
__device__ __forceinline__ double q_poly(double dot, double gamma, double c0, int p) {
  const double t = gamma * dot + c0;
  if (p == 1) return t;
  const double t2 = t * t;
  if (p == 2) return t2;
  return p == 3 ? t2 * t : t2 * t2;
}

// Block b takes the 64 x 64 tiles b, b + gridDim.x, ... of the NA x NB kernel matrix (tile t = ti * ntb + tj) and leaves
// part[b] = the sum of their sums in that order.  Four waves, each a 32 x 32 quarter as 2 x 2 MFMA tiles; the operand maps
// are at f64x4 in csrc/dense.h.  Tile sum: every lane adds its 16 elements in register order, the xor butterfly
// folds a wave, the four waves are added in wave order.  skip_diag leaves out the elements with row == col (a on a).
__global__ __launch_bounds__(256) void q_poly_kernel(const float* __restrict__ a, size_t lda, int NA,
                                                     const float* __restrict__ b, size_t ldb, int NB, int D, int p,
                                                     double gamma, double c0, int skip_diag, long long ntiles, int ntb,
                                                     double* __restrict__ part, int* __restrict__ flags) {
  __shared__ float sa[kPolyTile][kQLd];
  __shared__ float sb[kPolyTile][kQLd];
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const int wr = (w >> 1) * 32, wc = (w & 1) * 32;
  double total = 0.0;
  bool bad = false;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int r0 = (int)(t / ntb) * kPolyTile, c0t = (int)(t % ntb) * kPolyTile;
    f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int d0 = 0; d0 < D; d0 += kQChunk) {
      __syncthreads();
      bad |= q_load_rows<kPolyTile, 256>(sa, a, lda, r0, NA, d0, D);
      bad |= q_load_rows<kPolyTile, 256>(sb, b, ldb, c0t, NB, d0, D);
      __syncthreads();
      const int dn = min(kQChunk, (D - d0 + 3) & ~3);
      for (int kk = 0; kk < dn; kk += 4) {
        const double a0 = (double)sa[wr + lr][kk + lk], a1 = (double)sa[wr + 16 + lr][kk + lk];
        const double b0 = (double)sb[wc + lr][kk + lk], b1 = (double)sb[wc + 16 + lr][kk + lk];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    }
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = r0 + wr + 16 * m + lk + 4 * i, col = c0t + wc + 16 * n + lr;
          if (row < NA && col < NB && !(skip_diag && row == col)) s += q_poly(acc[m][n][i], gamma, c0, p);
        }
    s = wave_sum(s);
    __syncthreads();
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (tid == 0) total += ((red[0] + red[1]) + red[2]) + red[3];
  }
  if (bad) atomicOr(&flags[0], 1);
  if (tid == 0) part[blockIdx.x] = total;
}

// threads 0..2 fold the partials of Sxx, Syy, Sxy in ascending order; thread 0 forms the unbiased estimate
__global__ __launch_bounds__(64) void q_poly_finish_kernel(const double* __restrict__ part, int gxx, int gyy, int gxy, int N,
                                                           int M, double* __restrict__ res) {
  __shared__ double s[3];
  const int t = threadIdx.x;
  if (t < 3) s[t] = fold_strided(0.0, part + (size_t)t * kPolyParts, (size_t)1, t == 0 ? gxx : (t == 1 ? gyy : gxy));
  __syncthreads();
  if (t == 0) {
    const double n = (double)N, m = (double)M;
    res[0] = s[0], res[1] = s[1], res[2] = s[2];
    res[3] = (s[0] / (n * (n - 1.0)) + s[1] / (m * (m - 1.0))) - (2.0 * s[2]) / (n * m);
  }
}

// ---- Frechet distance --------------------------------------------------------------------------------------------------
// One block of 1024 threads.  A[D][lda] is the working matrix (LDS, or the third D x D block of the workspace); the first
// two blocks of the workspace hold T = (C2 + eps I) L and M.  The Cholesky factorisation and the Jacobi sweep are
// block_cholesky and block_jacobi (csrc/dense.h); the sweep runs on M itself.
template <bool IN_LDS>
__global__ __launch_bounds__(kMatrixThreads) void q_frechet_kernel(const double* __restrict__ m1, const double* __restrict__ c1,
                                                               const double* __restrict__ m2, const double* __restrict__ c2,
                                                               int D, double eps, double* __restrict__ ws,
                                                               double* __restrict__ res, double* __restrict__ eig,
                                                               int* __restrict__ info) {
  extern __shared__ double q_lds[];
  __shared__ JacobiScratch js;
  const int tid = threadIdx.x, T = kMatrixThreads;
  const int lda = IN_LDS ? (D | 1) : D;
  double* A = IN_LDS ? q_lds : ws + 2 * (size_t)D * D;
  double* Tm = ws;
  double* Mm = ws + (size_t)D * D;
  const double nan = __builtin_nan("");

  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    A[(size_t)i * lda + j] = i == j ? c1[e] + eps : c1[e];
  }
  __syncthreads();
  const int fail_dim = block_cholesky<kMatrixThreads>(A, lda, D);
  if (fail_dim >= 0) {
    if (tid == 0) {
      info[0] = 1, info[1] = fail_dim, info[2] = 0, info[3] = 0, info[4] = 0;
      for (int i = 0; i < 5; ++i) res[i] = nan;
    }
    for (int d = tid; d < D; d += T) eig[d] = nan;
    return;
  }
  // T = (C2 + eps I) L: L is lower triangular, so column j of the product takes k = j .. D - 1, ascending
  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    double s = 0.0;
    for (int k = j; k < D; ++k) {
      const double b = i == k ? c2[(size_t)i * D + k] + eps : c2[(size_t)i * D + k];
      s += b * A[(size_t)k * lda + j];
    }
    Tm[e] = s;
  }
  __syncthreads();
  // M = L^T T: the upper triangle, k = i .. D - 1 ascending, mirrored
  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    if (i > j) continue;
    double s = 0.0;
    for (int k = i; k < D; ++k) s += A[(size_t)k * lda + i] * Tm[(size_t)k * D + j];
    Mm[(size_t)i * D + j] = s;
    Mm[(size_t)j * D + i] = s;
  }
  __syncthreads();
  for (int e = tid; e < D * D; e += T) {
    const int i = e / D, j = e - i * D;
    A[(size_t)i * lda + j] = Mm[e];
  }
  __syncthreads();
  int sweeps;
  const bool conv = block_jacobi<kMatrixThreads>(A, lda, D, &js, &sweeps);
  for (int d = tid; d < D; d += T) eig[d] = A[(size_t)d * lda + d];
  if (tid == 0) {
    double dm = 0.0, tr1 = 0.0, tr2 = 0.0, trs = 0.0;
    int clipped = 0;
    for (int d = 0; d < D; ++d) {
      const double t = m1[d] - m2[d];
      dm += t * t;
      tr1 += c1[(size_t)d * D + d] + eps;
      tr2 += c2[(size_t)d * D + d] + eps;
      const double lam = A[(size_t)d * lda + d];
      clipped += lam < 0.0;
      trs += sqrt(fmax(lam, 0.0));
    }
    res[0] = ((dm + tr1) + tr2) - 2.0 * trs;
    res[1] = dm, res[2] = tr1, res[3] = tr2, res[4] = trs;
    info[0] = 0, info[1] = -1, info[2] = conv ? 0 : 1, info[3] = sweeps, info[4] = clipped;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int q_shape(const char* name, const char* nwhat, int N, int D) {
  return need_dim(name, nwhat, N, 2, kQMaxN, "2..2^20") || need_dim(name, "D = %lld", D, 1, kQMaxD, "1..2048");
}
struct QSlices {
  int slice, ns;
};
// the candidate slices of NC candidates for NQ queries: `splits` of them (0: until the grid has kQFillBlocks blocks), at
// most one per candidate tile and at most kQMaxSplits; slices that would be empty are not made
static inline QSlices q_slices(int NQ, int NC, int splits) {
  int s = splits > 0 ? splits : cdiv(kQFillBlocks, cdiv(NQ, kQRows));
  const int most = cdiv(NC, kQCand) < kQMaxSplits ? cdiv(NC, kQCand) : kQMaxSplits;
  s = s < 1 ? 1 : (s > most ? most : s);
  QSlices q;
  q.slice = cdiv(NC, s), q.ns = cdiv(NC, q.slice);
  return q;
}
static inline int poly_grid(int NA, int NB, long long* ntiles, int* ntb) {
  *ntb = cdiv(NB, kPolyTile);
  *ntiles = (long long)cdiv(NA, kPolyTile) * *ntb;
  return (int)(*ntiles < kPolyParts ? *ntiles : kPolyParts);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_knn_radius_workspace(int N, int D, int k, int splits) {
  if (N < 2 || N > kQMaxN || D < 1 || D > kQMaxD || k < 1 || k > kQMaxK || k >= N || splits < 0) return 0;
  return (size_t)q_slices(N, N, splits).ns * N * (k + 1) * sizeof(double);
}

int itcv_knn_radius(const float* x, size_t ld, int N, int D, int k, int splits, double* r2, int* flags, void* ws,
                    size_t ws_bytes, void* stream) {
  const char* name = "itcv_knn_radius";
  if (q_shape(name, "N = %lld rows", N, D) || need_dim(name, "k = %lld", k, 1, kQMaxK, "1..16")) return 1;
  if (k >= N) return fail("%s: k = %lld needs more than %lld rows", name, k, N);
  if (need_dim(name, "splits = %lld", splits, 0, INT32_MAX, "0..") || need_pointers(name, x && r2 && flags) ||
      need_stride(name, "a", ld, "D", D))
    return 1;
  const QSlices q = q_slices(N, N, splits);
  ITCV_REQUIRE(ws && ws_bytes >= (size_t)q.ns * N * (k + 1) * sizeof(double), "itcv_knn_radius(workspace)");
  double* lists = static_cast<double*>(ws);
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(q_pairs_kernel<false>, dim3(cdiv(N, kQRows), q.ns), dim3(kQThreads), 0, st, x, ld, N, x, ld, N, D,
                     q.slice, k + 1, lists, (const double*)nullptr, (const double*)nullptr, (int*)nullptr, (int*)nullptr,
                     (unsigned long long*)nullptr, flags);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(q_merge_kernel, dim3(cdiv(N, kQThreads)), dim3(kQThreads), 0, st, (const double*)lists, q.ns, N, k + 1,
                     r2);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_prdc_counts(const float* real, size_t ldr, const float* fake, size_t ldf, int N, int M, int D,
                     const double* r2_real, const double* r2_fake, int splits, int* fake_hits, int* real_covered,
                     double* real_min, int* flags, void* stream) {
  const char* name = "itcv_prdc_counts";
  if (q_shape(name, "N = %lld real rows", N, D) || need_dim(name, "M = %lld fake rows", M, 2, kQMaxN, "2..2^20") ||
      need_dim(name, "splits = %lld", splits, 0, INT32_MAX, "0..") ||
      need_pointers(name, real && fake && r2_real && r2_fake && fake_hits && real_covered && real_min && flags) ||
      need_stride(name, "real's", ldr, "D", D) || need_stride(name, "fake's", ldf, "D", D))
    return 1;
  const QSlices q = q_slices(N, M, splits);
  hipStream_t st = S(stream);
  unsigned long long* qmin = reinterpret_cast<unsigned long long*>(real_min);
  hipLaunchKernelGGL(q_counts_init_kernel, dim3(stream_grid((size_t)(N > M ? N : M), 1)), dim3(256), 0, st, fake_hits, M,
                     real_covered, qmin, N);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(q_pairs_kernel<true>, dim3(cdiv(N, kQRows), q.ns), dim3(kQThreads), 0, st, real, ldr, N, fake, ldf, M,
                     D, q.slice, 0, (double*)nullptr, r2_real, r2_fake, fake_hits, real_covered, qmin, flags);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_poly_mmd_workspace(int N, int M, int D) {
  if (N < 2 || N > kQMaxN || M < 2 || M > kQMaxN || D < 1 || D > kQMaxD) return 0;
  return (size_t)3 * kPolyParts * sizeof(double);
}

int itcv_poly_mmd(const float* x, size_t ldx, const float* y, size_t ldy, int N, int M, int D, int degree, double gamma,
                  double coef0, double* res, int* flags, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_poly_mmd";
  if (q_shape(name, "N = %lld rows of x", N, D) || need_dim(name, "M = %lld rows of y", M, 2, kQMaxN, "2..2^20") ||
      need_dim(name, "degree = %lld", degree, 1, 4, "1..4"))
    return 1;
  if (!itcv::finite(gamma) || gamma < 0.0 || !itcv::finite(coef0))
    return fail("%s: gamma must be finite and >= 0, coef0 finite", name);
  if (need_pointers(name, x && y && res && flags) || need_stride(name, "x's", ldx, "D", D) ||
      need_stride(name, "y's", ldy, "D", D))
    return 1;
  ITCV_REQUIRE(ws && ws_bytes >= (size_t)3 * kPolyParts * sizeof(double), "itcv_poly_mmd(workspace)");
  double* part = static_cast<double*>(ws);
  const double g = gamma == 0.0 ? 1.0 / (double)D : gamma;
  hipStream_t st = S(stream);
  int grids[3];
  for (int which = 0; which < 3; ++which) {
    const float* a = which == 1 ? y : x;
    const float* b = which == 0 ? x : y;
    const size_t la = which == 1 ? ldy : ldx, lb = which == 0 ? ldx : ldy;
    const int na = which == 1 ? M : N, nb = which == 0 ? N : M;
    long long ntiles;
    int ntb;
    grids[which] = poly_grid(na, nb, &ntiles, &ntb);
    hipLaunchKernelGGL(q_poly_kernel, dim3(grids[which]), dim3(256), 0, st, a, la, na, b, lb, nb, D, degree, g, coef0,
                       which < 2 ? 1 : 0, ntiles, ntb, part + (size_t)which * kPolyParts, flags);
    ITCV_CHECK_LAUNCH(name);
  }
  hipLaunchKernelGGL(q_poly_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)part, grids[0], grids[1], grids[2], N, M,
                     res);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_frechet_workspace(int D) {
  if (D < 1 || D > kFrMaxD) return 0;
  return (size_t)(D <= kLdsMatrixDim ? 2 : 3) * D * D * sizeof(double);
}

int itcv_frechet(const double* m1, const double* c1, const double* m2, const double* c2, int D, double eps, double* res,
                 double* eig, int* info, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "itcv_frechet";
  if (need_dim(name, "D = %lld", D, 1, kFrMaxD, "1..512")) return 1;
  if (!itcv::finite(eps) || eps < 0.0) return fail("%s: eps must be finite and >= 0", name);
  if (need_pointers(name, m1 && c1 && m2 && c2 && res && eig && info)) return 1;
  ITCV_REQUIRE(ws && ws_bytes >= itcv_frechet_workspace(D), "itcv_frechet(workspace)");
  hipStream_t st = S(stream);
  if (D <= kLdsMatrixDim)
    launch_lds<q_frechet_kernel<true>>(dim3(1), dim3(kMatrixThreads), (size_t)D * (D | 1) * sizeof(double), st, m1, c1, m2, c2, D,
                                       eps, static_cast<double*>(ws), res, eig, info);
  else
    hipLaunchKernelGGL(q_frechet_kernel<false>, dim3(1), dim3(kMatrixThreads), 0, st, m1, c1, m2, c2, D, eps,
                       static_cast<double*>(ws), res, eig, info);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
