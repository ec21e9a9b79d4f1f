// What the score and density kernels share: unsup_scores.hip, quality.hip and gmm.hip take the block Cholesky, the cyclic
// Jacobi sweep and the f64-MFMA covariance pass from here; disent.hip, logreg.hip, gbt.hip, extra_scores.hip and udr.hip the
// finite test, the f64x4 type, the slice rule of their column passes and the class / factor plan.  This header includes
// common.h alone and is included by those files alone.
//
// Every one of these kernels has a fixed order of operations and none may contract a multiply and an add into a fused
// multiply-add, but not every file says so at file scope.  So, as in objective.h, EVERY arithmetic helper here carries
// `#pragma clang fp contract(off)` in its own body, the header has no file-scope pragma, and every device helper is
// __forceinline__: a helper gives the same bits wherever it is included, and after inlining the compiler still sees whether
// a caller's matrix lies in LDS or in global memory, as it did when the loops stood in the kernels.
//
// Deliberately NOT here: the column statistics of fvae_gvar_kernel and lr_colsum_* (their summation orders differ from
// the covariance pass, sharing would change bits) and the forward substitution of gmm_factor_kernel (one user).
#pragma once
#include "common.h"

namespace itcv {

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }   // false for NaN too

// Operand maps of v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result
// register i of lane l is C[row (l >> 4) + 4 i][col l & 15].
typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- one block on one dense symmetric matrix -------------------------------------------------------------------------
constexpr int kMatrixMaxDim = 512;        // largest D of the callers of block_cholesky / block_jacobi
constexpr int kMatrixThreads = 1024;      // their block: the Cholesky update is 32 x 32
constexpr int kLdsMatrixDim = 128;        // the matrix sits in LDS up to here: 128 x 129 doubles = 129 KiB of the CU's 160 KiB
constexpr int kJacobiMaxSweeps = 60;
constexpr double kJacobiTol = 1e-14;

// Cholesky of A[D][lda] (LDS, or global memory: a __syncthreads orders the block's own global writes), right-looking, the
// lower triangle in place; the upper triangle is left as it was.  Returns -1, or the dimension whose pivot is not a
// positive finite number; the test is block-uniform (every thread reads the same value), and on failure the columns
// before it hold the factor.
template <int THREADS>
__device__ __forceinline__ int block_cholesky(double* A, int lda, int D) {
#pragma clang fp contract(off)
  static_assert(THREADS == 1024, "the update takes 32 rows x 32 columns a step");
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  for (int j = 0; j < D; ++j) {
    const double piv = A[(size_t)j * lda + j];
    if (!(piv > 0.0) || !(piv <= DBL_MAX)) return j;
    const double l = sqrt(piv);
    __syncthreads();
    if (tid == 0) A[(size_t)j * lda + j] = l;
    for (int i = j + 1 + tid; i < D; i += THREADS) A[(size_t)i * lda + j] = A[(size_t)i * lda + j] / l;
    __syncthreads();
    for (int i = j + 1 + ty; i < D; i += 32) {
      const double lij = A[(size_t)i * lda + j];
      for (int k = j + 1 + tx; k <= i; k += 32) A[(size_t)i * lda + k] = A[(size_t)i * lda + k] - lij * A[(size_t)k * lda + j];
    }
    __syncthreads();
  }
  return -1;
}

struct JacobiScratch {                    // __shared__ in the calling kernel
  double rc[kMatrixMaxDim / 2], rs[kMatrixMaxDim / 2], npp[kMatrixMaxDim / 2], nqq[kMatrixMaxDim / 2];
  int pp[kMatrixMaxDim / 2], qq[kMatrixMaxDim / 2];
  double red[kMatrixThreads / 64];
};

// Cyclic Jacobi on the symmetric A[D][lda] until off_F <= kJacobiTol |A|_F (returns true) or kJacobiMaxSweeps sweeps are
// done (false); the eigenvalues are left on the diagonal, *sweeps is the number taken.  Round r of a sweep rotates the
// disjoint pairs of the round-robin schedule on Dp = D rounded up to even: (r, Dp - 1) and ((r + k) mod (Dp - 1),
// (r - k) mod (Dp - 1)), k = 1 .. Dp / 2 - 1; a pair that touches index D (odd D) or whose off-diagonal element is exactly 0
// is skipped, and an element a with |A_pp| + |a| == |A_pp| and |A_qq| + |a| == |A_qq| is set to 0 without a rotation
// (without that rule a matrix with two eigenvalues of multiplicity 64 each is still unconverged after 60 sweeps).
template <int THREADS>
__device__ __forceinline__ bool block_jacobi(double* A, int lda, int D, JacobiScratch* s, int* sweeps) {
#pragma clang fp contract(off)
  static_assert(THREADS <= kMatrixThreads, "red[] holds one element a wave");
  const int tid = threadIdx.x;
  const int Dp = (D + 1) & ~1, np = Dp / 2, M = Dp - 1;
  int done = 0;
  for (;;) {
    double off = 0.0, tot = 0.0;
    for (int e = tid; e < D * D; e += THREADS) {
      const int i = e / D, j = e - i * D;
      const double v = A[(size_t)i * lda + j];
      const double sq = v * v;
      tot += sq;
      if (i != j) off += sq;
    }
    off = block_sum(off, s->red);
    tot = block_sum(tot, s->red);
    const bool conv = sqrt(off) <= kJacobiTol * sqrt(tot);
    if (conv || done == kJacobiMaxSweeps) {
      *sweeps = done;
      return conv;
    }
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
            const double g = fabs(apq);
            if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
              // negligible against both diagonal elements: dropped by the identity rotation.  Inside a cluster of equal
              // eigenvalues tau is a quotient of two rounding errors; rotating by it refills what the sweep has cleared.
              s->rc[k] = 1.0, s->rs[k] = 0.0;
              s->npp[k] = app, s->nqq[k] = aqq;
            } else {
              const double tau = (aqq - app) / (2.0 * apq);
              const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
              const double c = 1.0 / sqrt(1.0 + t * t);
              s->rc[k] = c, s->rs[k] = t * c;
              s->npp[k] = app - t * apq, s->nqq[k] = aqq + t * apq;
            }
            po = p;
          }
        }
        s->pp[k] = po, s->qq[k] = q;
      }
      __syncthreads();
      for (int e = tid; e < np * D; e += THREADS) {    // rows p, q of J^T A
        const int k = e / D, j = e - k * D;
        const int p = s->pp[k];
        if (p < 0) continue;
        const int q = s->qq[k];
        const double c = s->rc[k], sn = s->rs[k];
        const double ap = A[(size_t)p * lda + j], aq = A[(size_t)q * lda + j];
        A[(size_t)p * lda + j] = c * ap - sn * aq;
        A[(size_t)q * lda + j] = sn * ap + c * aq;
      }
      __syncthreads();
      for (int e = tid; e < np * D; e += THREADS) {    // columns p, q of (J^T A) J; the 2 x 2 block takes its closed form
        const int i = e / np, k = e - i * np;
        const int p = s->pp[k];
        if (p < 0) continue;
        const int q = s->qq[k];
        const double c = s->rc[k], sn = s->rs[k];
        const double ap = A[(size_t)i * lda + p], aq = A[(size_t)i * lda + q];
        double vp = c * ap - sn * aq, vq = sn * ap + c * aq;
        if (i == p) vp = s->npp[k], vq = 0.0;
        if (i == q) vp = 0.0, vq = s->nqq[k];
        A[(size_t)i * lda + p] = vp;
        A[(size_t)i * lda + q] = vq;
      }
      __syncthreads();
    }
    ++done;
  }
}

// ---- the covariance pass: column sums, then 16 x 16 tile pairs on the f64 matrix cores ----------------------------------
// Rows are cut into slices, a function of N alone: 512 rows while that gives at most 64 slices, a multiple of 4 always.
// WEIGHTED: row n counts w[n * ldw] times (the weight multiplies the centred value of the A operand); otherwise the
// expressions have no weight in them at all.
constexpr int kCovSliceRows = 512;
constexpr int kCovMaxSlices = 64;
inline int cov_slice_rows(int N) {
  int ns = cdiv(N, kCovSliceRows);
  if (ns > kCovMaxSlices) ns = kCovMaxSlices;
  return cdiv(cdiv(N, ns), 4) * 4;
}

// tile pair p of the nt (nt + 1) / 2 pairs ti <= tj, row-major over the upper triangle
__device__ __forceinline__ void tile_pair(int p, int nt, int* ti, int* tj) {
  int i = 0;
  while (p >= nt - i) p -= nt - i, ++i;
  *ti = i, *tj = i + p;
}

// Column d of rows [r0, r1) by a block of four waves, lanes along the columns: wave w sums rows r0 + w, r0 + w + 4, ... in
// ascending order, the four are added in wave order; the result is valid in every thread.  Columns d >= D give 0, but
// WEIGHTED column D gives the sum of the weights.  *bad is set on a non-finite element.
template <bool WEIGHTED>
__device__ __forceinline__ double block_colsum(const float* __restrict__ x, size_t ld, int d, int D, int r0, int r1,
                                               const double* __restrict__ w, size_t ldw, double (*sm)[64], bool* bad) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  double s = 0.0;
  if (d < D) {
    for (int r = r0 + wid; r < r1; r += 4) {
      const float v = x[(size_t)r * ld + d];
      *bad |= !finite_f(v);
      if constexpr (WEIGHTED)
        s += w[(size_t)r * ldw] * (double)v;
      else
        s += (double)v;
    }
  } else if (WEIGHTED && d == D) {
    for (int r = r0 + wid; r < r1; r += 4) s += w[(size_t)r * ldw];
  }
  sm[wid][lane] = s;
  __syncthreads();
  return ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}

// One wave: the 16 x 16 tile (ti, tj) of sum_n a_n b_n^T over rows [r0, r1), four rows a product.  A is the transposed tile
// of centred columns ti (times the row's weight), B the tile of centred columns tj; rows past r1 and columns past D enter as
// zeros.
template <bool WEIGHTED>
__device__ __forceinline__ f64x4 cov_tile_rows(const float* __restrict__ x, size_t ld, int D, int ti, int tj, int r0, int r1,
                                               const double* __restrict__ mean, const double* __restrict__ w, size_t ldw) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  const int ci = ti * 16 + lr, cj = tj * 16 + lr;
  const bool iok = ci < D, jok = cj < D;
  const double mi = iok ? mean[ci] : 0.0, mj = jok ? mean[cj] : 0.0;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r += 4) {
    const int n = r + lk;
    const bool rok = n < r1;
    double a;
    if constexpr (WEIGHTED)
      a = (rok && iok) ? w[(size_t)n * ldw] * ((double)x[(size_t)n * ld + ci] - mi) : 0.0;
    else
      a = (rok && iok) ? (double)x[(size_t)n * ld + ci] - mi : 0.0;
    const double b = (rok && jok) ? (double)x[(size_t)n * ld + cj] - mj : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  return acc;
}
// the wave's tile to out[16][16]
__device__ __forceinline__ void cov_tile_store(double* __restrict__ out, f64x4 acc) {
  const int lr = threadIdx.x & 15, lk = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[(lk + 4 * i) * 16 + lr] = acc[i];
}
// the element (i, j) that thread a * 16 + b of a 256-thread block folds for tile pair p: false below the diagonal of a
// diagonal tile and past D, where there is none
__device__ __forceinline__ bool cov_fold_element(int p, int nt, int D, int* i, int* j) {
  int ti, tj;
  tile_pair(p, nt, &ti, &tj);
  const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
  *i = ti * 16 + a, *j = tj * 16 + b;
  return *i < D && *j < D && !(ti == tj && a > b);
}

// ---- host side -------------------------------------------------------------------------------------------------------
// slices of a column pass over N rows: rows0 rows each, doubled until there are at most max_slices
inline int doubling_slices(int N, int rows0, int max_slices, int* rows) {
  int r = rows0;
  while (cdiv(N, r) > max_slices) r *= 2;
  *rows = r;
  return cdiv(N, r);
}

// K segments (the classes of K problems, the values of K factors) laid end to end
constexpr int kSegMaxK = 16;
struct SegPlan {
  int K;
  int off[kSegMaxK + 1];   // prefix sums of the sizes; their sum is off[K]
};
// a file's nouns in the refusals: `k` words K with a %lld ("K = %lld problems"), `missing` is the message for sizes ==
// nullptr (nullptr: the caller has checked), `size` words one segment with two %lld ("problem %lld has %lld classes")
struct SegWords {
  const char *k, *missing, *size;
};
inline int seg_plan(const char* name, int K, const int* sizes, int max_size, const SegWords& words, SegPlan* pl) {
  if (need_dim(name, words.k, K, 1, kSegMaxK, "1..16")) return 1;
  char fmt[128];
  if (!sizes && words.missing) {
    snprintf(fmt, sizeof(fmt), "%%s: %s", words.missing);
    return fail(fmt, name);
  }
  pl->K = K, pl->off[0] = 0;
  for (int k = 0; k < K; ++k) {
    if (sizes[k] < 1 || sizes[k] > max_size) {
      snprintf(fmt, sizeof(fmt), "%%s: %s, outside 1..%d", words.size, max_size);
      return fail(fmt, name, k, sizes[k]);
    }
    pl->off[k + 1] = pl->off[k] + sizes[k];
  }
  return 0;
}

}  // namespace itcv
