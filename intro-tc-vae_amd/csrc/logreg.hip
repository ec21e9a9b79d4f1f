// Classifier-based disentanglement scores on the device: what the reference's evaluation package does with sklearn on
// the host (beta-VAE score: evaluation/metrics.py:20-79, utils.py:60-174; explicitness: metrics.py:237-304,
// utils.py:277-320) needs five pieces of arithmetic, all in fp64 on fp32 representations x[N][D] (row stride ld):
//   colstats : StandardScaler's mean[D] and scale[D] (population variance, scale = 1 where the variance is 0);
//   valgrad  : value and gradient of K L2-regularised softmax regressions at once (the rule is in include/itcv_hip.h);
//   proba    : P[N][csum] and pred[N][K] at a given theta;
//   auc      : one-vs-rest ROC AUC of every class as integer pair counts;
//   zdiff    : mean_b |a[b][d] - b[b][d]|, one row of the beta-VAE score's training set.
// The two GEMMs of valgrad (logits X.W and gradient X^T (P - Y)) run on v_mfma_f64_16x16x4_f64.  Every floating-point
// reduction has a fixed order (per-block partials folded in ascending block order, no floating-point atomics); the pair
// counts are integers.  Two calls with the same inputs return the same bits.
#include "dense.h"

namespace itcv {

constexpr int kLrMaxCsize = 256;
constexpr int kLrMaxD = 512;
constexpr int kLrMaxN = 1 << 30;
constexpr int kLrStatRows = 256;        // rows per block of the column statistics
constexpr int kLrStatMaxSlices = 1024;
constexpr int kLrMaxBlocks = 1024;      // row-tile owners of valgrad: each keeps one partial gradient
constexpr size_t kLrPartBudget = (size_t)256 << 20;   // bytes of partial gradients at the most
constexpr size_t kLrLdsTwoTiles = 96 * 1024;          // 32 rows per tile while the block's LDS stays below this
constexpr int kAucRows = 256;           // rows i per block of the pair count (one per thread)
constexpr int kAucTj = 16;              // rows j per LDS tile

// ---- column statistics ---------------------------------------------------------------------------------------------
// grid (64-column tile, row slice).  center == nullptr: partial sums of x; else partial sums of (x - center)^2.
__global__ __launch_bounds__(256) void lr_colsum_part_kernel(const float* __restrict__ x, size_t ld, int N, int D, int rows,
                                                             const double* __restrict__ center, double* __restrict__ part,
                                                             int* __restrict__ flags) {
  __shared__ double sm[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  double s = 0.0;
  bool bad = false;
  if (d < D) {
    const double c = center ? center[d] : 0.0;
    for (int r = r0 + wid; r < r1; r += 4) {
      const float v = x[(size_t)r * ld + d];
      bad |= !finite_f(v);
      const double t = (double)v - c;
      s += center ? t * t : t;
    }
  }
  sm[wid][lane] = s;
  if (bad) atomicOr(&flags[0], 1);
  __syncthreads();
  if (wid == 0 && d < D) part[(size_t)blockIdx.y * D + d] = ((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane];
}
// mode 0: out = sum / N (the mean); mode 1: out = sqrt(sum / N), or 1 where the sum is 0 (the scale)
__global__ __launch_bounds__(256) void lr_colsum_fold_kernel(const double* __restrict__ part, int ns, int D, int N, int mode,
                                                             double* __restrict__ out) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  const double m = fold_strided(0.0, part + d, (size_t)D, ns) / (double)N;
  out[d] = mode == 0 ? m : (m == 0.0 ? 1.0 : sqrt(m));
}

// ---- softmax regression: value + gradient, or probabilities + predictions ------------------------------------------
// A block owns row tiles t = blockIdx.x, blockIdx.x + gridDim.x, ... of 16 * MT rows.  Per tile: x is read ONCE, standardised
// into LDS as fp64, and serves every problem p in turn:
//   logits   Z[rows][S_p] = Xs . W[:, seg_p] + b      (MFMA, A from LDS, B = theta from global / L2)      -> LDS
//   softmax  over the valid classes of every row; R = P - Y (0 for rows whose label is not a valid class)   in place
//   gradient G[D + 1][S_p] = [Xs 1]^T . R             (MFMA, both operands from LDS)   -> this block's partial gradient
// The f64 MFMA operand maps are at f64x4 in csrc/dense.h.
template <int MT, bool GRAD>
__global__ __launch_bounds__(256) void lr_softmax_kernel(const float* __restrict__ x, size_t ld,
                                                         const double* __restrict__ mean, const double* __restrict__ scale,
                                                         const int* __restrict__ y, int N, int D, SegPlan pl, int segmax,
                                                         const int* __restrict__ cvalid, const double* __restrict__ theta,
                                                         double* __restrict__ part, double* __restrict__ fpart,
                                                         int* __restrict__ cnt, double* __restrict__ P,
                                                         int* __restrict__ pred, int* __restrict__ flags) {
  extern __shared__ double lds[];
  constexpr int RT = 16 * MT;
  const int ldx = D | 1, ldz = segmax | 1;
  double* xs = lds;                                  // [RT][ldx]
  double* zs = xs + (size_t)RT * ldx;                // [RT][ldz]
  double* fs = zs + (size_t)RT * ldz;                // [4][kSegMaxK]
  int* cs = reinterpret_cast<int*>(fs + 4 * kSegMaxK);   // [4][kSegMaxK]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int K = pl.K, csum = pl.off[K];
  const int ntiles = cdiv(N, RT);
  const size_t gsz = (size_t)(D + 1) * csum;
  double* mypart = GRAD ? part + (size_t)blockIdx.x * gsz : nullptr;
  if (tid < 4 * kSegMaxK) fs[tid] = 0.0, cs[tid] = 0;
  bool bad_x = false, bad_y = false;

  for (int t = blockIdx.x, it = 0; t < ntiles; t += gridDim.x, ++it) {
    const int r0 = t * RT;
    __syncthreads();
    for (int e = tid; e < RT * D; e += 256) {
      const int r = e / D, d = e - r * D;
      double v = 0.0;
      if (r0 + r < N) {
        const float xv = x[(size_t)(r0 + r) * ld + d];
        bad_x |= !finite_f(xv);
        v = (double)xv;
        if (mean) v = (v - mean[d]) / scale[d];
      }
      xs[(size_t)r * ldx + d] = v;
    }
    for (int p = 0; p < K; ++p) {
      const int c0 = pl.off[p], S = pl.off[p + 1] - c0, nct = cdiv(S, 16);
      __syncthreads();                               // xs is complete; zs of the previous problem is no longer read
      for (int u = wid; u < nct * MT; u += 4) {
        const int m = u % MT, ct = u / MT;
        const int col = ct * 16 + lr;
        const bool cok = col < S;
        const double* xrow = xs + (size_t)(m * 16 + lr) * ldx;
        const double* th = theta + c0 + (cok ? col : 0);
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < D; k0 += 4) {
          const int k = k0 + lk;
          const bool kok = k < D;
          const double a = kok ? xrow[k] : 0.0;
          const double b = (kok && cok) ? th[(size_t)k * csum] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (cok) {
          const double b0 = th[(size_t)D * csum];
#pragma unroll
          for (int i = 0; i < 4; ++i) zs[(size_t)(m * 16 + lk + 4 * i) * ldz + col] = acc[i] + b0;
        }
      }
      __syncthreads();
      // softmax: one wave per row, lanes over the classes
      for (int r = wid; r < RT; r += 4) {
        const int row = r0 + r;
        if (row >= N) {                              // wave-uniform
          if (GRAD)
            for (int c = lane; c < S; c += 64) zs[(size_t)r * ldz + c] = 0.0;
          continue;
        }
        const int yv = y[(size_t)row * K + p];
        const bool yin = (unsigned)yv < (unsigned)S;
        bad_y |= !yin;
        const bool rok = yin && cvalid[c0 + (yin ? yv : 0)] != 0;
        double* z = zs + (size_t)r * ldz;
        double mx = -INFINITY;
        int am = 0x7fffffff;
        for (int c = lane; c < S; c += 64)
          if (cvalid[c0 + c]) {
            const double v = z[c];
            if (v > mx) mx = v, am = c;              // ascending c per lane: the lane's first maximum
          }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double om = __shfl_xor(mx, o, 64);
          const int oa = __shfl_xor(am, o, 64);
          if (om > mx || (om == mx && oa < am)) mx = om, am = oa;
        }
        double se = 0.0;
        for (int c = lane; c < S; c += 64)
          if (cvalid[c0 + c]) se += exp(z[c] - mx);
        se = wave_sum(se);
        if (!GRAD) {
          if (lane == 0) pred[(size_t)row * K + p] = am == 0x7fffffff ? 0 : am;
          for (int c = lane; c < S; c += 64)
            P[(size_t)row * csum + c0 + c] = (rok && cvalid[c0 + c]) ? exp(z[c] - mx) / se : 0.0;
        } else {
          if (rok && lane == 0) {
            fs[wid * kSegMaxK + p] += (mx + log(se)) - z[yv];
            cs[wid * kSegMaxK + p] += 1;
          }
          for (int c = lane; c < S; c += 64) {
            double g = 0.0;
            if (rok && cvalid[c0 + c]) g = exp(z[c] - mx) / se - (c == yv ? 1.0 : 0.0);
            z[c] = g;
          }
        }
      }
      if (!GRAD) continue;
      __syncthreads();
      const int ndt = cdiv(D + 1, 16);
      for (int u = wid; u < ndt * nct; u += 4) {
        const int dt = u % ndt, ct = u / ndt;
        const int da = dt * 16 + lr, col = ct * 16 + lr;
        const bool cok = col < S;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < RT / 4; ++s) {
          const int k = 4 * s + lk;                  // row of the tile
          const double a = da < D ? xs[(size_t)k * ldx + da] : (da == D ? 1.0 : 0.0);
          const double b = cok ? zs[(size_t)k * ldz + col] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (cok) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int d = dt * 16 + lk + 4 * i;
            if (d <= D) {
              double* q = mypart + (size_t)d * csum + c0 + col;
              *q = it == 0 ? acc[i] : *q + acc[i];
            }
          }
        }
      }
    }
  }
  if (bad_x) atomicOr(&flags[0], 1);
  if (bad_y) atomicOr(&flags[1], 1);
  if (GRAD) {
    __syncthreads();
    if (tid < K) {
      fpart[(size_t)blockIdx.x * K + tid] = ((fs[tid] + fs[kSegMaxK + tid]) + fs[2 * kSegMaxK + tid]) + fs[3 * kSegMaxK + tid];
      cnt[(size_t)blockIdx.x * K + tid] = cs[tid] + cs[kSegMaxK + tid] + cs[2 * kSegMaxK + tid] + cs[3 * kSegMaxK + tid];
    }
  }
}

// One block per problem: n = its valid rows, lambda = m / (C n), f = data / n + (lambda / 2) sum_{valid c} |W_c|^2.
// sc[p] = 1 / n (0 for a problem without rows), sc[K + p] = lambda.
__global__ __launch_bounds__(256) void lr_fold_value_kernel(const double* __restrict__ fpart, const int* __restrict__ cnt,
                                                            int nb, int D, SegPlan pl, const int* __restrict__ cvalid,
                                                            const double* __restrict__ theta, double C,
                                                            double* __restrict__ f, double* __restrict__ sc) {
  __shared__ double scratch[4];
  const int p = blockIdx.x, K = pl.K, csum = pl.off[K];
  const int c0 = pl.off[p], S = pl.off[p + 1] - c0;
  double w2 = 0.0;
  for (int e = threadIdx.x; e < D * S; e += 256) {
    const int d = e / S, c = e - d * S;
    if (cvalid[c0 + c]) {
      const double w = theta[(size_t)d * csum + c0 + c];
      w2 += w * w;
    }
  }
  w2 = block_sum(w2, scratch);
  if (threadIdx.x) return;
  long long n = 0;
  for (int b = 0; b < nb; ++b) n += cnt[(size_t)b * K + p];
  const double data = fold_strided(0.0, fpart + p, (size_t)K, nb);
  int nv = 0;
  for (int c = 0; c < S; ++c) nv += cvalid[c0 + c] != 0;
  const double inv = n > 0 ? 1.0 / (double)n : 0.0;
  const double lam = n > 0 ? (nv == 2 ? 2.0 : 1.0) / (C * (double)n) : 0.0;
  f[p] = data * inv + 0.5 * lam * w2;
  sc[p] = inv, sc[K + p] = lam;
}
__global__ __launch_bounds__(256) void lr_fold_grad_kernel(const double* __restrict__ part, int nb, int D, SegPlan pl,
                                                           const int* __restrict__ cvalid, const double* __restrict__ theta,
                                                           const double* __restrict__ sc, double* __restrict__ grad) {
  const int K = pl.K, csum = pl.off[K];
  const size_t gsz = (size_t)(D + 1) * csum;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= gsz) return;
  const int d = (int)(e / csum), c = (int)(e - (size_t)d * csum);
  if (!cvalid[c]) {
    grad[e] = 0.0;
    return;
  }
  int p = 0;
  while (p + 1 < K && c >= pl.off[p + 1]) ++p;
  double g = fold_strided(0.0, part + e, gsz, nb) * sc[p];
  if (d < D) g += sc[K + p] * theta[e];
  grad[e] = g;
}

// ---- one-vs-rest AUC by pair counting ------------------------------------------------------------------------------
// grid (256-row tile of i, problem, slice of j).  Thread i keeps s_i = P[i][y_i] and streams the rows j of its slice through
// LDS; a pair counts when both labels are valid classes and differ.
__global__ __launch_bounds__(kAucRows) void lr_auc_kernel(const double* __restrict__ P, const int* __restrict__ y, int N,
                                                          SegPlan pl, const int* __restrict__ cvalid, int jrows,
                                                          unsigned long long* __restrict__ count2,
                                                          unsigned long long* __restrict__ pos, int* __restrict__ flags) {
  extern __shared__ double tile[];                   // [kAucTj][S], then the labels [kAucTj]
  const int p = blockIdx.y, K = pl.K, csum = pl.off[K];
  const int c0 = pl.off[p], S = pl.off[p + 1] - c0;
  int* yj = reinterpret_cast<int*>(tile + (size_t)kAucTj * S);
  const int tid = threadIdx.x, i = blockIdx.x * kAucRows + tid;
  int ci = -1;
  double si = 0.0;
  if (i < N) {
    const int yv = y[(size_t)i * K + p];
    if ((unsigned)yv >= (unsigned)S) {
      atomicOr(&flags[1], 1);
    } else if (cvalid[c0 + yv]) {
      ci = yv, si = P[(size_t)i * csum + c0 + yv];
    }
  }
  const int j0 = blockIdx.z * jrows, j1 = min(N, j0 + jrows);
  unsigned long long acc = 0;
  for (int jb = j0; jb < j1; jb += kAucTj) {
    const int nj = min(kAucTj, j1 - jb);
    __syncthreads();
    for (int e = tid; e < nj * S; e += kAucRows) {
      const int r = e / S, c = e - r * S;
      tile[e] = P[(size_t)(jb + r) * csum + c0 + c];
    }
    if (tid < nj) {
      const int yv = y[(size_t)(jb + tid) * K + p];
      yj[tid] = ((unsigned)yv < (unsigned)S && cvalid[c0 + yv]) ? yv : -1;
    }
    __syncthreads();
    if (ci >= 0)
      for (int r = 0; r < nj; ++r) {
        const int cj = yj[r];
        if (cj < 0 || cj == ci) continue;
        const double sj = tile[(size_t)r * S + ci];
        acc += si > sj ? 2u : (si == sj ? 1u : 0u);
      }
  }
  if (ci >= 0) {
    if (acc) atomicAdd(&count2[c0 + ci], acc);
    if (blockIdx.z == 0) atomicAdd(&pos[c0 + ci], 1ull);
  }
}
// neg[c] = (valid rows of the problem) - pos[c] for a valid class, 0 otherwise
__global__ __launch_bounds__(256) void lr_auc_neg_kernel(SegPlan pl, const int* __restrict__ cvalid,
                                                         const unsigned long long* __restrict__ pos,
                                                         unsigned long long* __restrict__ neg) {
  const int p = blockIdx.x, c0 = pl.off[p], S = pl.off[p + 1] - c0;
  unsigned long long n = 0;
  for (int c = 0; c < S; ++c) n += pos[c0 + c];
  for (int c = threadIdx.x; c < S; c += 256) neg[c0 + c] = cvalid[c0 + c] ? n - pos[c0 + c] : 0ull;
}

// ---- z_diff --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lr_zdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t ld,
                                                       int B, int D, float* __restrict__ out) {
  __shared__ double sm[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  double s = 0.0;
  if (d < D)
    for (int r = wid; r < B; r += 4) s += fabs((double)a[(size_t)r * ld + d] - (double)b[(size_t)r * ld + d]);
  sm[wid][lane] = s;
  __syncthreads();
  if (wid == 0 && d < D) out[d] = (float)((((sm[0][lane] + sm[1][lane]) + sm[2][lane]) + sm[3][lane]) / (double)B);
}

// ---- host side -----------------------------------------------------------------------------------------------------
static int lr_plan(const char* name, int N, int D, int K, const int* csize, SegPlan* pl, int* segmax) {
  const SegWords words = {"K = %lld problems", "no class counts", "problem %lld has %lld classes"};
  if (need_dim(name, "N = %lld", N, 1, kLrMaxN, "1..2^30") || need_dim(name, "D = %lld", D, 1, kLrMaxD, "1..512") ||
      seg_plan(name, K, csize, kLrMaxCsize, words, pl))
    return 1;
  *segmax = 0;
  for (int k = 0; k < K; ++k) *segmax = csize[k] > *segmax ? csize[k] : *segmax;
  return 0;
}
static inline size_t lr_lds(int mt, int D, int segmax) {
  return ((size_t)16 * mt * ((D | 1) + (segmax | 1)) + 4 * kSegMaxK) * sizeof(double) + 4 * kSegMaxK * sizeof(int);
}
static inline int lr_mt(int D, int segmax) { return lr_lds(2, D, segmax) <= kLrLdsTwoTiles ? 2 : 1; }
static inline int lr_blocks(int N, int D, int csum, int mt) {
  const size_t gsz = (size_t)(D + 1) * csum * sizeof(double);
  size_t nb = kLrPartBudget / gsz;
  nb = nb > (size_t)kLrMaxBlocks ? kLrMaxBlocks : (nb < 1 ? 1 : nb);
  const int nt = cdiv(N, 16 * mt);
  return nt < (int)nb ? nt : (int)nb;
}
struct LrWs {
  size_t part, fpart, cnt, sc, total;
};
static inline LrWs lr_ws(int nb, int D, int csum, int K) {
  LrWs w;
  w.part = 0;
  w.fpart = w.part + (size_t)nb * (D + 1) * csum * sizeof(double);
  w.sc = w.fpart + (size_t)nb * K * sizeof(double);
  w.cnt = w.sc + (size_t)2 * K * sizeof(double);
  w.total = w.cnt + (size_t)nb * K * sizeof(int);
  return w;
}

template <bool GRAD, typename... Args>
static void lr_launch(int mt, int nb, size_t lds, hipStream_t st, Args... args) {
  if (mt == 2)
    launch_lds<lr_softmax_kernel<2, GRAD>>(dim3(nb), dim3(256), lds, st, args...);
  else
    launch_lds<lr_softmax_kernel<1, GRAD>>(dim3(nb), dim3(256), lds, st, args...);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_logreg_colstats_workspace(int N, int D) {
  if (N < 1 || N > kLrMaxN || D < 1) return 0;
  int rows;
  return (size_t)doubling_slices(N, kLrStatRows, kLrStatMaxSlices, &rows) * D * sizeof(double);
}

int itcv_logreg_colstats(const float* x, size_t ld, int N, int D, double* mean, double* scale, int* flags, void* ws,
                         size_t ws_bytes, void* stream) {
  ITCV_REQUIRE(x && mean && scale && flags && N >= 1 && N <= kLrMaxN && D >= 1 && ld >= (size_t)D, "itcv_logreg_colstats");
  ITCV_REQUIRE(ws && ws_bytes >= itcv_logreg_colstats_workspace(N, D), "itcv_logreg_colstats(workspace)");
  int rows;
  const int ns = doubling_slices(N, kLrStatRows, kLrStatMaxSlices, &rows), nct = cdiv(D, 64);
  double* part = static_cast<double*>(ws);
  hipStream_t st = S(stream);
  for (int mode = 0; mode < 2; ++mode) {
    hipLaunchKernelGGL(lr_colsum_part_kernel, dim3(nct, ns), dim3(256), 0, st, x, ld, N, D, rows,
                       mode ? (const double*)mean : (const double*)nullptr, part, flags);
    ITCV_CHECK_LAUNCH("itcv_logreg_colstats(partials)");
    hipLaunchKernelGGL(lr_colsum_fold_kernel, dim3(cdiv(D, 256)), dim3(256), 0, st, part, ns, D, N, mode,
                       mode ? scale : mean);
    ITCV_CHECK_LAUNCH("itcv_logreg_colstats(fold)");
  }
  return 0;
}

size_t itcv_logreg_workspace(int N, int D, int K, int csum) {
  if (N < 1 || N > kLrMaxN || D < 1 || D > kLrMaxD || K < 1 || K > kSegMaxK || csum < K || csum > K * kLrMaxCsize) return 0;
  // the tile height depends on the largest class count: take the larger of the two possible block counts
  const int nb1 = lr_blocks(N, D, csum, 1), nb2 = lr_blocks(N, D, csum, 2);
  return lr_ws(nb1 > nb2 ? nb1 : nb2, D, csum, K).total;
}

int itcv_logreg_valgrad(const float* x, size_t ld, const double* mean, const double* scale, const int* y, int N, int D,
                        int K, const int* csize, const int* cvalid, const double* theta, double C, double* f,
                        double* grad, int* flags, void* ws, size_t ws_bytes, void* stream) {
  SegPlan pl;
  int segmax;
  if (int e = lr_plan("itcv_logreg_valgrad", N, D, K, csize, &pl, &segmax)) return e;
  ITCV_REQUIRE(x && y && cvalid && theta && f && grad && flags && ld >= (size_t)D && (!mean) == (!scale) && C > 0.0,
               "itcv_logreg_valgrad");
  const int csum = pl.off[K], mt = lr_mt(D, segmax), nb = lr_blocks(N, D, csum, mt);
  const LrWs w = lr_ws(nb, D, csum, K);
  ITCV_REQUIRE(ws && ws_bytes >= w.total, "itcv_logreg_valgrad(workspace)");
  char* base = static_cast<char*>(ws);
  double* part = reinterpret_cast<double*>(base + w.part);
  double* fpart = reinterpret_cast<double*>(base + w.fpart);
  double* sc = reinterpret_cast<double*>(base + w.sc);
  int* cnt = reinterpret_cast<int*>(base + w.cnt);
  hipStream_t st = S(stream);
  lr_launch<true>(mt, nb, lr_lds(mt, D, segmax), st, x, ld, mean, scale, y, N, D, pl, segmax, cvalid, theta, part, fpart,
                  cnt, (double*)nullptr, (int*)nullptr, flags);
  ITCV_CHECK_LAUNCH("itcv_logreg_valgrad");
  hipLaunchKernelGGL(lr_fold_value_kernel, dim3(K), dim3(256), 0, st, (const double*)fpart, (const int*)cnt, nb, D, pl,
                     cvalid, theta, C, f, sc);
  ITCV_CHECK_LAUNCH("itcv_logreg_valgrad(value)");
  const size_t gsz = (size_t)(D + 1) * csum;
  hipLaunchKernelGGL(lr_fold_grad_kernel, dim3((unsigned)cdivz(gsz, 256)), dim3(256), 0, st, (const double*)part, nb, D,
                     pl, cvalid, theta, (const double*)sc, grad);
  ITCV_CHECK_LAUNCH("itcv_logreg_valgrad(gradient)");
  return 0;
}

int itcv_logreg_proba(const float* x, size_t ld, const double* mean, const double* scale, const int* y, int N, int D,
                      int K, const int* csize, const int* cvalid, const double* theta, double* P, int* pred, int* flags,
                      void* stream) {
  SegPlan pl;
  int segmax;
  if (int e = lr_plan("itcv_logreg_proba", N, D, K, csize, &pl, &segmax)) return e;
  ITCV_REQUIRE(x && y && cvalid && theta && P && pred && flags && ld >= (size_t)D && (!mean) == (!scale),
               "itcv_logreg_proba");
  const int mt = lr_mt(D, segmax);
  const int nt = cdiv(N, 16 * mt), nb = nt < 4 * kLrMaxBlocks ? nt : 4 * kLrMaxBlocks;
  lr_launch<false>(mt, nb, lr_lds(mt, D, segmax), S(stream), x, ld, mean, scale, y, N, D, pl, segmax, cvalid, theta,
                   (double*)nullptr, (double*)nullptr, (int*)nullptr, P, pred, flags);
  ITCV_CHECK_LAUNCH("itcv_logreg_proba");
  return 0;
}

int itcv_logreg_auc(const double* P, const int* y, int N, int K, const int* csize, const int* cvalid,
                    unsigned long long* count2, unsigned long long* pos, unsigned long long* neg, int* flags,
                    void* stream) {
  SegPlan pl;
  int segmax;
  if (int e = lr_plan("itcv_logreg_auc", N, 1, K, csize, &pl, &segmax)) return e;
  ITCV_REQUIRE(P && y && cvalid && count2 && pos && neg && flags, "itcv_logreg_auc");
  const int csum = pl.off[K];
  hipStream_t st = S(stream);
  if (hipMemsetAsync(count2, 0, (size_t)csum * sizeof(unsigned long long), st) != hipSuccess ||
      hipMemsetAsync(pos, 0, (size_t)csum * sizeof(unsigned long long), st) != hipSuccess)
    return fail("%s: clearing the counts failed", "itcv_logreg_auc");
  const int ni = cdiv(N, kAucRows);
  int js = cdiv(2048, ni * K);                       // enough blocks to fill the device, slices of whole LDS tiles
  js = js < 1 ? 1 : (js > 64 ? 64 : js);
  const int jrows = cdiv(cdiv(N, js), kAucTj) * kAucTj;
  js = cdiv(N, jrows);
  ITCV_REQUIRE(ni >= 1 && ni <= 0x7fffffff && K <= 65535 && js >= 1 && js <= 65535, "itcv_logreg_auc(grid)");
  const size_t lds = (size_t)kAucTj * segmax * sizeof(double) + kAucTj * sizeof(int);
  hipLaunchKernelGGL(lr_auc_kernel, dim3(ni, K, js), dim3(kAucRows), lds, st, P, y, N, pl, cvalid, jrows, count2, pos,
                     flags);
  ITCV_CHECK_LAUNCH("itcv_logreg_auc");
  hipLaunchKernelGGL(lr_auc_neg_kernel, dim3(K), dim3(256), 0, st, pl, cvalid, (const unsigned long long*)pos, neg);
  ITCV_CHECK_LAUNCH("itcv_logreg_auc(neg)");
  return 0;
}

int itcv_zdiff_row(const float* a, const float* b, size_t ld, int B, int D, float* out, void* stream) {
  ITCV_REQUIRE(a && b && out && B >= 1 && B <= kLrMaxN && D >= 1 && ld >= (size_t)D, "itcv_zdiff_row");
  hipLaunchKernelGGL(lr_zdiff_kernel, dim3(cdiv(D, 64)), dim3(256), 0, S(stream), a, b, ld, B, D, out);
  ITCV_CHECK_LAUNCH("itcv_zdiff_row");
  return 0;
}

}  // extern "C"
