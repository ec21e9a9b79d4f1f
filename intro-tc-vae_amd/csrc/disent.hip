// Disentanglement scores on the device: the arithmetic the reference's evaluation package does with the encoder means
// on the host (evaluation/utils.py:245-273: np.histogram + np.digitize per column, then one sklearn
// mutual_info_score per (latent, factor) pair), as three kernels:
//   minmax : per-column minimum / maximum of mu[N][D] (+ a flag for non-finite elements);
//   hist   : counts[d][k][b][f] = #{n : bin(mu[n][d]) == b + 1, v[n][k] == f} and the factor marginals vcount[k][f];
//   mi     : MI[d][k] and H[k] from the integer tables, in fp64.
// MIG (evaluation/metrics.py:213-219) and modularity (utils.py:323-335) are a handful of fp64 operations on MI and H
// (hipvae/disentangle.py).  The histogram is the only stage with real work: N * D * K integer adds.  They go to an LDS
// table with ds_add_u32 and are flushed with integer global atomics: integer sums do not depend on arrival order, so
// the tables -- and everything computed from them in a fixed order -- are bitwise reproducible.
#include "dense.h"

namespace itcv {

constexpr int kDisMaxBins = 32;
constexpr int kDisMaxFsize = 256;
constexpr int kDisMaxN = 1 << 30;       // row arithmetic is 32-bit: slices are rounded up to whole blocks of rows
constexpr int kMmRows = 256;            // rows of mu per block of the minmax kernel
constexpr int kMmMaxSlices = 1024;
constexpr int kHistRows = 512;          // rows of mu per block of the histogram kernel
constexpr int kHistU = 4;               // rows per thread whose loads are in flight before the first LDS add
// LDS budget of one histogram block: 64 KB is what a kernel gets without opting in, and leaves two blocks on a CU's
// 160 KB.  One factor at the top of the range needs 32 bins * 256 values * 4 B = 32 KB for one column, so every input of
// the supported range has a plan.
constexpr size_t kHistLds = 64 * 1024;

// The binning rule (include/itcv_hip.h): np.histogram's edges lo + j * ((hi - lo) / bins) followed by np.digitize on
// edges[:-1], evaluated in fp64 as numpy evaluates it: quotient, product, sum, each rounded (no fused multiply-add).
struct BinRange {
  double lo, w;
};
__device__ __forceinline__ BinRange bin_range(float mn, float mx, int bins) {
#pragma clang fp contract(off)
  double lo = (double)mn, hi = (double)mx;
  if (lo == hi) lo -= 0.5, hi += 0.5;
  return BinRange{lo, (hi - lo) / (double)bins};
}
__device__ __forceinline__ int bin_of(float xf, BinRange r, int bins) {
#pragma clang fp contract(off)
  const double x = (double)xf;
  int b = 0;
  for (int j = 0; j < bins; ++j) {
    const double step = (double)j * r.w;
    const double edge = r.lo + step;
    b += x >= edge ? 1 : 0;
  }
  return b;   // 1..bins for lo <= x <= hi
}

// ---- (a) per-column min / max --------------------------------------------------------------------------------------
// grid (64-column tile, row slice); lanes run along the contiguous D direction, the four waves take rows 4 apart.
__global__ __launch_bounds__(256) void disent_minmax_part_kernel(const float* __restrict__ mu, size_t ld, int N, int D,
                                                                 int rows, float* __restrict__ pmn,
                                                                 float* __restrict__ pmx, int* __restrict__ flags) {
  __shared__ float smn[4][64], smx[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  float mn = INFINITY, mx = -INFINITY;
  bool bad = false;
  if (d < D) {
    int r = r0 + wid;
    for (; r + 12 < r1; r += 16) {
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = mu[(size_t)(r + 4 * u) * ld + d];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        mn = fminf(mn, x[u]), mx = fmaxf(mx, x[u]);
        bad |= !finite_f(x[u]);
      }
    }
    for (; r < r1; r += 4) {
      const float x = mu[(size_t)r * ld + d];
      mn = fminf(mn, x), mx = fmaxf(mx, x);
      bad |= !finite_f(x);
    }
  }
  smn[wid][lane] = mn, smx[wid][lane] = mx;
  if (bad) atomicOr(&flags[0], 1);
  __syncthreads();
  if (wid == 0 && d < D) {
    pmn[(size_t)blockIdx.y * D + d] = fminf(fminf(smn[0][lane], smn[1][lane]), fminf(smn[2][lane], smn[3][lane]));
    pmx[(size_t)blockIdx.y * D + d] = fmaxf(fmaxf(smx[0][lane], smx[1][lane]), fmaxf(smx[2][lane], smx[3][lane]));
  }
}
__global__ __launch_bounds__(256) void disent_minmax_fold_kernel(const float* __restrict__ pmn,
                                                                 const float* __restrict__ pmx, int ns, int D,
                                                                 float* __restrict__ mn, float* __restrict__ mx) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  float a = INFINITY, b = -INFINITY;
  for (int s = 0; s < ns; ++s) a = fminf(a, pmn[(size_t)s * D + d]), b = fmaxf(b, pmx[(size_t)s * D + d]);
  mn[d] = a, mx[d] = b;
}

// bins[n][d] in 1..bins (utils.py:245-253 on a dense int32 output)
__global__ __launch_bounds__(256) void disent_bins_kernel(const float* __restrict__ mu, size_t ld, int N, int D,
                                                          const float* __restrict__ mn, const float* __restrict__ mx,
                                                          int bins, int* __restrict__ out) {
  const size_t total = (size_t)N * D;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t n = e / D;
    const int d = (int)(e - n * D);
    out[e] = bin_of(mu[n * ld + d], bin_range(mn[d], mx[d], bins), bins);
  }
}

// ---- (b) joint histograms ------------------------------------------------------------------------------------------
// Factors are cut into groups of consecutive factors whose tables fit the LDS budget; a block owns (TC columns) x (a
// slice of kHistRows rows) x (one group).  The table of column d is counts[d][bins * off[k] + b * fsize[k] + f]: the
// group's part of it is one contiguous range, in LDS and in global memory alike.
struct HistPlan : SegPlan {  // K and off[]: the prefix sums of fsize
  int ng;
  int gk[kSegMaxK + 1];     // group g covers factors [gk[g], gk[g + 1])
};

__global__ __launch_bounds__(256) void disent_hist_kernel(const float* __restrict__ mu, size_t ld,
                                                          const int* __restrict__ v, int N, int D,
                                                          const float* __restrict__ mn, const float* __restrict__ mx,
                                                          int bins, HistPlan pl, int tc, int nct,
                                                          unsigned* __restrict__ counts, unsigned* __restrict__ vcount,
                                                          int* __restrict__ flags) {
  extern __shared__ unsigned tab[];                        // [tc][bins * gsum], then the marginals [gsum]
  const int tid = threadIdx.x;
  const int ct = blockIdx.x % nct, sl = blockIdx.x / nct, g = blockIdx.y;
  const int k0 = pl.gk[g], nk = pl.gk[g + 1] - k0;
  const int f0 = pl.off[k0], gsum = pl.off[k0 + nk] - f0;
  const int gw = bins * gsum;                              // words of one column's table
  unsigned* vt = tab + (size_t)tc * gw;
  const bool marg = ct == 0;                               // the column tile that also counts the factor marginals
  for (int e = tid; e < tc * gw + gsum; e += 256) tab[e] = 0u;

  const int c = tid & (tc - 1), rl = tid / tc, rp = 256 / tc;
  const int d = ct * tc + c;
  const bool act = d < D;
  BinRange br{0.0, 0.0};
  if (act) br = bin_range(mn[d], mx[d], bins);
  unsigned* mytab = tab + (size_t)c * gw;
  const int r_end = min(N, (sl + 1) * kHistRows);
  bool bad = false;
  __syncthreads();
  for (int r0 = sl * kHistRows + rl; r0 < r_end; r0 += rp * kHistU) {
    // every load of these kHistU rows is issued before the first LDS add
    float x[kHistU];
    int vv[kHistU][kSegMaxK];
#pragma unroll
    for (int u = 0; u < kHistU; ++u) {
      const int r = r0 + u * rp;
      const bool have = act && r < r_end;
      x[u] = have ? mu[(size_t)r * ld + d] : 0.f;
#pragma unroll
      for (int kk = 0; kk < kSegMaxK; ++kk) vv[u][kk] = (have && kk < nk) ? v[(size_t)r * pl.K + k0 + kk] : 0;
    }
#pragma unroll
    for (int u = 0; u < kHistU; ++u) {
      const int r = r0 + u * rp;
      if (!(act && r < r_end)) continue;
      int b = bin_of(x[u], br, bins) - 1;
      b = b < 0 ? 0 : b;                                   // only a non-finite x gets here: flagged by the minmax pass
#pragma unroll
      for (int kk = 0; kk < kSegMaxK; ++kk) {
        if (kk >= nk) continue;
        const int fo = pl.off[k0 + kk] - f0, fs = pl.off[k0 + kk + 1] - pl.off[k0 + kk];
        const int f = vv[u][kk];
        if ((unsigned)f >= (unsigned)fs) {                 // never index with such a value
          bad = true;
          continue;
        }
        atomicAdd(&mytab[bins * fo + b * fs + f], 1u);
        if (marg && c == 0) atomicAdd(&vt[fo + f], 1u);
      }
    }
  }
  if (bad) atomicOr(&flags[1], 1);
  __syncthreads();
  const size_t T = (size_t)bins * pl.off[pl.K];            // words of one column's full table
  for (int e = tid; e < tc * gw; e += 256) {
    const int cc = e / gw, w = e - cc * gw;
    const unsigned n = tab[e];
    if (n && ct * tc + cc < D) atomicAdd(&counts[(size_t)(ct * tc + cc) * T + (size_t)bins * f0 + w], n);
  }
  if (marg)
    for (int e = tid; e < gsum; e += 256)
      if (vt[e]) atomicAdd(&vcount[f0 + e], vt[e]);
}

// ---- (c) mutual information and entropies --------------------------------------------------------------------------
// One wave per (d, k) pair, then one per factor for H.  Lanes run over the factor values (<= 4 each), row sums live in
// lane b.  sklearn.metrics.mutual_info_score: sum over the non-zero cells of (c/N)(log c - log r_b - log s_f + log N),
// clipped at 0; calculate_entropy is that score of a factor with itself: -sum (s/N) log(s/N).  Fixed orders throughout.
__global__ __launch_bounds__(256) void disent_mi_kernel(const unsigned* __restrict__ counts,
                                                        const unsigned* __restrict__ vcount, int N, int D, int bins,
                                                        HistPlan pl, double* __restrict__ mi, double* __restrict__ h) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), npair = (long long)D * pl.K;
  const double dn = (double)N, logn = log(dn);
  if (p >= npair + pl.K) return;                            // wave-uniform: no block-level barrier below
  if (p >= npair) {
    const int k = (int)(p - npair), fs = pl.off[k + 1] - pl.off[k];
    double a = 0.0;
    for (int f = lane; f < fs; f += 64) {
      const unsigned s = vcount[pl.off[k] + f];
      if (s) {
        const double q = (double)s / dn;
        a += -q * log(q);
      }
    }
    a = wave_sum(a);
    if (lane == 0) h[k] = a;
    return;
  }
  const int d = (int)(p / pl.K), k = (int)(p - (long long)d * pl.K);
  const int fs = pl.off[k + 1] - pl.off[k];
  const unsigned* t = counts + (size_t)d * bins * pl.off[pl.K] + (size_t)bins * pl.off[k];   // [bins][fs]
  constexpr int kFL = kDisMaxFsize / 64;
  unsigned s[kFL];
#pragma unroll
  for (int i = 0; i < kFL; ++i) s[i] = 0u;
  unsigned myr = 0u;
  for (int b = 0; b < bins; ++b) {
    unsigned rs = 0u;
#pragma unroll
    for (int i = 0; i < kFL; ++i) {
      const int f = lane + 64 * i;
      const unsigned cv = f < fs ? t[b * fs + f] : 0u;
      s[i] += cv, rs += cv;
    }
    rs = wave_sum(rs);
    if (lane == b) myr = rs;
  }
  double ls[kFL];
#pragma unroll
  for (int i = 0; i < kFL; ++i) ls[i] = s[i] ? log((double)s[i]) : 0.0;
  double a = 0.0;
  for (int b = 0; b < bins; ++b) {
    const unsigned rb = __shfl(myr, b, 64);
    if (!rb) continue;                                     // wave-uniform
    const double lr = log((double)rb);
#pragma unroll
    for (int i = 0; i < kFL; ++i) {
      const int f = lane + 64 * i;
      const unsigned cv = f < fs ? t[b * fs + f] : 0u;
      if (cv) a += ((double)cv / dn) * (log((double)cv) - lr - ls[i] + logn);
    }
  }
  a = wave_sum(a);
  if (lane == 0) mi[p] = a > 0.0 ? a : 0.0;
}

// Host side of the supported range and the histogram's tiling.  Returns 0 and fills *pl, *tc (columns per block, a power
// of two) and *lds, or fails.
static int hist_plan(const char* name, int D, int K, const int* fsize, int bins, HistPlan* pl, int* tc, size_t* lds) {
  if (bins < 1 || bins > kDisMaxBins) return fail("%s: bins = %lld is outside 1..32", name, bins);
  const SegWords words = {"K = %lld factors", nullptr, "factor %lld has size %lld"};   // the callers require fsize
  if (seg_plan(name, K, fsize, kDisMaxFsize, words, pl)) return 1;
  // greedy groups of consecutive factors: (bins + 1) * gsum words for one column must fit the budget
  const size_t cap = kHistLds / sizeof(unsigned) / (size_t)(bins + 1);
  int ng = 0, gmax = 0;
  pl->gk[0] = 0;
  for (int k = 0, gs = 0; k < K; ++k) {
    if (gs && (size_t)(gs + fsize[k]) > cap) pl->gk[++ng] = k, gs = 0;
    gs += fsize[k];
    gmax = gs > gmax ? gs : gmax;
  }
  pl->gk[++ng] = K;
  pl->ng = ng;
  int t = 64;                                              // shrink the column tile until the largest group fits
  while (t > 1 && (t / 2 >= D || ((size_t)t * bins + 1) * gmax * sizeof(unsigned) > kHistLds)) t /= 2;
  *tc = t;
  *lds = ((size_t)t * bins + 1) * gmax * sizeof(unsigned);
  if (*lds > kHistLds) return fail("%s: internal: the histogram table does not fit LDS", name);
  return 0;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_disent_minmax_workspace(int N, int D) {
  if (N < 1 || N > kDisMaxN || D < 1) return 0;
  int rows;
  return (size_t)2 * doubling_slices(N, kMmRows, kMmMaxSlices, &rows) * D * sizeof(float);
}

int itcv_disent_minmax(const float* mu, size_t ld, int N, int D, float* mn, float* mx, int* flags, void* ws,
                       size_t ws_bytes, void* stream) {
  ITCV_REQUIRE(mu && mn && mx && flags && N >= 1 && N <= kDisMaxN && D >= 1 && ld >= (size_t)D, "itcv_disent_minmax");
  ITCV_REQUIRE(ws && ws_bytes >= itcv_disent_minmax_workspace(N, D), "itcv_disent_minmax(workspace)");
  int rows;
  const int ns = doubling_slices(N, kMmRows, kMmMaxSlices, &rows), nct = cdiv(D, 64);
  float* pmn = static_cast<float*>(ws);
  float* pmx = pmn + (size_t)ns * D;
  hipLaunchKernelGGL(disent_minmax_part_kernel, dim3(nct, ns), dim3(256), 0, S(stream), mu, ld, N, D, rows,
                     ns == 1 ? mn : pmn, ns == 1 ? mx : pmx, flags);
  ITCV_CHECK_LAUNCH("itcv_disent_minmax(partials)");
  if (ns > 1) {
    hipLaunchKernelGGL(disent_minmax_fold_kernel, dim3(cdiv(D, 256)), dim3(256), 0, S(stream), pmn, pmx, ns, D, mn, mx);
    ITCV_CHECK_LAUNCH("itcv_disent_minmax(fold)");
  }
  return 0;
}

int itcv_disent_bins(const float* mu, size_t ld, int N, int D, const float* mn, const float* mx, int bins, int* out,
                     void* stream) {
  ITCV_REQUIRE(mu && mn && mx && out && N >= 1 && N <= kDisMaxN && D >= 1 && ld >= (size_t)D, "itcv_disent_bins");
  if (bins < 1 || bins > kDisMaxBins) return fail("%s: bins = %lld is outside 1..32", "itcv_disent_bins", bins);
  size_t nb = cdivz((size_t)N * D, 256);
  nb = nb > 4096 ? 4096 : nb;
  hipLaunchKernelGGL(disent_bins_kernel, dim3((unsigned)nb), dim3(256), 0, S(stream), mu, ld, N, D, mn, mx, bins, out);
  ITCV_CHECK_LAUNCH("itcv_disent_bins");
  return 0;
}

size_t itcv_disent_counts_elems(int D, int fsum, int bins) {
  return D >= 1 && fsum >= 1 && bins >= 1 ? (size_t)D * bins * fsum : 0;
}

int itcv_disent_hist(const float* mu, size_t ld, const int* v, int N, int D, int K, const int* fsize, int bins,
                     const float* mn, const float* mx, unsigned* counts, unsigned* vcount, int* flags, void* stream) {
  ITCV_REQUIRE(mu && v && fsize && mn && mx && counts && vcount && flags && N >= 1 && N <= kDisMaxN && D >= 1 && ld >= (size_t)D,
               "itcv_disent_hist");
  HistPlan pl;
  int tc;
  size_t lds;
  if (int e = hist_plan("itcv_disent_hist", D, K, fsize, bins, &pl, &tc, &lds)) return e;
  const int nct = cdiv(D, tc), nsl = cdiv(N, kHistRows);
  ITCV_REQUIRE((long long)nct * nsl <= 0x7fffffffLL, "itcv_disent_hist(grid)");
  const int fsum = pl.off[K];
  hipStream_t st = S(stream);
  if (hipMemsetAsync(counts, 0, itcv_disent_counts_elems(D, fsum, bins) * sizeof(unsigned), st) != hipSuccess ||
      hipMemsetAsync(vcount, 0, (size_t)fsum * sizeof(unsigned), st) != hipSuccess)
    return fail("%s: clearing the tables failed", "itcv_disent_hist");
  hipLaunchKernelGGL(disent_hist_kernel, dim3(nct * nsl, pl.ng), dim3(256), lds, st, mu, ld, v, N, D, mn, mx, bins, pl,
                     tc, nct, counts, vcount, flags);
  ITCV_CHECK_LAUNCH("itcv_disent_hist");
  return 0;
}

int itcv_disent_hist_tiling(int D, int K, const int* fsize, int bins, int* out) {
  ITCV_REQUIRE(fsize && out && D >= 1, "itcv_disent_hist_tiling");
  HistPlan pl;
  int tc;
  size_t lds;
  if (int e = hist_plan("itcv_disent_hist_tiling", D, K, fsize, bins, &pl, &tc, &lds)) return e;
  out[0] = tc, out[1] = cdiv(D, tc), out[2] = pl.ng, out[3] = (int)lds;
  for (int g = 0; g <= kSegMaxK; ++g) out[4 + g] = g <= pl.ng ? pl.gk[g] : 0;
  return 0;
}

int itcv_disent_mi(const unsigned* counts, const unsigned* vcount, int N, int D, int K, const int* fsize, int bins,
                   double* mi, double* h, void* stream) {
  ITCV_REQUIRE(counts && vcount && fsize && mi && h && N >= 1 && N <= kDisMaxN && D >= 1, "itcv_disent_mi");
  HistPlan pl;
  int tc;
  size_t lds;
  if (int e = hist_plan("itcv_disent_mi", D, K, fsize, bins, &pl, &tc, &lds)) return e;
  const long long waves = (long long)D * K + K;
  ITCV_REQUIRE(waves <= 4LL * 0x7fffffff, "itcv_disent_mi(grid)");
  hipLaunchKernelGGL(disent_mi_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, S(stream), counts, vcount, N, D,
                     bins, pl, mi, h);
  ITCV_CHECK_LAUNCH("itcv_disent_mi");
  return 0;
}

}  // extern "C"
