// Histogram gradient-boosted trees on the device: the classifier behind the DCI score (evaluation/metrics.py:82-161,
// utils.py:178-241 of the reference, which asks xgboost for tree_method="gpu_hist").  The rule is fixed in
// include/itcv_hip.h; the stages are
//   cuts / bin : per-feature quantile cuts of the sorted training column, then uint8 bins, feature-major [D][N];
//   grad       : margins -> fp64 softmax over the valid classes -> g, h quantised to int64 (2^24 units);
//   hist       : int64 (G, H) tables per (class, node of the level, feature, bin) -- the hot path;
//   split      : prefix-scan every (class, node, feature) row, evaluate the gains, reduce to the best, write the tree;
//   advance    : move every row's node id one level down;   margins: add the leaf values;
//   predict    : first argmax over the valid classes and integer correct-counts;
//   importance : xgboost's `gain` importance from the tree arrays, summed in the order round, class, node.
// Every sum of gradients is an integer sum, so it does not depend on arrival order: LDS atomics and global atomics may
// be used freely and the trees are bitwise reproducible.  The histogram uses the node-id-per-row form: rows
// are never moved, each carries the heap index of the node it sits in (root 0, children of i at 2 i + 1 and 2 i + 2).
#include "dense.h"

namespace itcv {

constexpr int kGbtMaxK = kSegMaxK;                      // the name is part of the wording of the requirements below
constexpr int kGbtMaxCsize = 256;
constexpr int kGbtMaxD = 512;
constexpr int kGbtMaxN = 1 << 30;
constexpr int kGbtMaxDepth = 6;
constexpr int kGbtMaxBin = 256;
constexpr int kGbtNodes = ITCV_GBT_TREE_NODES;          // heap slots of a tree of depth 6
constexpr size_t kGbtTableBudget = ITCV_GBT_TABLE_BUDGET;
constexpr int kGbtHistThreads = 512;
constexpr int kGbtHistRows = 8192;                      // rows per histogram block: amortises clearing and flushing the table
constexpr size_t kGbtHistLds = 64 * 1024;               // two blocks per CU while a level's nodes allow it
constexpr int kGbtHistMaxTf = 32;                       // features per block at the shallow levels
constexpr double kGbtQ = 16777216.0;                    // 2^24
constexpr long long kGbtOneQ = 1LL << 24;               // min_child_weight = 1 in table units
constexpr double kGbtMinGain = 1e-6;

// ---- (a) cuts and bins -----------------------------------------------------------------------------------------------
// One thread per feature: candidates s[(j * N) / B], j = 1..B-1, keep the distinct values above s[0].
__global__ __launch_bounds__(64) void gbt_cuts_kernel(const float* __restrict__ sorted, int N, int D, int B,
                                                      float* __restrict__ cuts, int* __restrict__ nbins) {
  const int d = blockIdx.x * 64 + threadIdx.x;
  if (d >= D) return;
  const float* s = sorted + (size_t)d * N;
  float* out = cuts + (size_t)d * (B - 1);
  const float s0 = s[0];
  float last = s0;
  int n = 0;
  for (int j = 1; j < B; ++j) {
    const float v = s[(size_t)(((long long)j * N) / B)];
    if (v > s0 && v != last) out[n++] = v, last = v;
  }
  nbins[d] = n + 1;
}

// grid (row block, feature): bin(x) = #{cuts <= x}, an upper bound by binary search over the feature's cuts in LDS
__global__ __launch_bounds__(256) void gbt_bin_kernel(const float* __restrict__ x, size_t ld, int N, int B,
                                                      const float* __restrict__ cuts, const int* __restrict__ nbins,
                                                      uint8_t* __restrict__ bins, int* __restrict__ flags) {
  __shared__ float sc[kGbtMaxBin];
  const int d = blockIdx.y;
  int nc = nbins[d] - 1;
  nc = nc < 0 ? 0 : (nc > B - 1 ? B - 1 : nc);
  for (int i = threadIdx.x; i < nc; i += 256) sc[i] = cuts[(size_t)d * (B - 1) + i];
  __syncthreads();
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float v = x[(size_t)n * ld + d];
  int lo = 0, hi = nc;                                    // first cut > v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sc[mid] <= v) lo = mid + 1; else hi = mid;
  }
  if (!finite_f(v)) {
    atomicOr(&flags[0], 1);
    lo = 0;
  }
  bins[(size_t)d * N + n] = (uint8_t)lo;
}

// ---- (b) gradients ---------------------------------------------------------------------------------------------------
// One thread per (row, problem); the margins are class-major [csum][N], so a wave reads consecutive rows of one class.
__global__ __launch_bounds__(256) void gbt_grad_kernel(const double* __restrict__ F, const int* __restrict__ y, int N,
                                                       SegPlan pl, const int* __restrict__ cvalid,
                                                       long long* __restrict__ gq, long long* __restrict__ hq,
                                                       double* __restrict__ gout, double* __restrict__ hout,
                                                       int* __restrict__ flags) {
#pragma clang fp contract(off)
  const int n = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (n >= N) return;
  const int c0 = pl.off[k], cs = pl.off[k + 1] - c0;
  const int lab = y[(size_t)n * pl.K + k];
  const bool inrange = (unsigned)lab < (unsigned)cs;
  if (!inrange) atomicOr(&flags[1], 1);
  const bool rowvalid = inrange && cvalid[c0 + (inrange ? lab : 0)] != 0;
  double m = -INFINITY;
  for (int c = 0; c < cs; ++c)
    if (cvalid[c0 + c]) m = fmax(m, F[(size_t)(c0 + c) * N + n]);
  double s = 0.0;
  for (int c = 0; c < cs; ++c)
    if (cvalid[c0 + c]) s += exp(F[(size_t)(c0 + c) * N + n] - m);
  for (int c = 0; c < cs; ++c) {
    const size_t e = (size_t)(c0 + c) * N + n;
    double g = 0.0, h = 0.0;
    if (rowvalid && cvalid[c0 + c]) {
      const double p = exp(F[e] - m) / s;
      g = p - (lab == c ? 1.0 : 0.0);
      h = fmax((2.0 * p) * (1.0 - p), 1e-16);
    }
    gq[e] = llrint(g * kGbtQ), hq[e] = llrint(h * kGbtQ);
    if (gout) gout[e] = g, hout[e] = h;
  }
}

// ---- (c) histograms: the hot path ------------------------------------------------------------------------------------
// grid (row slice, feature tile, class of the chunk).  A thread owns a row: it reads the row's node id and (gq, hq)
// once and walks the tile's features, so a wave reads 64 consecutive rows of one feature (64 B of the feature-major bin
// matrix) per step.  The block's table [node][feature of the tile][bin][G, H] lives in LDS as 64-bit integers
// (ds_add_u64); the non-zero words are flushed with 64-bit global atomics.  Integer adds commute, so neither the LDS
// nor the global arrival order shows in the result.
__global__ __launch_bounds__(kGbtHistThreads) void gbt_hist_kernel(
    const uint8_t* __restrict__ bins, int N, int D, int B, const long long* __restrict__ gq,
    const long long* __restrict__ hq, const uint8_t* __restrict__ node, const int* __restrict__ cvalid, int c0,
    int level, int tf, unsigned long long* __restrict__ tab) {
  extern __shared__ unsigned long long lt[];              // [nn][tf][B][2]
  const int c = c0 + blockIdx.z;
  if (!cvalid[c]) return;                                 // block-uniform
  const int tid = threadIdx.x;
  const int nn = 1 << level, base = nn - 1;
  const int d0 = blockIdx.y * tf, nf = min(tf, D - d0);
  const int words = nn * tf * B * 2;
  for (int e = tid; e < words; e += kGbtHistThreads) lt[e] = 0ull;
  __syncthreads();
  const int r_end = min(N, (int)min((long long)N, ((long long)blockIdx.x + 1) * kGbtHistRows));
  const size_t row0 = (size_t)c * N;
  for (int r = blockIdx.x * kGbtHistRows + tid; r < r_end; r += kGbtHistThreads) {
    const int nid = (int)node[row0 + r] - base;
    if ((unsigned)nid >= (unsigned)nn) continue;          // the row sits in a leaf above this level
    const unsigned long long g = (unsigned long long)gq[row0 + r], h = (unsigned long long)hq[row0 + r];
    unsigned long long* mine = lt + (size_t)nid * tf * B * 2;
#pragma unroll 4
    for (int f = 0; f < nf; ++f) {
      const int b = bins[(size_t)(d0 + f) * N + r];
      if (b >= B) continue;                               // never index with such a value
      unsigned long long* w = mine + ((size_t)f * B + b) * 2;
      atomicAdd(w, g);
      atomicAdd(w + 1, h);
    }
  }
  __syncthreads();
  unsigned long long* out = tab + (size_t)blockIdx.z * nn * D * B * 2;
  for (int e = tid; e < words; e += kGbtHistThreads) {
    const unsigned long long v = lt[e];
    if (!v) continue;
    int t = e >> 1;
    const int b = t % B;
    t /= B;
    const int f = t % tf, nid = t / tf;
    if (f < nf) atomicAdd(&out[(((size_t)nid * D + d0 + f) * B + b) * 2 + (e & 1)], v);
  }
}

// ---- (d) splits --------------------------------------------------------------------------------------------------------
// The rule's arithmetic, each operation rounded on its own.
__device__ __forceinline__ double gbt_score(long long Gq, long long Hq, double lam) {
#pragma clang fp contract(off)
  const double G = (double)Gq * (1.0 / kGbtQ), H = (double)Hq * (1.0 / kGbtQ);
  const double num = G * G, den = H + lam;
  return num / den;
}
__device__ __forceinline__ double gbt_gain(double sl, double sr, double sp) {
#pragma clang fp contract(off)
  const double a = sl + sr;
  const double b = a - sp;
  return 0.5 * b;
}
__device__ __forceinline__ double gbt_leaf(long long Gq, long long Hq, double lam, double eta) {
#pragma clang fp contract(off)
  const double G = (double)Gq * (1.0 / kGbtQ), H = (double)Hq * (1.0 / kGbtQ);
  const double den = H + lam;
  const double q = (-G) / den;
  return q * eta;
}

struct GbtBest {
  double gain;
  int key;                  // d * 256 + b: the tie rule is "smallest key"
  long long gl, hl;
};
__device__ __forceinline__ bool gbt_better(double g, int key, const GbtBest& b) {
  return g > b.gain || (g == b.gain && key < b.key);
}

// grid (node of the level, class of the chunk), 4 waves.  A wave takes a feature at a time: lanes hold 64 consecutive
// bins, an inclusive wave scan of the int64 pairs gives (GL, HL) of every candidate, the carry moves to the next 64.
__global__ __launch_bounds__(256) void gbt_split_kernel(const long long* __restrict__ tab, const int* __restrict__ nbins,
                                                        int D, int B, const int* __restrict__ cvalid, int c0, int level,
                                                        double lam, double eta, long long* __restrict__ nsum,
                                                        int* __restrict__ tfeat, int* __restrict__ tbin,
                                                        double* __restrict__ tvalue, double* __restrict__ tgain) {
  __shared__ long long sp[2];
  __shared__ GbtBest sb[4];
  const int c = c0 + blockIdx.y;
  if (!cvalid[c]) return;
  const int nn = 1 << level, nid = nn - 1 + blockIdx.x;
  const size_t tn = (size_t)c * kGbtNodes;
  if (level > 0 && tfeat[tn + (nid - 1) / 2] < 0) return;  // the parent is a leaf: this node does not exist
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const long long* t = tab + ((size_t)blockIdx.y * nn + blockIdx.x) * D * B * 2;
  if (level == 0) {                                        // the root's sums: every row has one bin of feature 0
    if (wid == 0) {
      long long g = 0, h = 0;
      const int nb = min(nbins[0], B);
      for (int b = lane; b < nb; b += 64) g += t[(size_t)b * 2], h += t[(size_t)b * 2 + 1];
      g = wave_sum(g), h = wave_sum(h);
      if (lane == 0) sp[0] = g, sp[1] = h;
    }
  } else if (threadIdx.x == 0) {
    sp[0] = nsum[(tn + nid) * 2], sp[1] = nsum[(tn + nid) * 2 + 1];
  }
  __syncthreads();
  const long long GP = sp[0], HP = sp[1];
  const double scp = gbt_score(GP, HP, lam);
  GbtBest best{-INFINITY, 0x7fffffff, 0, 0};
  for (int d = wid; d < D; d += 4) {
    const int nb = min(nbins[d], B);
    long long cg = 0, ch = 0;
    for (int b0 = 0; b0 < nb - 1; b0 += 64) {
      const int b = b0 + lane;
      long long g = 0, h = 0;
      if (b < nb) {
        const longlong2 v = *reinterpret_cast<const longlong2*>(t + ((size_t)d * B + b) * 2);
        g = v.x, h = v.y;
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const long long ug = __shfl_up(g, o, 64), uh = __shfl_up(h, o, 64);
        if (lane >= o) g += ug, h += uh;
      }
      g += cg, h += ch;
      cg = __shfl(g, 63, 64), ch = __shfl(h, 63, 64);
      const long long hr = HP - h;
      if (b < nb - 1 && h >= kGbtOneQ && hr >= kGbtOneQ) {
        const double gain = gbt_gain(gbt_score(g, h, lam), gbt_score(GP - g, hr, lam), scp);
        const int key = d * 256 + b;
        if (gbt_better(gain, key, best)) best = GbtBest{gain, key, g, h};
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    GbtBest u;
    u.gain = __shfl_xor(best.gain, o, 64), u.key = __shfl_xor(best.key, o, 64);
    u.gl = __shfl_xor(best.gl, o, 64), u.hl = __shfl_xor(best.hl, o, 64);
    if (gbt_better(u.gain, u.key, best)) best = u;
  }
  if (lane == 0) sb[wid] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    GbtBest w = sb[0];
    for (int i = 1; i < 4; ++i)
      if (gbt_better(sb[i].gain, sb[i].key, w)) w = sb[i];
    if (level == 0) {
      nsum[tn * 2] = GP, nsum[tn * 2 + 1] = HP;
      tvalue[tn] = gbt_leaf(GP, HP, lam, eta);
    }
    if (w.key != 0x7fffffff && w.gain > kGbtMinGain) {
      tfeat[tn + nid] = w.key >> 8, tbin[tn + nid] = w.key & 255, tgain[tn + nid] = w.gain;
      const int l = 2 * nid + 1;
      nsum[(tn + l) * 2] = w.gl, nsum[(tn + l) * 2 + 1] = w.hl;
      nsum[(tn + l + 1) * 2] = GP - w.gl, nsum[(tn + l + 1) * 2 + 1] = HP - w.hl;
      tvalue[tn + l] = gbt_leaf(w.gl, w.hl, lam, eta);
      tvalue[tn + l + 1] = gbt_leaf(GP - w.gl, HP - w.hl, lam, eta);
    }
  }
}

// ---- (e) node ids and margins ----------------------------------------------------------------------------------------
// grid (row block, class)
__global__ __launch_bounds__(256) void gbt_advance_kernel(const uint8_t* __restrict__ bins, int N,
                                                          const int* __restrict__ cvalid, const int* __restrict__ tfeat,
                                                          const int* __restrict__ tbin, int level,
                                                          uint8_t* __restrict__ node) {
  const int n = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (n >= N || !cvalid[c]) return;
  const int nn = 1 << level;
  const size_t e = (size_t)c * N + n;
  const int nid = node[e];
  if ((unsigned)(nid - (nn - 1)) >= (unsigned)nn) return;
  const int f = tfeat[(size_t)c * kGbtNodes + nid];
  if (f < 0) return;
  node[e] = (uint8_t)(2 * nid + 1 + (bins[(size_t)f * N + n] > tbin[(size_t)c * kGbtNodes + nid] ? 1 : 0));
}

// F[c][n] += value of the row's leaf: the leaf is node[c][n] where the node ids are at hand (the training rows), else
// the row walks the tree from the root (the test rows).
__global__ __launch_bounds__(256) void gbt_margins_kernel(const uint8_t* __restrict__ bins, int N,
                                                          const int* __restrict__ cvalid,
                                                          const uint8_t* __restrict__ node,
                                                          const int* __restrict__ tfeat, const int* __restrict__ tbin,
                                                          const double* __restrict__ tvalue, int max_depth,
                                                          double* __restrict__ F) {
  const int n = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;
  if (n >= N || !cvalid[c]) return;
  const size_t e = (size_t)c * N + n, tn = (size_t)c * kGbtNodes;
  int nid = 0;
  if (node) {
    nid = node[e];
    nid = nid < kGbtNodes ? nid : 0;
  } else {
    for (int i = 0; i < max_depth; ++i) {
      const int f = tfeat[tn + nid];
      if (f < 0) break;
      nid = 2 * nid + 1 + (bins[(size_t)f * N + n] > tbin[tn + nid] ? 1 : 0);
    }
  }
  F[e] += tvalue[tn + nid];
}

// ---- (f) predictions -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gbt_predict_kernel(const double* __restrict__ F, const int* __restrict__ y, int N,
                                                          SegPlan pl, const int* __restrict__ cvalid,
                                                          int* __restrict__ pred, unsigned long long* __restrict__ correct,
                                                          int* __restrict__ flags) {
  const int n = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  bool hit = false;
  if (n < N) {
    const int c0 = pl.off[k], cs = pl.off[k + 1] - c0;
    int arg = -1;
    double m = 0.0;
    for (int c = 0; c < cs; ++c) {
      if (!cvalid[c0 + c]) continue;
      const double v = F[(size_t)(c0 + c) * N + n];
      if (arg < 0 || v > m) arg = c, m = v;
    }
    const int lab = y[(size_t)n * pl.K + k];
    if ((unsigned)lab >= (unsigned)cs) atomicOr(&flags[1], 1);
    pred[(size_t)n * pl.K + k] = arg;
    hit = arg >= 0 && lab == arg;
  }
  const unsigned long long mask = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&correct[k], (unsigned long long)__popcll(mask));
}

// ---- (g) importances -------------------------------------------------------------------------------------------------
// One block per problem; a thread owns a feature and reads every node of the problem's trees in the order round, class,
// node (all threads read the same word: one broadcast load per wave), so each total is an fp64 sum in that fixed order.
__global__ __launch_bounds__(256) void gbt_importance_kernel(const int* __restrict__ tfeat,
                                                             const double* __restrict__ tgain, int rounds, SegPlan pl,
                                                             int D, double* __restrict__ imp) {
  __shared__ double raw[kGbtMaxD];
  __shared__ double total;
  const int k = blockIdx.x, c0 = pl.off[k], cs = pl.off[k + 1] - c0, csum = pl.off[pl.K];
  for (int d = threadIdx.x; d < D; d += 256) {
    double s = 0.0;
    long long cnt = 0;
    for (int r = 0; r < rounds; ++r) {
      const size_t e0 = ((size_t)r * csum + c0) * kGbtNodes, ne = (size_t)cs * kGbtNodes;
      for (size_t e = 0; e < ne; ++e)
        if (tfeat[e0 + e] == d) s += tgain[e0 + e], ++cnt;
    }
    raw[d] = cnt ? s / (double)cnt : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += raw[d];
    total = s;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) imp[(size_t)k * D + d] = total > 0.0 ? raw[d] / total : 0.0;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int gbt_shape(const char* name, long long N, long long D, long long max_bin, long long min_n = 1) {
  if (N < min_n || N > kGbtMaxN) return fail("%s: N = %lld rows is outside %lld..2^30", name, N, min_n);
  if (D < 1 || D > kGbtMaxD) return fail("%s: D = %lld features is outside 1..512", name, D);
  if (max_bin < 2 || max_bin > kGbtMaxBin) return fail("%s: max_bin = %lld is outside 2..256", name, max_bin);
  return 0;
}
static int gbt_depth(const char* name, long long max_depth) {
  if (max_depth < 1 || max_depth > kGbtMaxDepth) return fail("%s: max_depth = %lld is outside 1..6", name, max_depth);
  return 0;
}
static int gbt_plan(const char* name, int K, const int* csize, SegPlan* pl) {
  const SegWords words = {"K = %lld problems", "csize is NULL", "problem %lld has csize %lld"};
  return seg_plan(name, K, csize, kGbtMaxCsize, words, pl);
}
static inline size_t gbt_class_bytes(int D, int max_depth, int max_bin) {
  return ((size_t)1 << (max_depth - 1)) * D * max_bin * 2 * sizeof(long long);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_gbt_workspace(int N, int D, int K, int csum, int max_depth, int max_bin) {
  if (gbt_shape("itcv_gbt_workspace", N, D, max_bin, 2) || gbt_depth("itcv_gbt_workspace", max_depth)) return 0;
  if (K < 1 || K > kGbtMaxK || csum < K || csum > K * kGbtMaxCsize) return 0;
  const size_t per = gbt_class_bytes(D, max_depth, max_bin);
  size_t chunk = kGbtTableBudget / per;
  chunk = chunk < 1 ? 1 : (chunk > (size_t)csum ? (size_t)csum : chunk);
  return chunk * per;
}

int itcv_gbt_cuts(const float* sorted, int N, int D, int max_bin, float* cuts, int* nbins, void* stream) {
  if (int e = gbt_shape("itcv_gbt_cuts", N, D, max_bin, 2)) return e;
  ITCV_REQUIRE(sorted && cuts && nbins, "itcv_gbt_cuts");
  hipLaunchKernelGGL(gbt_cuts_kernel, dim3(cdiv(D, 64)), dim3(64), 0, S(stream), sorted, N, D, max_bin, cuts, nbins);
  ITCV_CHECK_LAUNCH("itcv_gbt_cuts");
  return 0;
}

int itcv_gbt_bin(const float* x, size_t ld, int N, int D, int max_bin, const float* cuts, const int* nbins,
                 unsigned char* bins, int* flags, void* stream) {
  if (int e = gbt_shape("itcv_gbt_bin", N, D, max_bin)) return e;
  ITCV_REQUIRE(x && cuts && nbins && bins && flags && ld >= (size_t)D, "itcv_gbt_bin");
  hipLaunchKernelGGL(gbt_bin_kernel, dim3(cdiv(N, 256), D), dim3(256), 0, S(stream), x, ld, N, max_bin, cuts, nbins, bins,
                     flags);
  ITCV_CHECK_LAUNCH("itcv_gbt_bin");
  return 0;
}

int itcv_gbt_grad(const double* F, const int* y, int N, int K, const int* csize, const int* cvalid, long long* gq,
                  long long* hq, double* g, double* h, int* flags, void* stream) {
  SegPlan pl;
  if (int e = gbt_plan("itcv_gbt_grad", K, csize, &pl)) return e;
  ITCV_REQUIRE(F && y && cvalid && gq && hq && flags && N >= 1 && N <= kGbtMaxN && (!g) == (!h), "itcv_gbt_grad");
  hipLaunchKernelGGL(gbt_grad_kernel, dim3(cdiv(N, 256), K), dim3(256), 0, S(stream), F, y, N, pl, cvalid, gq, hq, g, h,
                     flags);
  ITCV_CHECK_LAUNCH("itcv_gbt_grad");
  return 0;
}

int itcv_gbt_hist(const unsigned char* bins, int N, int D, int max_bin, const long long* gq, const long long* hq,
                  const unsigned char* node, const int* cvalid, int c0, int nc, int level, long long* tab,
                  size_t tab_bytes, void* stream) {
  if (int e = gbt_shape("itcv_gbt_hist", N, D, max_bin)) return e;
  if (level < 0 || level >= kGbtMaxDepth) return fail("%s: level = %lld is outside 0..5", "itcv_gbt_hist", level);
  ITCV_REQUIRE(bins && gq && hq && node && cvalid && tab && c0 >= 0 && nc >= 1 && nc <= kGbtMaxK * kGbtMaxCsize,
               "itcv_gbt_hist");
  const int nn = 1 << level;
  const size_t bytes = (size_t)nc * nn * D * max_bin * 2 * sizeof(long long);
  ITCV_REQUIRE(tab_bytes >= bytes, "itcv_gbt_hist(table)");
  const size_t per_feat = (size_t)nn * max_bin * 2 * sizeof(long long);
  int tf = (int)(kGbtHistLds / per_feat);
  tf = tf < 1 ? 1 : (tf > kGbtHistMaxTf ? kGbtHistMaxTf : tf);
  tf = tf > D ? D : tf;
  const size_t lds = per_feat * tf;                        // <= 128 KiB: 32 nodes x 256 bins x 16 B for one feature
  hipStream_t st = S(stream);
  if (hipMemsetAsync(tab, 0, bytes, st) != hipSuccess) return fail("%s: clearing the table failed", "itcv_gbt_hist");
  launch_lds<gbt_hist_kernel>(dim3(cdiv(N, kGbtHistRows), cdiv(D, tf), nc), dim3(kGbtHistThreads), lds, st, bins, N, D,
                              max_bin, gq, hq, node, cvalid, c0, level, tf, reinterpret_cast<unsigned long long*>(tab));
  ITCV_CHECK_LAUNCH("itcv_gbt_hist");
  return 0;
}

int itcv_gbt_split(const long long* tab, const int* nbins, int D, int max_bin, const int* cvalid, int c0, int nc,
                   int level, double lam, double eta, long long* nsum, int* tfeat, int* tbin, double* tvalue,
                   double* tgain, void* stream) {
  if (int e = gbt_shape("itcv_gbt_split", 2, D, max_bin)) return e;
  if (level < 0 || level >= kGbtMaxDepth) return fail("%s: level = %lld is outside 0..5", "itcv_gbt_split", level);
  ITCV_REQUIRE(tab && nbins && cvalid && nsum && tfeat && tbin && tvalue && tgain && c0 >= 0 && nc >= 1 &&
                   nc <= kGbtMaxK * kGbtMaxCsize && lam >= 0.0,
               "itcv_gbt_split");
  hipLaunchKernelGGL(gbt_split_kernel, dim3(1 << level, nc), dim3(256), 0, S(stream), tab, nbins, D, max_bin, cvalid, c0,
                     level, lam, eta, nsum, tfeat, tbin, tvalue, tgain);
  ITCV_CHECK_LAUNCH("itcv_gbt_split");
  return 0;
}

int itcv_gbt_advance(const unsigned char* bins, int N, int csum, const int* cvalid, const int* tfeat, const int* tbin,
                     int level, unsigned char* node, void* stream) {
  ITCV_REQUIRE(bins && cvalid && tfeat && tbin && node && N >= 1 && N <= kGbtMaxN && csum >= 1 &&
                   csum <= kGbtMaxK * kGbtMaxCsize && level >= 0 && level < kGbtMaxDepth,
               "itcv_gbt_advance");
  hipLaunchKernelGGL(gbt_advance_kernel, dim3(cdiv(N, 256), csum), dim3(256), 0, S(stream), bins, N, cvalid, tfeat, tbin,
                     level, node);
  ITCV_CHECK_LAUNCH("itcv_gbt_advance");
  return 0;
}

int itcv_gbt_margins(const unsigned char* bins, int N, int csum, const int* cvalid, const unsigned char* node,
                     const int* tfeat, const int* tbin, const double* tvalue, int max_depth, double* F, void* stream) {
  if (int e = gbt_depth("itcv_gbt_margins", max_depth)) return e;
  ITCV_REQUIRE(bins && cvalid && tfeat && tbin && tvalue && F && N >= 1 && N <= kGbtMaxN && csum >= 1 &&
                   csum <= kGbtMaxK * kGbtMaxCsize,
               "itcv_gbt_margins");
  hipLaunchKernelGGL(gbt_margins_kernel, dim3(cdiv(N, 256), csum), dim3(256), 0, S(stream), bins, N, cvalid, node, tfeat,
                     tbin, tvalue, max_depth, F);
  ITCV_CHECK_LAUNCH("itcv_gbt_margins");
  return 0;
}

int itcv_gbt_predict(const double* F, const int* y, int N, int K, const int* csize, const int* cvalid, int* pred,
                     unsigned long long* correct, int* flags, void* stream) {
  SegPlan pl;
  if (int e = gbt_plan("itcv_gbt_predict", K, csize, &pl)) return e;
  ITCV_REQUIRE(F && y && cvalid && pred && correct && flags && N >= 1 && N <= kGbtMaxN, "itcv_gbt_predict");
  hipStream_t st = S(stream);
  if (hipMemsetAsync(correct, 0, (size_t)K * sizeof(unsigned long long), st) != hipSuccess)
    return fail("%s: clearing the counts failed", "itcv_gbt_predict");
  hipLaunchKernelGGL(gbt_predict_kernel, dim3(cdiv(N, 256), K), dim3(256), 0, st, F, y, N, pl, cvalid, pred, correct,
                     flags);
  ITCV_CHECK_LAUNCH("itcv_gbt_predict");
  return 0;
}

int itcv_gbt_importance(const int* tfeat, const double* tgain, int rounds, int K, const int* csize, int D, double* imp,
                        void* stream) {
  SegPlan pl;
  if (int e = gbt_plan("itcv_gbt_importance", K, csize, &pl)) return e;
  if (D < 1 || D > kGbtMaxD) return fail("%s: D = %lld features is outside 1..512", "itcv_gbt_importance", D);
  if (rounds < 1) return fail("%s: rounds = %lld is below 1", "itcv_gbt_importance", rounds);
  ITCV_REQUIRE(tfeat && tgain && imp, "itcv_gbt_importance");
  hipLaunchKernelGGL(gbt_importance_kernel, dim3(K), dim3(256), 0, S(stream), tfeat, tgain, rounds, pl, D, imp);
  ITCV_CHECK_LAUNCH("itcv_gbt_importance");
  return 0;
}

// One boosting round as a fixed launch sequence: gradients, then per level (histogram, split) per class chunk and one
// advance, then the margins of the training rows (by node id) and of the test rows (by walking the new trees).
int itcv_gbt_round(const unsigned char* bins, int N, int D, int max_bin, const int* nbins, const int* y, int K,
                   const int* csize, const int* cvalid, double* F, const unsigned char* bins_test, int Nt, double* Ft,
                   int max_depth, double lam, double eta, long long* gq, long long* hq, unsigned char* node,
                   long long* nsum, long long* tab, size_t tab_bytes, int* tfeat, int* tbin, double* tvalue,
                   double* tgain, int* flags, void* stream) {
  const char* name = "itcv_gbt_round";
  if (int e = gbt_shape(name, N, D, max_bin, 2)) return e;
  if (int e = gbt_depth(name, max_depth)) return e;
  SegPlan pl;
  if (int e = gbt_plan(name, K, csize, &pl)) return e;
  const int csum = pl.off[K];
  ITCV_REQUIRE(bins && nbins && y && cvalid && F && gq && hq && node && nsum && tab && tfeat && tbin && tvalue && tgain &&
                   flags && Nt >= 0 && Nt <= kGbtMaxN && (Nt == 0 || (bins_test && Ft)) && lam >= 0.0,
               name);
  const size_t per = gbt_class_bytes(D, max_depth, max_bin);
  ITCV_REQUIRE(tab_bytes >= per, "itcv_gbt_round(table)");
  size_t chunk = tab_bytes / per;
  chunk = chunk > (size_t)csum ? (size_t)csum : chunk;
  hipStream_t st = S(stream);
  if (int e = itcv_gbt_grad(F, y, N, K, csize, cvalid, gq, hq, nullptr, nullptr, flags, stream)) return e;
  if (hipMemsetAsync(node, 0, (size_t)csum * N, st) != hipSuccess) return fail("%s: clearing the node ids failed", name);
  for (int level = 0; level < max_depth; ++level) {
    for (int c0 = 0; c0 < csum; c0 += (int)chunk) {
      const int nc = csum - c0 < (int)chunk ? csum - c0 : (int)chunk;
      if (int e = itcv_gbt_hist(bins, N, D, max_bin, gq, hq, node, cvalid, c0, nc, level, tab, tab_bytes, stream)) return e;
      if (int e = itcv_gbt_split(tab, nbins, D, max_bin, cvalid, c0, nc, level, lam, eta, nsum, tfeat, tbin, tvalue, tgain,
                                 stream))
        return e;
    }
    if (int e = itcv_gbt_advance(bins, N, csum, cvalid, tfeat, tbin, level, node, stream)) return e;
  }
  if (int e = itcv_gbt_margins(bins, N, csum, cvalid, node, tfeat, tbin, tvalue, max_depth, F, stream)) return e;
  if (Nt > 0)
    if (int e = itcv_gbt_margins(bins_test, Nt, csum, cvalid, nullptr, tfeat, tbin, tvalue, max_depth, Ft, stream)) return e;
  return 0;
}

}  // extern "C"
