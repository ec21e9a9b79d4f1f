// The FactorVAE score (Kim & Mnih 2018) and the SAP score (Kumar et al. 2018) on the device.  The reference has neither;
// both are fixed rules in include/itcv_hip.h, all arithmetic in fp64 on fp32 representations x[N][D] (row stride ld):
//   fvae_gvar     : ddof = 1 variance of every column (two passes: the mean, then the squared deviations);
//   fvae_votes    : one wave per group of L rows: per-dimension ddof = 1 variance, arg-min of lvar / gvar over the active
//                   dimensions, one 64-bit integer atomic into votes[D][K];
//   fvae_classify : the majority-vote classifier and the two accuracies from the integer tables;
//   sap_svc_fit   : every (latent, factor, class) squared-hinge classifier of the SAP matrix, solved to convergence by a
//                   damped Newton iteration inside ONE launch, one wave per problem;
//   sap_svc_score : predictions on the test rows and the integer counts of correct ones.
// Every floating-point reduction has a fixed order (per-lane partials over ascending rows, then the xor butterfly of the
// wave, whose sums are the same bits in every lane because an fp64 add commutes); there is no floating-point atomic.  The
// order of operations is part of the rule: nothing in this file may be contracted into a fused multiply-add.
#include "dense.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kXsMaxCsize = 256;
constexpr int kXsMaxD = 512;
constexpr int kXsMaxN = 1 << 24;          // rows of any one call
constexpr int kXsMaxL = 1 << 16;          // rows of a FactorVAE group
constexpr int kSvcThreads = 512;          // 8 waves: 8 problems of one (latent, factor) pair in flight
constexpr int kSvcLdsRows = 12800;        // 5 bytes a row (fp32 x, uint8 y): 62.5 KiB, two blocks per CU
constexpr int kSvcMaxHalvings = 50;       // step lengths tried per Newton step: 1, 1/2, ..., 2^-50
constexpr double kSvcArmijo = 1e-4;

// ---- FactorVAE: global variances -----------------------------------------------------------------------------------
// One block of 16 waves per tile of 32 columns; a wave covers 2 rows x 32 columns per step (128-byte segments), so lane
// (r = lane >> 5, c = lane & 31) of wave w sums rows 2 w + r, 2 w + r + 32, ... in ascending order.  The 32 row slots of a
// column are folded in slot order.  Pass 1: the mean; pass 2: the squared deviations, divided by N - 1.
__global__ __launch_bounds__(1024) void fvae_gvar_kernel(const float* __restrict__ x, size_t ld, int N, int D,
                                                         double* __restrict__ gvar, int* __restrict__ flags) {
  __shared__ double part[32][33];
  __shared__ double mean_s[32];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int slot = 2 * wid + (lane >> 5), cl = lane & 31;
  const int d = blockIdx.x * 32 + cl;
  bool bad = false;
  for (int pass = 0; pass < 2; ++pass) {
    const double m = pass ? mean_s[cl] : 0.0;
    double s = 0.0;
    if (d < D)
      for (int r = slot; r < N; r += 32) {
        const float v = x[(size_t)r * ld + d];
        bad |= !finite_f(v);
        const double t = (double)v - m;
        s += pass ? t * t : t;
      }
    part[slot][cl] = s;
    __syncthreads();
    if (threadIdx.x < 32) {
      double tot = 0.0;
      for (int k = 0; k < 32; ++k) tot += part[k][threadIdx.x];
      if (pass == 0)
        mean_s[threadIdx.x] = tot / (double)N;
      else if (blockIdx.x * 32 + (int)threadIdx.x < D)
        gvar[blockIdx.x * 32 + threadIdx.x] = tot / (double)(N - 1);
    }
    __syncthreads();
  }
  if (bad) atomicOr(&flags[0], 1);
}

// ---- FactorVAE: the votes ------------------------------------------------------------------------------------------
// A wave per group, 4 groups per block; lanes over the dimensions (a row of the group is read in 256-byte segments).
__global__ __launch_bounds__(256) void fvae_votes_kernel(const float* __restrict__ mu, size_t ld, int M, int L, int D,
                                                         const double* __restrict__ gvar, double threshold,
                                                         const int* __restrict__ fidx, int K,
                                                         unsigned long long* __restrict__ votes,
                                                         int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= M) return;                                  // wave-uniform
  const float* rows = mu + (size_t)g * L * ld;
  double best = INFINITY;
  int arg = 0x7fffffff;
  bool bad = false;
  for (int d = lane; d < D; d += 64) {
    double s = 0.0;
    for (int r = 0; r < L; ++r) {
      const float v = rows[(size_t)r * ld + d];
      bad |= !finite_f(v);
      s += (double)v;
    }
    const double m = s / (double)L;
    double q = 0.0;
    for (int r = 0; r < L; ++r) {
      const double t = (double)rows[(size_t)r * ld + d] - m;
      q += t * t;
    }
    const double gv = gvar[d];
    if (sqrt(gv) >= threshold) {
      const double ratio = (q / (double)(L - 1)) / gv;
      if (ratio < best) best = ratio, arg = d;         // ascending d per lane: the lane's first minimum
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ob < best || (ob == best && oa < arg)) best = ob, arg = oa;
  }
  if (__ballot(bad) && lane == 0) atomicOr(&flags[0], 1);
  if (lane) return;
  const int k = fidx[g];
  if ((unsigned)k >= (unsigned)K) {
    atomicOr(&flags[1], 1);
    return;
  }
  if (arg != 0x7fffffff) atomicAdd(&votes[(size_t)arg * K + k], 1ull);
}

// One block: classifier[d] = first argmax_k votes_train[d][k]; res = {train accuracy, eval accuracy, active dimensions}.
__global__ __launch_bounds__(256) void fvae_classify_kernel(const unsigned long long* __restrict__ vt,
                                                            const unsigned long long* __restrict__ ve, int D, int K, int Mt,
                                                            int Me, const double* __restrict__ gvar, double threshold,
                                                            int* __restrict__ classifier, double* __restrict__ res) {
  __shared__ unsigned long long scratch[4];
  unsigned long long ht = 0, he = 0, na = 0;
  for (int d = threadIdx.x; d < D; d += 256) {
    int am = 0;
    unsigned long long mx = vt[(size_t)d * K];
    for (int k = 1; k < K; ++k) {
      const unsigned long long v = vt[(size_t)d * K + k];
      if (v > mx) mx = v, am = k;
    }
    classifier[d] = am;
    ht += mx;
    he += ve[(size_t)d * K + am];
    na += sqrt(gvar[d]) >= threshold ? 1 : 0;
  }
  ht = block_sum(ht, scratch);
  he = block_sum(he, scratch);
  na = block_sum(na, scratch);
  if (threadIdx.x == 0) {
    res[0] = na ? (double)ht / (double)Mt : 0.0;
    res[1] = na ? (double)he / (double)Me : 0.0;
    res[2] = (double)na;
  }
}

// ---- SAP: feature-major copies and class counts --------------------------------------------------------------------
// grid (64-row tile, 64-column tile): xt[D][N] = x^T through an LDS tile; the blocks of column tile 0 also write the labels
// as yt[K][N] uint8 (255 for a label outside its range, which sets flags[1]) and count the classes with integer atomics.
__global__ __launch_bounds__(256) void svc_prep_kernel(const float* __restrict__ x, size_t ld, const int* __restrict__ y,
                                                       int N, int D, SegPlan pl, float* __restrict__ xt,
                                                       unsigned char* __restrict__ yt, int* __restrict__ counts,
                                                       int* __restrict__ flags) {
  __shared__ float tile[64][65];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  bool bad = false;
  for (int r = wid; r < 64; r += 4) {
    float v = 0.f;
    if (r0 + r < N && c0 + lane < D) {
      v = x[(size_t)(r0 + r) * ld + c0 + lane];
      bad |= !finite_f(v);
    }
    tile[r][lane] = v;
  }
  if (bad) atomicOr(&flags[0], 1);
  __syncthreads();
  for (int c = wid; c < 64; c += 4)
    if (c0 + c < D && r0 + lane < N) xt[(size_t)(c0 + c) * N + r0 + lane] = tile[lane][c];
  if (blockIdx.y) return;
  const int K = pl.K, n = r0 + lane;
  if (n >= N) return;
  for (int k = wid; k < K; k += 4) {
    const int S = pl.off[k + 1] - pl.off[k];
    const int yv = y[(size_t)n * K + k];
    const bool ok = (unsigned)yv < (unsigned)S;
    yt[(size_t)k * N + n] = ok ? (unsigned char)yv : (unsigned char)255;
    if (ok)
      atomicAdd(&counts[pl.off[k] + yv], 1);
    else
      atomicOr(&flags[1], 1);
  }
}

// ---- SAP: the squared-hinge classifiers ----------------------------------------------------------------------------
struct SvcEval {
  double F, gw, gb, hww, hwb, hbb;
};
// F, its gradient and its generalised Hessian at (w, b) for the problem "class c against the rest" with the weights cp
// (rows of class c) and cn (the others); all 64 lanes call and all receive the same bits.
template <typename XP, typename YP>
__device__ __forceinline__ SvcEval svc_eval(XP xs, YP ys, int N, int c, double cp, double cn, double w, double b) {
  const int lane = threadIdx.x & 63;
  double sF = 0.0, sw = 0.0, sb = 0.0, hxx = 0.0, hx = 0.0, h1 = 0.0;
  for (int n = lane; n < N; n += 64) {
    const double x = (double)xs[n];
    const bool pos = (int)ys[n] == c;
    const double t = pos ? 1.0 : -1.0, cw = pos ? cp : cn;
    const double z = w * x + b;
    const double xi = 1.0 - t * z;
    if (xi > 0.0) {
      const double a = cw * xi;
      const double at = a * t, cx = cw * x;
      sF += a * xi;
      sw += at * x;
      sb += at;
      hxx += cx * x;
      hx += cx;
      h1 += cw;
    }
  }
  sF = wave_sum(sF), sw = wave_sum(sw), sb = wave_sum(sb);
  hxx = wave_sum(hxx), hx = wave_sum(hx), h1 = wave_sum(h1);
  SvcEval e;
  e.F = 0.5 * (w * w + b * b) + sF;
  e.gw = w - 2.0 * sw;
  e.gb = b - 2.0 * sb;
  e.hww = 1.0 + 2.0 * hxx;
  e.hwb = 2.0 * hx;
  e.hbb = 1.0 + 2.0 * h1;
  return e;
}

// Damped Newton from (0, 0).  Returns the iteration count; *conv says whether max(|dF/dw|, |dF/db|) <= gtol was reached.
template <typename XP, typename YP>
__device__ __forceinline__ int svc_solve(XP xs, YP ys, int N, int c, double cp, double cn, double gtol, int max_iter,
                                         double* wo, double* bo, double* gn_out, bool* conv) {
  double w = 0.0, b = 0.0;
  SvcEval e = svc_eval(xs, ys, N, c, cp, cn, w, b);
  double gn = fmax(fabs(e.gw), fabs(e.gb));
  int it = 0;
  while (!(gn <= gtol) && it < max_iter) {
    const double det = e.hww * e.hbb - e.hwb * e.hwb;
    const double dw = -((e.hbb * e.gw - e.hwb * e.gb) / det);
    const double db = -((e.hww * e.gb - e.hwb * e.gw) / det);
    const double slope = e.gw * dw + e.gb * db;
    double alpha = 1.0;
    bool accepted = false;
    for (int h = 0; h <= kSvcMaxHalvings; ++h) {
      const double wt = w + alpha * dw, bt = b + alpha * db;
      const SvcEval et = svc_eval(xs, ys, N, c, cp, cn, wt, bt);
      const double gt = fmax(fabs(et.gw), fabs(et.gb));
      // a trial point that already meets the stopping rule is taken as it is: next to the optimum the decrease of F
      // falls below its rounding error and the Armijo test alone could no longer be passed
      if (et.F <= e.F + (kSvcArmijo * alpha) * slope || gt <= gtol) {
        w = wt, b = bt, e = et, gn = gt, accepted = true;
        break;
      }
      alpha *= 0.5;
    }
    if (!accepted) break;
    ++it;
  }
  *wo = w, *bo = b, *gn_out = gn, *conv = gn <= gtol;
  return it;
}

// grid (latent i, factor j), 8 waves.  The column and the labels are staged in LDS (IN_LDS) or read from the feature-major
// copies; the waves then take the problems of the pair in turn: every present class when there are 3 or more, the larger
// class value alone when there are 2, none when there is 1.
template <bool IN_LDS>
__global__ __launch_bounds__(kSvcThreads) void svc_fit_kernel(const float* __restrict__ xt, const unsigned char* __restrict__ yt,
                                                              const int* __restrict__ counts, int N, int D, SegPlan pl,
                                                              double C, double gtol, int max_iter,
                                                              double* __restrict__ theta, double* __restrict__ gnorm,
                                                              int* __restrict__ iters, int* __restrict__ cvalid,
                                                              int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char svc_lds[];
  const int i = blockIdx.x, j = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int K = pl.K, csum = pl.off[K], c0 = pl.off[j], S = pl.off[j + 1] - c0;
  const float* xg = xt + (size_t)i * N;
  const unsigned char* yg = yt + (size_t)j * N;
  float* xs = reinterpret_cast<float*>(svc_lds);
  unsigned char* ys = svc_lds + (size_t)(IN_LDS ? N : 0) * sizeof(float);
  if (IN_LDS) {
    for (int n = threadIdx.x; n < N; n += kSvcThreads) xs[n] = xg[n], ys[n] = yg[n];
    __syncthreads();
  }
  int nv = 0, first = -1, last = -1;
  for (int c = 0; c < S; ++c)
    if (counts[c0 + c] > 0) {
      if (first < 0) first = c;
      last = c, ++nv;
    }
  const size_t base = (size_t)i * csum + c0;
  // slots without a problem of their own
  for (int c = threadIdx.x; c < S; c += kSvcThreads) {
    if (i == 0) cvalid[c0 + c] = counts[c0 + c] > 0;
    const bool solved = counts[c0 + c] > 0 && (nv >= 3 || (nv == 2 && c == last));
    if (!solved) theta[(base + c) * 2] = 0.0, theta[(base + c) * 2 + 1] = 0.0, gnorm[base + c] = 0.0, iters[base + c] = 0;
  }
  if (nv < 2) return;
  int q = 0;
  for (int c = (nv == 2 ? last : 0); c < S; ++c) {
    const int cnt = counts[c0 + c];
    if (cnt <= 0) continue;
    if ((q++ & (kSvcThreads / 64 - 1)) != wid) continue;          // wave-uniform
    const double cp = C * ((double)N / ((double)nv * (double)cnt));
    const double cn = nv == 2 ? C * ((double)N / ((double)nv * (double)counts[c0 + first])) : C;
    double w, b, gn;
    bool conv;
    int it;
    if (IN_LDS)
      it = svc_solve((const float*)xs, (const unsigned char*)ys, N, c, cp, cn, gtol, max_iter, &w, &b, &gn, &conv);
    else
      it = svc_solve(xg, yg, N, c, cp, cn, gtol, max_iter, &w, &b, &gn, &conv);
    if (lane == 0) {
      theta[(base + c) * 2] = w, theta[(base + c) * 2 + 1] = b;
      gnorm[base + c] = gn, iters[base + c] = it;
      if (!conv) atomicOr(&flags[2], 1);
    }
  }
}

// grid (256-row tile, latent i): a thread per test row.  correct[i][j] counts the rows whose prediction equals the label.
__global__ __launch_bounds__(256) void svc_score_kernel(const float* __restrict__ x, size_t ld, const int* __restrict__ y,
                                                        int Nt, int D, SegPlan pl, const int* __restrict__ cvalid,
                                                        const double* __restrict__ theta,
                                                        unsigned long long* __restrict__ correct, int* __restrict__ pred,
                                                        int* __restrict__ flags) {
  __shared__ int nv_s[kSegMaxK], first_s[kSegMaxK], last_s[kSegMaxK], cnt_s[kSegMaxK];
  const int i = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  const int K = pl.K, csum = pl.off[K];
  if ((int)threadIdx.x < K) {
    const int c0 = pl.off[threadIdx.x], S = pl.off[threadIdx.x + 1] - c0;
    int nv = 0, first = -1, last = -1;
    for (int c = 0; c < S; ++c)
      if (cvalid[c0 + c]) {
        if (first < 0) first = c;
        last = c, ++nv;
      }
    nv_s[threadIdx.x] = nv, first_s[threadIdx.x] = first, last_s[threadIdx.x] = last, cnt_s[threadIdx.x] = 0;
  }
  __syncthreads();
  const bool live = n < Nt;
  const float xv = live ? x[(size_t)n * ld + i] : 0.f;
  if (live && !finite_f(xv)) atomicOr(&flags[0], 1);
  const double xd = (double)xv;
  const double* th = theta + (size_t)i * csum * 2;
  for (int j = 0; j < K; ++j) {
    const int c0 = pl.off[j], S = pl.off[j + 1] - c0, nv = nv_s[j];
    int p = -1;
    if (nv == 1) {
      p = first_s[j];
    } else if (nv == 2) {
      const int c = last_s[j];
      const double dec = th[(size_t)(c0 + c) * 2] * xd + th[(size_t)(c0 + c) * 2 + 1];
      p = dec > 0.0 ? c : first_s[j];
    } else if (nv >= 3) {
      double best = -INFINITY;
      for (int c = 0; c < S; ++c) {
        if (!cvalid[c0 + c]) continue;
        const double dec = th[(size_t)(c0 + c) * 2] * xd + th[(size_t)(c0 + c) * 2 + 1];
        if (dec > best || p < 0) best = dec, p = c;    // ascending c, strict: ties go to the smallest class
      }
    }
    bool hit = false;
    if (live) {
      const int yv = y[(size_t)n * K + j];
      if ((unsigned)yv >= (unsigned)S) atomicOr(&flags[1], 1);
      hit = p == yv;
      if (pred) pred[((size_t)i * K + j) * Nt + n] = p;
    }
    const unsigned long long mask = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&cnt_s[j], (int)__popcll(mask));
  }
  __syncthreads();
  if ((int)threadIdx.x < K && cnt_s[threadIdx.x])
    atomicAdd(&correct[(size_t)i * K + threadIdx.x], (unsigned long long)cnt_s[threadIdx.x]);
}

// ---- host side -----------------------------------------------------------------------------------------------------
constexpr SegWords kXsWords = {"K = %lld problems", "no class counts", "problem %lld has %lld classes"};
static int xs_plan(const char* name, int N, int D, int K, const int* csize, SegPlan* pl) {
  return need_dim(name, "N = %lld", N, 1, kXsMaxN, "1..2^24") || need_dim(name, "D = %lld", D, 1, kXsMaxD, "1..512") ||
         seg_plan(name, K, csize, kXsMaxCsize, kXsWords, pl);
}
struct SvcWs {
  size_t xt, yt, counts, total;
};
static inline SvcWs svc_ws(int N, int D, int K, int csum) {
  SvcWs w;
  w.xt = 0;
  w.yt = w.xt + (size_t)D * N * sizeof(float);
  w.counts = align_up(w.yt + (size_t)K * N, 16);
  w.total = w.counts + (size_t)csum * sizeof(int);
  return w;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_fvae_gvar(const float* mu, size_t ld, int N, int D, double* gvar, int* flags, void* stream) {
  if (need_dim("itcv_fvae_gvar", "N = %lld rows", N, 2, kXsMaxN, "2..2^24") ||
      need_dim("itcv_fvae_gvar", "D = %lld", D, 1, kXsMaxD, "1..512"))
    return 1;
  ITCV_REQUIRE(mu && gvar && flags && ld >= (size_t)D, "itcv_fvae_gvar");
  hipLaunchKernelGGL(fvae_gvar_kernel, dim3(cdiv(D, 32)), dim3(1024), 0, S(stream), mu, ld, N, D, gvar, flags);
  ITCV_CHECK_LAUNCH("itcv_fvae_gvar");
  return 0;
}

int itcv_fvae_votes(const float* mu, size_t ld, int M, int L, int D, const double* gvar, double threshold, const int* fidx,
                    int K, long long* votes, int* flags, void* stream) {
  const char* name = "itcv_fvae_votes";
  if (need_dim(name, "L = %lld rows a group", L, 2, kXsMaxL, "2..2^16")) return 1;
  if (M < 1 || (long long)M * L > kXsMaxN) return fail("%s: M = %lld groups (M * L rows) is outside 1..2^24 rows", name, M);
  if (need_dim(name, "D = %lld", D, 1, kXsMaxD, "1..512") || need_dim(name, "K = %lld factors", K, 1, kXsMaxCsize, "1..256"))
    return 1;
  ITCV_REQUIRE(mu && gvar && fidx && votes && flags && ld >= (size_t)D, name);
  hipStream_t st = S(stream);
  if (hipMemsetAsync(votes, 0, (size_t)D * K * sizeof(long long), st) != hipSuccess)
    return fail("%s: clearing the votes failed", name);
  hipLaunchKernelGGL(fvae_votes_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, mu, ld, M, L, D, gvar, threshold, fidx, K,
                     reinterpret_cast<unsigned long long*>(votes), flags);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_fvae_classify(const long long* votes_train, const long long* votes_eval, int D, int K, int Mt, int Me,
                       const double* gvar, double threshold, int* classifier, double* res, void* stream) {
  const char* name = "itcv_fvae_classify";
  if (need_dim(name, "D = %lld", D, 1, kXsMaxD, "1..512") || need_dim(name, "K = %lld factors", K, 1, kXsMaxCsize, "1..256"))
    return 1;
  ITCV_REQUIRE(votes_train && votes_eval && gvar && classifier && res && Mt >= 1 && Me >= 1, name);
  hipLaunchKernelGGL(fvae_classify_kernel, dim3(1), dim3(256), 0, S(stream),
                     reinterpret_cast<const unsigned long long*>(votes_train),
                     reinterpret_cast<const unsigned long long*>(votes_eval), D, K, Mt, Me, gvar, threshold, classifier, res);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_sap_svc_lds_rows(void) { return kSvcLdsRows; }

size_t itcv_sap_svc_workspace(int N, int D, int K, int csum) {
  if (N < 1 || N > kXsMaxN || D < 1 || D > kXsMaxD || K < 1 || K > kSegMaxK || csum < K || csum > K * kXsMaxCsize) return 0;
  return svc_ws(N, D, K, csum).total;
}

int itcv_sap_svc_fit(const float* x, size_t ld, const int* y, int N, int D, int K, const int* csize, double C, double gtol,
                     int max_iter, double* theta, double* gnorm, int* iters, int* cvalid, int* flags, void* ws,
                     size_t ws_bytes, void* stream) {
  const char* name = "itcv_sap_svc_fit";
  SegPlan pl;
  if (int e = xs_plan(name, N, D, K, csize, &pl)) return e;
  ITCV_REQUIRE(x && y && theta && gnorm && iters && cvalid && flags && ld >= (size_t)D && C > 0.0 && gtol > 0.0 &&
                   max_iter >= 1,
               name);
  const int csum = pl.off[K];
  const SvcWs w = svc_ws(N, D, K, csum);
  ITCV_REQUIRE(ws && ws_bytes >= w.total, "itcv_sap_svc_fit(workspace)");
  char* base = static_cast<char*>(ws);
  float* xt = reinterpret_cast<float*>(base + w.xt);
  unsigned char* yt = reinterpret_cast<unsigned char*>(base + w.yt);
  int* counts = reinterpret_cast<int*>(base + w.counts);
  hipStream_t st = S(stream);
  if (hipMemsetAsync(counts, 0, (size_t)csum * sizeof(int), st) != hipSuccess)
    return fail("%s: clearing the class counts failed", name);
  hipLaunchKernelGGL(svc_prep_kernel, dim3(cdiv(N, 64), cdiv(D, 64)), dim3(256), 0, st, x, ld, y, N, D, pl, xt, yt, counts,
                     flags);
  ITCV_CHECK_LAUNCH("itcv_sap_svc_fit(copies)");
  if (N <= kSvcLdsRows)
    launch_lds<svc_fit_kernel<true>>(dim3(D, K), dim3(kSvcThreads), (size_t)N * 5, st, (const float*)xt,
                                     (const unsigned char*)yt, (const int*)counts, N, D, pl, C, gtol, max_iter, theta,
                                     gnorm, iters, cvalid, flags);
  else
    hipLaunchKernelGGL(svc_fit_kernel<false>, dim3(D, K), dim3(kSvcThreads), 0, st, (const float*)xt,
                       (const unsigned char*)yt, (const int*)counts, N, D, pl, C, gtol, max_iter, theta, gnorm, iters,
                       cvalid, flags);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_sap_svc_score(const float* x, size_t ld, const int* y, int Nt, int D, int K, const int* csize, const int* cvalid,
                       const double* theta, long long* correct, int* pred, int* flags, void* stream) {
  const char* name = "itcv_sap_svc_score";
  SegPlan pl;
  if (int e = xs_plan(name, Nt, D, K, csize, &pl)) return e;
  ITCV_REQUIRE(x && y && cvalid && theta && correct && flags && ld >= (size_t)D, name);
  hipStream_t st = S(stream);
  if (hipMemsetAsync(correct, 0, (size_t)D * K * sizeof(long long), st) != hipSuccess)
    return fail("%s: clearing the counts failed", name);
  hipLaunchKernelGGL(svc_score_kernel, dim3(cdiv(Nt, 256), D), dim3(256), 0, st, x, ld, y, Nt, D, pl, cvalid, theta,
                     reinterpret_cast<unsigned long long*>(correct), pred, flags);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
