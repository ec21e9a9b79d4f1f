// The importance-weighted bound (Burda, Grosse and Salakhutdinov 2016, "Importance Weighted Autoencoders") as a training
// objective and as a streaming estimate of log p(x), with the doubly reparameterised (Tucker et al. 2019) and
// sticking-the-landing (Roeder et al. 2017) gradient estimators.  The rules are in include/itcv_hip.h.  Row r = k B + b is
// sample k of image b.
//   iwae_sample      : ONE wave per row, four rows per 256-thread block, the blocks stride over the rows.  Lane d, d + 64, ..
//                      holds its columns' terms of lat in fp64 from the fp32 inputs; one wave reduction gives the row's.
//   iwae_sample_bwd  : ONE thread per element of [B, D]; it walks the K samples of its image in k order.
//   iwae_rows_partial: the broadcast reconstruction rows.  A block takes slice s of image b and the rows k = kg, kg + KG, ..
//                      of that image: the slice of x is read from HBM once and then from cache.  A row's sum is
//                      recon_slice_acc's, the body itcv_recon_rows_fwd runs: with x materialised K times the two give the
//                      same bits.  (Two rows at a time in one loop moved the last bit of bce rows: the compiler contracts
//                      the interleaved fp32 terms differently.)
//   iwae_rows_bwd    : the same blocking, drecon = g[r] err'.
//   iwae_combine     : ONE wave per image, lanes striding over k: max, sum of e^(logw - max), normalised weights, the
//                      weighted means of the two terms.  iwae_finish: ONE block adds the per-image values in image order
//                      (objective.h's ordered_sum).
//   iwae_accumulate / iwae_finalize: the same wave per image over one chunk, merged into a per-image fp64 state.
// Every sum has a fixed order, there is no atomic, and nothing depends on the grid or on timing: the same inputs give the
// same bits.  Nothing in this file's fp64 arithmetic may be contracted into a fused multiply-add: the pragma stands inside
// every fp64 body and not at file scope, because the fp32 error terms of recon_rows.h have to be compiled here exactly as
// loss_optim.hip compiles them.
#include "objective.h"
#include "recon_rows.h"

namespace itcv {

constexpr int kIwaeMaxD = 512;
constexpr int kIwaeMaxK = 1024;
constexpr int kIwaeMaxRows = 1 << 24;
constexpr int kIwaeThreads = 256;
constexpr int kIwaeRowsPerBlock = kIwaeThreads / kWave;
constexpr int kIwaeMaxBlocks = 2048;
constexpr int kIwaeEstIwae = 0, kIwaeEstDreg = 2;     // 1: stl

__global__ __launch_bounds__(kIwaeThreads) void iwae_sample_kernel(const float* __restrict__ mu, size_t ldm,
                                                                   const float* __restrict__ logvar, size_t ldl,
                                                                   const float* __restrict__ eps, size_t lde,
                                                                   float* __restrict__ z, double* __restrict__ lat, int B,
                                                                   int R, int D) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = blockIdx.x * kIwaeRowsPerBlock + w; r < R; r += gridDim.x * kIwaeRowsPerBlock) {   // wave-uniform
    const int b = r % B;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
      const double m = mu[(size_t)b * ldm + d], l = logvar[(size_t)b * ldl + d], e = eps[(size_t)r * lde + d];
      const double zz = m + exp(0.5 * l) * e;
      z[(size_t)r * D + d] = (float)zz;
      acc += (zz * zz - e * e) - l;
    }
    acc = wave_sum(acc);
    if (lane == 0) lat[r] = 0.5 * acc;
  }
}

__global__ __launch_bounds__(kIwaeThreads) void iwae_sample_bwd_kernel(const float* __restrict__ dz, size_t ldz,
                                                                       const double* __restrict__ h,
                                                                       const double* __restrict__ wt,
                                                                       const float* __restrict__ mu, size_t ldm,
                                                                       const float* __restrict__ logvar, size_t ldl,
                                                                       const float* __restrict__ eps, size_t lde,
                                                                       float* __restrict__ dmu, float* __restrict__ dlv,
                                                                       int B, int K, int D, int est) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * kIwaeThreads + threadIdx.x;
  if (i >= (size_t)B * D) return;
  const int b = (int)(i / D), d = (int)(i - (size_t)b * D);
  const double m = mu[(size_t)b * ldm + d], l = logvar[(size_t)b * ldl + d];
  const double sg = exp(0.5 * l);
  double am = 0.0, al = 0.0;
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    const size_t r = (size_t)k * B + b;
    const double e = eps[r * lde + d], g = dz[r * ldz + d], hr = h[r];
    const double zz = m + sg * e;
    if (est == kIwaeEstIwae) {
      const double t = g + hr * zz;
      am += t;
      al += (t * e) * sg * 0.5 - hr * 0.5;
    } else {
      double p = g + hr * (zz - e / sg);
      if (est == kIwaeEstDreg) p *= wt[r];
      am += p;
      al += (p * e) * sg * 0.5;
    }
  }
  dmu[i] = (float)am;
  dlv[i] = (float)al;
}

// grid (B, splits, KG): part[(k B + b) splits + s] for k = kg, kg + KG, ..
template <int LT>
__global__ __launch_bounds__(256) void iwae_rows_partial_kernel(const float* __restrict__ x, const float* __restrict__ recon,
                                                               double* __restrict__ part, int B, int K, size_t P,
                                                               int splits, int vec4) {
  __shared__ double scratch[4];
  const int b = blockIdx.x, s = blockIdx.y, KG = gridDim.z;
  size_t beg, end;
  recon_slice(P, splits, s, beg, end);
  const float* xr = x + (size_t)b * P;
  for (int k = blockIdx.z; k < K; k += KG) {            // block-uniform
    const size_t r = (size_t)k * B + b;
    const double acc = block_sum(recon_slice_acc<LT>(xr, recon + r * P, beg, end, vec4), scratch);
    if (threadIdx.x == 0) part[r * splits + s] = acc;
  }
}
__global__ void iwae_rows_fold_kernel(const double* __restrict__ part, float* __restrict__ rows, int R, int splits) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  rows[r] = (float)fold_strided(0.0, part + (size_t)r * splits, (size_t)1, splits);
}

// grid (B, splits, KG): drecon[r][p] = g[r] err'(recon[r][p], x[b][p])
template <int LT>
__global__ __launch_bounds__(256) void iwae_rows_bwd_kernel(const float* __restrict__ x, const float* __restrict__ recon,
                                                           const float* __restrict__ g, float* __restrict__ drecon, int B,
                                                           int K, size_t P, int splits, int vec4) {
  const int b = blockIdx.x, s = blockIdx.y, KG = gridDim.z;
  size_t beg, end;
  recon_slice(P, splits, s, beg, end);
  const float* xr = x + (size_t)b * P;
  for (int k = blockIdx.z; k < K; k += KG) {
    const size_t r = (size_t)k * B + b;
    const float gr = g[r];
    const float* rr = recon + r * P;
    float* dr = drecon + r * P;
    if (vec4) {
      for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
        const float4 t = *reinterpret_cast<const float4*>(xr + i);
        const float4 v = *reinterpret_cast<const float4*>(rr + i);
        float4 o;
        o.x = gr * rec_derr<LT>(v.x, t.x);
        o.y = gr * rec_derr<LT>(v.y, t.y);
        o.z = gr * rec_derr<LT>(v.z, t.z);
        o.w = gr * rec_derr<LT>(v.w, t.w);
        *reinterpret_cast<float4*>(dr + i) = o;
      }
    } else {
      for (size_t i = beg + threadIdx.x; i < end; i += 256) dr[i] = gr * rec_derr<LT>(rr[i], xr[i]);
    }
  }
}

// what one wave knows of the K samples of an image after its two passes; valid in every lane
struct IwaeWave {
  double m, s1, s2, sl, srow, slat;
};
// logw_k = -(beta_rec rows[k B + b] + beta_kl lat[k B + b]), k < K, lanes striding over k; wt (may be NULL) receives
// e^(logw - m) / s1
__device__ __forceinline__ IwaeWave iwae_wave(const float* __restrict__ rows, const double* __restrict__ lat, int b, int B,
                                              int K, double beta_rec, double beta_kl, double* __restrict__ wt) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  IwaeWave o;
  double m = -INFINITY;
  for (int k = lane; k < K; k += 64) {
    const size_t r = (size_t)k * B + b;
    const double lw = -(beta_rec * (double)rows[r] + beta_kl * lat[r]);
    m = lw > m ? lw : m;
  }
  o.m = wave_max(m);
  double s1 = 0.0, s2 = 0.0, sl = 0.0;
  for (int k = lane; k < K; k += 64) {
    const size_t r = (size_t)k * B + b;
    const double lw = -(beta_rec * (double)rows[r] + beta_kl * lat[r]);
    const double e = exp(lw - o.m);
    s1 += e;
    s2 += e * e;
    sl += lw;
  }
  o.s1 = wave_sum(s1), o.s2 = wave_sum(s2), o.sl = wave_sum(sl);
  double srow = 0.0, slat = 0.0;
  if (wt) {
    for (int k = lane; k < K; k += 64) {
      const size_t r = (size_t)k * B + b;
      const double rw = rows[r], lt = lat[r];
      const double w = exp(-(beta_rec * rw + beta_kl * lt) - o.m) / o.s1;
      wt[r] = w;
      srow += w * rw;
      slat += w * lt;
    }
  }
  o.srow = wave_sum(srow), o.slat = wave_sum(slat);
  return o;
}

// img [4][B]: bound, ess, sum_k wt rows, sum_k wt lat
__global__ __launch_bounds__(kIwaeThreads) void iwae_combine_kernel(const float* __restrict__ rows,
                                                                    const double* __restrict__ lat, double beta_rec,
                                                                    double beta_kl, double* __restrict__ wt,
                                                                    double* __restrict__ img, int B, int K) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = blockIdx.x * kIwaeRowsPerBlock + w; b < B; b += gridDim.x * kIwaeRowsPerBlock) {   // wave-uniform
    const IwaeWave v = iwae_wave(rows, lat, b, B, K, beta_rec, beta_kl, wt);
    if (lane == 0) {
      img[b] = (v.m + log(v.s1)) - log((double)K);
      img[(size_t)B + b] = (v.s1 * v.s1) / v.s2;
      img[2 * (size_t)B + b] = v.srow;
      img[3 * (size_t)B + b] = v.slat;
    }
  }
}

__global__ __launch_bounds__(kIwaeThreads) void iwae_finish_kernel(const double* __restrict__ img, int B, double beta_rec,
                                                                   double beta_kl, float* __restrict__ out,
                                                                   float* __restrict__ terms) {
#pragma clang fp contract(off)
  __shared__ double red[kIwaeThreads];
  const double bound = ordered_sum<kIwaeThreads>(img, B, red);
  const double ess = ordered_sum<kIwaeThreads>(img + B, B, red);
  const double rec = ordered_sum<kIwaeThreads>(img + 2 * (size_t)B, B, red);
  const double kl = ordered_sum<kIwaeThreads>(img + 3 * (size_t)B, B, red);
  if (threadIdx.x == 0) {
    const double inv = 1.0 / (double)B;
    out[0] = (float)(-(bound * inv));
    terms[0] = (float)(beta_rec * (rec * inv));
    terms[1] = (float)(beta_kl * (kl * inv));
    terms[2] = (float)(bound * inv);
    terms[3] = (float)(ess * inv);
  }
}

__global__ void iwae_combine_bwd_kernel(const float* __restrict__ g, const double* __restrict__ wt, double beta_rec,
                                        double beta_kl, float* __restrict__ g_rows, double* __restrict__ g_lat, int B,
                                        size_t R) {
#pragma clang fp contract(off)
  const double gb = (double)g[0] / (double)B;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (size_t)gridDim.x * blockDim.x) {
    const double a = gb * wt[r];
    g_rows[r] = (float)(beta_rec * a);
    g_lat[r] = beta_kl * a;
  }
}

// state [5][B]; a count of 0 marks an empty state, whatever the other four hold
__global__ __launch_bounds__(kIwaeThreads) void iwae_accumulate_kernel(const float* __restrict__ rows,
                                                                       const double* __restrict__ lat, double beta_rec,
                                                                       double beta_kl, double* __restrict__ state, int B,
                                                                       int K) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = blockIdx.x * kIwaeRowsPerBlock + w; b < B; b += gridDim.x * kIwaeRowsPerBlock) {   // wave-uniform
    const IwaeWave v = iwae_wave(rows, lat, b, B, K, beta_rec, beta_kl, nullptr);
    if (lane == 0) {
      double* st = state + b;
      const double n = st[4 * (size_t)B];
      double m = v.m, s1 = v.s1, s2 = v.s2, sl = v.sl;
      if (n > 0.0) {
        const double m0 = st[0], M = m0 > m ? m0 : m;
        const double f0 = exp(m0 - M), f1 = exp(m - M);
        s1 = st[(size_t)B] * f0 + s1 * f1;
        s2 = st[2 * (size_t)B] * (f0 * f0) + s2 * (f1 * f1);
        sl = st[3 * (size_t)B] + sl;
        m = M;
      }
      st[0] = m;
      st[(size_t)B] = s1;
      st[2 * (size_t)B] = s2;
      st[3 * (size_t)B] = sl;
      st[4 * (size_t)B] = (n > 0.0 ? n : 0.0) + (double)K;
    }
  }
}
__global__ void iwae_finalize_kernel(const double* __restrict__ state, double* __restrict__ log_px,
                                     double* __restrict__ elbo, double* __restrict__ ess, int B) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double m = state[b], s1 = state[(size_t)B + b], s2 = state[2 * (size_t)B + b], sl = state[3 * (size_t)B + b];
  const double n = state[4 * (size_t)B + b];
  log_px[b] = (m + log(s1)) - log(n);
  elbo[b] = sl / n;
  ess[b] = (s1 * s1) / s2;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline bool iwae_shape_ok(int B, int K) {
  return B >= 1 && K >= 1 && K <= kIwaeMaxK && (long long)B * K <= kIwaeMaxRows;
}
// nothing is launched on a failure
static int iwae_check(const char* name, bool ptrs, int B, int K) {
  if (need_pointers(name, ptrs)) return 1;
  if (B < 1) return fail("%s: B = %lld images is below 1", name, B);
  if (need_dim(name, "K = %lld samples", K, 1, kIwaeMaxK, "1..1024")) return 1;
  if ((long long)B * K > kIwaeMaxRows) return fail("%s: B K = %lld rows exceed 2^24", name, (long long)B * K);
  return 0;
}
static int iwae_check_d(const char* name, int D, size_t ld_mu, size_t ld_logvar, size_t ld_eps) {
  return need_dim(name, "D = %lld", D, 1, kIwaeMaxD, "1..512") || need_stride(name, "mu's", ld_mu, "D", D) ||
         need_stride(name, "logvar's", ld_logvar, "D", D) || need_stride(name, "eps's", ld_eps, "D", D);
}
static inline bool iwae_betas_ok(double beta_rec, double beta_kl) {
  return finite(beta_rec) && finite(beta_kl);
}
// k-groups of the broadcast kernels' grid: enough blocks to fill the device, never more than K
static inline int iwae_kgroups(int B, int K, int splits) {
  const long long per = (long long)B * splits;
  long long kg = (2048 + per - 1) / per;
  if (kg > K) kg = K;
  if (kg > 65535) kg = 65535;
  return kg < 1 ? 1 : (int)kg;
}
static inline int iwae_vec4(const float* x, const float* a, const float* b, size_t P) {
  return (P & 3) == 0 && (((uintptr_t)x | (uintptr_t)a | (uintptr_t)b) & 15) == 0;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_iwae_sample_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps,
                         size_t ld_eps, float* z, double* lat, int B, int K, int D, void* stream) {
  const char* name = "itcv_iwae_sample_fwd";
  if (int e = iwae_check(name, mu && logvar && eps && z && lat, B, K)) return e;
  if (int e = iwae_check_d(name, D, ld_mu, ld_logvar, ld_eps)) return e;
  const int R = B * K;
  const dim3 grid(row_grid(R, kIwaeRowsPerBlock, kIwaeMaxBlocks));
  hipLaunchKernelGGL(iwae_sample_kernel, grid, dim3(kIwaeThreads), 0, S(stream), mu, ld_mu, logvar, ld_logvar, eps, ld_eps,
                     z, lat, B, R, D);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_iwae_sample_bwd(const float* dz, size_t ld_dz, const double* h, const double* wt, const float* mu, size_t ld_mu,
                         const float* logvar, size_t ld_logvar, const float* eps, size_t ld_eps, float* dmu, float* dlogvar,
                         int B, int K, int D, int estimator, void* stream) {
  const char* name = "itcv_iwae_sample_bwd";
  const bool ptrs = dz && h && mu && logvar && eps && dmu && dlogvar && (estimator != kIwaeEstDreg || wt);
  if (int e = iwae_check(name, ptrs, B, K)) return e;
  if (int e = iwae_check_d(name, D, ld_mu, ld_logvar, ld_eps)) return e;
  if (need_stride(name, "dz's", ld_dz, "D", D)) return 1;
  if (estimator < kIwaeEstIwae || estimator > kIwaeEstDreg)
    return fail("%s: estimator %lld is not 0 (iwae), 1 (stl) or 2 (dreg)", name, estimator);
  hipLaunchKernelGGL(iwae_sample_bwd_kernel, dim3((unsigned)cdivz((size_t)B * D, kIwaeThreads)), dim3(kIwaeThreads), 0,
                     S(stream), dz, ld_dz, h, wt, mu, ld_mu, logvar, ld_logvar, eps, ld_eps, dmu, dlogvar, B, K, D,
                     estimator);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

size_t itcv_iwae_rows_workspace(int B, int K, size_t P) {
  return iwae_shape_ok(B, K) && P > 0 ? (size_t)B * K * recon_splits(B * K, P) * sizeof(double) : 0;
}

int itcv_iwae_rows_fwd(const float* x, const float* recon, float* rows, int B, int K, size_t P, int loss_type, void* ws,
                       size_t ws_bytes, void* stream) {
  const char* name = "itcv_iwae_rows_fwd";
  if (int e = iwae_check(name, x && recon && rows && ws, B, K)) return e;
  if (P < 1) return fail("%s: P = %lld elements a row is below 1", name, (long long)P);
  if (loss_type != ITCV_LOSS_MSE && loss_type != ITCV_LOSS_L1 && loss_type != ITCV_LOSS_BCE)
    return fail("%s: unknown loss type %lld", name, loss_type);
  const int R = B * K, splits = recon_splits(R, P);
  if (ws_bytes < (size_t)R * splits * sizeof(double)) return fail("%s: the workspace is too small", name);
  double* part = static_cast<double*>(ws);
  const int vec4 = iwae_vec4(x, recon, nullptr, P);
  const dim3 grid(B, splits, iwae_kgroups(B, K, splits));
  hipStream_t st = S(stream);
  if (loss_type == ITCV_LOSS_MSE)
    hipLaunchKernelGGL(iwae_rows_partial_kernel<ITCV_LOSS_MSE>, grid, dim3(256), 0, st, x, recon, part, B, K, P, splits, vec4);
  else if (loss_type == ITCV_LOSS_L1)
    hipLaunchKernelGGL(iwae_rows_partial_kernel<ITCV_LOSS_L1>, grid, dim3(256), 0, st, x, recon, part, B, K, P, splits, vec4);
  else
    hipLaunchKernelGGL(iwae_rows_partial_kernel<ITCV_LOSS_BCE>, grid, dim3(256), 0, st, x, recon, part, B, K, P, splits, vec4);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(iwae_rows_fold_kernel, dim3(cdiv(R, 256)), dim3(256), 0, st, (const double*)part, rows, R, splits);
  ITCV_CHECK_LAUNCH("itcv_iwae_rows_fwd(fold)");
  return 0;
}

int itcv_iwae_rows_bwd(const float* x, const float* recon, const float* g, float* drecon, int B, int K, size_t P,
                       int loss_type, void* stream) {
  const char* name = "itcv_iwae_rows_bwd";
  if (int e = iwae_check(name, x && recon && g && drecon, B, K)) return e;
  if (P < 1) return fail("%s: P = %lld elements a row is below 1", name, (long long)P);
  if (loss_type != ITCV_LOSS_MSE && loss_type != ITCV_LOSS_L1 && loss_type != ITCV_LOSS_BCE)
    return fail("%s: unknown loss type %lld", name, loss_type);
  const int splits = recon_splits(B * K, P);
  const int vec4 = iwae_vec4(x, recon, drecon, P);
  const dim3 grid(B, splits, iwae_kgroups(B, K, splits));
  hipStream_t st = S(stream);
  if (loss_type == ITCV_LOSS_MSE)
    hipLaunchKernelGGL(iwae_rows_bwd_kernel<ITCV_LOSS_MSE>, grid, dim3(256), 0, st, x, recon, g, drecon, B, K, P, splits, vec4);
  else if (loss_type == ITCV_LOSS_L1)
    hipLaunchKernelGGL(iwae_rows_bwd_kernel<ITCV_LOSS_L1>, grid, dim3(256), 0, st, x, recon, g, drecon, B, K, P, splits, vec4);
  else
    hipLaunchKernelGGL(iwae_rows_bwd_kernel<ITCV_LOSS_BCE>, grid, dim3(256), 0, st, x, recon, g, drecon, B, K, P, splits, vec4);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_iwae_combine_fwd(const float* rows, const double* lat, double beta_rec, double beta_kl, double* wt, double* img,
                          float* out, float* terms, int B, int K, void* stream) {
  const char* name = "itcv_iwae_combine_fwd";
  if (int e = iwae_check(name, rows && lat && wt && img && out && terms, B, K)) return e;
  if (!iwae_betas_ok(beta_rec, beta_kl)) return fail("%s: beta_rec and beta_kl must be finite numbers", name);
  hipStream_t st = S(stream);
  const dim3 grid(row_grid(B, kIwaeRowsPerBlock, kIwaeMaxBlocks));
  hipLaunchKernelGGL(iwae_combine_kernel, grid, dim3(kIwaeThreads), 0, st, rows, lat, beta_rec, beta_kl, wt, img, B, K);
  ITCV_CHECK_LAUNCH(name);
  hipLaunchKernelGGL(iwae_finish_kernel, dim3(1), dim3(kIwaeThreads), 0, st, (const double*)img, B, beta_rec, beta_kl, out,
                     terms);
  ITCV_CHECK_LAUNCH("itcv_iwae_combine_fwd(finish)");
  return 0;
}

int itcv_iwae_combine_bwd(const float* g, const double* wt, double beta_rec, double beta_kl, float* g_rows, double* g_lat,
                          int B, int K, void* stream) {
  const char* name = "itcv_iwae_combine_bwd";
  if (int e = iwae_check(name, g && wt && g_rows && g_lat, B, K)) return e;
  if (!iwae_betas_ok(beta_rec, beta_kl)) return fail("%s: beta_rec and beta_kl must be finite numbers", name);
  const size_t R = (size_t)B * K;
  hipLaunchKernelGGL(iwae_combine_bwd_kernel, dim3(stream_grid(R, 1)), dim3(256), 0, S(stream), g, wt, beta_rec, beta_kl,
                     g_rows, g_lat, B, R);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_iwae_accumulate(const float* rows, const double* lat, double beta_rec, double beta_kl, double* state, int B, int K,
                         void* stream) {
  const char* name = "itcv_iwae_accumulate";
  if (int e = iwae_check(name, rows && lat && state, B, K)) return e;
  if (!iwae_betas_ok(beta_rec, beta_kl)) return fail("%s: beta_rec and beta_kl must be finite numbers", name);
  const dim3 grid(row_grid(B, kIwaeRowsPerBlock, kIwaeMaxBlocks));
  hipLaunchKernelGGL(iwae_accumulate_kernel, grid, dim3(kIwaeThreads), 0, S(stream), rows, lat, beta_rec, beta_kl, state, B,
                     K);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

int itcv_iwae_finalize(const double* state, double* log_px, double* elbo, double* ess, int B, void* stream) {
  const char* name = "itcv_iwae_finalize";
  if (int e = iwae_check(name, state && log_px && elbo && ess, B, 1)) return e;
  hipLaunchKernelGGL(iwae_finalize_kernel, dim3(cdiv(B, 256)), dim3(256), 0, S(stream), state, log_px, elbo, ess, B);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
