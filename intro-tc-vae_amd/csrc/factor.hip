// The FactorVAE objective's own device primitives (Kim & Mnih 2018; disentanglement_lib's `factor_vae`).  The rules are
// in include/itcv_hip.h; the discriminator's dense layers are the skinny GEMMs of conv_igemm.hip (itcv_linear_lrelu_fwd,
// itcv_linear_dgrad_lrelu).
//   permute_dims : ONE block per latent dimension.  Every key becomes a 64-bit word, the monotone uint32 image of the
//                  float (csrc/udr.hip's rank key) above the row index, so the words of a column are distinct whatever the
//                  keys are (ties, +-0, +-inf, NaN) and their ascending order is a stable sort of the keys.  The words are
//                  sorted in LDS by the bitonic network of udr_rank_kernel (every compare-exchange points upwards, a
//                  pair whose upper index is past B is skipped: any B, no padding); row r of the output then takes the
//                  value of the row whose index sits in word r.
//   disc_head    : ONE block.  Thread t folds rows t, t + 256, ... in ascending order in fp64, then the block's partial
//                  sums are added in thread order by thread 0: a fixed order, no atomics, the same bits every run.
// Nothing in this file may be contracted into a fused multiply-add.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kPermMaxB = 4096;           // 32 KiB of 64-bit words in LDS
constexpr int kPermMaxD = 512;
constexpr int kPermThreads = 1024;
constexpr int kHeadThreads = 256;
constexpr int kHeadMaxR = 1 << 24;

// ascending in the numeric order of finite floats; +0 and -0 share one key (csrc/udr.hip: rank_key)
__device__ __forceinline__ uint32_t perm_key(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kPermThreads) void permute_dims_kernel(const float* __restrict__ z, size_t ldz,
                                                                    const float* __restrict__ keys, size_t ldk,
                                                                    float* __restrict__ out, float* __restrict__ zcopy,
                                                                    int B, int D) {
  __shared__ unsigned long long words[kPermMaxB];
  const int d = blockIdx.x, tid = threadIdx.x, T = kPermThreads;
  for (int n = tid; n < B; n += T)
    words[n] = ((unsigned long long)perm_key(keys[(size_t)n * ldk + d]) << 32) | (unsigned)n;
  __syncthreads();
  int np2 = 1;
  while (np2 < B) np2 <<= 1;
  const int half = np2 >> 1;
  for (int k = 2; k <= np2; k <<= 1) {
    for (int s = k >> 1; s >= 1; s >>= 1) {
      const bool mirror = s == (k >> 1);
      for (int p = tid; p < half; p += T) {
        const int i = ((p & ~(s - 1)) << 1) | (p & (s - 1));
        const int j = mirror ? (i ^ (k - 1)) : (i | s);
        if (j < B) {                                  // i < j always
          const unsigned long long a = words[i], b = words[j];
          if (a > b) words[i] = b, words[j] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < B; r += T) {
    const int src = (int)(words[r] & 0xFFFFFFFFull);   // < B: the low half of a word is a row index
    out[(size_t)r * D + d] = z[(size_t)src * ldz + d];
    if (zcopy) zcopy[(size_t)r * D + d] = z[(size_t)r * ldz + d];
  }
}

// log(1 + exp(x)) and 1 / (1 + exp(-x)) without overflow
__device__ __forceinline__ double softplus64(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sigmoid64(double x) {
  const double e = exp(-fabs(x));
  return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// sums of the block's per-thread values, added in thread order by thread 0 (valid in thread 0 only)
template <int NQ>
__device__ __forceinline__ void head_fold(double (&v)[NQ], double* scratch) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < NQ; ++q) scratch[q * kHeadThreads + tid] = v[q];
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double s = 0.0;
      for (int t = 0; t < kHeadThreads; ++t) s += scratch[q * kHeadThreads + t];
      v[q] = s;
    }
  }
}

__global__ __launch_bounds__(kHeadThreads) void disc_head_fwd_kernel(const float* __restrict__ logits, int R, int R0,
                                                                     float* __restrict__ out) {
  __shared__ double scratch[4 * kHeadThreads];
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // sum d over the first R0 rows, CE of label 0, CE of label 1, correct rows
  for (int i = threadIdx.x; i < R; i += kHeadThreads) {
    const double d = (double)logits[2 * (size_t)i] - (double)logits[2 * (size_t)i + 1];
    if (i < R0) {
      v[0] += d;
      v[1] += softplus64(-d);
      v[3] += d >= 0.0 ? 1.0 : 0.0;       // argmax takes the first of two equal logits: class 0
    } else {
      v[2] += softplus64(d);
      v[3] += d < 0.0 ? 1.0 : 0.0;
    }
  }
  head_fold(v, scratch);
  if (threadIdx.x == 0) {
    const int R1 = R - R0;
    out[0] = (float)(v[0] / R0);
    out[1] = (float)(0.5 * (v[1] / R0) + (R1 > 0 ? 0.5 * (v[2] / R1) : 0.0));
    out[2] = (float)(v[3] / R);
  }
}

// mode 0: d tc / d logits over the first R0 rows; mode 1: d d_loss / d logits over all R rows
__global__ __launch_bounds__(256) void disc_head_bwd_kernel(const float* __restrict__ g, const float* __restrict__ logits,
                                                            float* __restrict__ dlogits, int R, int R0, int mode) {
  const int rows = mode == 0 ? R0 : R;
  const double gc = (double)g[0];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < rows; i += gridDim.x * 256) {
    double w;
    if (mode == 0) {
      w = gc / R0;
    } else {
      const double d = (double)logits[2 * (size_t)i] - (double)logits[2 * (size_t)i + 1];
      w = i < R0 ? -(0.5 * gc / R0) * sigmoid64(-d) : (0.5 * gc / (R - R0)) * sigmoid64(d);
    }
    dlogits[2 * (size_t)i] = (float)w;
    dlogits[2 * (size_t)i + 1] = (float)-w;
  }
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_permute_dims(const float* z, size_t ldz, const float* keys, size_t ldk, float* out, float* zcopy, int B, int D,
                      void* stream) {
  ITCV_REQUIRE(z && keys && out, "itcv_permute_dims");
  ITCV_REQUIRE(B >= 1 && B <= kPermMaxB && D >= 1 && D <= kPermMaxD, "itcv_permute_dims");
  ITCV_REQUIRE(ldz >= (size_t)D && ldk >= (size_t)D, "itcv_permute_dims");
  hipLaunchKernelGGL(permute_dims_kernel, dim3(D), dim3(kPermThreads), 0, S(stream), z, ldz, keys, ldk, out, zcopy, B, D);
  ITCV_CHECK_LAUNCH("itcv_permute_dims");
  return 0;
}

int itcv_disc_head_fwd(const float* logits, int R, int R0, float* out, void* stream) {
  ITCV_REQUIRE(logits && out, "itcv_disc_head_fwd");
  ITCV_REQUIRE(R0 >= 1 && R0 <= R && R <= kHeadMaxR, "itcv_disc_head_fwd");
  hipLaunchKernelGGL(disc_head_fwd_kernel, dim3(1), dim3(kHeadThreads), 0, S(stream), logits, R, R0, out);
  ITCV_CHECK_LAUNCH("itcv_disc_head_fwd");
  return 0;
}

int itcv_disc_head_bwd(const float* g, const float* logits, float* dlogits, int R, int R0, int mode, void* stream) {
  ITCV_REQUIRE(g && logits && dlogits, "itcv_disc_head_bwd");
  ITCV_REQUIRE(R0 >= 1 && R0 <= R && R <= kHeadMaxR, "itcv_disc_head_bwd");
  ITCV_REQUIRE(mode == 0 || (mode == 1 && R0 < R), "itcv_disc_head_bwd");
  const int rows = mode == 0 ? R0 : R;
  hipLaunchKernelGGL(disc_head_bwd_kernel, dim3(stream_grid((size_t)rows, 1)), dim3(256), 0, S(stream), g, logits, dlogits,
                     R, R0, mode);
  ITCV_CHECK_LAUNCH("itcv_disc_head_bwd");
  return 0;
}

}  // extern "C"
