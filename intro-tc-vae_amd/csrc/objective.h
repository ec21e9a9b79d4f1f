// What the objective kernels share: dip.hip, mmd.hip, sw.hip, ada.hip, joint.hip, sup.hip, iwae.hip and vamp.hip include
// this header, and nothing else does.  Device side: the ordered block sum of their finish kernels, the mean KL of the local
// rows (dip, mmd, sw) and the fp64 reparameterised sample, its KL term and their gradient (ada, joint; vamp the sample).  Host
// side: the capped row grid.  The host's finite test and the refusals that every entry point words alike are in common.h:
// nothing ties them to objectives.
//
// None of these files may contract a multiply and an add into a fused multiply-add -- that is what keeps their bits --
// but they say so in different places: seven at file scope, iwae.hip inside its fp64 bodies only.  So EVERY arithmetic
// helper here carries `#pragma clang fp contract(off)` in its own body and the header has no file-scope pragma: a helper
// gives the same bits wherever it is included, and the header changes nothing of the code around it.
//
// Deliberately NOT here: the three tile backward kernels that stage a 16 x 64 x 32 block through LDS (dip_bwd_kernel,
// mmd_bwd_kernel, sup_cov_bwd_kernel).  They look alike, but they differ in the types of their operands and in what is
// fp64 (dip: fp64 rows against fp32 weights; mmd: both fp32, widened per product; sup: both fp64), and one template over
// them would put their bits and their occupancy at risk for a few dozen lines.
#pragma once
#include <float.h>
#include <math.h>

#include "common.h"

namespace itcv {

// a[0] + a[1] + ... + a[n - 1] by one block of THREADS: thread t folds the run [t * per, (t + 1) * per) in order, thread 0
// the run totals in thread order; the result is valid in thread 0.  The leading barrier lets one red[THREADS] serve
// several calls back to back.
template <int THREADS>
__device__ __forceinline__ double ordered_sum(const double* __restrict__ a, size_t n, double* red) {
#pragma clang fp contract(off)
  const size_t per = (n + THREADS - 1) / THREADS;
  const size_t lo = threadIdx.x * per, hi = lo + per < n ? lo + per : n;
  double s = 0.0;
  for (size_t i = lo; i < hi; ++i) s += a[i];
  __syncthreads();
  red[threadIdx.x] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < THREADS; ++k) t += red[k];
  return t;
}

// mean over the Bl rows of mu / lv (row stride ld) of -1/2 sum_d (1 + l - e^l - m^2) by one block of 1024 threads: the
// arithmetic of kl_loss_fwd_kernel, fp32 inside a row and fp64 across rows.  Wave w takes the rows w, w + 16, ...; thread 0
// adds the 16 wave totals klw[16] in wave order; the result is valid in thread 0.
__device__ __forceinline__ double mean_kl_rows(const float* __restrict__ mu, const float* __restrict__ lv, size_t ld, int Bl,
                                               int D, double* klw) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int j = w; j < Bl; j += 16) {
    float a = 0.f;
    for (int l = lane; l < D; l += 64) {
      const float v = lv[(size_t)j * ld + l], mm = mu[(size_t)j * ld + l];
      a += 1.f + v - expf(v) - mm * mm;
    }
    acc += (double)(-0.5f * wave_sum(a));
  }
  if (lane == 0) klw[w] = acc;
  __syncthreads();
  double kl = 0.0;
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += klw[k];
    kl = t / (double)Bl;
  }
  return kl;
}

// One element of a diagonal Gaussian posterior (mean m, log-variance l, draw n) in fp64: the reparameterised sample, the
// term of -2 KL(q || N(0, 1)), and the gradient in m and in l of  g * sample + k * (-1/2 term)  -- g the sample's upstream
// gradient, k the coefficient of the KL.
__device__ __forceinline__ double posterior_sample(double m, double l, double n) {
#pragma clang fp contract(off)
  return m + n * exp(0.5 * l);
}
__device__ __forceinline__ double posterior_kl_term(double m, double l) {
#pragma clang fp contract(off)
  return 1.0 + l - m * m - exp(l);
}
__device__ __forceinline__ double posterior_dmu(double g, double m, double k) {
#pragma clang fp contract(off)
  return g + k * m;
}
__device__ __forceinline__ double posterior_dlv(double g, double n, double l, double k) {
#pragma clang fp contract(off)
  return 0.5 * exp(0.5 * l) * (g * n) + k * (0.5 * (exp(l) - 1.0));
}

// ---- host side -------------------------------------------------------------------------------------------------------
// blocks of a kernel that takes rows_per_block rows a trip: at most max_blocks, the rest is walked by the stride
inline int row_grid(int rows, int rows_per_block, int max_blocks) {
  const int blocks = cdiv(rows, rows_per_block);
  return blocks < max_blocks ? blocks : max_blocks;
}

}  // namespace itcv
