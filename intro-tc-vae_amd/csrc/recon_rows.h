// The per-element reconstruction errors and the per-row slice sum shared by the reconstruction kernels of loss_optim.hip
// and the broadcast rows of iwae.hip.  One body, so that both sum a row in the same order and give the same bits.
#pragma once
#include <math.h>

#include "common.h"

namespace itcv {

template <int LT>
__device__ __forceinline__ float rec_err(float r, float t) {
  if (LT == ITCV_LOSS_MSE) {
    const float d = r - t;
    return d * d;
  }
  if (LT == ITCV_LOSS_L1) return fabsf(r - t);
  // F.binary_cross_entropy clamps both log terms at -100
  return -(t * fmaxf(logf(r), -100.f) + (1.f - t) * fmaxf(logf(1.f - r), -100.f));
}
template <int LT>
__device__ __forceinline__ float rec_derr(float r, float t) {
  if (LT == ITCV_LOSS_MSE) return 2.f * (r - t);
  if (LT == ITCV_LOSS_L1) return r > t ? 1.f : (r < t ? -1.f : 0.f);
  return (r - t) / fmaxf((1.f - r) * r, 1e-12f);  // ATen binary_cross_entropy_backward
}

// slices of a row of P elements (B rows in all): enough blocks to fill the device, none shorter than 2048 elements
static inline int recon_splits(int B, size_t P) {
  int s = cdiv(1024, B);
  const size_t maxs = cdivz(P, 2048);
  if ((size_t)s > maxs) s = (int)maxs;
  return s < 1 ? 1 : s;
}
// [beg, end) of slice s of `splits`
__device__ __forceinline__ void recon_slice(size_t P, int splits, int s, size_t& beg, size_t& end) {
  const size_t chunk = ((P + splits - 1) / splits + 3) & ~(size_t)3;
  beg = (size_t)s * chunk;
  end = beg + chunk < P ? beg + chunk : P;
}
// this thread's share of sum_{i in [beg, end)} err(rr[i], xr[i]), by a block of 256 threads.  vec4: xr and rr start on a
// 16-byte boundary and P % 4 == 0, so the slices can be read as float4
template <int LT>
__device__ __forceinline__ double recon_slice_acc(const float* __restrict__ xr, const float* __restrict__ rr, size_t beg,
                                                  size_t end, int vec4) {
  double acc = 0.0;
  if (vec4) {
    for (size_t i = beg + (size_t)threadIdx.x * 4; i < end; i += 1024) {
      const float4 t = *reinterpret_cast<const float4*>(xr + i);
      const float4 r = *reinterpret_cast<const float4*>(rr + i);
      acc += (double)(rec_err<LT>(r.x, t.x) + rec_err<LT>(r.y, t.y)) +
             (double)(rec_err<LT>(r.z, t.z) + rec_err<LT>(r.w, t.w));
    }
  } else {
    for (size_t i = beg + threadIdx.x; i < end; i += 256) acc += (double)rec_err<LT>(rr[i], xr[i]);
  }
  return acc;
}

}  // namespace itcv
