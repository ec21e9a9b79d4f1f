// Device-resident image tables: "look up these images" as one launch (dataset.py:75-81,141-147 -- Image.fromarray +
// ToTensor per image on the host -- and the LatentGenerator / FactorSampler lookups built on it).
// The table is planar uint8 in HBM; a gather reads 1 byte and writes 4 per element, so it is HBM-bound.  The value rule
// (include/itcv_hip.h) is the correctly rounded fp32 division by 255, which `/` is here: hipcc divides fp32 to IEEE
// rounding unless asked otherwise, and no file of this library asks.
#include "common.h"

namespace itcv {

__device__ __forceinline__ float unit_of_byte(unsigned int b) { return (float)b / 255.0f; }

__device__ __forceinline__ float4 unit_of_word(unsigned int w) {
  return make_float4(unit_of_byte(w & 0xffu), unit_of_byte((w >> 8) & 0xffu), unit_of_byte((w >> 16) & 0xffu),
                     unit_of_byte(w >> 24));
}

// W % 16 == 0: an aligned 16-byte chunk never straddles a row.  One thread takes chunk c = j * cpi + k (image j of the
// batch, chunk k of the image) with one 128-bit load and writes it as four float4.  The grid-stride walk keeps (j, k)
// by addition -- (sj, sk) is the stride split the same way by the host -- so the loop holds no 64-bit division.
__global__ __launch_bounds__(256) void gather_u8_chunks_kernel(const unsigned char* __restrict__ table, long long num_images,
                                                               unsigned int cpi, unsigned int cpr,
                                                               const long long* __restrict__ idx,
                                                               const unsigned char* __restrict__ flip,
                                                               float* __restrict__ out, int* __restrict__ flags, int n,
                                                               unsigned int sj, unsigned int sk) {
  const unsigned int t = blockIdx.x * 256u + threadIdx.x;      // < 2048 * 256
  unsigned int j = t / cpi, k = t - j * cpi;
  for (; j < (unsigned int)n; j += sj, k += sk) {
    if (k >= cpi) k -= cpi, ++j;
    if (j >= (unsigned int)n) break;
    const long long id = idx[j];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (id < 0 || id >= num_images) {
      if (k == 0) atomicOr(flags, 1);
    } else {
      const bool mirrored = flip != nullptr && flip[j] != 0;
      unsigned int src = k;
      if (mirrored) {                                          // the mirrored chunk of the same row
        const unsigned int row = k / cpr;
        src = row * cpr + (cpr - 1u - (k - row * cpr));
      }
      v = *reinterpret_cast<const uint4*>(table + ((size_t)id * cpi + src) * 16u);
      if (mirrored)                                            // its 16 bytes in reverse order
        v = make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
    }
    float4* o = reinterpret_cast<float4*>(out) + ((size_t)j * cpi + k) * 4u;
    o[0] = unit_of_word(v.x);
    o[1] = unit_of_word(v.y);
    o[2] = unit_of_word(v.z);
    o[3] = unit_of_word(v.w);
  }
}

// every other shape: one output element per thread and iteration
__global__ __launch_bounds__(256) void gather_u8_scalar_kernel(const unsigned char* __restrict__ table, long long num_images,
                                                               size_t image_bytes, int W, const long long* __restrict__ idx,
                                                               const unsigned char* __restrict__ flip,
                                                               float* __restrict__ out, int* __restrict__ flags, size_t total) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
    const size_t j = i / image_bytes, e = i - j * image_bytes;
    const long long id = idx[j];
    float r = 0.f;
    if (id < 0 || id >= num_images) {
      if (e == 0) atomicOr(flags, 1);
    } else {
      size_t src = e;
      if (flip != nullptr && flip[j] != 0) {
        const size_t row = e / (size_t)W;
        src = row * (size_t)W + ((size_t)W - 1u - (e - row * (size_t)W));
      }
      r = unit_of_byte(table[(size_t)id * image_bytes + src]);
    }
    out[i] = r;
  }
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_gather_u8(const unsigned char* table, long long num_images, int rows_per_image, int W, const long long* idx,
                   int n, const unsigned char* flip, float* out, int* flags, void* stream) {
  ITCV_REQUIRE(table && idx && out && flags, "itcv_gather_u8");
  ITCV_REQUIRE(num_images > 0 && rows_per_image > 0 && W > 0 && n > 0, "itcv_gather_u8");
  ITCV_REQUIRE((long long)rows_per_image * W < (1ll << 31), "itcv_gather_u8");
  const size_t image_bytes = (size_t)rows_per_image * (size_t)W;
  const size_t total = (size_t)n * image_bytes;
  const bool chunks = W % 16 == 0 && (reinterpret_cast<uintptr_t>(table) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  if (chunks) {
    const unsigned int cpi = (unsigned int)(image_bytes / 16), cpr = (unsigned int)(W / 16);
    const int blocks = stream_grid(total / 16, 1);
    const size_t stride = (size_t)blocks * 256u;
    hipLaunchKernelGGL(gather_u8_chunks_kernel, dim3(blocks), dim3(256), 0, S(stream), table, num_images, cpi, cpr, idx,
                       flip, out, flags, n, (unsigned int)(stride / cpi), (unsigned int)(stride % cpi));
  } else {
    hipLaunchKernelGGL(gather_u8_scalar_kernel, dim3(stream_grid(total, 1)), dim3(256), 0, S(stream), table, num_images,
                       image_bytes, W, idx, flip, out, flags, total);
  }
  ITCV_CHECK_LAUNCH("itcv_gather_u8");
  return 0;
}

}  // extern "C"
