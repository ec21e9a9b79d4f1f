// Shared helpers for libitcv_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/itcv_hip.h"

namespace itcv {

extern thread_local char g_err[512];

inline int fail(const char* fmt, const char* a = "", long long b = 0, long long c = 0) {
  snprintf(g_err, sizeof(g_err), fmt, a, b, c);
  return 1;
}

#define ITCV_CHECK_LAUNCH(name)                                                        \
  do {                                                                                 \
    hipError_t e_ = hipGetLastError();                                                 \
    if (e_ != hipSuccess) return itcv::fail("%s: launch failed: %lld", name, (long long)e_); \
  } while (0)

#define ITCV_REQUIRE(cond, name)                                              \
  do {                                                                        \
    if (!(cond)) return itcv::fail("%s: requirement failed: " #cond, name);   \
  } while (0)

inline bool finite(double x) { return fabs(x) <= DBL_MAX; }   // false for NaN too

// The refusals: each returns 0 when the call may go on; otherwise it leaves the message and returns fail()'s 1, so a chain
// of them joined with || stops at the first failure.
inline int need_pointers(const char* name, bool all) { return all ? 0 : fail("%s: a required pointer is NULL", name); }
// `what` names the dimension with a %lld for its value ("B = %lld pairs"), `range` words lo..hi ("1..2^30")
inline int need_dim(const char* name, const char* what, long long v, long long lo, long long hi, const char* range) {
  if (v >= lo && v <= hi) return 0;
  char fmt[128];
  snprintf(fmt, sizeof(fmt), "%%s: %s is outside %s", what, range);
  return fail(fmt, name, v);
}
// `whose` is "a" or the operand's name ("mu's"), `dim` the name of the width the stride has to cover
inline int need_stride(const char* name, const char* whose, size_t ld, const char* dim, long long width) {
  if (ld >= (size_t)width) return 0;
  char fmt[128];
  snprintf(fmt, sizeof(fmt), "%%s: %s row stride of %%lld is below %s = %%lld", whose, dim);
  return fail(fmt, name, (long long)ld, width);
}

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

__host__ __device__ inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t cdivz(size_t a, size_t b) { return (a + b - 1) / b; }
inline size_t align_up(size_t a, size_t b) { return cdivz(a, b) * b; }

constexpr int kWave = 64;

// blocks of 256 threads for a grid-stride streaming kernel over n items, `per_thread` items a thread: at most 2048
// (8 blocks on each of the 256 CUs), the rest of the range is walked by the stride
inline int stream_grid(size_t n, int per_thread) {
  size_t b = cdivz(cdivz(n, per_thread), 256);
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// ---- wave / block reductions (wave = 64 lanes) -------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    T u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    T u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
// block-wide sum; result valid in every thread.  `scratch` holds >= blockDim/64 elements.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  T r = 0;
  for (int i = 0; i < nw; ++i) r += scratch[i];  // fixed order: deterministic
  return r;
}

// 128-bit buffer resource for raw buffer loads with hardware bounds checking: an offset
// >= num_bytes returns 0, which is how padding / tile tails are zero-filled without branches.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint32_t num_bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, num_bytes, 0x00020000);
}
__device__ __forceinline__ float buf_load(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
constexpr uint32_t kOOB = 0xFFFFFFFFu;

// ---- stream policy (option "stream_nt", include/itcv_hip.h: one ITCV_STREAM_NT_* bit per kernel family) ----------------
// A tensor a kernel reads for the last time, or writes for a reader more than a cache's worth of traffic away, is loaded /
// stored non-temporally (`nt` on the instruction): it moves at the same rate and is not kept in front of the lines the
// next kernel asks for.  Hand-offs (the next kernel reads the bytes) always stay plain.  NT is a template argument
// reached through pick<2>(stream_nt(bit)); a policy bit changes no value, so both forms are bitwise equal (tests).
extern int g_stream_nt;   // abi.hip
inline int stream_nt(int bit) { return (g_stream_nt & bit) ? 1 : 0; }
typedef float f32x4n __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float* p) {
  if constexpr (NT) {
    const f32x4n v = __builtin_nontemporal_load(reinterpret_cast<const f32x4n*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const float4*>(p);
  }
}
template <bool NT>
__device__ __forceinline__ float2 ld2(const float* p) {
  typedef float f32x2n __attribute__((ext_vector_type(2)));
  if constexpr (NT) {
    const f32x2n v = __builtin_nontemporal_load(reinterpret_cast<const f32x2n*>(p));
    return make_float2(v.x, v.y);
  } else {
    return *reinterpret_cast<const float2*>(p);
  }
}
template <bool NT>
__device__ __forceinline__ float ld1(const float* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, const float4& v) {
  if constexpr (NT) {
    const f32x4n t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4n*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}
template <bool NT>
__device__ __forceinline__ void st1(float* p, float v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// init + p[0] + p[stride] + ... (n terms, ascending: a fixed order, bitwise reproducible) with the loads of 8 terms in
// flight -- a plain `for (k) s += p[k*stride]` is one exposed memory round trip per term.
template <typename T>
__device__ __forceinline__ T fold_strided(T init, const T* __restrict__ p, size_t stride, int n) {
  T s = init;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(k + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k + 2 <= n; k += 2) {
    const T v0 = p[(size_t)k * stride], v1 = p[(size_t)(k + 1) * stride];
    s += v0;
    s += v1;
  }
  for (; k < n; ++k) s += p[(size_t)k * stride];
  return s;
}

// ---- split operands: x = sum_p plane_p(x); 8 values -> one 16-byte chunk per plane -------------------------------
// bf16 planes (formats 2 and 3): each plane is the bf16 rounding of the remaining residual.
// fp16 planes (format ITCV_PLANES_F16X2, "f16x3"): hi = fp16(S*x), lo = fp16(S*x - hi) with a power-of-two scale S per
// tensor: 22 significand bits in two planes, so the same THREE matrix-core products as bf16x3 (hi*lo + lo*hi + hi*hi)
// reach ~2^-21 per product -- fp32 class -- where two bf16 planes reach 2^-16.  fp16's narrow exponent is what the scale is
// for: S maps the tensor's magnitude bound just under 2^15, and the fp16 matrix cores keep subnormal inputs (measured on
// gfx950: tools/f16_probe.hip), so values far below the bound degrade gracefully (absolute error 2^-25 / S) instead of
// flushing.  The product of two such operands comes out scaled by Sa*Sb; the consumer's epilogue multiplies by the exact
// inverse.  Every scaled tensor carries its {S, 1/S} next to the data (ScaleRec, "trailer" of a planes buffer).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct ScaleRec {   // 16 bytes: lives behind the last plane of an fp16 planes buffer
  float scale, inv;
  float pad[2];
};
constexpr int kWeightScaleLog2 = 8;   // packed fp16 weights are stored times 2^8 (|w| < 255 representable; typical |w| ~ 0.02 -> 5)

// power-of-two scale that maps `bound` (>= every |value| of the tensor) into [2^14, 2^15); 1 for 0 / inf / nan bounds
__host__ __device__ inline float scale_for_bound(float bound) {
  if (!(bound > 0.f) || !(bound < 3.0e38f)) return 1.f;
  int e;
  (void)frexpf(bound, &e);          // bound = m * 2^e, m in [0.5, 1)  =>  bound < 2^e
  int k = 15 - e;                   // bound * 2^k < 2^15
  k = k > 126 ? 126 : (k < -126 ? -126 : k);
  return ldexpf(1.f, k);
}

template <int NS, bool F16 = false>
__device__ __forceinline__ void split8(const float (&v)[8], u32x4 (&out)[NS], float scale = 1.f) {
  if constexpr (F16) {
    static_assert(NS == 2, "fp16 planes come in pairs");
    f16x8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float r = v[j] * scale;
      const _Float16 h = (_Float16)r;
      hi[j] = h;
      lo[j] = (_Float16)(r - (float)h);
    }
    out[0] = __builtin_bit_cast(u32x4, hi), out[1] = __builtin_bit_cast(u32x4, lo);
  } else {
    bf16x8 pl[NS];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float r = v[j];
#pragma unroll
      for (int p = 0; p < NS; ++p) {
        const __bf16 b = (__bf16)r;
        pl[p][j] = b;
        r -= (float)b;
      }
    }
#pragma unroll
    for (int p = 0; p < NS; ++p) out[p] = __builtin_bit_cast(u32x4, pl[p]);
  }
}

// matrix-core products on 16-byte fragments (8 x 16-bit) of either element type
typedef float mm_f32x4 __attribute__((ext_vector_type(4)));
typedef float mm_f32x16 __attribute__((ext_vector_type(16)));
template <bool F16>
__device__ __forceinline__ mm_f32x4 mma16x16x32(bf16x8 a, bf16x8 b, mm_f32x4 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ mm_f32x16 mma32x32x16(bf16x8 a, bf16x8 b, mm_f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// 1/S of a scale record as a wave-uniform value in a scalar register: loaded ONCE where this is called (left as a plain
// load the compiler re-issues it next to every use when it cannot prove that the epilogue's stores do not alias it)
__device__ __forceinline__ float inv_scale_of(const ScaleRec* r) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, r->inv)));
}

// max of n non-negative floats at p, by one wave (all 64 lanes call; result in every lane)
__device__ __forceinline__ float wave_absmax_of(const float* __restrict__ p, int n) {
  float m = 0.f;
  for (int i = threadIdx.x & 63; i < n; i += 64) m = fmaxf(m, p[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}
constexpr int kAbsmaxParts = 256;   // block maxima written by itcv_absmax (one float each)

// ---- optional per-launch timing of the GEMM-class kernels (bench.py's roofline leg) ------------
// When enabled, a HIP event pair is recorded on the launch stream immediately around the MAIN kernel
// of a conv call (not its split-K reduce), tagged with the kernel family / template parameters and the
// algorithmic FLOP of the launch.  Off by default; never used under graph capture.
// Which kernel family a record belongs to.  The values are part of the record's code, which hipvae/functional.py decodes
// by number (LaunchProfile.KINDS): keep the two in step.
enum ProfKind : int {
  kProfFwd = 0,             // conv_fwd_kernel
  kProfFwdB = 1,            // conv_fwd_bf16s_ws_kernel
  kProfWgrad = 2,           // conv_wgrad_kernel
  kProfWgradB = 3,          // conv_wgrad_bf16s_kernel
  kProfSmallCout = 4,       // conv_small_cout_kernel
  kProfSmallCin = 5,        // conv_small_cin_kernel
  kProfFwdP = 6,            // conv_fwd_bf16p_kernel
  kProfWgradP = 7,          // conv_wgrad_bf16p_kernel
  kProfFwdBand = 8,         // conv_fwd_bf16p2_kernel
  kProfFwdBandPersist = 9,  // conv_fwd_bf16p3_kernel
  kProfSmallCoutP = 10,     // conv_small_cout_planes_kernel
  kProfSmallCinMfma = 11,   // conv_small_cin_mfma_kernel
  kProfWgrad5 = 12,         // conv_wgrad5_planes_kernel
  kProfBnFwd = 13,          // bn_act_fwd_planes_kernel
  kProfBnBwd = 14,          // bn_bwd_apply_planes
};
struct ProfScope {
  hipStream_t st;
  int slot;
  ProfScope(hipStream_t stream, ProfKind kind, int ks, int bm, int up2, int ns, double flop);
  ~ProfScope();
};
// Event pair of the innermost live ProfScope (null when not profiling).  launch_timed() hands it to
// hipExtLaunchKernelGGL, which stamps the events at the kernel's own start and end: the record is the kernel's
// execution time (what rocprofv3 reports), free of the dispatch latency a hipEventRecord pair would include
// whenever the stream runs dry.
extern thread_local hipEvent_t g_prof_start, g_prof_stop;

template <typename K, typename... Args>
inline void launch_timed(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  if (g_prof_start) {
    hipExtLaunchKernelGGL(kernel, grid, block, lds, st, g_prof_start, g_prof_stop, 0, args...);
    g_prof_start = nullptr;   // one kernel per scope: a second launch in the same scope is not part of the record
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  }
}

// Dynamic LDS above the default limit needs the kernel's attribute raised first: done once per kernel, again only when a
// later call asks for more (the band kernels' LDS size varies per call).  The state is keyed on the kernel VALUE: a static
// inside `template <typename K>` would be shared by every instantiation with the same parameter list (one pointer type).
template <auto Kernel, typename... Args>
inline void launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
  static size_t have = 0;
  if (have < lds) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    have = lds;
  }
  launch_timed(Kernel, grid, block, lds, st, args...);
}

// ---- run-time switches -> template arguments ----------------------------------------------------
// The one place where they turn: pick<N>(v, f) calls f(std::integral_constant<int, v>) for v in [0, N) (0 for anything
// else); pick_of<A, B, ..., Z>(v, f) calls it with the listed value equal to v (Z for anything else).  Nested for several
// switches; an `if constexpr` inside the innermost callable keeps combinations that have no kernel from being instantiated.
template <int N, typename F>
inline void pick(int v, F&& f) {
  if constexpr (N > 1) {
    if (v == N - 1) return f(std::integral_constant<int, N - 1>{});
    return pick<N - 1>(v, f);
  } else {
    f(std::integral_constant<int, 0>{});
  }
}
template <int V0, int... Vs, typename F>
inline void pick_of(int v, F&& f) {
  if constexpr (sizeof...(Vs) > 0) {
    if (v != V0) return pick_of<Vs...>(v, f);
  }
  f(std::integral_constant<int, V0>{});
}

}  // namespace itcv
