// Log density of a sample under a whole dataset's aggregate posterior q(z) = sum_i w_i q(z | x_i), and under the
// product of its marginals: the two logsumexps over ALL N components that the MI / TC / dimension-wise-KL decomposition
// of the aggregate KL needs (the beta-TC-VAE paper's evaluation; the minibatch form is latent.hip's itcv_tc_fwd).
//
//   lp[j,i,l] = max(log N(z_jl; mu_il, exp(lv_il)), -50)              (ops.py:24-29: variance of component i, clamp per
//   lse[j,l]  = logsumexp_i(logw_i + lp[j,i,l])                         element inside the sum over l)
//   logqz[j]  = logsumexp_i(logw_i + sum_l lp[j,i,l])
//
// S * N * D exponentials and nothing of size S x N anywhere: a streaming kernel.
//   * A block owns a tile of rows (each of its four waves R rows, held in registers with their running (max, sum)
//     pairs) and one slice of the component range, which it streams through LDS in chunks.  A staged component element
//     is the float4 {mu, a, c, w} with  lp * log2(e) = max(a * d^2 + c, floor),  a = -0.5 log2(e) exp(-lv),
//     c = -0.5 log2(e) (lv + log 2 pi),  w = logw * log2(e):  exp(-lv) is evaluated once per component per block, and
//     every staged value is used by all 4 R rows of the block.  The next chunk's global loads are in flight (in
//     registers) while the current chunk is consumed.
//   * Everything runs in base 2, so the one transcendental per element is a bare v_exp_f32.  The running maximum costs
//     no second one:  e = 2^-|v - m|  serves both cases,  s = v > m ? s * e + 1 : s + e  (a rescale and an addition are
//     the same exponential with the roles swapped); no branch, so a wave never pays both sides.
//   * Lanes: for D <= 64 a wave holds 64 / P components at once, P = next_pow2(D) lanes each (lane = g * P + l), and
//     sum_l lp is a DPP reduction inside the P lanes; a lane with l >= D stages a = c = 0 and so adds exactly 0.  For
//     D > 64 the lanes run over l with DL = ceil(D / 64) values per lane and one component per wave step.  The joint
//     term's own exponential is issued once per wave step for all R rows: lane l of a group takes row l's sum (P >= R;
//     the three narrowest tiers P < 8 do it per row).
//   * Each slice leaves one (max, sum) partial per (row, l) and one per row; a second kernel merges them in slice
//     order.  No atomics, every order fixed: bitwise reproducible, and for a given slice count a row's results depend
//     on nothing but that row and the components (its place in a tile or a wave changes no operation's operands).
#include <math.h>

#include "common.h"

namespace itcv {

constexpr float kAggLog2e = 1.4426950408889634f;
constexpr float kAggLn2 = 0.6931471805599453f;
constexpr float kAggLog2Pi = 1.8378770664093453f;
constexpr float kAggFloor2 = -50.f * 1.4426950408889634f;   // the -50 clamp of ops.py:29 in base 2
constexpr int kAggDMax = 512;
constexpr int kAggMaxSplits = 1024;
constexpr int kAggTargetBlocks = 512;     // two blocks on each of the 256 CUs

template <int CTRL>
__device__ __forceinline__ float agg_dpp(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
// sum over the P lanes of a lane group (P a power of two, groups aligned); every lane of the group gets the same bits
template <int P>
__device__ __forceinline__ float group_sum(float x) {
  if constexpr (P >= 2) x += agg_dpp<0xB1>(x);    // quad_perm [1,0,3,2]
  if constexpr (P >= 4) x += agg_dpp<0x4E>(x);    // quad_perm [2,3,0,1]
  if constexpr (P >= 8) x += agg_dpp<0x141>(x);   // row_half_mirror: the other quad of the 8
  if constexpr (P >= 16) x += agg_dpp<0x140>(x);  // row_mirror: the other half of the 16
  if constexpr (P >= 32) x += __shfl_xor(x, 16, 64);
  if constexpr (P >= 64) x += __shfl_xor(x, 32, 64);
  return x;
}

// online base-2 logsumexp: (m, s) <- (m, s) + 2^v with ONE exponential; `pad`: v is the -inf of a component that does
// not exist (m may still be -inf then, and -inf - -inf is no number)
__device__ __forceinline__ void lse_push(float v, bool pad, float& m, float& s) {
  float e = __builtin_amdgcn_exp2f(-fabsf(v - m));
  e = pad ? 0.f : e;
  s = v > m ? fmaf(s, e, 1.f) : s + e;
  m = fmaxf(m, v);
}
// (m, s) <- (m, s) + (mo, so); either side may be empty (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float mo, float so) {
  const float M = fmaxf(m, mo);
  const float a = m == -INFINITY ? 0.f : s * exp2f(m - M);
  const float b = mo == -INFINITY ? 0.f : so * exp2f(mo - M);
  m = M, s = a + b;
}

struct AggPlan {
  int P, DL, R, CC;      // lanes per component, values of l per lane, rows per wave, components per LDS chunk
  int tiles, splits;     // grid: row tiles x component slices
  int64_t len;           // components per slice
};

__host__ __device__ constexpr int agg_chunk_elems(int DL) { return DL >= 4 ? 2048 : 1024; }   // float4 each: 16 / 32 KB

// splits <= 0: the library's choice -- enough slices for kAggTargetBlocks blocks, none shorter than four LDS chunks
static int agg_plan(int64_t S, int64_t N, int D, int splits, AggPlan* p) {
  if (D < 1 || D > kAggDMax) return fail("%s: latent size %lld outside [1, 512]", "itcv_aggregate_logdensity", D);
  if (S < 1 || N < 1) return fail("%s: needs at least one sample and one component", "itcv_aggregate_logdensity");
  int P = 1;
  while (P < D && P < 64) P *= 2;
  p->P = P;
  p->DL = D <= 64 ? 1 : (D <= 128 ? 2 : (D <= 256 ? 4 : 8));
  p->R = p->DL <= 2 ? 8 : (p->DL == 4 ? 4 : 2);
  p->CC = agg_chunk_elems(p->DL) / (P * p->DL);
  const int64_t tiles = (S + 4 * p->R - 1) / (4 * p->R);
  if (tiles > 0x7fffffffll) return fail("%s: too many samples for one call", "itcv_aggregate_logdensity");
  p->tiles = (int)tiles;
  int64_t sp = splits;
  if (sp <= 0) {
    const int64_t want = (kAggTargetBlocks + tiles - 1) / tiles, cap = N / (4 * p->CC);
    sp = want < cap ? want : cap;
  }
  sp = sp < 1 ? 1 : (sp > kAggMaxSplits ? kAggMaxSplits : sp);
  sp = sp > N ? N : sp;
  p->len = (N + sp - 1) / sp;
  p->splits = (int)((N + p->len - 1) / p->len);   // no empty slice
  return 0;
}

template <int P, int DL, int R>
__global__ __launch_bounds__(256) void agg_part_kernel(const float* __restrict__ z, const float* __restrict__ mu,
                                                       const float* __restrict__ logvar, const float* __restrict__ logw,
                                                       float lw_uniform, float* __restrict__ pm, float* __restrict__ ps,
                                                       int64_t S, int64_t N, int D, int splits, int64_t len) {
  constexpr int G = 64 / P;                 // components per wave step
  constexpr int EPC = P * DL;               // staged elements per component
  constexpr int CE = agg_chunk_elems(DL);   // staged elements per chunk
  constexpr int CC = CE / EPC;              // components per chunk
  constexpr int EPT = CE / 256;             // staged elements per thread
  constexpr bool DIST = P >= R;             // the joint term of row r is kept by lane r of each group
  constexpr int NJ = DIST ? 1 : R;
  static_assert(DL == 1 || P == 64, "several values per lane only when the lanes run over l");
  __shared__ float4 comp[CE];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane / P, gl = lane & (P - 1);
  const int sp = blockIdx.y;
  const int64_t j0 = ((int64_t)blockIdx.x * 4 + wid) * R;
  const int64_t i_begin = (int64_t)sp * len, i_end = i_begin + len < N ? i_begin + len : N;

  float zr[R][DL], m[R][DL], s[R][DL], jm[NJ], js[NJ];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int k = 0; k < DL; ++k) {
      const int l = gl + P * k;
      zr[r][k] = (j0 + r < S && l < D) ? z[(size_t)(j0 + r) * D + l] : 0.f;
      m[r][k] = -INFINITY, s[r][k] = 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < NJ; ++r) jm[r] = -INFINITY, js[r] = 0.f;

  // the chunk in flight: raw (mu, logvar, logw) of this thread's staged elements
  float fmu[EPT], flv[EPT], flw[EPT];
  auto fetch = [&](int64_t c0) {
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
      const int e = tid + 256 * u, il = e / EPC, l = e % EPC;
      const int64_t i = c0 + il;
      fmu[u] = 0.f, flv[u] = 0.f, flw[u] = -INFINITY;
      if (i < i_end) {
        flw[u] = logw ? logw[i] * kAggLog2e : lw_uniform;
        if (l < D) fmu[u] = mu[(size_t)i * D + l], flv[u] = logvar[(size_t)i * D + l];
      }
    }
  };
  fetch(i_begin);
  for (int64_t c0 = i_begin; c0 < i_end; c0 += CC) {
    __syncthreads();                        // the previous chunk has been consumed
#pragma unroll
    for (int u = 0; u < EPT; ++u) {
      const int e = tid + 256 * u, l = e % EPC;
      const bool live = l < D && flw[u] != -INFINITY;
      comp[e] = make_float4(fmu[u], live ? -0.5f * kAggLog2e * expf(-flv[u]) : 0.f,
                            live ? -0.5f * kAggLog2e * (flv[u] + kAggLog2Pi) : 0.f, flw[u]);
    }
    __syncthreads();
    if (c0 + CC < i_end) fetch(c0 + CC);
    const int64_t left = i_end - c0;
    const int steps = left >= CC ? CC / G : (int)((left + G - 1) / G);    // block-uniform
    for (int t = 0; t < steps; ++t) {
      const int il = t * G + g;
      float4 cv[DL];
#pragma unroll
      for (int k = 0; k < DL; ++k) cv[k] = comp[il * EPC + k * P + gl];
      const float lw = cv[0].w;
      const bool pad = lw == -INFINITY;
      float q[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < DL; ++k) {
          const float d = zr[r][k] - cv[k].x;
          const float lp = fmaxf(fmaf(d * d, cv[k].y, cv[k].z), kAggFloor2);
          acc += lp;
          lse_push(lp + lw, pad, m[r][k], s[r][k]);
        }
        q[r] = group_sum<P>(acc);
      }
      if constexpr (DIST) {
        float t0 = q[0];
#pragma unroll
        for (int r = 1; r < R; ++r) t0 = gl == r ? q[r] : t0;
        lse_push(t0 + lw, pad, jm[0], js[0]);
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) lse_push(q[r] + lw, pad, jm[r], js[r]);
      }
    }
  }

  // the lane groups of a wave saw different components: fold them (fixed butterfly), group 0 writes
#pragma unroll
  for (int o = P; o < 64; o *= 2) {
#pragma unroll
    for (int r = 0; r < R; ++r)
      lse_merge(m[r][0], s[r][0], __shfl_xor(m[r][0], o, 64), __shfl_xor(s[r][0], o, 64));   // G > 1 only when DL == 1
#pragma unroll
    for (int r = 0; r < NJ; ++r) lse_merge(jm[r], js[r], __shfl_xor(jm[r], o, 64), __shfl_xor(js[r], o, 64));
  }
  if (g != 0) return;
  const size_t W = (size_t)D + 1;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (j0 + r >= S) continue;
    const size_t base = ((size_t)(j0 + r) * splits + sp) * W;
#pragma unroll
    for (int k = 0; k < DL; ++k) {
      const int l = gl + P * k;
      if (l < D) pm[base + l] = m[r][k], ps[base + l] = s[r][k];
    }
    if constexpr (DIST) {
      if (gl == r) pm[base + D] = jm[0], ps[base + D] = js[0];
    } else {
      if (gl == 0) pm[base + D] = jm[r], ps[base + D] = js[r];
    }
  }
}

// slice partials -> lse[j][l] (l < D) and logqz[j] (l == D), in slice order, back in natural units
__global__ __launch_bounds__(256) void agg_merge_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                        float* __restrict__ logqz, float* __restrict__ lse, int64_t S,
                                                        int D, int splits) {
  const size_t W = (size_t)D + 1, total = (size_t)S * W;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t j = e / W, l = e - j * W;
    const float* a = pm + j * splits * W + l;
    const float* b = ps + j * splits * W + l;
    float M = -INFINITY;
    for (int k = 0; k < splits; ++k) M = fmaxf(M, a[(size_t)k * W]);
    float sum = 0.f;
    for (int k = 0; k < splits; ++k) sum += b[(size_t)k * W] * exp2f(a[(size_t)k * W] - M);
    const float r = kAggLn2 * (M + log2f(sum));
    if (l == (size_t)D) logqz[j] = r;
    else lse[j * D + l] = r;
  }
}

}  // namespace itcv

using namespace itcv;

extern "C" {

size_t itcv_aggregate_workspace(int64_t S, int64_t N, int D, int splits) {
  AggPlan p;
  if (agg_plan(S, N, D, splits, &p)) return 0;
  return (size_t)2 * (size_t)S * p.splits * ((size_t)D + 1) * sizeof(float);
}

int itcv_aggregate_logdensity(const float* z, const float* mu, const float* logvar, const float* logw, float* logqz,
                              float* lse, int64_t S, int64_t N, int D, int splits, void* ws, size_t ws_bytes,
                              void* stream) {
  AggPlan p;
  if (int e = agg_plan(S, N, D, splits, &p)) return e;
  ITCV_REQUIRE(z && mu && logvar && logqz && lse, "itcv_aggregate_logdensity");
  ITCV_REQUIRE(ws && ws_bytes >= itcv_aggregate_workspace(S, N, D, splits), "itcv_aggregate_logdensity(workspace)");
  float* pm = static_cast<float*>(ws);
  float* ps = pm + (size_t)S * p.splits * ((size_t)D + 1);
  const float lwu = (float)(-log2((double)N));
  const dim3 grid(p.tiles, p.splits), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);   // (`S` is the sample count here)
#define ITCV_AGG(P, DL, R)                                                                                          \
  hipLaunchKernelGGL((agg_part_kernel<P, DL, R>), grid, block, 0, st, z, mu, logvar, logw, lwu, pm, ps, S, N, D, \
                     p.splits, p.len)
  if (p.DL == 8) ITCV_AGG(64, 8, 2);
  else if (p.DL == 4) ITCV_AGG(64, 4, 4);
  else if (p.DL == 2) ITCV_AGG(64, 2, 8);
  else if (p.P == 64) ITCV_AGG(64, 1, 8);
  else if (p.P == 32) ITCV_AGG(32, 1, 8);
  else if (p.P == 16) ITCV_AGG(16, 1, 8);
  else if (p.P == 8) ITCV_AGG(8, 1, 8);
  else if (p.P == 4) ITCV_AGG(4, 1, 8);
  else if (p.P == 2) ITCV_AGG(2, 1, 8);
  else ITCV_AGG(1, 1, 8);
#undef ITCV_AGG
  ITCV_CHECK_LAUNCH("itcv_aggregate_logdensity(partials)");
  const size_t total = (size_t)S * ((size_t)D + 1);
  hipLaunchKernelGGL(agg_merge_kernel, dim3(stream_grid(total, 1)), block, 0, st, pm, ps, logqz, lse, S, D, p.splits);
  ITCV_CHECK_LAUNCH("itcv_aggregate_logdensity(merge)");
  return 0;
}

}  // extern "C"
