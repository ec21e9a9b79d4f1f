// Fused optimiser updates over the flat fp32 buffers of a model half (hipvae/flat.py): torch.optim.Adam / AdamW
// (weight decay, amsgrad, maximize), SGD, Adagrad and RMSprop, each one streaming launch.  Plain Adam keeps its own
// kernel (loss_optim.hip, itcv_adam_step_dev).
//
// Every kernel repeats the arithmetic of the matching single-tensor update of torch/optim/*.py in the same order:
// Python-float hyper-parameters reach the tensor ops as fp32 scalars (cast once on the host), and the step-dependent
// scalars (bias corrections, Adagrad's clr, SGD's first step) are formed per thread in fp64 from the DEVICE step
// count, so a captured launch (hipGraph replay) advances them.  The step count is bumped by a second one-thread launch.
// Flags are template parameters; the only per-element branch is the optional `live` mask (one byte per float4, 0 for a
// parameter torch never sees a gradient for, which must stay untouched).
#include <math.h>

#include <type_traits>

#include "common.h"

// Roundings follow ATen's CPU kernels: Tensor.add(other, alpha) and lerp are one fused multiply-add there (vec::fmadd),
// every other op rounds on its own, so the compiler may not contract anything else.
#pragma clang fp contract(off)

namespace itcv {

// at::lerp (ATen/native/Lerp.h, lerp_vec): the two-sided form torch's exp_avg.lerp_(grad, w) evaluates
__device__ __forceinline__ float lerp_t(float s, float e, float w) {
  return fabsf(w) < 0.5f ? fmaf(w, e - s, s) : fmaf(w - 1.f, e - s, e);
}

struct AdamArgs {
  double lr, beta1, beta2;
  float one_m_b1, b2, one_m_b2, eps, wd, decay;
};
struct SgdArgs {
  float neg_lr, wd, momentum, one_m_damp;
};
struct AdagradArgs {
  double lr, lr_decay;
  float wd, eps;
};
struct RmspropArgs {
  float neg_lr, alpha, one_m_alpha, eps, wd, momentum;
};

// WD: 0 none, 1 L2 (grad += wd * p), 2 decoupled (p *= 1 - lr * wd)
template <int WD, bool AMSGRAD, bool MAXIMIZE>
__global__ __launch_bounds__(256) void adamx_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                    float4* __restrict__ m, float4* __restrict__ v,
                                                    float4* __restrict__ vmax, const uint8_t* __restrict__ live,
                                                    size_t n4, AdamArgs a, const int* __restrict__ step_dev) {
  const double step = (double)(step_dev[0] + 1);
  const double bc1 = 1.0 - pow(a.beta1, step), bc2 = 1.0 - pow(a.beta2, step);
  const float neg_step_size = (float)(-(a.lr / bc1)), bc2_sqrt = (float)sqrt(bc2);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    if (live && !live[i]) continue;
    float4 P = p[i], G = g[i], M = m[i], V = v[i], X;
    if (AMSGRAD) X = vmax[i];
    float* pp = &P.x;
    float* gp = &G.x;
    float* mp = &M.x;
    float* vp = &V.x;
    float* xp = &X.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk = MAXIMIZE ? -gp[k] : gp[k];
      if (WD == 2) pp[k] = pp[k] * a.decay;
      if (WD == 1) gk = fmaf(pp[k], a.wd, gk);
      mp[k] = lerp_t(mp[k], gk, a.one_m_b1);
      vp[k] = vp[k] * a.b2 + a.one_m_b2 * gk * gk;
      float den;
      if (AMSGRAD) {
        xp[k] = fmaxf(xp[k], vp[k]);
        den = sqrtf(xp[k]) / bc2_sqrt + a.eps;
      } else {
        den = sqrtf(vp[k]) / bc2_sqrt + a.eps;
      }
      pp[k] = pp[k] + neg_step_size * mp[k] / den;
    }
    p[i] = P, m[i] = M, v[i] = V;
    if (AMSGRAD) vmax[i] = X;
  }
}

// the momentum buffer starts as a copy of the first step's gradient (torch: ``buf is None`` -> buf = grad.clone())
template <bool MOMENTUM, bool NESTEROV, bool WD, bool MAXIMIZE>
__global__ __launch_bounds__(256) void sgd_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                  float4* __restrict__ buf, const uint8_t* __restrict__ live, size_t n4,
                                                  SgdArgs a, const int* __restrict__ step_dev) {
  const bool first = step_dev[0] == 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    if (live && !live[i]) continue;
    float4 P = p[i], G = g[i], B;
    if (MOMENTUM && !first) B = buf[i];
    float* pp = &P.x;
    float* gp = &G.x;
    float* bp = &B.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk = MAXIMIZE ? -gp[k] : gp[k];
      if (WD) gk = fmaf(pp[k], a.wd, gk);
      if (MOMENTUM) {
        bp[k] = first ? gk : fmaf(gk, a.one_m_damp, bp[k] * a.momentum);
        gk = NESTEROV ? fmaf(bp[k], a.momentum, gk) : bp[k];
      }
      pp[k] = fmaf(gk, a.neg_lr, pp[k]);
    }
    p[i] = P;
    if (MOMENTUM) buf[i] = B;
  }
}

template <bool WD, bool MAXIMIZE>
__global__ __launch_bounds__(256) void adagrad_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                      float4* __restrict__ sum, const uint8_t* __restrict__ live,
                                                      size_t n4, AdagradArgs a, const int* __restrict__ step_dev) {
  const double step = (double)(step_dev[0] + 1);
  const float neg_clr = (float)(-(a.lr / (1.0 + (step - 1.0) * a.lr_decay)));
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    if (live && !live[i]) continue;
    float4 P = p[i], G = g[i], S = sum[i];
    float* pp = &P.x;
    float* gp = &G.x;
    float* sp = &S.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk = MAXIMIZE ? -gp[k] : gp[k];
      if (WD) gk = fmaf(pp[k], a.wd, gk);
      sp[k] = sp[k] + gk * gk;
      const float std = sqrtf(sp[k]) + a.eps;
      pp[k] = pp[k] + neg_clr * gk / std;
    }
    p[i] = P, sum[i] = S;
  }
}

template <bool WD, bool MAXIMIZE, bool CENTERED, bool MOMENTUM>
__global__ __launch_bounds__(256) void rmsprop_kernel(float4* __restrict__ p, const float4* __restrict__ g,
                                                      float4* __restrict__ sq, float4* __restrict__ buf,
                                                      float4* __restrict__ gavg, const uint8_t* __restrict__ live,
                                                      size_t n4, RmspropArgs a) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    if (live && !live[i]) continue;
    float4 P = p[i], G = g[i], Q = sq[i], B, A;
    if (MOMENTUM) B = buf[i];
    if (CENTERED) A = gavg[i];
    float* pp = &P.x;
    float* gp = &G.x;
    float* qp = &Q.x;
    float* bp = &B.x;
    float* ap = &A.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk = MAXIMIZE ? -gp[k] : gp[k];
      if (WD) gk = fmaf(pp[k], a.wd, gk);
      qp[k] = qp[k] * a.alpha + a.one_m_alpha * gk * gk;
      float avg;
      if (CENTERED) {
        ap[k] = lerp_t(ap[k], gk, a.one_m_alpha);
        avg = sqrtf(qp[k] - ap[k] * ap[k]);
      } else {
        avg = sqrtf(qp[k]);
      }
      avg = avg + a.eps;
      if (MOMENTUM) {
        bp[k] = bp[k] * a.momentum + gk / avg;
        pp[k] = fmaf(bp[k], a.neg_lr, pp[k]);
      } else {
        pp[k] = pp[k] + a.neg_lr * gk / avg;
      }
    }
    p[i] = P, sq[i] = Q;
    if (MOMENTUM) buf[i] = B;
    if (CENTERED) gavg[i] = A;
  }
}

__global__ void optim_bump_step_kernel(int* step_dev) { step_dev[0] += 1; }

// calls f(std::integral_constant<bool, b>{})
template <typename F>
static inline void with_bool(bool b, F&& f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}

static inline dim3 optim_grid(size_t n4) {
  const size_t b = cdivz(n4, 256);
  return dim3((unsigned)(b > 2048 ? 2048 : (b < 1 ? 1 : b)));
}

static inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

static int bump(int* step_dev, void* stream, const char* name) {
  hipLaunchKernelGGL(optim_bump_step_kernel, dim3(1), dim3(1), 0, S(stream), step_dev);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace itcv

using namespace itcv;

// shared argument checks: buffers present and 16-byte aligned, n a multiple of 4, no unknown flag bits
#define ITCV_OPTIM_COMMON(name, allowed_flags)                                                              \
  ITCV_REQUIRE(p && g && step_dev, name);                                                                   \
  ITCV_REQUIRE(n % 4 == 0, name);                                                                          \
  ITCV_REQUIRE(aligned16(p) && aligned16(g), name);                                                        \
  ITCV_REQUIRE((flags & ~(allowed_flags)) == 0, name);                                                     \
  ITCV_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, name)

extern "C" {

int itcv_adamx_step_dev(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq,
                        const unsigned char* live, size_t n, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int flags, int* step_dev, void* stream) {
  ITCV_OPTIM_COMMON("itcv_adamx_step_dev", ITCV_OPT_MAXIMIZE | ITCV_OPT_AMSGRAD | ITCV_OPT_DECOUPLED_WD);
  const bool ams = flags & ITCV_OPT_AMSGRAD, maximize = flags & ITCV_OPT_MAXIMIZE;
  ITCV_REQUIRE(exp_avg && exp_avg_sq && aligned16(exp_avg) && aligned16(exp_avg_sq), "itcv_adamx_step_dev");
  ITCV_REQUIRE(!ams || (max_exp_avg_sq && aligned16(max_exp_avg_sq)), "itcv_adamx_step_dev(amsgrad)");
  ITCV_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, "itcv_adamx_step_dev");
  const int wd = weight_decay == 0.0 ? 0 : (flags & ITCV_OPT_DECOUPLED_WD ? 2 : 1);
  AdamArgs a;
  a.lr = lr, a.beta1 = beta1, a.beta2 = beta2;
  a.one_m_b1 = (float)(1.0 - beta1), a.b2 = (float)beta2, a.one_m_b2 = (float)(1.0 - beta2), a.eps = (float)eps;
  a.wd = (float)weight_decay, a.decay = (float)(1.0 - lr * weight_decay);
  const size_t n4 = n / 4;
  if (n4) {
    auto launch = [&](auto WDc, auto AMSc, auto MAXc) {
      hipLaunchKernelGGL((adamx_kernel<decltype(WDc)::value, decltype(AMSc)::value, decltype(MAXc)::value>),
                         optim_grid(n4), dim3(256), 0, S(stream), (float4*)p, (const float4*)g, (float4*)exp_avg,
                         (float4*)exp_avg_sq, (float4*)max_exp_avg_sq, live, n4, a, step_dev);
    };
    with_bool(ams, [&](auto A) {
      with_bool(maximize, [&](auto M) {
        if (wd == 0) launch(std::integral_constant<int, 0>{}, A, M);
        else if (wd == 1) launch(std::integral_constant<int, 1>{}, A, M);
        else launch(std::integral_constant<int, 2>{}, A, M);
      });
    });
    ITCV_CHECK_LAUNCH("itcv_adamx_step_dev");
  }
  return bump(step_dev, stream, "itcv_adamx_step_dev(bump)");
}

int itcv_sgd_step_dev(float* p, const float* g, float* momentum_buffer, const unsigned char* live, size_t n, double lr,
                      double momentum, double dampening, double weight_decay, int flags, int* step_dev, void* stream) {
  ITCV_OPTIM_COMMON("itcv_sgd_step_dev", ITCV_OPT_MAXIMIZE | ITCV_OPT_NESTEROV);
  const bool mom = momentum != 0.0, nesterov = flags & ITCV_OPT_NESTEROV;
  ITCV_REQUIRE(momentum >= 0.0, "itcv_sgd_step_dev");
  ITCV_REQUIRE(!mom || (momentum_buffer && aligned16(momentum_buffer)), "itcv_sgd_step_dev(momentum_buffer)");
  // torch.optim.SGD: "Nesterov momentum requires a momentum and zero dampening"
  ITCV_REQUIRE(!nesterov || (mom && dampening == 0.0), "itcv_sgd_step_dev(nesterov)");
  SgdArgs a;
  a.neg_lr = (float)(-lr), a.wd = (float)weight_decay, a.momentum = (float)momentum;
  a.one_m_damp = (float)(1.0 - dampening);
  const size_t n4 = n / 4;
  if (n4) {
    with_bool(mom, [&](auto MOM) {
      with_bool(nesterov && mom, [&](auto NES) {
        with_bool(weight_decay != 0.0, [&](auto WD) {
          with_bool(flags & ITCV_OPT_MAXIMIZE, [&](auto MAX) {
            hipLaunchKernelGGL((sgd_kernel<decltype(MOM)::value, decltype(NES)::value, decltype(WD)::value,
                                           decltype(MAX)::value>),
                               optim_grid(n4), dim3(256), 0, S(stream), (float4*)p, (const float4*)g,
                               (float4*)momentum_buffer, live, n4, a, step_dev);
          });
        });
      });
    });
    ITCV_CHECK_LAUNCH("itcv_sgd_step_dev");
  }
  return bump(step_dev, stream, "itcv_sgd_step_dev(bump)");
}

int itcv_adagrad_step_dev(float* p, const float* g, float* sum, const unsigned char* live, size_t n, double lr,
                          double lr_decay, double weight_decay, double eps, int flags, int* step_dev, void* stream) {
  ITCV_OPTIM_COMMON("itcv_adagrad_step_dev", ITCV_OPT_MAXIMIZE);
  ITCV_REQUIRE(sum && aligned16(sum), "itcv_adagrad_step_dev(sum)");
  ITCV_REQUIRE(lr_decay >= 0.0 && eps >= 0.0, "itcv_adagrad_step_dev");
  AdagradArgs a;
  a.lr = lr, a.lr_decay = lr_decay, a.wd = (float)weight_decay, a.eps = (float)eps;
  const size_t n4 = n / 4;
  if (n4) {
    with_bool(weight_decay != 0.0, [&](auto WD) {
      with_bool(flags & ITCV_OPT_MAXIMIZE, [&](auto MAX) {
        hipLaunchKernelGGL((adagrad_kernel<decltype(WD)::value, decltype(MAX)::value>), optim_grid(n4), dim3(256), 0,
                           S(stream), (float4*)p, (const float4*)g, (float4*)sum, live, n4, a, step_dev);
      });
    });
    ITCV_CHECK_LAUNCH("itcv_adagrad_step_dev");
  }
  return bump(step_dev, stream, "itcv_adagrad_step_dev(bump)");
}

int itcv_rmsprop_step_dev(float* p, const float* g, float* square_avg, float* momentum_buffer, float* grad_avg,
                          const unsigned char* live, size_t n, double lr, double alpha, double eps,
                          double weight_decay, double momentum, int flags, int* step_dev, void* stream) {
  ITCV_OPTIM_COMMON("itcv_rmsprop_step_dev", ITCV_OPT_MAXIMIZE | ITCV_OPT_CENTERED);
  const bool mom = momentum > 0.0, centered = flags & ITCV_OPT_CENTERED;
  ITCV_REQUIRE(alpha >= 0.0 && eps >= 0.0 && momentum >= 0.0, "itcv_rmsprop_step_dev");
  ITCV_REQUIRE(square_avg && aligned16(square_avg), "itcv_rmsprop_step_dev(square_avg)");
  ITCV_REQUIRE(!mom || (momentum_buffer && aligned16(momentum_buffer)), "itcv_rmsprop_step_dev(momentum_buffer)");
  ITCV_REQUIRE(!centered || (grad_avg && aligned16(grad_avg)), "itcv_rmsprop_step_dev(grad_avg)");
  RmspropArgs a;
  a.neg_lr = (float)(-lr), a.alpha = (float)alpha, a.one_m_alpha = (float)(1.0 - alpha), a.eps = (float)eps;
  a.wd = (float)weight_decay, a.momentum = (float)momentum;
  const size_t n4 = n / 4;
  if (n4) {
    with_bool(weight_decay != 0.0, [&](auto WD) {
      with_bool(flags & ITCV_OPT_MAXIMIZE, [&](auto MAX) {
        with_bool(centered, [&](auto CEN) {
          with_bool(mom, [&](auto MOM) {
            hipLaunchKernelGGL((rmsprop_kernel<decltype(WD)::value, decltype(MAX)::value, decltype(CEN)::value,
                                               decltype(MOM)::value>),
                               optim_grid(n4), dim3(256), 0, S(stream), (float4*)p, (const float4*)g,
                               (float4*)square_avg, (float4*)momentum_buffer, (float4*)grad_avg, live, n4, a);
          });
        });
      });
    });
    ITCV_CHECK_LAUNCH("itcv_rmsprop_step_dev");
  }
  return bump(step_dev, stream, "itcv_rmsprop_step_dev(bump)");
}

}  // extern "C"
