// The latent op of Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020; disentanglement_lib's `weak` module, GroupVAEBase with
// aggregate_argmax) with its gradient.  The rules are in include/itcv_hip.h:
//   ada_fwd    : ONE wave per pair (rows b and B + b), four pairs per 256-thread block, the blocks stride over the pairs.
//                Lane l holds dimensions l, l + 64, ... of both rows in registers (NR = ceil(D / 64) <= 8 of them; the
//                kernel is instantiated for NR = 1, 2, 4, 8).  delta, its min and max over the pair (two wave
//                reductions), the threshold, the mask, the averaged posteriors, both samples and the KL sums of the two
//                adapted rows (two more wave reductions) are fp64 from the fp32 inputs.  The wave writes z, the mask, and
//                three fp64 numbers per pair: the KL of its two rows and its count of shared dimensions.
//   ada_finish : ONE block sums the 2B KL partials in row order and the B counts in pair order (objective.h's ordered_sum)
//                into the scalar and the two logged terms.
//   ada_bwd    : ONE launch with the forward's mapping; with the mask a constant, the gradient is a function of the pair's
//                dimension alone, so it needs no reduction.
// Every sum has a fixed order, there is no atomic, and nothing depends on the grid or on timing: the same inputs give the
// same bits.  Nothing in this file may be contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kAdaMaxD = 512;
constexpr int kAdaMaxB = 1 << 30;         // 2B rows are counted in an int
constexpr int kAdaThreads = 256;
constexpr int kAdaPairs = kAdaThreads / kWave;
constexpr int kAdaMaxBlocks = 256;        // 1024 pairs a trip; the rest of the batch is walked by the stride
constexpr int kAdaGvae = 1, kAdaMlvae = 2;

// the averaged posterior of one shared dimension: mean and variance (logvar = log of it)
__device__ __forceinline__ void ada_average(int averaging, double m1, double l1, double m2, double l2, double& mb,
                                            double& vb) {
  const double e1 = exp(l1), e2 = exp(l2);
  if (averaging == kAdaGvae) {
    mb = 0.5 * (m1 + m2);
    vb = 0.5 * (e1 + e2);
  } else {
    vb = 2.0 * e1 * e2 / (e1 + e2);
    mb = 0.5 * vb * (m1 * exp(-l1) + m2 * exp(-l2));
  }
}

template <int NR>
__global__ __launch_bounds__(kAdaThreads) void ada_fwd_kernel(const float* __restrict__ mu, size_t ldm,
                                                              const float* __restrict__ lv, size_t ldl,
                                                              const float* __restrict__ eps, size_t lde,
                                                              const uint8_t* __restrict__ own_in, int B, int D,
                                                              int averaging, float* __restrict__ z,
                                                              uint8_t* __restrict__ own, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = blockIdx.x * kAdaPairs + w; b < B; b += gridDim.x * kAdaPairs) {   // wave-uniform
    const size_t r1 = (size_t)b, r2 = (size_t)B + b;
    float m1[NR], l1[NR], m2[NR], l2[NR];
    double delta[NR];
    double mn = DBL_MAX, mx = -DBL_MAX;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int d = lane + 64 * r;
      if (d < D) {
        m1[r] = mu[r1 * ldm + d], l1[r] = lv[r1 * ldl + d];
        m2[r] = mu[r2 * ldm + d], l2[r] = lv[r2 * ldl + d];
        const double a1 = m1[r], b1 = l1[r], a2 = m2[r], b2 = l2[r];
        const double dm = a2 - a1;
        const double dl = exp(b1 - b2) + dm * dm * exp(-b2) - 1.0 + b2 - b1;
        delta[r] = dl;
        mn = dl < mn ? dl : mn;
        mx = dl > mx ? dl : mx;
      } else {
        m1[r] = l1[r] = m2[r] = l2[r] = 0.f;
        delta[r] = 0.0;
      }
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    const double tau = 0.5 * (mn + mx);
    double kl1 = 0.0, kl2 = 0.0, shared = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int d = lane + 64 * r;
      if (d < D) {
        const size_t at = (size_t)b * D + d;
        const bool mine = own_in ? own_in[at] != 0 : delta[r] >= tau;
        own[at] = mine ? 1 : 0;
        const double a1 = m1[r], b1 = l1[r], a2 = m2[r], b2 = l2[r];
        const double n1 = eps[r1 * lde + d], n2 = eps[r2 * lde + d];
        if (mine) {
          z[r1 * D + d] = (float)posterior_sample(a1, b1, n1);
          z[r2 * D + d] = (float)posterior_sample(a2, b2, n2);
          kl1 += posterior_kl_term(a1, b1);
          kl2 += posterior_kl_term(a2, b2);
        } else {
          double mb, vb;
          ada_average(averaging, a1, b1, a2, b2, mb, vb);
          const double sd = sqrt(vb), t = 1.0 + log(vb) - mb * mb - vb;
          z[r1 * D + d] = (float)(mb + n1 * sd);
          z[r2 * D + d] = (float)(mb + n2 * sd);
          kl1 += t;
          kl2 += t;
          shared += 1.0;
        }
      }
    }
    kl1 = wave_sum(kl1);
    kl2 = wave_sum(kl2);
    shared = wave_sum(shared);
    if (lane == 0) {
      part[r1] = -0.5 * kl1;
      part[r2] = -0.5 * kl2;
      part[2 * (size_t)B + b] = shared;
    }
  }
}

// out[0] = beta * mean_{2B rows} KL; terms[2] = {mean KL, mean number of shared dimensions per pair}
__global__ __launch_bounds__(kAdaThreads) void ada_finish_kernel(const double* __restrict__ part, int B, double beta,
                                                                 float* __restrict__ out, float* __restrict__ terms) {
  __shared__ double red[kAdaThreads];
  const double kl = ordered_sum<kAdaThreads>(part, 2 * (size_t)B, red);
  const double sh = ordered_sum<kAdaThreads>(part + 2 * (size_t)B, (size_t)B, red);
  if (threadIdx.x == 0) {
    const double mean = kl / (2.0 * (double)B);
    out[0] = (float)(beta != 0.0 ? beta * mean : 0.0);
    terms[0] = (float)mean;
    terms[1] = (float)(sh / (double)B);
  }
}

__global__ __launch_bounds__(kAdaThreads) void ada_bwd_kernel(const float* __restrict__ dz, size_t ldz,
                                                              const float* __restrict__ g, const float* __restrict__ mu,
                                                              size_t ldm, const float* __restrict__ lv, size_t ldl,
                                                              const float* __restrict__ eps, size_t lde,
                                                              const uint8_t* __restrict__ own, int B, int D, int averaging,
                                                              double beta, float* __restrict__ dmu,
                                                              float* __restrict__ dlv) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double gk = beta != 0.0 ? (double)g[0] * beta / (2.0 * (double)B) : 0.0;
  for (int b = blockIdx.x * kAdaPairs + w; b < B; b += gridDim.x * kAdaPairs) {
    const size_t r1 = (size_t)b, r2 = (size_t)B + b;
    for (int d = lane; d < D; d += 64) {
      const double m1 = mu[r1 * ldm + d], l1 = lv[r1 * ldl + d], m2 = mu[r2 * ldm + d], l2 = lv[r2 * ldl + d];
      const double n1 = eps[r1 * lde + d], n2 = eps[r2 * lde + d];
      const double g1 = dz[r1 * ldz + d], g2 = dz[r2 * ldz + d];
      double dm1, dm2, dl1, dl2;
      if (own[(size_t)b * D + d]) {
        dm1 = posterior_dmu(g1, m1, gk);
        dm2 = posterior_dmu(g2, m2, gk);
        dl1 = posterior_dlv(g1, n1, l1, gk);
        dl2 = posterior_dlv(g2, n2, l2, gk);
      } else {
        double mb, vb;
        ada_average(averaging, m1, l1, m2, l2, mb, vb);
        const double Gm = (g1 + g2) + 2.0 * gk * mb;                               // d / d mean of the shared posterior
        const double Gl = 0.5 * sqrt(vb) * (g1 * n1 + g2 * n2) + gk * (vb - 1.0);   // d / d its log-variance
        if (averaging == kAdaGvae) {
          const double e1 = exp(l1), e2 = exp(l2), s = e1 + e2;
          dm1 = dm2 = 0.5 * Gm;
          dl1 = Gl * (e1 / s);
          dl2 = Gl * (e2 / s);
        } else {
          // precisions p_i = exp(-l_i), P = p_1 + p_2: mean = sum m_i p_i / P, log-variance = log 2 - log P
          const double p1 = exp(-l1), p2 = exp(-l2), P = p1 + p2;
          const double w1 = p1 / P, w2 = p2 / P;
          dm1 = Gm * w1;
          dm2 = Gm * w2;
          dl1 = Gl * w1 + Gm * (w1 * (mb - m1));
          dl2 = Gl * w2 + Gm * (w2 * (mb - m2));
        }
      }
      dmu[r1 * D + d] = (float)dm1, dmu[r2 * D + d] = (float)dm2;
      dlv[r1 * D + d] = (float)dl1, dlv[r2 * D + d] = (float)dl2;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
// nothing is launched on a failure
static int ada_check(const char* name, bool ptrs, int B, int D, int averaging, double beta, size_t ld_min) {
  if (need_pointers(name, ptrs) || need_dim(name, "B = %lld pairs", B, 1, kAdaMaxB, "1..2^30") ||
      need_dim(name, "D = %lld", D, 1, kAdaMaxD, "1..512"))
    return 1;
  if (averaging != kAdaGvae && averaging != kAdaMlvae)
    return fail("%s: averaging %lld is not 1 (gvae) or 2 (mlvae)", name, averaging);
  if (!finite(beta)) return fail("%s: beta must be a finite number", name);
  return need_stride(name, "a", ld_min, "D", D);
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_ada_group_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps,
                       size_t ld_eps, const uint8_t* own_in, float* z, uint8_t* own, double* part, float* out,
                       float* terms, int B, int D, int averaging, double beta, void* stream) {
  const char* name = "itcv_ada_group_fwd";
  const size_t ld_min = ld_mu < ld_logvar ? (ld_mu < ld_eps ? ld_mu : ld_eps) : (ld_logvar < ld_eps ? ld_logvar : ld_eps);
  if (int e = ada_check(name, mu && logvar && eps && z && own && part && out && terms, B, D, averaging, beta, ld_min))
    return e;
  hipStream_t st = S(stream);
  const dim3 grid(row_grid(B, kAdaPairs, kAdaMaxBlocks)), block(kAdaThreads);
  pick_of<1, 2, 4, 8>(D <= 64 ? 1 : D <= 128 ? 2 : D <= 256 ? 4 : 8, [&](auto nr) {
    hipLaunchKernelGGL(ada_fwd_kernel<decltype(nr)::value>, grid, block, 0, st, mu, ld_mu, logvar, ld_logvar, eps, ld_eps,
                       own_in, B, D, averaging, z, own, part);
  });
  ITCV_CHECK_LAUNCH("itcv_ada_group_fwd(pairs)");
  hipLaunchKernelGGL(ada_finish_kernel, dim3(1), block, 0, st, (const double*)part, B, beta, out, terms);
  ITCV_CHECK_LAUNCH("itcv_ada_group_fwd(finish)");
  return 0;
}

int itcv_ada_group_bwd(const float* dz, size_t ld_dz, const float* g, const float* mu, size_t ld_mu, const float* logvar,
                       size_t ld_logvar, const float* eps, size_t ld_eps, const uint8_t* own, float* dmu, float* dlogvar,
                       int B, int D, int averaging, double beta, void* stream) {
  const char* name = "itcv_ada_group_bwd";
  size_t ld_min = ld_dz < ld_mu ? ld_dz : ld_mu;
  ld_min = ld_logvar < ld_min ? ld_logvar : ld_min;
  ld_min = ld_eps < ld_min ? ld_eps : ld_min;
  if (int e = ada_check(name, dz && g && mu && logvar && eps && own && dmu && dlogvar, B, D, averaging, beta, ld_min))
    return e;
  const dim3 grid(row_grid(B, kAdaPairs, kAdaMaxBlocks));
  hipLaunchKernelGGL(ada_bwd_kernel, grid, dim3(kAdaThreads), 0, S(stream), dz, ld_dz, g, mu, ld_mu, logvar, ld_logvar, eps,
                     ld_eps, own, B, D, averaging, beta, dmu, dlogvar);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
