// The latent op of JointVAE (Dupont 2018, "Learning Disentangled Joint Continuous and Discrete Representations") and, with no
// discrete variables, of AnnealedVAE (Burgess et al. 2018; disentanglement_lib's `annealed_vae`) with its gradient.  The
// rules are in include/itcv_hip.h:
//   joint_fwd    : ONE wave per row, four rows per 256-thread block, the blocks stride over the rows.  Lane l holds columns
//                  l, l + 64, ...: the continuous ones are reparameterised and their KL summed by a wave reduction; the
//                  row's logits a and tempered logits (a + g) / tau are staged in LDS, and every lane then walks, for each of
//                  its own discrete columns, the columns of that column's group IN ORDER (max, sums, sum alpha log alpha),
//                  so every lane of a group gets the same fixed-order numbers with no cross-lane traffic and a group may
//                  lie anywhere across the 64-lane edges.  The wave writes z and two fp64 numbers per row.
//   joint_finish : ONE block sums the 2B partials in row order (objective.h's ordered_sum), READS THE TWO CAPACITIES FROM
//                  DEVICE MEMORY and writes the loss, the two signs and the four logged terms.
//   joint_bwd    : ONE launch with the forward's mapping and the stored signs.
// Every sum has a fixed order, there is no atomic, and nothing depends on the grid or on timing: the same inputs give the
// same bits.  Nothing in this file may be contracted into a fused multiply-add.
#include "objective.h"

#pragma clang fp contract(off)

namespace itcv {

constexpr int kJointMaxD = 512;
constexpr int kJointMaxB = 1 << 30;
constexpr int kJointThreads = 256;
constexpr int kJointRows = kJointThreads / kWave;
constexpr int kJointMaxBlocks = 256;      // 1024 rows a trip; the rest of the batch is walked by the stride

// the group [s, e) of discrete column j (columns counted from the first discrete one), held inside 0 <= s <= j < e <= n
__device__ __forceinline__ void joint_segment(const int* __restrict__ seg, int j, int n, int& s, int& e) {
  s = seg[2 * j], e = seg[2 * j + 1];
  s = s < 0 ? 0 : (s > j ? j : s);
  e = e > n ? n : (e <= j ? j + 1 : e);
}

// of the group [s, e) of one row, every sum in column order: lse = logsumexp(a), mt = max t, st = sum exp(t - mt),
// ent = sum_k alpha_k log alpha_k with log alpha = a - lse
__device__ __forceinline__ void joint_group(const double* a, const double* t, int s, int e, double& lse, double& mt,
                                            double& st, double& ent) {
  double ma = a[s];
  mt = t[s];
  for (int k = s + 1; k < e; ++k) {
    ma = a[k] > ma ? a[k] : ma;
    mt = t[k] > mt ? t[k] : mt;
  }
  double sa = 0.0;
  st = 0.0;
  for (int k = s; k < e; ++k) {
    sa += exp(a[k] - ma);
    st += exp(t[k] - mt);
  }
  lse = ma + log(sa);
  ent = 0.0;
  for (int k = s; k < e; ++k) {
    const double la = a[k] - lse;
    ent += exp(la) * la;
  }
}

// the Gumbel draw of a uniform one: torch.rand's fp32 values are multiples of 2^-24 in [0, 1); 0 becomes 2^-25
__device__ __forceinline__ double joint_gumbel(float u) {
  const double v = u > 0.f ? (double)u : 0x1p-25;
  return -log(-log(v));
}

__global__ __launch_bounds__(kJointThreads) void joint_fwd_kernel(const float* __restrict__ mu, size_t ldm,
                                                                  const float* __restrict__ lv, size_t ldl,
                                                                  const float* __restrict__ eps, size_t lde,
                                                                  const float* __restrict__ u, size_t ldu,
                                                                  const int* __restrict__ seg, int B, int nc, int nd,
                                                                  double tau, int hard, float* __restrict__ z,
                                                                  double* __restrict__ part) {
  __shared__ double sa[kJointRows][kJointMaxD], st[kJointRows][kJointMaxD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, D = nc + nd;
  for (int base = blockIdx.x * kJointRows; base < B; base += gridDim.x * kJointRows) {   // block-uniform: barriers inside
    const bool live = base + w < B;                                                       // wave-uniform
    const size_t r = (size_t)(base + w);
    double klz = 0.0, klc = 0.0;
    if (live) {
      for (int d = lane; d < nc; d += 64) {
        const float mf = mu[r * ldm + d];
        if (hard) {
          z[r * D + d] = mf;
        } else {
          const double m = mf, l = lv[r * ldl + d], n = eps[r * lde + d];
          z[r * D + d] = (float)posterior_sample(m, l, n);
          klz += posterior_kl_term(m, l);
        }
      }
      for (int j = lane; j < nd; j += 64) {
        const double a = mu[r * ldm + nc + j];
        sa[w][j] = a;
        st[w][j] = hard ? a : (a + joint_gumbel(u[r * ldu + j])) / tau;
      }
    }
    __syncthreads();
    if (live) {
      int ps = -1, best = 0;
      double lse = 0.0, mt = 0.0, sum = 1.0, ent = 0.0;
      for (int j = lane; j < nd; j += 64) {
        int s, e;
        joint_segment(seg, j, nd, s, e);
        if (hard) {
          if (s != ps) {
            best = s;                                   // the first maximum: ties take the lowest index
            for (int k = s + 1; k < e; ++k) best = sa[w][k] > sa[w][best] ? k : best;
          }
          z[r * D + nc + j] = j == best ? 1.f : 0.f;
        } else {
          if (s != ps) joint_group(sa[w], st[w], s, e, lse, mt, sum, ent);
          z[r * D + nc + j] = (float)(exp(st[w][j] - mt) / sum);
          if (j == s) klc += log((double)(e - s)) + ent;      // once per group, by the lane of its first column
        }
        ps = s;
      }
      if (!hard) {
        klz = wave_sum(klz);
        klc = wave_sum(klc);
        if (lane == 0) {
          part[r] = -0.5 * klz;
          part[(size_t)B + r] = klc;
        }
      }
    }
    __syncthreads();                                    // the staged row is overwritten by the next trip
  }
}

__device__ __forceinline__ double joint_sign(double v) { return (double)(v > 0.0) - (double)(v < 0.0); }

// out[0] = beta (gz |KL_z - C_z| + gc |KL_c - C_c|) with (C_z, C_c) = cap[0], cap[1] READ HERE; sgn[2] the signs of the two
// differences (0 at 0, as torch.abs differentiates); terms[4] = {KL_z, KL_c, C_z, C_c}
__global__ __launch_bounds__(kJointThreads) void joint_finish_kernel(const double* __restrict__ part, int B,
                                                                     const double* __restrict__ cap, double beta,
                                                                     double gz, double gc, float* __restrict__ out,
                                                                     float* __restrict__ sgn, float* __restrict__ terms) {
  __shared__ double red[kJointThreads];
  const double sz = ordered_sum<kJointThreads>(part, (size_t)B, red);
  const double sc = ordered_sum<kJointThreads>(part + (size_t)B, (size_t)B, red);
  if (threadIdx.x == 0) {
    const double klz = sz / (double)B, klc = sc / (double)B, cz = cap[0], cc = cap[1];
    const double dz = klz - cz, dc = klc - cc;
    out[0] = (float)(beta * (gz * fabs(dz) + gc * fabs(dc)));
    sgn[0] = (float)joint_sign(dz), sgn[1] = (float)joint_sign(dc);
    terms[0] = (float)klz, terms[1] = (float)klc, terms[2] = (float)cz, terms[3] = (float)cc;
  }
}

__global__ __launch_bounds__(kJointThreads) void joint_bwd_kernel(const float* __restrict__ dz, size_t ldz,
                                                                  const float* __restrict__ g,
                                                                  const float* __restrict__ sgn,
                                                                  const float* __restrict__ mu, size_t ldm,
                                                                  const float* __restrict__ lv, size_t ldl,
                                                                  const float* __restrict__ eps, size_t lde,
                                                                  const float* __restrict__ u, size_t ldu,
                                                                  const int* __restrict__ seg, int B, int nc, int nd,
                                                                  double tau, double beta, double gz, double gc,
                                                                  float* __restrict__ dmu, float* __restrict__ dlv) {
  __shared__ double sa[kJointRows][kJointMaxD], st[kJointRows][kJointMaxD], sg[kJointRows][kJointMaxD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, D = nc + nd;
  const double kz = (double)g[0] * beta * gz * (double)sgn[0] / (double)B;
  const double kc = (double)g[0] * beta * gc * (double)sgn[1] / (double)B;
  for (int base = blockIdx.x * kJointRows; base < B; base += gridDim.x * kJointRows) {
    const bool live = base + w < B;
    const size_t r = (size_t)(base + w);
    if (live) {
      for (int d = lane; d < nc; d += 64) {
        const double m = mu[r * ldm + d], l = lv[r * ldl + d], n = eps[r * lde + d], gd = dz[r * ldz + d];
        dmu[r * D + d] = (float)posterior_dmu(gd, m, kz);
        dlv[r * D + d] = (float)posterior_dlv(gd, n, l, kz);
      }
      for (int j = lane; j < nd; j += 64) {
        const double a = mu[r * ldm + nc + j];
        sa[w][j] = a;
        st[w][j] = (a + joint_gumbel(u[r * ldu + j])) / tau;
        sg[w][j] = dz[r * ldz + nc + j];
      }
    }
    __syncthreads();
    if (live) {
      int ps = -1;
      double lse = 0.0, mt = 0.0, sum = 1.0, ent = 0.0, ydz = 0.0;
      for (int j = lane; j < nd; j += 64) {
        int s, e;
        joint_segment(seg, j, nd, s, e);
        if (s != ps) {
          joint_group(sa[w], st[w], s, e, lse, mt, sum, ent);
          ydz = 0.0;                                    // sum_k y_k dz_k, in column order
          for (int k = s; k < e; ++k) ydz += exp(st[w][k] - mt) / sum * sg[w][k];
          ps = s;
        }
        const double y = exp(st[w][j] - mt) / sum, la = sa[w][j] - lse;
        dmu[r * D + nc + j] = (float)(y * (sg[w][j] - ydz) / tau + kc * (exp(la) * (la - ent)));
        dlv[r * D + nc + j] = 0.f;                      // the logvar columns of the discrete block are not part of the model
      }
    }
    __syncthreads();
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
static inline bool joint_weight_ok(double v) { return v >= 0.0 && finite(v); }

// nothing is launched on a failure
static int joint_check(const char* name, bool ptrs, int B, int nc, int nd, bool soft, double tau, double gz, double gc,
                       double beta) {
  if (need_pointers(name, ptrs) || need_dim(name, "B = %lld rows", B, 1, kJointMaxB, "1..2^30")) return 1;
  if (nc < 0 || nd < 0) return fail("%s: n_cont = %lld and n_disc = %lld must not be negative", name, nc, nd);
  if (need_dim(name, "D = n_cont + n_disc = %lld", nc + (long long)nd, 1, kJointMaxD, "1..512")) return 1;
  if (!soft) return 0;
  if (!(tau > 0.0 && finite(tau))) return fail("%s: the temperature must be a finite number above 0", name);
  if (!joint_weight_ok(gz) || !joint_weight_ok(gc))
    return fail("%s: gamma_cont and gamma_disc must be finite and not negative", name);
  if (!finite(beta)) return fail("%s: beta must be a finite number", name);
  return 0;
}

static int joint_strides(const char* name, size_t ld_mu, size_t ld_logvar, size_t ld_eps, size_t ld_u, int nc, int nd,
                         bool soft) {
  const long long D = (long long)nc + nd;
  if (need_stride(name, "a", ld_mu, "D", D)) return 1;
  if (!soft) return 0;
  if (nc && (need_stride(name, "a", ld_logvar, "D", D) || need_stride(name, "a", ld_eps, "n_cont", nc))) return 1;
  return nd ? need_stride(name, "a", ld_u, "n_disc", nd) : 0;
}

}  // namespace itcv

using namespace itcv;

extern "C" {

int itcv_joint_latent_fwd(const float* mu, size_t ld_mu, const float* logvar, size_t ld_logvar, const float* eps,
                          size_t ld_eps, const float* u, size_t ld_u, const int* seg, const double* cap, float* z,
                          double* part, float* out, float* sgn, float* terms, int B, int n_cont, int n_disc, int hard,
                          double tau, double gamma_cont, double gamma_disc, double beta, void* stream) {
  const char* name = "itcv_joint_latent_fwd";
  const bool soft = hard == 0;
  const bool ptrs = mu && z && (n_disc <= 0 || seg) &&
                    (!soft || (cap && part && out && sgn && terms && (n_cont <= 0 || (logvar && eps)) && (n_disc <= 0 || u)));
  if (int e = joint_check(name, ptrs, B, n_cont, n_disc, soft, tau, gamma_cont, gamma_disc, beta)) return e;
  if (int e = joint_strides(name, ld_mu, ld_logvar, ld_eps, ld_u, n_cont, n_disc, soft)) return e;
  hipStream_t st = S(stream);
  const dim3 block(kJointThreads);
  const dim3 grid(row_grid(B, kJointRows, kJointMaxBlocks));
  hipLaunchKernelGGL(joint_fwd_kernel, grid, block, 0, st, mu, ld_mu, logvar, ld_logvar, eps, ld_eps, u, ld_u, seg, B,
                     n_cont, n_disc, soft ? tau : 1.0, soft ? 0 : 1, z, part);
  ITCV_CHECK_LAUNCH("itcv_joint_latent_fwd(rows)");
  if (!soft) return 0;
  hipLaunchKernelGGL(joint_finish_kernel, dim3(1), block, 0, st, (const double*)part, B, cap, beta, gamma_cont, gamma_disc,
                     out, sgn, terms);
  ITCV_CHECK_LAUNCH("itcv_joint_latent_fwd(finish)");
  return 0;
}

int itcv_joint_latent_bwd(const float* dz, size_t ld_dz, const float* g, const float* sgn, const float* mu, size_t ld_mu,
                          const float* logvar, size_t ld_logvar, const float* eps, size_t ld_eps, const float* u,
                          size_t ld_u, const int* seg, float* dmu, float* dlogvar, int B, int n_cont, int n_disc,
                          double tau, double gamma_cont, double gamma_disc, double beta, void* stream) {
  const char* name = "itcv_joint_latent_bwd";
  const bool ptrs = dz && g && sgn && mu && dmu && dlogvar && (n_cont <= 0 || (logvar && eps)) && (n_disc <= 0 || (u && seg));
  if (int e = joint_check(name, ptrs, B, n_cont, n_disc, true, tau, gamma_cont, gamma_disc, beta)) return e;
  if (int e = joint_strides(name, ld_mu < ld_dz ? ld_mu : ld_dz, ld_logvar, ld_eps, ld_u, n_cont, n_disc, true)) return e;
  const dim3 grid(row_grid(B, kJointRows, kJointMaxBlocks));
  hipLaunchKernelGGL(joint_bwd_kernel, grid, dim3(kJointThreads), 0, S(stream), dz, ld_dz, g, sgn, mu, ld_mu, logvar,
                     ld_logvar, eps, ld_eps, u, ld_u, seg, B, n_cont, n_disc, tau, beta, gamma_cont, gamma_disc, dmu,
                     dlogvar);
  ITCV_CHECK_LAUNCH(name);
  return 0;
}

}  // extern "C"
