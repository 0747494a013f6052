// The losses of the DrQ-v2 update as launches of their own: TruncatedNormal sample (utils.py:112-126), TD target + twin
// MSE (drqv2.py:185-189) and its prioritized form, actor loss (drqv2.py:212-216, 225-226) and its DrQ+BC form.  qout.hip
// computes the same losses inside the Q-output backward.  Fixed-order reductions: run-to-run bit-stable.
#include "common.h"
#include "internal.h"
#include "device_sums.h"

namespace {

// ------------------------------------------------------------------------------------------------
// policy head output: mu = tanh(pre); a = clampST(mu + clamp(noise*std, +-clip))   (utils.py:117-126)
// ------------------------------------------------------------------------------------------------
__global__ void sample_action_kernel(const float* pre, const float* noise, float std, float clip, int use_clip,
                                     float* mu_out, float* a_out, long lda_out, int B, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * A) return;
  const int b = i / A, j = i - b * A;
  const float mu = tanhf(pre[i]);
  float eps = noise[i] * std;
  if (use_clip) eps = fminf(fmaxf(eps, -clip), clip);
  const float x = mu + eps;
  const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
  const float a = fminf(fmaxf(x, lo), hi);
  if (mu_out) mu_out[i] = mu;
  a_out[(long)b * lda_out + j] = a;
}

__global__ void copy_cols_kernel(const float* src, int ld_src, float* dst, long ld_dst, int B, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * A) return;
  const int b = i / A, j = i - b * A;
  dst[(long)b * ld_dst + j] = src[(long)b * ld_src + j];
}

// ------------------------------------------------------------------------------------------------
// TD target + twin MSE (drqv2.py:185-189).  Single block.  invB = 1/global batch.
// sums[0..4] = sum reward, sum target_q, sum q1, sum q2, sum (q1-y)^2+(q2-y)^2  (un-normalised: the
// data-parallel path adds them across ranks before dividing).
// PW (prioritized replay, drq_td_mse_w): row b carries the importance weight w[b].  dq_k is the plain expression
// multiplied by w[b] LAST, so that w == 1 gives the plain bits; sums[4] adds w (e1^2 + e2^2); sums[0..3] stay
// unweighted; td_abs[b] = (|e1| + |e2|) / 2, unweighted, is what the priorities are made of.
// ------------------------------------------------------------------------------------------------
template <bool PW>
__global__ void td_loss_kernel(const float* tq1, const float* tq2, const float* q1, const float* q2,
                               const float* reward, const float* discount, float* dq1, float* dq2, float* sums,
                               int B, float invB, const float* w, float* td_abs) {
  __shared__ float sm[4][256];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  float sr = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float y = reward[b] + discount[b] * fminf(tq1[b], tq2[b]);
    const float e1 = q1[b] - y, e2 = q2[b] - y;
    if constexpr (PW) {
      const float wb = w[b];
      dq1[b] = (2.f * e1 * invB) * wb;
      dq2[b] = (2.f * e2 * invB) * wb;
      td_abs[b] = 0.5f * (fabsf(e1) + fabsf(e2));
    } else {
      dq1[b] = 2.f * e1 * invB;
      dq2[b] = 2.f * e2 * invB;
    }
    s[0] += y;
    s[1] += q1[b];
    s[2] += q2[b];
    if constexpr (PW) s[3] += w[b] * (e1 * e1 + e2 * e2);
    else s[3] += e1 * e1 + e2 * e2;
    sr += reward[b];
  }
  block_sum4(s, sm);
  float r4[4] = {sr, 0.f, 0.f, 0.f};
  block_sum4(r4, sm);
  if (threadIdx.x == 0) {
    sums[0] = r4[0];
    sums[1] = s[0];
    sums[2] = s[1];
    sums[3] = s[2];
    sums[4] = s[3];
  }
}

// ------------------------------------------------------------------------------------------------
// actor loss (drqv2.py:212-216): L = -mean(min(q1,q2)); gradient routed to the smaller head, ties split.
// sums[5] = sum -min(q1,q2), sums[6] = sum_b sum_A log N(a|mu,std)
// ------------------------------------------------------------------------------------------------
__global__ void actor_loss_kernel(const float* q1, const float* q2, const float* a, long lda, const float* mu,
                                  float std, float* dq1, float* dq2, float* sums, int B, int A, float invB,
                                  float* sums_host, unsigned seq) {
  __shared__ float sm[4][256];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  const float log_std = logf(std);
  const float c = 0.91893853320467274178f;   // log(sqrt(2*pi))
  const float var2 = 2.f * std * std;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float x = q1[b], y = q2[b];
    s[0] += -fminf(x, y);
    const float g = -invB;
    dq1[b] = x < y ? g : (x == y ? 0.5f * g : 0.f);
    dq2[b] = y < x ? g : (x == y ? 0.5f * g : 0.f);
  }
  // log-probabilities element by element over the flattened [B][A] array (consecutive lanes, consecutive addresses),
  // thread t adding elements t, t + 256, ... in that order: the scheme of the fused form in qout_bwd_kernel
  const int nel = B * A;
  for (int e0 = threadIdx.x; e0 < nel; e0 += 4 * 256) {
    float av[4], mv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * 256 < nel ? e0 + u * 256 : nel - 1;
      const int m = e / A, jj = e - m * A;
      av[u] = a[(long)m * lda + jj];
      mv[u] = mu[e];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + u * 256 < nel) {
        const float d = av[u] - mv[u];
        s[1] += -(d * d) / var2 - log_std - c;
      }
  }
  block_sum4(s, sm);
  if (threadIdx.x == 0) {
    sums[5] = s[0];
    sums[6] = s[1];
    if (sums_host) {   // metrics mirror (DrqStep.sums_host): all eight sums, then the sequence word
      float v8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v8[i] = i == 5 ? s[0] : (i == 6 ? s[1] : sums[i]);
      drq_publish_mirror(sums_host, v8, seq);
    }
  }
}

// d(pre-tanh policy output) = (da1 + da2) * (1 - mu^2): straight-through clamp (utils.py:112-115),
// da_k = action columns of head k's layer-1 input gradient.
__global__ void actor_dmu_kernel(const float* dha1, const float* dha2, long ld, int col0, const float* mu,
                                 float* dpre, int B, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * A) return;
  const int b = i / A, j = i - b * A;
  const float da = dha1[(long)b * ld + col0 + j] + dha2[(long)b * ld + col0 + j];
  const float m = mu[i];
  dpre[i] = da * (1.f - m * m);
}

// ------------------------------------------------------------------------------------------------
// DrQ+BC (TD3+BC on the DrQ-v2 actor; new functionality, the reference has no such loss):
//   lambda = alpha / mean_i |min(q1,q2)_i|   (a constant of the backward),   bc = mean_{i,j} (a - a_beh)^2,
//   L = -lambda mean_i min(q1,q2)_i + bc;   dq_k[i] = -lambda / B_global on the smaller head (ties split),
//   dmu = da_1 + da_2 + 2 (a - a_beh) / (B_global A).
// The batch sum behind lambda and the scale of dq are bc_abs_qmin_sum and bc_dq_scale (device_sums.h), which the fused
// form in qout_bwd_kernel calls as well.
// ------------------------------------------------------------------------------------------------
// actor_loss_kernel with the BC terms.  sums[5], sums[6] as there (sums[5] stays sum -min(q1,q2): the host forms the
// loss from it), sums[9] = sum (a - a_beh)^2 over [B][A], sums[10] = sum |min(q1,q2)|; the mirror gets slots 9, 10 too.
__global__ void actor_loss_bc_kernel(const float* q1, const float* q2, const float* a, long lda, const float* abeh,
                                     long ldb, const float* mu, float std, float alpha, float* dq1, float* dq2,
                                     float* sums, int B, int A, float invB, float* sums_host, unsigned seq) {
  __shared__ float sm[4][256];
  __shared__ float sc[4];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  const float log_std = logf(std);
  const float c = 0.91893853320467274178f;   // log(sqrt(2*pi))
  const float var2 = 2.f * std * std;
  const float sabs = bc_abs_qmin_sum(q1, q2, B, sc);
  const float g = bc_dq_scale(alpha, B, sabs, invB);
  for (int b = threadIdx.x; b < B; b += 256) {
    const float x = q1[b], y = q2[b];
    s[0] += -fminf(x, y);
    dq1[b] = x < y ? g : (x == y ? 0.5f * g : 0.f);
    dq2[b] = y < x ? g : (x == y ? 0.5f * g : 0.f);
  }
  const int nel = B * A;
  for (int e0 = threadIdx.x; e0 < nel; e0 += 4 * 256) {
    float av[4], mv[4], bv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * 256 < nel ? e0 + u * 256 : nel - 1;
      const int m = e / A, jj = e - m * A;
      av[u] = a[(long)m * lda + jj];
      bv[u] = abeh[(long)m * ldb + jj];
      mv[u] = mu[e];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (e0 + u * 256 < nel) {
        const float d = av[u] - mv[u];
        s[1] += -(d * d) / var2 - log_std - c;
        const float e = av[u] - bv[u];
        s[2] += e * e;
      }
  }
  block_sum4(s, sm);
  if (threadIdx.x == 0) {
    sums[5] = s[0];
    sums[6] = s[1];
    sums[9] = s[2];
    sums[10] = sabs;
    if (sums_host) {
      float v8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v8[i] = i == 5 ? s[0] : (i == 6 ? s[1] : sums[i]);
      drq_publish_mirror_bc(sums_host, v8, s[2], sabs, seq);
    }
  }
}

// actor_dmu_kernel with the BC pull: dpre = (da1 + da2 + bc_scale (a - a_beh)) (1 - mu^2), bc_scale = 2 / (B_global A)
__global__ void actor_dmu_bc_kernel(const float* dha1, const float* dha2, long ld, int col0, const float* mu,
                                    const float* act, long lda, const float* abeh, long ldb, float bc_scale,
                                    float* dpre, int B, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * A) return;
  const int b = i / A, j = i - b * A;
  const float da = dha1[(long)b * ld + col0 + j] + dha2[(long)b * ld + col0 + j];
  const float dm = __fmaf_rn(act[(long)b * lda + j] - abeh[(long)b * ldb + j], bc_scale, da);
  const float m = mu[i];
  dpre[i] = dm * (1.f - m * m);
}

}  // namespace

DRQ_API int drq_trunc_normal_sample(const float* pre_tanh, const float* noise, float std, float clip, int use_clip,
                            float* mu_out, float* a_out, long lda_out, int B, int A, hipStream_t st) {
  if (!pre_tanh || !noise || !a_out || B <= 0 || A <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(sample_action_kernel, dim3((B * A + 255) / 256), dim3(256), 0, st, pre_tanh, noise, std, clip,
                     use_clip, mu_out, a_out, lda_out, B, A);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_copy_cols(const float* src, int ld_src, float* dst, long ld_dst, int B, int A, hipStream_t st) {
  if (!src || !dst || B <= 0 || A <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(copy_cols_kernel, dim3((B * A + 255) / 256), dim3(256), 0, st, src, ld_src, dst, ld_dst, B, A);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_td_mse(const float* tq1, const float* tq2, const float* q1, const float* q2, const float* reward,
               const float* discount, float* dq1, float* dq2, float* sums, int B, float inv_global_B,
               hipStream_t st) {
  if (!tq1 || !tq2 || !q1 || !q2 || !reward || !discount || !dq1 || !dq2 || !sums || B <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(td_loss_kernel<false>, dim3(1), dim3(256), 0, st, tq1, tq2, q1, q2, reward, discount, dq1, dq2,
                     sums, B, inv_global_B, nullptr, nullptr);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_td_mse_w(const float* tq1, const float* tq2, const float* q1, const float* q2, const float* reward,
                         const float* discount, const float* w, float* dq1, float* dq2, float* td_abs, float* sums,
                         int B, float inv_global_B, hipStream_t st) {
  if (!tq1 || !tq2 || !q1 || !q2 || !reward || !discount || !w || !dq1 || !dq2 || !td_abs || !sums || B <= 0)
    return DRQ_EARG;
  hipLaunchKernelGGL(td_loss_kernel<true>, dim3(1), dim3(256), 0, st, tq1, tq2, q1, q2, reward, discount, dq1, dq2,
                     sums, B, inv_global_B, w, td_abs);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// internal form used by the step: also publishes the sums to the pinned host mirror (DrqStep.sums_host) when one is
// given.  a_beh != null: the DrQ+BC loss (mirror slots 0..7, 9, 10, then 8); null: the plain loss, ldb and alpha unused.
int drq_actor_loss_ex(const float* q1, const float* q2, const float* a, long lda, const float* a_beh, long ldb,
                      const float* mu, float std, float alpha, float* dq1, float* dq2, float* sums, int B, int A,
                      float inv_global_B, float* sums_host, unsigned seq, hipStream_t st) {
  if (!q1 || !q2 || !a || !mu || !dq1 || !dq2 || !sums || B <= 0 || A <= 0) return DRQ_EARG;
  if (a_beh && (lda < A || ldb < A || !(alpha > 0.f))) return DRQ_EARG;
  if (a_beh)
    hipLaunchKernelGGL(actor_loss_bc_kernel, dim3(1), dim3(256), 0, st, q1, q2, a, lda, a_beh, ldb, mu, std, alpha, dq1,
                       dq2, sums, B, A, inv_global_B, sums_host, seq);
  else
    hipLaunchKernelGGL(actor_loss_kernel, dim3(1), dim3(256), 0, st, q1, q2, a, lda, mu, std, dq1, dq2, sums, B, A,
                       inv_global_B, sums_host, seq);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_actor_loss(const float* q1, const float* q2, const float* a, long lda, const float* mu, float std,
                   float* dq1, float* dq2, float* sums, int B, int A, float inv_global_B, hipStream_t st) {
  return drq_actor_loss_ex(q1, q2, a, lda, nullptr, 0, mu, std, 0.f, dq1, dq2, sums, B, A, inv_global_B, nullptr, 0u, st);
}

DRQ_API int drq_actor_loss_bc(const float* q1, const float* q2, const float* a, long lda, const float* a_beh, long ldb,
                              const float* mu, float std, float alpha, float* dq1, float* dq2, float* sums, int B, int A,
                              float inv_global_B, hipStream_t st) {
  if (!a_beh) return DRQ_EARG;
  return drq_actor_loss_ex(q1, q2, a, lda, a_beh, ldb, mu, std, alpha, dq1, dq2, sums, B, A, inv_global_B, nullptr, 0u,
                           st);
}

DRQ_API int drq_actor_dmu_bc(const float* dha1, const float* dha2, long ld, int col0, const float* mu, const float* act,
                             long lda, const float* a_beh, long ldb, float bc_scale, float* dpre, int B, int A,
                             hipStream_t st) {
  if (!dha1 || !dha2 || !mu || !act || !a_beh || !dpre || B <= 0 || A <= 0 || lda < A || ldb < A) return DRQ_EARG;
  hipLaunchKernelGGL(actor_dmu_bc_kernel, dim3((B * A + 255) / 256), dim3(256), 0, st, dha1, dha2, ld, col0, mu, act, lda,
                     a_beh, ldb, bc_scale, dpre, B, A);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_actor_dmu(const float* dha1, const float* dha2, long ld, int col0, const float* mu, float* dpre, int B,
                  int A, hipStream_t st) {
  if (!dha1 || !dha2 || !mu || !dpre || B <= 0 || A <= 0) return DRQ_EARG;
  hipLaunchKernelGGL(actor_dmu_kernel, dim3((B * A + 255) / 256), dim3(256), 0, st, dha1, dha2, ld, col0, mu, dpre,
                     B, A);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
