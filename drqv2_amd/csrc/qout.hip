// Output layer of the Q heads (drqv2.py:106,111), forward and backward; the backward can compute the TD loss
// (drqv2.py:185-189) or the actor loss (drqv2.py:212-216) inside it, with their prioritized and DrQ+BC forms (losses.hip
// has the same losses as launches of their own).  Fixed-order reductions: run-to-run bit-stable.
#include "common.h"
#include "internal.h"
#include "device_sums.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Output layer of a Q head (nn.Linear(hidden,1), drqv2.py:106,111): a GEMM with N = 1 is a row dot
// product; forward = one wave per row, backward = dgrad (outer product, ReLU-masked), wgrad and bias
// gradient in ONE pass over the hidden activations.  Up to 8 (net, head) problems per launch.
// ------------------------------------------------------------------------------------------------
struct QOutArgs {
  const float* h[8];    // [B][H] hidden activations (post-ReLU)
  const float* w[8];    // [H]
  const float* b[8];    // [1]
  float* q[8];          // [B]
  int B, H;
};

__global__ void qout_fwd_kernel(QOutArgs a) {
  const int z = blockIdx.y;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.B) return;
  const float* h = a.h[z] + (long)row * a.H;
  const float* w = a.w[z];
  float s0 = 0.f, s1 = 0.f;
  if (a.H <= 1024) {
    // all (up to) 32 loads of the row in flight at once; same summation order as the loop below
    float hv[16], wv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = min(lane + 64 * q, a.H - 1);
      hv[q] = h[i];
      wv[q] = (lane + 64 * q < a.H) ? w[i] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; q += 2) {
      s0 = __fmaf_rn(hv[q], wv[q], s0);
      s1 = __fmaf_rn(hv[q + 1], wv[q + 1], s1);
    }
  } else {
    int i = lane;
    for (; i + 64 < a.H; i += 128) {
      s0 = __fmaf_rn(h[i], w[i], s0);
      s1 = __fmaf_rn(h[i + 64], w[i + 64], s1);
    }
    if (i < a.H) s0 = __fmaf_rn(h[i], w[i], s0);
  }
  const float s = wave_sum(s0 + s1);
  if (lane == 0) a.q[z][row] = s + a.b[z][0];
}

struct QOutBwdArgs {
  const float* dq[8];   // [B]
  const float* h[8];    // [B][H]
  const float* w[8];    // [H]
  float* dh[8];         // [B][H] = dq*w masked by h > 0
  float* dw[8];         // [H] or null
  float* db[8];         // [1] or null
  int B, H;
  // optional fused TD loss (drqv2.py:185-189, two heads: z = 0, 1): dq is not given but computed per row from the
  // Q values; workgroup (0, 0) also leaves sums[0..4] like td_loss_kernel
  // td == 2: the actor loss instead (drqv2.py:212-216, actor_loss_kernel's arithmetic): dq routed to the smaller head,
  // ties split; workgroup (0, 0) leaves sums[5..6] and publishes all eight sums to the host mirror when one is given
  int td;
  const float *tq1, *tq2, *q1, *q2, *reward, *discount;
  float invB;
  float* sums;
  const float *act, *mu;   // td == 2: the sampled action [B][lda] and its mean [B][A]
  long lda;
  int A;
  float std;
  float* sums_host;
  unsigned seq;
  // BC form of td == 2 (qout_bwd_kernel<CW, true>): the behavioural action [B][ldb] and alpha
  const float* abeh;
  long ldb;
  float alpha;
  // weighted form of td == 1 (qout_bwd_kernel<CW, false, true>, prioritized replay): the importance weights [B] and
  // the per-sample error (|q1 - y| + |q2 - y|) / 2 [B] that workgroup (0, 0) leaves beside the sums
  const float* isw;
  float* td_abs;
};

// Workgroup = 64 columns x 16 row groups (1024 threads).  The per-row scalars dq[B] go to LDS once; the only global
// stream of the row loop is h, 16 rows of it in flight per thread.
// CW columns per workgroup, NRG = 1024 / CW row groups.  64 x 16 is the shape for batches up to a few hundred rows
// (16 workgroups per head at hidden_dim 1024); at batch 2,048 that left 32 workgroups walking 2,048 rows each (60 us per
// launch): 16 columns x 64 row groups gives four times as many (drq_qout_bwd_cw).  The row-group sums are added in
// the same fixed order either way (deterministic); the two shapes group them differently (rounding-level).
// BC (td == 2 only): the DrQ+BC actor loss, see bc_abs_qmin_sum; BC = false compiles to the kernel as it was.
// PW (td == 1 only): the TD loss weighted per row (td_loss_kernel<true>'s arithmetic); PW = false likewise.
template <int CW, bool BC, bool PW>
__global__ __launch_bounds__(1024) void qout_bwd_kernel(QOutBwdArgs a) {
  constexpr int NRG = 1024 / CW;
  extern __shared__ float dql[];            // [B] then NRG x CW + 64 floats of reduction scratch
  float* s = dql + a.B;
  float* sb = s + (a.td ? 5 * 1024 : 1024);
  const int z = blockIdx.y;
  const int c = threadIdx.x % CW, rg = threadIdx.x / CW;
  const int n = blockIdx.x * CW + c;
  const bool nok = n < a.H;
  const int nc = nok ? n : a.H - 1;
  const float* h = a.h[z];
  float* dh = a.dh[z];
  const float wn = a.w[z][nc];
  // the first 16 rows of h of this thread do not depend on dq: requested now, so that their round trip overlaps the
  // dq stage's (a kernel of this size is a chain of dependent memory round trips; every load issued late is one more)
  float hv0[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) hv0[u] = h[(long)min(rg + NRG * u, a.B - 1) * a.H + nc];
  float bc_sabs = 0.f;   // BC: sum |min(q1,q2)| over the batch, the same bits in every workgroup
  if (a.td == 2) {
    const float *qz = z == 0 ? a.q1 : a.q2, *qo = z == 0 ? a.q2 : a.q1;
    if constexpr (BC) {
      // the Q values of this thread's first four rows are requested before the batch sum, like hv0: only the scale waits
      float xq[4], yq[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = min((int)threadIdx.x + 1024 * u, a.B - 1);
        xq[u] = qz[m];
        yq[u] = qo[m];
      }
      bc_sabs = bc_abs_qmin_sum(a.q1, a.q2, a.B, sb);
      const float g = bc_dq_scale(a.alpha, a.B, bc_sabs, a.invB);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int m = threadIdx.x + 1024 * u;
        if (m < a.B) dql[m] = xq[u] < yq[u] ? g : (xq[u] == yq[u] ? 0.5f * g : 0.f);
      }
      for (int m = threadIdx.x + 4096; m < a.B; m += 1024) {
        const float x = qz[m], y = qo[m];
        dql[m] = x < y ? g : (x == y ? 0.5f * g : 0.f);
      }
    } else {
      const float g = -a.invB;
      for (int m = threadIdx.x; m < a.B; m += 1024) {
        const float x = qz[m], y = qo[m];
        dql[m] = x < y ? g : (x == y ? 0.5f * g : 0.f);
      }
    }
  } else if (a.td) {
    const float* qz = z == 0 ? a.q1 : a.q2;
    for (int m = threadIdx.x; m < a.B; m += 1024) {
      const float y = a.reward[m] + a.discount[m] * fminf(a.tq1[m], a.tq2[m]);
      if constexpr (PW) dql[m] = (2.f * (qz[m] - y) * a.invB) * a.isw[m];
      else dql[m] = 2.f * (qz[m] - y) * a.invB;
    }
  } else {
    const float* dq = a.dq[z];
    for (int m = threadIdx.x; m < a.B; m += 1024) dql[m] = dq[m];
  }
  __syncthreads();
  float acc = 0.f, bacc = 0.f;
  for (int m0 = rg; m0 < a.B; m0 += NRG * 16) {
    float hv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) hv[u] = m0 == rg ? hv0[u] : h[(long)min(m0 + NRG * u, a.B - 1) * a.H + nc];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int m = m0 + NRG * u;
      if (m < a.B) {
        const float d = dql[m];
        bacc += d;
        if (nok) dh[(long)m * a.H + n] = hv[u] > 0.f ? d * wn : 0.f;
        acc = __fmaf_rn(d, hv[u], acc);
      }
    }
  }
  s[rg * CW + c] = acc;
  if (c == 0) sb[rg] = bacc;
  __syncthreads();
  if (rg == 0) {
    if (a.dw[z] && nok) {
      float t = 0.f;
#pragma unroll
      for (int g2 = 0; g2 < NRG; ++g2) t += s[g2 * CW + c];
      a.dw[z][n] = t;
    }
    if (a.db[z] && blockIdx.x == 0 && c == 0) {
      float t = 0.f;
#pragma unroll
      for (int g2 = 0; g2 < NRG; ++g2) t += sb[g2];
      a.db[z][0] = t;
    }
  }
  // metric sums of the actor loss: workgroup (0, 0), the same fixed tree; then the host mirror
  if (a.td == 2 && blockIdx.x == 0 && z == 0) {
    __syncthreads();
    float v[3] = {0.f, 0.f, 0.f};   // v[2] (BC): sum (a - a_beh)^2, element by element like the log-probabilities
    const float log_std = logf(a.std);
    const float c0 = 0.91893853320467274178f;   // log(sqrt(2*pi))
    const float var2 = 2.f * a.std * a.std;
    for (int m = threadIdx.x; m < a.B; m += 1024) v[0] += -fminf(a.q1[m], a.q2[m]);
    // log-probabilities: element by element over the flattened [B][A] array, so that a wave reads consecutive addresses
    // (one row per lane reads 64 different cache lines per instruction, and this is ONE workgroup: 65 us at 2,048 rows
    // x 21 actions, measured).  Thread t adds elements t, t + 1024, ... in that order, then the fixed tree: deterministic;
    // the grouping differs from a row-by-row sum at rounding level.
    const int nel = a.B * a.A;
    for (int e0 = threadIdx.x; e0 < nel; e0 += 4 * 1024) {
      float av[4], mv[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * 1024 < nel ? e0 + u * 1024 : nel - 1;
        const int m = e / a.A, jj = e - m * a.A;
        av[u] = a.act[(long)m * a.lda + jj];
        mv[u] = a.mu[e];
        if constexpr (BC) bv[u] = a.abeh[(long)m * a.ldb + jj];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u * 1024 < nel) {
          const float d = av[u] - mv[u];
          v[1] += -(d * d) / var2 - log_std - c0;
          if constexpr (BC) {
            const float e = av[u] - bv[u];
            v[2] += e * e;
          }
        }
    }
    s[threadIdx.x] = v[0];
    s[1024 + threadIdx.x] = v[1];
    if constexpr (BC) s[2048 + threadIdx.x] = v[2];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) {
        s[threadIdx.x] += s[threadIdx.x + o];
        s[1024 + threadIdx.x] += s[1024 + threadIdx.x + o];
        if constexpr (BC) s[2048 + threadIdx.x] += s[2048 + threadIdx.x + o];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float s5 = s[0], s6 = s[1024];
      a.sums[5] = s5;
      a.sums[6] = s6;
      if constexpr (BC) {
        a.sums[9] = s[2048];
        a.sums[10] = bc_sabs;
      }
      if (a.sums_host) {   // metrics mirror (DrqStep.sums_host): all eight sums, then the sequence word
        float v8[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v8[i] = i == 5 ? s5 : (i == 6 ? s6 : a.sums[i]);
        if constexpr (BC) drq_publish_mirror_bc(a.sums_host, v8, s[2048], bc_sabs, a.seq);
        else drq_publish_mirror(a.sums_host, v8, a.seq);
      }
    }
  }
  // metric sums of the TD loss: workgroup (0, 0), per-thread partials over rows tid, tid+1024, ... then a fixed tree
  if (a.td == 1 && blockIdx.x == 0 && z == 0) {
    __syncthreads();
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int m = threadIdx.x; m < a.B; m += 1024) {
      const float r = a.reward[m];
      const float y = r + a.discount[m] * fminf(a.tq1[m], a.tq2[m]);
      const float e1 = a.q1[m] - y, e2 = a.q2[m] - y;
      if constexpr (PW) {
        v[0] += r; v[1] += y; v[2] += a.q1[m]; v[3] += a.q2[m]; v[4] += a.isw[m] * (e1 * e1 + e2 * e2);
        a.td_abs[m] = 0.5f * (fabsf(e1) + fabsf(e2));
      } else {
        v[0] += r; v[1] += y; v[2] += a.q1[m]; v[3] += a.q2[m]; v[4] += e1 * e1 + e2 * e2;
      }
    }
    // one tree for the five sums (scratch: 5 x 1024 floats behind dq)
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q * 1024 + threadIdx.x] = v[q];
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) {
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q * 1024 + threadIdx.x] += s[q * 1024 + threadIdx.x + o];
      }
      __syncthreads();
    }
    if (threadIdx.x < 5) a.sums[threadIdx.x] = s[threadIdx.x * 1024];
  }
}

// What every backward launch shares.  The caller has set the loss fields of `a` (a.td and what goes with it); this adds
// the nz problems' pointers and the shape, sizes the LDS (the sums tree of a loss needs 5 x 1024 floats, the plain form
// 1024) and picks the kernel: 64 columns per workgroup below 1,024 rows, 16 beyond (see qout_bwd_kernel).
template <bool BC = false, bool PW = false>
int launch_qout_bwd(QOutBwdArgs& a, int nz, const float* const* h, const float* const* w, float* const* dh,
                    float* const* dw, float* const* db, int B, int H, hipStream_t st) {
  if (!h || !w || !dh || B <= 0 || H <= 0) return DRQ_EARG;
  for (int z = 0; z < nz; ++z) {
    if (!h[z] || !w[z] || !dh[z]) return DRQ_EARG;
    a.h[z] = h[z]; a.w[z] = w[z]; a.dh[z] = dh[z];
    a.dw[z] = dw ? dw[z] : nullptr;
    a.db[z] = db ? db[z] : nullptr;
  }
  a.B = B; a.H = H;
  const size_t lds = ((size_t)B + (a.td ? 5 * 1024 : 1024) + 64) * sizeof(float);
  if (lds > 60 * 1024) return DRQ_EARG;
  if (B >= 1024) hipLaunchKernelGGL((qout_bwd_kernel<16, BC, PW>), dim3((H + 15) / 16, nz), dim3(1024), lds, st, a);
  else hipLaunchKernelGGL((qout_bwd_kernel<64, BC, PW>), dim3((H + 63) / 64, nz), dim3(1024), lds, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

}  // namespace

// nz (<= 8) Q-head output layers in one launch; host arrays of device pointers
DRQ_API int drq_qout_fwd(int nz, const float* const* h, const float* const* w, const float* const* b, float* const* q, int B,
                 int H, hipStream_t st) {
  if (nz <= 0 || nz > 8 || !h || !w || !b || !q || B <= 0 || H <= 0) return DRQ_EARG;
  QOutArgs a{};
  for (int z = 0; z < nz; ++z) {
    if (!h[z] || !w[z] || !b[z] || !q[z]) return DRQ_EARG;
    a.h[z] = h[z]; a.w[z] = w[z]; a.b[z] = b[z]; a.q[z] = q[z];
  }
  a.B = B; a.H = H;
  hipLaunchKernelGGL(qout_fwd_kernel, dim3((B + 3) / 4, nz), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// dh = (dq w^T) * (h > 0);  dw = dq^T h, db = sum dq when the dw/db arrays are given
DRQ_API int drq_qout_bwd(int nz, const float* const* dq, const float* const* h, const float* const* w, float* const* dh,
                 float* const* dw, float* const* db, int B, int H, hipStream_t st) {
  if (nz <= 0 || nz > 8 || !dq) return DRQ_EARG;
  QOutBwdArgs a{};
  for (int z = 0; z < nz; ++z) {
    if (!dq[z]) return DRQ_EARG;
    a.dq[z] = dq[z];
  }
  return launch_qout_bwd(a, nz, h, w, dh, dw, db, B, H, st);
}

// internal (step.hip): the twin-Q output layer backward with the TD loss (drq_td_mse) computed inside it:
// dq1/dq2 never exist in memory, sums[0..4] are written by the same launch.  is_weight and td_abs given: the loss
// weighted per row (prioritized replay): dq_k[i] carries is_weight[i], sums[4] is the weighted sum, td_abs[i] =
// (|q1 - y| + |q2 - y|) / 2 is written by workgroup (0, 0).  Both null: the plain loss.
int drq_qout_bwd_td(const float* tq1, const float* tq2, const float* q1, const float* q2, const float* reward,
                    const float* discount, const float* is_weight, float inv_global_B, float* sums, float* td_abs,
                    const float* const* h, const float* const* w, float* const* dh, float* const* dw, float* const* db,
                    int B, int H, hipStream_t st) {
  if (!tq1 || !tq2 || !q1 || !q2 || !reward || !discount || !sums || (!is_weight != !td_abs)) return DRQ_EARG;
  QOutBwdArgs a{};
  a.td = 1; a.tq1 = tq1; a.tq2 = tq2; a.q1 = q1; a.q2 = q2; a.reward = reward; a.discount = discount;
  a.invB = inv_global_B; a.sums = sums;
  a.isw = is_weight; a.td_abs = td_abs;
  return is_weight ? launch_qout_bwd<false, true>(a, 2, h, w, dh, dw, db, B, H, st)
                   : launch_qout_bwd(a, 2, h, w, dh, dw, db, B, H, st);
}

// internal (step.hip, single-GPU schedule): the same backward (input gradient only) with the actor loss (drq_actor_loss)
// computed inside it: sums[5..6] and the host mirror, when one is given, are written by workgroup (0, 0) of this
// launch.  a_beh != null: the DrQ+BC loss (mirror slots 0..7, 9, 10, then 8); null: the plain loss, ldb and alpha unused.
int drq_qout_bwd_actor(const float* q1, const float* q2, const float* act, long lda, const float* a_beh, long ldb,
                       const float* mu, float std, float alpha, int A, float inv_global_B, float* sums,
                       float* sums_host, unsigned seq, const float* const* h, const float* const* w, float* const* dh,
                       int B, int H, hipStream_t st) {
  if (!q1 || !q2 || !act || !mu || !sums || A <= 0) return DRQ_EARG;
  if (a_beh && (lda < A || ldb < A || !(alpha > 0.f))) return DRQ_EARG;
  QOutBwdArgs a{};
  a.td = 2; a.q1 = q1; a.q2 = q2; a.invB = inv_global_B; a.sums = sums;
  a.act = act; a.lda = lda; a.mu = mu; a.A = A; a.std = std; a.sums_host = sums_host; a.seq = seq;
  if (a_beh) {
    a.abeh = a_beh; a.ldb = ldb; a.alpha = alpha;
    return launch_qout_bwd<true>(a, 2, h, w, dh, nullptr, nullptr, B, H, st);
  }
  return launch_qout_bwd(a, 2, h, w, dh, nullptr, nullptr, B, H, st);
}

DRQ_API int drq_qout_bwd_actor_bc(const float* q1, const float* q2, const float* act, long lda, const float* a_beh,
                                  long ldb, const float* mu, float std, float alpha, int A, float inv_global_B,
                                  float* sums, const float* const* h, const float* const* w, float* const* dh, int B,
                                  int H, hipStream_t st) {
  if (!a_beh) return DRQ_EARG;
  return drq_qout_bwd_actor(q1, q2, act, lda, a_beh, ldb, mu, std, alpha, A, inv_global_B, sums, nullptr, 0u, h, w, dh, B,
                            H, st);
}
