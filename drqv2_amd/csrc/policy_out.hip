// Output layer of the policy (drqv2.py:81,86-90), forward with the TruncatedNormal sample (utils.py:117-126) and
// backward with its DrQ+BC form.  Fixed-order reductions: run-to-run bit-stable.
#include "common.h"
#include "internal.h"
#include "device_sums.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Policy output layer Linear(H, A) (drqv2.py:81,86-90), A <= 64.  Forward: one wave per row computes the A dot
// products (row in registers, W3 rows from L1), adds the bias and -- for rows >= srow0 when a noise table is
// given -- samples the action (tanh, clipped noise, straight-through clamp: utils.py:117-126) in the same pass.
// Backward: dpre = (da1+da2)(1-mu^2), then dp2 = (dpre W3)*(p2>0), dW3 = dpre^T p2, db3 = sum dpre in one kernel.
// Both replace a GEMM with N or M = action_dim (plus split-K reduce and elementwise launches).
// ------------------------------------------------------------------------------------------------
struct PolOutArgs {
  const float* h2;      // [rows][H]
  const float* w;       // [A][H]
  const float* b;       // [A]
  float* p3;            // [rows][A] pre-tanh output
  const float* noise;   // [rows - srow0][A] or null
  float* mu_out;        // [rows - srow0][A] or null
  float* a_out;         // action columns of the critic input, row stride lda_out
  long lda_out;
  int rows, H, A, srow0, use_clip;
  float std, clip;
  // optional second sampling job for rows [0, srow0): its own noise table and outputs (the actor update's action
  // for the obs rows, drqv2.py:210-211, drawn from the same policy output)
  const float* noise0;
  float* mu_out0;
  float* a_out0;
  long lda_out0;
};

__global__ void policy_out_kernel(PolOutArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  const float* h = a.h2 + (long)row * a.H;
  float mine = 0.f;
  if (a.H <= 1024) {
    // the row in 16 registers; the weights of 2 outputs (32 loads) in flight per round trip
    float hv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) hv[q] = (lane + 64 * q < a.H) ? h[lane + 64 * q] : 0.f;
    for (int j = 0; j < a.A; j += 2) {
      const int j1 = j + 1 < a.A ? j + 1 : j;
      const float* w0 = a.w + (long)j * a.H;
      const float* w1 = a.w + (long)j1 * a.H;
      float x0[16], x1[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int i = min(lane + 64 * q, a.H - 1);      // hv is 0 past H: the clamped weight does not matter
        x0[q] = w0[i];
        x1[q] = w1[i];
      }
      float s0 = 0.f, s1 = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        s0 = __fmaf_rn(hv[q], x0[q], s0);
        s1 = __fmaf_rn(hv[q], x1[q], s1);
      }
      s0 = wave_sum(s0) + a.b[j];
      s1 = wave_sum(s1) + a.b[j1];
      if (lane == j) mine = s0;
      if (lane == j + 1) mine = s1;
    }
  } else {
    for (int j = 0; j < a.A; ++j) {
      const float* w = a.w + (long)j * a.H;
      float s0 = 0.f;
      for (int i = lane; i < a.H; i += 64) s0 = __fmaf_rn(h[i], w[i], s0);
      const float s = wave_sum(s0) + a.b[j];
      if (lane == j) mine = s;
    }
  }
  if (lane >= a.A) return;
  a.p3[(long)row * a.A + lane] = mine;
  const bool hi_job = a.noise && row >= a.srow0, lo_job = a.noise0 && row < a.srow0;
  if (hi_job || lo_job) {
    const long r = hi_job ? row - a.srow0 : row;
    const float* nz = hi_job ? a.noise : a.noise0;
    float* mo = hi_job ? a.mu_out : a.mu_out0;
    float* ao = hi_job ? a.a_out : a.a_out0;
    const long ld = hi_job ? a.lda_out : a.lda_out0;
    const float mu = tanhf(mine);
    float eps = nz[r * a.A + lane] * a.std;
    if (a.use_clip) eps = fminf(fmaxf(eps, -a.clip), a.clip);
    const float lo = (float)(-1.0 + 1e-6), hi = (float)(1.0 - 1e-6);
    if (mo) mo[r * a.A + lane] = mu;
    ao[r * ld + lane] = fminf(fmaxf(mu + eps, lo), hi);
  }
}

struct PolBwdArgs {
  const float* da1;     // [B][ld]: action-column gradient from Q head 1 (columns col0..col0+A)
  const float* da2;
  long ld;
  int col0;
  const float* mu;      // [B][A]
  const float* p2;      // [B][H] post-ReLU input of the layer
  const float* w;       // [A][H]
  float* dp2;           // [B][H]
  float* dw;            // [A][H]
  float* db;            // [A]
  int B, H, A;
  const float* part;    // optional: da1/da2 as split-K partials [2*splitk][B][A] of the two dgrad GEMMs
  int splitk;
  // BC form (policy_out_bwd_kernel<.., true>): dmu also gets bc_scale (act - abeh), see actor_dmu_bc_kernel
  const float* act;     // [B][lda] the sampled action
  long lda;
  const float* abeh;    // [B][ldb] the behavioural action
  long ldb;
  float bc_scale;
};

constexpr int kPolMaxA = 32;

// Workgroup = CW columns of H x NRG = 1024 / CW row groups.  dpre[B][A] (tiny) is computed once per workgroup into LDS;
// the only global stream in the row loop is p2, up to 16 rows of it in flight per thread.  CW = 16 (64 workgroups at
// hidden_dim 1024) is what the update uses: with 64 columns the launch kept 16 CUs busy with 2*A FMAs per row and
// thread -- 14.6 us at A = 6, 40 us at A = 21 (batch 256), 47 us at A = 12 (batch 512); CW = 64 remains for tiny H.
// AMAX: action_dim rounded up to 8 / 16 / 32 (the per-output loops are unrolled over it); BC: the DrQ+BC pull in dmu
template <int AMAX, int CW, bool BC>
__global__ __launch_bounds__(1024) void policy_out_bwd_kernel(PolBwdArgs a) {
  constexpr int NRG = 1024 / CW;
  extern __shared__ float dpre[];           // [B][A], then 4 x NRG x CW = 4096 floats of reduction scratch
  float* sm = dpre + a.B * a.A;
  const int c = threadIdx.x % CW, rg = threadIdx.x / CW;
  const int n = blockIdx.x * CW + c;
  const bool nok = n < a.H;
  const int nc = nok ? n : a.H - 1;
  // first batch of p2 rows: independent of dpre, requested before the dpre stage (see qout_bwd_kernel)
  float hv0[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) hv0[u] = a.p2[(long)min(rg + NRG * u, a.B - 1) * a.H + nc];
  for (int i = threadIdx.x; i < a.B * a.A; i += 1024) {
    const int m = i / a.A, j = i - m * a.A;
    const float mv = a.mu[i];
    float pull = 0.f;
    if constexpr (BC) pull = a.act[(long)m * a.lda + j] - a.abeh[(long)m * a.ldb + j];
    float d1, d2;
    if (a.part) {
      const long slab = (long)a.B * a.A;
      d1 = sum_partials(a.part + i, slab, a.splitk);
      d2 = sum_partials(a.part + (long)a.splitk * slab + i, slab, a.splitk);
    } else {
      d1 = a.da1[(long)m * a.ld + a.col0 + j];
      d2 = a.da2[(long)m * a.ld + a.col0 + j];
    }
    if constexpr (BC) dpre[i] = __fmaf_rn(pull, a.bc_scale, d1 + d2) * (1.f - mv * mv);
    else dpre[i] = (d1 + d2) * (1.f - mv * mv);
  }
  float wn[AMAX], acc[AMAX];
#pragma unroll
  for (int j = 0; j < AMAX; ++j) {
    wn[j] = j < a.A ? a.w[(long)j * a.H + nc] : 0.f;
    acc[j] = 0.f;
  }
  __syncthreads();
  for (int m0 = rg; m0 < a.B; m0 += NRG * 16) {
    float hv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) hv[u] = m0 == rg ? hv0[u] : a.p2[(long)min(m0 + NRG * u, a.B - 1) * a.H + nc];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int m = m0 + NRG * u;
      if (m < a.B) {
        const float* dp = dpre + m * a.A;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < AMAX; ++j) {
          if (j < a.A) {
            const float dv = dp[j];
            d = __fmaf_rn(dv, wn[j], d);
            acc[j] = __fmaf_rn(dv, hv[u], acc[j]);
          }
        }
        if (nok) a.dp2[(long)m * a.H + n] = hv[u] > 0.f ? d : 0.f;
      }
    }
  }
  // dW3: the row groups of a column are summed in order through LDS, FOUR output rows per barrier pair (one at a
  // time cost two workgroup barriers per action dimension: 21 rounds for humanoid_run)
  for (int j0 = 0; j0 < a.A; j0 += 4) {
#pragma unroll
    for (int q = 0; q < AMAX; ++q)
      if (q >= j0 && q < j0 + 4 && q < a.A) sm[((q - j0) * NRG + rg) * CW + c] = acc[q];
    __syncthreads();
    if (threadIdx.x < 4 * CW) {
      const int jj = threadIdx.x / CW;                 // c = threadIdx.x % CW here as well
      if (j0 + jj < a.A && nok) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < NRG; ++g) t += sm[(jj * NRG + g) * CW + c];
        a.dw[(long)(j0 + jj) * a.H + n] = t;
      }
    }
    __syncthreads();
  }
  // db3: workgroup 0; thread t sums rows t/32, t/32 + 32, ... of dpre[:, t%32], the 32 partials are added in order
  if (blockIdx.x == 0) {
    const int jb = threadIdx.x & 31, gb = threadIdx.x >> 5;
    float t = 0.f;
    if (jb < a.A)
      for (int m = gb; m < a.B; m += 32) t += dpre[m * a.A + jb];
    sm[gb * 32 + jb] = t;
    __syncthreads();
    if (gb == 0 && jb < a.A) {
      float tot = 0.f;
#pragma unroll
      for (int g = 0; g < 32; ++g) tot += sm[g * 32 + jb];
      a.db[jb] = tot;
    }
  }
}

template <bool BC>
void launch_policy_out_bwd(const PolBwdArgs& a, size_t lds, hipStream_t st) {
  const int H = a.H, A = a.A;
  if (H >= 256) {          // 16 columns per workgroup
    const dim3 g((H + 15) / 16);
    if (A <= 8) hipLaunchKernelGGL((policy_out_bwd_kernel<8, 16, BC>), g, dim3(1024), lds, st, a);
    else if (A <= 16) hipLaunchKernelGGL((policy_out_bwd_kernel<16, 16, BC>), g, dim3(1024), lds, st, a);
    else hipLaunchKernelGGL((policy_out_bwd_kernel<32, 16, BC>), g, dim3(1024), lds, st, a);
  } else {
    const dim3 g((H + 63) / 64);
    if (A <= 8) hipLaunchKernelGGL((policy_out_bwd_kernel<8, 64, BC>), g, dim3(1024), lds, st, a);
    else if (A <= 16) hipLaunchKernelGGL((policy_out_bwd_kernel<16, 64, BC>), g, dim3(1024), lds, st, a);
    else hipLaunchKernelGGL((policy_out_bwd_kernel<32, 64, BC>), g, dim3(1024), lds, st, a);
  }
}

}  // namespace

// internal (step.hip): policy output layer forward (+ optional action sampling) and backward, see the kernels
int drq_policy_out_fwd(const float* h2, const float* w, const float* b, float* p3, int rows, int H, int A,
                       const float* noise, float std, float clip, int use_clip, int srow0, float* mu_out,
                       float* a_out, long lda_out, const float* noise0, float* mu_out0, float* a_out0, long lda_out0,
                       hipStream_t st) {
  if (!h2 || !w || !b || !p3 || rows <= 0 || H <= 0 || A <= 0 || A > 64) return DRQ_EARG;
  if (noise && (!a_out || srow0 < 0 || srow0 > rows)) return DRQ_EARG;
  if (noise0 && (!a_out0 || !noise)) return DRQ_EARG;
  PolOutArgs a{h2, w, b, p3, noise, mu_out, a_out, lda_out, rows, H, A, srow0, use_clip, std, clip,
               noise0, mu_out0, a_out0, lda_out0};
  hipLaunchKernelGGL(policy_out_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// a_beh != null: the DrQ+BC pull in dmu (see actor_dmu_bc_kernel): act [B][lda], a_beh [B][ldb]; null: the plain
// backward, the other four BC arguments unused
int drq_policy_out_bwd(const float* da1, const float* da2, long ld, int col0, const float* mu, const float* act,
                       long lda, const float* a_beh, long ldb, float bc_scale, const float* p2, const float* w,
                       float* dp2, float* dw, float* db, int B, int H, int A, const float* part, int splitk,
                       hipStream_t st) {
  if (((!da1 || !da2) && !part) || !mu || !p2 || !w || !dp2 || !dw || !db || B <= 0 || H <= 0 || A <= 0 ||
      A > kPolMaxA)
    return DRQ_EARG;
  if (a_beh && (!act || lda < A || ldb < A)) return DRQ_EARG;
  if (part && splitk < 1) return DRQ_EARG;
  const size_t lds = ((size_t)B * A + 4 * 16 * 64) * sizeof(float);
  if (lds > 60 * 1024) return DRQ_EARG;
  PolBwdArgs a{da1, da2, ld, col0, mu, p2, w, dp2, dw, db, B, H, A, part, splitk};
  if (a_beh) {
    a.act = act; a.lda = lda; a.abeh = a_beh; a.ldb = ldb; a.bc_scale = bc_scale;
    launch_policy_out_bwd<true>(a, lds, st);
  } else {
    launch_policy_out_bwd<false>(a, lds, st);
  }
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_policy_out_bwd_bc(const float* da1, const float* da2, long ld, int col0, const float* mu,
                                  const float* act, long lda, const float* a_beh, long ldb, float bc_scale,
                                  const float* p2, const float* w, float* dp2, float* dw, float* db, int B, int H, int A,
                                  const float* part, int splitk, hipStream_t st) {
  if (!act || !a_beh) return DRQ_EARG;
  return drq_policy_out_bwd(da1, da2, ld, col0, mu, act, lda, a_beh, ldb, bc_scale, p2, w, dp2, dw, db, B, H, A, part,
                            splitk, st);
}
