// LayerNorm+Tanh forward, backward and parameter gradients (drqv2.py:74-75), and the bias-gradient column sums.
// All reductions are fixed-order (no float atomics): results are run-to-run bit-stable.
#include "common.h"
#include "internal.h"
#include "device_sums.h"

namespace {

// ------------------------------------------------------------------------------------------------
// LayerNorm + tanh.  One wave per row, F <= 256.
// ------------------------------------------------------------------------------------------------
struct LnArgs {
  const float* z[4];      // [rows][ldz] pre-norm (bias already added)
  const float* gamma[4];
  const float* beta[4];
  float* out[4];          // [rows][ldo] tanh(LN(z))
  float* xhat[4];         // [rows][F] (may be null)
  float* rstd[4];         // [rows]   (may be null)
  int ldz[4], ldo[4];
  int rows, F;
  const float* tail[4];   // optional [rows][tail_ld]: copied into out columns [F, F+tail_n) (the [h, action] concat)
  int tail_ld[4];
  int tail_n;
  const float* part;      // optional: z is not given but split-K partials [n*splitk][rows][F] of the trunk GEMM
  const float* bias[4];   //           (gemm.hip layout) plus the layer bias; summed in splitk_reduce_kernel's order
  int splitk;
};

__global__ void ln_tanh_fwd_kernel(LnArgs a) {
  const int g = blockIdx.y;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  float v[4];
  float s = 0.f;
  if (a.part) {
    const long mn = (long)a.rows * a.F;
    const float* p = a.part + (long)g * a.splitk * mn + (long)row * a.F;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = lane + 64 * q;
      if (f < a.F) {
        v[q] = sum_partials(p + f, mn, a.splitk) + (a.bias[g] ? a.bias[g][f] : 0.f);
      } else {
        v[q] = 0.f;
      }
      s += v[q];
    }
  } else {
    const float* z = a.z[g] + (long)row * a.ldz[g];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = lane + 64 * q;
      v[q] = f < a.F ? z[f] : 0.f;
      s += v[q];
    }
  }
  const float mean = wave_sum(s) / (float)a.F;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int f = lane + 64 * q;
    const float d = f < a.F ? v[q] - mean : 0.f;
    ss += d * d;
  }
  const float var = wave_sum(ss) / (float)a.F;
  const float rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int f = lane + 64 * q;
    if (f < a.F) {
      const float xh = (v[q] - mean) * rstd;
      const float y = xh * a.gamma[g][f] + a.beta[g][f];
      a.out[g][(long)row * a.ldo[g] + f] = tanhf(y);
      if (a.xhat[g]) a.xhat[g][(long)row * a.F + f] = xh;
    }
  }
  if (lane == 0 && a.rstd[g]) a.rstd[g][row] = rstd;
  if (a.tail[g] && lane < a.tail_n) a.out[g][(long)row * a.ldo[g] + a.F + lane] = a.tail[g][(long)row * a.tail_ld[g] + lane];
}

struct LnBwdArgs {
  const float* dh0;     // [rows][ld0] gradient w.r.t. tanh output (source 0)
  const float* dh1;     // optional second source, summed
  const float* h;       // [rows][ldh] saved tanh output
  const float* xhat;    // [rows][F]
  const float* rstd;    // [rows]
  const float* gamma;
  float* dz;            // [rows][F]
  float* dln;           // [rows][F] scratch: gradient w.r.t. the LN output (for dgamma/dbeta)
  int ld0, ld1, ldh;
  int rows, F;
  // optional: the incoming gradient is given as split-K partials of `nprob` dgrad GEMMs ([nprob*splitk][rows][ldp],
  // gemm.hip layout) whose results are added (dh0/dh1 are then unused)
  const float* part;
  int splitk, nprob, ldp;
};

__global__ void ln_tanh_bwd_kernel(LnBwdArgs a) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= a.rows) return;
  float dxh[4], xh[4];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int f = lane + 64 * q;
    dxh[q] = 0.f;
    xh[q] = 0.f;
    if (f < a.F) {
      float d;
      if (a.part) {
        const long slab = (long)a.rows * a.ldp;
        const float* p = a.part + (long)row * a.ldp + f;
        d = sum_partials(p, slab, a.splitk);
        if (a.nprob > 1) d += sum_partials(p + (long)a.splitk * slab, slab, a.splitk);
      } else {
        d = a.dh0[(long)row * a.ld0 + f];
        if (a.dh1) d += a.dh1[(long)row * a.ld1 + f];
      }
      const float hv = a.h[(long)row * a.ldh + f];
      const float dl = d * (1.f - hv * hv);
      a.dln[(long)row * a.F + f] = dl;
      xh[q] = a.xhat[(long)row * a.F + f];
      dxh[q] = dl * a.gamma[f];
      s1 += dxh[q];
      s2 += dxh[q] * xh[q];
    }
  }
  const float m1 = wave_sum(s1) / (float)a.F;
  const float m2 = wave_sum(s2) / (float)a.F;
  const float rs = a.rstd[row];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int f = lane + 64 * q;
    if (f < a.F) a.dz[(long)row * a.F + f] = rs * (dxh[q] - m1 - xh[q] * m2);
  }
}

// dgamma[f] = sum_rows dln*xhat, dbeta[f] = sum_rows dln.  One block (256 threads) per column.
__global__ void ln_param_grad_kernel(const float* dln, const float* xhat, float* dgamma, float* dbeta, int rows,
                                     int F) {
  __shared__ float sg[256], sb[256];
  const int f = blockIdx.x;
  float g = 0.f, b = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const float d = dln[(long)r * F + f];
    g += d * xhat[(long)r * F + f];
    b += d;
  }
  sg[threadIdx.x] = g;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sg[threadIdx.x] += sg[threadIdx.x + o];
      sb[threadIdx.x] += sb[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    dgamma[f] = sg[0];
    dbeta[f] = sb[0];
  }
}

// ------------------------------------------------------------------------------------------------
// column sums (bias gradients): out[batch][n] = sum_m dy[batch][m][n].  Block = 64 columns x 4 row groups.
// ------------------------------------------------------------------------------------------------
// CW columns x 1024/CW row groups per workgroup: 64 x 16 for the batches of the reference's configs; from 1,024 rows on
// 16 x 64 (four times the workgroups and a quarter of the rows per thread: 21 -> 7 us for [2048][1024], five launches per
// bf16 update).  Fixed order either way.
template <int CW>
__global__ __launch_bounds__(1024) void colsum_kernel(const float* dy, long ld, long dy_bs, float* out, long out_bs,
                                                      int M, int N) {
  constexpr int NRG = 1024 / CW;
  __shared__ float s[NRG][CW];
  const int batch = blockIdx.y;
  const int c = threadIdx.x % CW;
  const int n = blockIdx.x * CW + c;
  const int rg = threadIdx.x / CW;
  const float* p = dy + batch * dy_bs;
  float a0 = 0.f, a1 = 0.f;
  if (n < N) {
    int m = rg;
    for (; m + NRG < M; m += 2 * NRG) {     // two independent chains, fixed order
      a0 += p[(long)m * ld + n];
      a1 += p[(long)(m + NRG) * ld + n];
    }
    if (m < M) a0 += p[(long)m * ld + n];
  }
  s[rg][c] = a0 + a1;
  __syncthreads();
  if (rg == 0 && n < N) {
    float t = 0.f;
#pragma unroll
    for (int g2 = 0; g2 < NRG; ++g2) t += s[g2][c];
    out[batch * out_bs + n] = t;
  }
}

}  // namespace

DRQ_API int drq_ln_tanh_fwd(const float* z, int ldz, const float* gamma, const float* beta, float* out, int ldo,
                    float* xhat, float* rstd, int rows, int F, hipStream_t st) {
  if (!z || !gamma || !beta || !out || rows <= 0 || F <= 0 || F > 256) return DRQ_EARG;
  LnArgs a{};
  a.z[0] = z; a.gamma[0] = gamma; a.beta[0] = beta; a.out[0] = out; a.xhat[0] = xhat; a.rstd[0] = rstd;
  a.ldz[0] = ldz; a.ldo[0] = ldo; a.rows = rows; a.F = F;
  hipLaunchKernelGGL(ln_tanh_fwd_kernel, dim3((rows + 3) / 4, 1), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// two LayerNorm+tanh problems of the same (rows, F) in one launch (actor trunk + critic trunk)
DRQ_API int drq_ln_tanh_fwd2(const float* z0, const float* z1, int ldz, const float* gamma0, const float* beta0,
                     const float* gamma1, const float* beta1, float* out0, int ldo0, float* out1, int ldo1,
                     float* xhat0, float* rstd0, float* xhat1, float* rstd1, int rows, int F, hipStream_t st) {
  if (!z0 || !z1 || !out0 || !out1 || rows <= 0 || F <= 0 || F > 256) return DRQ_EARG;
  LnArgs a{};
  a.z[0] = z0; a.gamma[0] = gamma0; a.beta[0] = beta0; a.out[0] = out0; a.xhat[0] = xhat0; a.rstd[0] = rstd0;
  a.z[1] = z1; a.gamma[1] = gamma1; a.beta[1] = beta1; a.out[1] = out1; a.xhat[1] = xhat1; a.rstd[1] = rstd1;
  a.ldz[0] = a.ldz[1] = ldz; a.ldo[0] = ldo0; a.ldo[1] = ldo1; a.rows = rows; a.F = F;
  hipLaunchKernelGGL(ln_tanh_fwd_kernel, dim3((rows + 3) / 4, 2), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_ln_tanh_bwd(const float* dh0, int ld0, const float* dh1, int ld1, const float* h, int ldh,
                    const float* xhat, const float* rstd, const float* gamma, float* dz, float* dln,
                    float* dgamma, float* dbeta, int rows, int F, hipStream_t st) {
  return drq_ln_tanh_bwd_part(dh0, ld0, dh1, ld1, h, ldh, xhat, rstd, gamma, dz, dln, dgamma, dbeta, rows, F, nullptr, 0,
                              0, 0, st);
}

// internal (step.hip): the incoming gradient may be the split-K partials of 1 or 2 dgrad GEMMs (see LnBwdArgs)
int drq_ln_tanh_bwd_part(const float* dh0, int ld0, const float* dh1, int ld1, const float* h, int ldh,
                         const float* xhat, const float* rstd, const float* gamma, float* dz, float* dln,
                         float* dgamma, float* dbeta, int rows, int F, const float* part, int splitk, int nprob,
                         int ldp, hipStream_t st) {
  // dgamma == dbeta == nullptr: the caller computes the parameter gradients elsewhere (from dln and xhat: the rider
  // workgroup of the trunk weight-gradient launch, or drq_ln_param_grad)
  if ((!dh0 && !part) || !h || !xhat || !rstd || !gamma || !dz || !dln || (!dgamma != !dbeta) || rows <= 0 || F <= 0 ||
      F > 256)
    return DRQ_EARG;
  if (part && (splitk < 1 || nprob < 1 || nprob > 2 || ldp < F)) return DRQ_EARG;
  LnBwdArgs a{dh0, dh1, h, xhat, rstd, gamma, dz, dln, ld0, ld1, ldh, rows, F, part, splitk, nprob, ldp};
  hipLaunchKernelGGL(ln_tanh_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  if (dgamma) {
    hipLaunchKernelGGL(ln_param_grad_kernel, dim3(F), dim3(256), 0, st, (const float*)dln, xhat, dgamma, dbeta, rows, F);
    DRQ_LAUNCH_CHECK();
  }
  return DRQ_OK;
}

// internal (step.hip): the parameter gradients alone
int drq_ln_param_grad(const float* dln, const float* xhat, float* dgamma, float* dbeta, int rows, int F, hipStream_t st) {
  if (!dln || !xhat || !dgamma || !dbeta || rows <= 0 || F <= 0 || F > 256) return DRQ_EARG;
  hipLaunchKernelGGL(ln_param_grad_kernel, dim3(F), dim3(256), 0, st, dln, xhat, dgamma, dbeta, rows, F);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// n (<= 4) LayerNorm+tanh problems of the same (rows, F) in one launch
DRQ_API int drq_ln_tanh_fwd_multi(int n, const float* const* z, int ldz, const float* const* gamma, const float* const* beta,
                          float* const* out, const int* ldo, float* const* xhat, float* const* rstd, int rows, int F,
                          hipStream_t st) {
  return drq_ln_tanh_fwd_multi_part(n, z, ldz, gamma, beta, out, ldo, xhat, rstd, rows, F, nullptr, nullptr, 0, nullptr,
                                    nullptr, 0, st);
}

// internal form used by the step: problem i may also copy tail_n (<= 64) columns of tail[i] behind its F outputs, and
// the pre-norm input may be given as split-K partials of the trunk GEMM (z may then be null)
int drq_ln_tanh_fwd_multi_part(int n, const float* const* z, int ldz, const float* const* gamma,
                               const float* const* beta, float* const* out, const int* ldo, float* const* xhat,
                               float* const* rstd, int rows, int F, const float* const* tail, const int* tail_ld,
                               int tail_n, const float* part, const float* const* bias, int splitk, hipStream_t st) {
  if (n <= 0 || n > 4 || (!z && !part) || !gamma || !beta || !out || !ldo || rows <= 0 || F <= 0 || F > 256)
    return DRQ_EARG;
  if (tail && (tail_n <= 0 || tail_n > 64 || !tail_ld)) return DRQ_EARG;
  if (part && splitk < 1) return DRQ_EARG;
  LnArgs a{};
  a.part = part;
  a.splitk = splitk;
  a.tail_n = tail ? tail_n : 0;
  for (int i = 0; i < n && tail; ++i) {
    a.tail[i] = tail[i];
    a.tail_ld[i] = tail_ld[i];
  }
  for (int i = 0; i < n; ++i) {
    if ((!part && !z[i]) || !gamma[i] || !beta[i] || !out[i]) return DRQ_EARG;
    a.z[i] = z ? z[i] : nullptr; a.gamma[i] = gamma[i]; a.beta[i] = beta[i]; a.out[i] = out[i];
    a.bias[i] = (part && bias) ? bias[i] : nullptr;
    a.xhat[i] = xhat ? xhat[i] : nullptr;
    a.rstd[i] = rstd ? rstd[i] : nullptr;
    a.ldz[i] = ldz; a.ldo[i] = ldo[i];
  }
  a.rows = rows; a.F = F;
  hipLaunchKernelGGL(ln_tanh_fwd_kernel, dim3((rows + 3) / 4, n), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_colsum(const float* dy, long ld, long dy_bs, float* out, long out_bs, int M, int N, int nbatch,
               hipStream_t st) {
  if (!dy || !out || M <= 0 || N <= 0 || nbatch <= 0) return DRQ_EARG;
  if (M >= 1024)
    hipLaunchKernelGGL(colsum_kernel<16>, dim3((N + 15) / 16, nbatch), dim3(1024), 0, st, dy, ld, dy_bs, out, out_bs, M, N);
  else
    hipLaunchKernelGGL(colsum_kernel<64>, dim3((N + 63) / 64, nbatch), dim3(1024), 0, st, dy, ld, dy_bs, out, out_bs, M, N);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
