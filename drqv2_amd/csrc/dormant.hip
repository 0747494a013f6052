// DrM building blocks (contract: include/drqv2_hip.h, "dormant ratio and perturbation"; new functionality, the reference
// has neither).  Three small HBM-bound passes, all deterministic: fixed summation orders, no float atomics.
//
//   drq_dormant_scores   score[j] = (sum_b |act[b][j]|) / rows -- the layout of colsum_kernel (layernorm.hip): a
//                        workgroup owns CW columns, its 1024 / CW row groups add their rows in two chains each, the
//                        row-group sums are added in index order.  64 x 16 below 1,024 rows, 16 x 64 from there on.
//   drq_dormant_count    ONE workgroup of 256 threads: the layer mean m in a fixed order (chain t adds scores t, t + 256,
//                        ...; the 256 chains are halved 128, 64, ..., 1), then the units with score <= tau * m.  Thread 0
//                        ADDS the two counts to count[0..1]: launches on one stream are ordered, so several layers
//                        accumulate into one pair and the host never reads a partial result.
//   drq_lerp_flat        p[i] = fmaf(a, p[i], (1 - a) * p0[i]) over a flat arena: 16-byte loads where p and p0 are
//                        misaligned by the same amount (scalar head up to the first 16-byte boundary, scalar tail), scalar
//                        loads throughout where they are not.
// All stores are plain vector stores.
#include "internal.h"
#include "../../include/drqv2_hip.h"

namespace {

template <int CW>
__global__ __launch_bounds__(1024) void dormant_scores_kernel(const float* act, long ld, int rows, int units,
                                                              float* score) {
  constexpr int NRG = 1024 / CW;
  __shared__ float s[NRG][CW];
  const int c = threadIdx.x % CW;
  const int n = blockIdx.x * CW + c;
  const int rg = threadIdx.x / CW;
  float a0 = 0.f, a1 = 0.f;
  if (n < units) {
    int m = rg;
    for (; m + NRG < rows; m += 2 * NRG) {     // two independent chains, fixed order
      a0 += fabsf(act[(long)m * ld + n]);
      a1 += fabsf(act[(long)(m + NRG) * ld + n]);
    }
    if (m < rows) a0 += fabsf(act[(long)m * ld + n]);
  }
  s[rg][c] = a0 + a1;
  __syncthreads();
  if (rg == 0 && n < units) {
    float t = 0.f;
#pragma unroll
    for (int g2 = 0; g2 < NRG; ++g2) t += s[g2][c];
    score[n] = t / (float)rows;
  }
}

constexpr int kCountThreads = 256;

__global__ __launch_bounds__(kCountThreads) void dormant_count_kernel(const float* score, int units, float tau,
                                                                      int* count, float* layer_mean) {
  __shared__ float sf[kCountThreads];
  __shared__ int si[kCountThreads];
  const int t = threadIdx.x;
  float c = 0.f;
  for (int j = t; j < units; j += kCountThreads) c += score[j];
  sf[t] = c;
  __syncthreads();
  for (int o = kCountThreads / 2; o > 0; o >>= 1) {
    if (t < o) sf[t] += sf[t + o];
    __syncthreads();
  }
  const float m = sf[0] / (float)units;
  const float thr = __fmul_rn(tau, m);
  int nd = 0;
  for (int j = t; j < units; j += kCountThreads) nd += (m == 0.f || score[j] <= thr) ? 1 : 0;
  si[t] = nd;
  __syncthreads();
  for (int o = kCountThreads / 2; o > 0; o >>= 1) {
    if (t < o) si[t] += si[t + o];
    __syncthreads();
  }
  if (t == 0) {
    count[0] += si[0];
    count[1] += units;
    if (layer_mean) layer_mean[0] = m;
  }
}

__device__ __forceinline__ float lerp1(float x, float x0, float a, float b) {
  const float q = __fmul_rn(b, x0);
  return a == 0.f ? q : __fmaf_rn(a, x, q);    // a == 0: p0 itself, whatever p held (0 * inf would be NaN)
}

// elements [0, head) and [head + 4 nvec, n) one by one, [head, head + 4 nvec) as nvec 16-byte vectors (p + head and
// p0 + head are 16-byte aligned when nvec > 0)
__global__ __launch_bounds__(256) void lerp_kernel(float* p, const float* p0, long n, long head, long nvec, float a,
                                                   float b) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  f32x4* pv = reinterpret_cast<f32x4*>(p + head);
  const f32x4* qv = reinterpret_cast<const f32x4*>(p0 + head);
  for (long i = gid; i < nvec; i += stride) {
    const f32x4 x = pv[i], x0 = qv[i];
    f32x4 y;
    y.x = lerp1(x.x, x0.x, a, b);
    y.y = lerp1(x.y, x0.y, a, b);
    y.z = lerp1(x.z, x0.z, a, b);
    y.w = lerp1(x.w, x0.w, a, b);
    pv[i] = y;
  }
  const long nscal = n - 4 * nvec;
  for (long s = gid; s < nscal; s += stride) {
    const long i = s < head ? s : s + 4 * nvec;
    p[i] = lerp1(p[i], p0[i], a, b);
  }
}

inline unsigned lerp_grid(long work) {
  long g = (work + 255) / 256;
  const long cap = 8L * drq_num_cus();
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

DRQ_API int drq_dormant_scores(const float* act, long ld, int rows, int units, float* score, drq_stream_t stream) {
  if (!act || !score || rows <= 0 || units <= 0 || ld < units) return DRQ_EARG;
  hipStream_t st = (hipStream_t)stream;
  if (rows >= 1024)
    hipLaunchKernelGGL(dormant_scores_kernel<16>, dim3((units + 15) / 16), dim3(1024), 0, st, act, ld, rows, units, score);
  else
    hipLaunchKernelGGL(dormant_scores_kernel<64>, dim3((units + 63) / 64), dim3(1024), 0, st, act, ld, rows, units, score);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_dormant_count(const float* score, int units, float tau, int* count, float* layer_mean,
                              drq_stream_t stream) {
  if (!score || !count || units <= 0 || !(tau >= 0.f) || tau > 3.0e38f) return DRQ_EARG;
  hipLaunchKernelGGL(dormant_count_kernel, dim3(1), dim3(kCountThreads), 0, (hipStream_t)stream, score, units, tau, count,
                     layer_mean);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_lerp_flat(float* p, const float* p0, long n, float a, drq_stream_t stream) {
  if (n < 0 || !(a >= 0.f && a <= 1.f)) return DRQ_EARG;
  if (n == 0) return DRQ_OK;
  if (!p || !p0 || (((uintptr_t)p | (uintptr_t)p0) & 3)) return DRQ_EARG;
  if (a == 1.f) return DRQ_OK;                 // the identity: nothing is launched, p keeps its bits (-0 and NaNs too)
  long head = 0, nvec = 0;
  if ((((uintptr_t)p ^ (uintptr_t)p0) & 15) == 0) {
    head = (long)(((16 - ((uintptr_t)p & 15)) & 15) / 4);
    if (head > n) head = n;
    nvec = (n - head) / 4;
  }
  const long work = nvec > n - 4 * nvec ? nvec : n - 4 * nvec;
  hipLaunchKernelGGL(lerp_kernel, dim3(lerp_grid(work)), dim3(256), 0, (hipStream_t)stream, p, p0, n, head, nvec, a,
                     1.0f - a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
