// Fixed-order sums that more than one file's kernels share: across a wave, across a workgroup of 256, over the
// split-K partial records of a GEMM (layernorm.hip, policy_out.hip), and the batch sum of the DrQ+BC actor loss
// (losses.hip, qout.hip).  No float atomics anywhere: every caller gets the same bits run after run.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// sum of the split-K partial slabs of one GEMM output element, in splitk_reduce_kernel's association
// (gemm.hip): p points at the element in slab 0, consecutive slabs are `slab` floats apart
__device__ __forceinline__ float sum_partials(const float* p, long slab, int splitk) {
  // four interleaved chains (slab k goes to chain k & 3), then a tree: splitk_reduce_kernel's order.  16 slabs are
  // loaded per batch so that a thread pays one memory round trip per 16 slabs, not one per 4.
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int k0 = 0; k0 < splitk; k0 += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = p[(long)min(k0 + u, splitk - 1) * slab];
#pragma unroll
    for (int u = 0; u < 16; u += 4) {
      if (k0 + u < splitk) s0 += v[u];
      if (k0 + u + 1 < splitk) s1 += v[u + 1];
      if (k0 + u + 2 < splitk) s2 += v[u + 2];
      if (k0 + u + 3 < splitk) s3 += v[u + 3];
    }
  }
  return (s0 + s1) + (s2 + s3);
}

// block-wide fixed-order sum of up to 4 values (256 threads)
__device__ __forceinline__ void block_sum4(float (&v)[4], float (*sm)[256]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) sm[q][threadIdx.x] = v[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sm[q][threadIdx.x] += sm[q][threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = sm[q][0];
  __syncthreads();
}

// DrQ+BC (losses.hip): lambda = alpha / mean_i |min(q1,q2)_i| needs the sum of |min(q1,q2)| over the whole batch before
// any dq exists.  Every workgroup that needs it adds the B values itself, in ONE order whatever its size, so that every
// workgroup of every kernel form gets the same bits: chain t (t < 256) adds rows t, t + 256, ... in that order (16 rows
// requested per round trip), a wave adds its 64 chains (wave_sum), the four wave sums are added in index order.  Called
// by all threads of a workgroup of >= 256; scratch = 4 floats of LDS that nobody writes again before the caller's next
// barrier.
__device__ __forceinline__ float bc_abs_qmin_sum(const float* q1, const float* q2, int B, float* scratch) {
  if (threadIdx.x < 256) {
    float t = 0.f;
    for (int m0 = threadIdx.x; m0 < B; m0 += 16 * 256) {
      float x[16], y[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int m = min(m0 + 256 * u, B - 1);
        x[u] = q1[m];
        y[u] = q2[m];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (m0 + 256 * u < B) t += fabsf(fminf(x[u], y[u]));
    }
    t = wave_sum(t);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = t;
  }
  __syncthreads();
  return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

// -lambda / B_global from that sum: the one place the scale of dq is formed (both loss kernels call it)
__device__ __forceinline__ float bc_dq_scale(float alpha, int B, float sum_abs, float invB) {
  const float lambda = alpha * (float)B / sum_abs;
  return -(lambda * invB);
}

}  // namespace
