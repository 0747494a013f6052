// The device helpers of the priority sum tree, shared by per.hip (episode store) and vecreplay.hip (step-major ring).
// Layout and rules are the contract of include/drqv2_hip.h; the memory-ordering argument is per.hip's header comment:
// ONE workgroup of kPerThreads threads walks the levels with __syncthreads() between them, nothing crosses workgroups.
#pragma once
#include "common.h"

namespace {

constexpr int kPerThreads = 1024;

inline bool pow2(long x) { return x > 0 && (x & (x - 1)) == 0; }

// tree[k] = tree[2k] + tree[2k+1] for the ancestors of the leaf nodes [a, b], level by level up to the root
__device__ __forceinline__ void per_rebuild_range(double* tree, long a, long b) {
  while (a > 1) {
    a >>= 1;
    b >>= 1;
    __syncthreads();
    for (long k = a + threadIdx.x; k <= b; k += kPerThreads) tree[k] = tree[2 * k] + tree[2 * k + 1];
  }
}

// block-wide maximum of non-negative doubles; every thread gets it
__device__ __forceinline__ double per_block_max(double v, double* sm) {
  __syncthreads();
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int o = kPerThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + o]);
    __syncthreads();
  }
  return sm[0];
}

__device__ __forceinline__ double per_weight(double leaf, double total, double n_valid, double beta) {
  return pow(n_valid * leaf / total, -beta);
}

// what a priority update stores for an error: a NaN or negative error counts as 0, an infinite one as the largest
// float, so the root stays finite
__device__ __forceinline__ double per_priority(float td_abs, double alpha, double eps) {
  double t = (double)td_abs;
  if (!(t >= 0.0)) t = 0.0;
  t = fmin(t, 3.4028234663852886e38);
  return pow(t + eps, alpha);
}

}  // namespace
