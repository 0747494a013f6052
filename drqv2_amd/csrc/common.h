// Shared declarations for the DrQ-v2 HIP library (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

// The library is built with -fvisibility=hidden: only the entry points declared in include/drqv2_hip.h carry
// DRQ_API, which exports them with C linkage; everything else (kernels' host stubs, the cross-file launchers of
// internal.h) stays hidden and keeps C++ linkage.
#define DRQ_API extern "C" __attribute__((visibility("default")))

#define DRQ_OK 0
#define DRQ_EARG (-1)      // bad argument / unsupported shape
#define DRQ_EWS (-2)       // workspace too small

// every launcher returns 0 or the hipError_t of the launch (positive)
#define DRQ_LAUNCH_CHECK()                         \
  do {                                             \
    hipError_t e__ = hipGetLastError();            \
    if (e__ != hipSuccess) return (int)e__;        \
  } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));

static constexpr int kCout = 32;   // output channels of every encoder layer (geometry: kEncH, conv_plan.h)

// Per-device host-side caches (the CU count, "kernel attribute already set" flags) are indexed by the current HIP
// device: an agent on cuda:1 must not reuse what was established for cuda:0.
static constexpr int kMaxDevices = 64;
static inline int drq_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
  return dev;
}

// The CU count of the current device as every planner sees it: the override of drq_set_num_cus() where one is set, else
// the hardware's.  ONE definition and one cache for the whole library (device.hip), hidden like every internal function.
int drq_num_cus();

// raises Kernel's dynamic LDS limit to `bytes`, once per device (every instantiation has its own flags): 0 or the hipError_t
template <auto Kernel>
int drq_max_dynamic_lds(int bytes) {
  static bool done[kMaxDevices] = {};
  bool& d = done[drq_device()];
  if (d) return DRQ_OK;
  const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  d = e == hipSuccess;
  return (int)e;
}

// f(std::integral_constant<int, H>) for the H of HS... that equals h; DRQ_EARG where none does
template <int... HS, class F>
int drq_dispatch(int h, F&& f) {
  int rc = DRQ_EARG;
  (void)((h == HS && ((rc = f(std::integral_constant<int, HS>{})), true)) || ...);
  return rc;
}

// grid of a flat grid-stride kernel over n elements: one thread per element up to eight workgroups per CU
static inline unsigned drq_grid_for(long n, int block = 256) {
  long g = (n + block - 1) / block;
  const long cap = 8L * drq_num_cus();
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

// The murmur3 finaliser: the hash of the device environment's reset draws (vecenv.hip) and of the sign matrix of the
// exploration bonus (explore.hip); the contract of either spells it out (include/drqv2_hip.h).
__host__ __device__ __forceinline__ unsigned drq_fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// Metrics mirror (DrqStep.sums_host): eight floats and a sequence word in pinned (fine-grained, uncached) host memory,
// written by ONE lane.  A system-scope release before the sequence word would write back every dirty line of the XCD's
// L2 first (it is what makes OTHER threads' cached stores visible) -- measured: 3.5 us of the publishing launch at batch
// 256, 66 us at batch 2,048, on the path the host waits on.  Nothing cached has to become visible here: the lane's own
// system-scope stores go straight out; they are drained (vmcnt(0)) before the sequence word follows them down the same
// ordered path, and the "memory" clobbers keep the compiler from moving either across the wait.
#if defined(__HIPCC__)
__device__ __forceinline__ void drq_publish_mirror(float* host, const float (&v)[8], unsigned seq) {
#pragma unroll
  for (int i = 0; i < 8; ++i) __hip_atomic_store(host + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __hip_atomic_store(reinterpret_cast<unsigned*>(host + 8), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("" ::: "memory");
}
// DrQ+BC: the two sums of the BC actor loss travel in slots 9 and 10, ahead of the sequence word like the other eight
__device__ __forceinline__ void drq_publish_mirror_bc(float* host, const float (&v)[8], float bc_sq, float abs_q,
                                                      unsigned seq) {
  __hip_atomic_store(host + 9, bc_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(host + 10, abs_q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  drq_publish_mirror(host, v, seq);
}
#endif
