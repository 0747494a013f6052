// Frame stacks out of a single-frame step-major ring (contract: include/drqv2_hip.h, "single-frame step-major replay").
// New functionality: the reference stacks frames in the environment wrapper (dmc.py:87-109) and stores every stack
// whole; here a slot holds the one new frame of its step and the stack is put together where it is read.
//
// drq_vec_stack_gather is one launch of n x 3 workgroups: workgroup (b, g) copies frame g (0 = oldest) of stack b in
// 16-byte pieces.  Which slot that is follows from the newest frame's slot and at most two `first` bytes
// (ring_stack_slots, replay_device.h: shared with the fused aug+conv1 launch, which gathers the same stacks on its own);
// every lane reads the same bytes, so the loads are broadcast.  Plain vector loads and stores, no atomics.
#include "common.h"
#include "replay_device.h"
#include "../../include/drqv2_hip.h"

namespace {

struct StackGatherArgs {
  const uint8_t* frames;
  const uint8_t* first;
  const long* slots;      // null: the slots of ring row `row`, environment b
  uint8_t* out;
  long R, N, row, frame_bytes;
  int n;
};

__global__ __launch_bounds__(256) void vec_stack_gather_kernel(StackGatherArgs a) {
  const int b = blockIdx.x, g = blockIdx.y;
  if (b >= a.n) return;
  const long p0 = a.slots ? a.slots[b] : a.row * a.N + b;
  if (p0 < 0 || p0 >= a.R * a.N) return;     // not a slot of this ring: the row is left as it was, nothing is read
  long s[3];
  ring_stack_slots(a.first, a.R, a.N, p0, s);
  const uint4* src = reinterpret_cast<const uint4*>(a.frames + s[g] * a.frame_bytes);
  uint4* dst = reinterpret_cast<uint4*>(a.out + ((long)b * 3 + g) * a.frame_bytes);
  const long n16 = a.frame_bytes >> 4;
  for (long i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
}

}  // namespace

DRQ_API int drq_vec_stack_gather(const uint8_t* frames, const uint8_t* first, long R, long N, long frame_bytes,
                                 const long* slots, long t, int n, uint8_t* out, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!frames || !first || !out) return DRQ_EARG;
  if (R <= 0 || N <= 0 || n <= 0 || frame_bytes <= 0 || frame_bytes % 16) return DRQ_EARG;
  if (N > INT32_MAX || R > INT64_MAX / N) return DRQ_EARG;
  if (!slots && (t < 0 || n != N)) return DRQ_EARG;     // the row form gathers the whole row
  if (((uintptr_t)frames | (uintptr_t)out) & 15) return DRQ_EARG;
  if (slots && ((uintptr_t)slots & 7)) return DRQ_EARG;
  StackGatherArgs a{frames, first, slots, out, R, N, slots ? 0 : t % R, frame_bytes, n};
  hipLaunchKernelGGL(vec_stack_gather_kernel, dim3((unsigned)n, 3), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
