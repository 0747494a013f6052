// Frame stacks out of a single-frame step-major ring (contract: include/drqv2_hip.h, "single-frame step-major replay").
// New functionality: the reference stacks frames in the environment wrapper (dmc.py:87-109) and stores every stack
// whole; here a slot holds the one new frame of its step and the stack is put together where it is read.
//
// drq_vec_stack_gather is one launch of n x 3 workgroups: workgroup (b, g) copies frame g (0 = oldest) of stack b in
// 16-byte pieces.  Which slot that is follows from the newest frame's slot and at most two `first` bytes
// (ring_stack_slots, replay_device.h: shared with the fused aug+conv1 launch, which gathers the same stacks on its own);
// every lane reads the same bytes, so the loads are broadcast.  Plain vector loads and stores, no atomics.
//
// drq_nstep_gather (below, beside nstep_gather_kernel) assembles a batch from an episode store of whole stacks.
// drq_nstep_gather_frames is the same for an episode store of single frames: a flat ring of R
// slots, N = 1, every episode contiguous with first = 1 on its first slot.  One launch of B x (6 P + 1) workgroups:
// workgroup (b, 6 P) with b < ceil(B / 256) does the scalars of 256 batch rows, one thread per row, with nstep_sum --
// drq_nstep_gather's arithmetic on the same operands; workgroup (b, g P + j) copies piece j of frame g of row b (g = 0 .. 2:
// the obs stack, 3 .. 5: the next_obs stack, oldest frame first), kFramePiece 16-byte chunks per thread, all of a
// thread's loads issued before its first store.  Consecutive lanes move consecutive 16-byte chunks: every wave
// instruction is 1 KiB, contiguous and aligned to 16 bytes.  No LDS, nothing crosses workgroups.
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

constexpr int kFramePiece = 2;      // 16-byte chunks per thread: 21,168-byte frames are 1,323 chunks = 3 pieces of 512

struct NstepFramesArgs {
  const uint8_t* frames;
  const uint8_t* first;
  const float* action;
  const float* reward;
  const float* discount;
  const long* pos;
  uint8_t* obs;           // null (with next_obs): the scalars only
  uint8_t* next_obs;
  float* act_out;
  float* rew_out;
  float* disc_out;
  long R, frame_bytes;
  int B, A, nstep, pieces;
  float gamma;
};

__global__ __launch_bounds__(256) void nstep_gather_frames_kernel(NstepFramesArgs a) {
  const int y = a.obs ? blockIdx.y : 6 * a.pieces;  // no output frames: the scalars only (grid.y == 1)
  if (y == 6 * a.pieces) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const long p = a.pos[b];
    if (p < 1 || p > a.R - a.nstep) return;         // slot p-1 or the window p .. p+nstep-1 is no part of the store
    for (int j = 0; j < a.A; ++j) a.act_out[(long)b * a.A + j] = a.action[p * a.A + j];
    float r, d;
    nstep_sum(a.reward, a.discount, a.gamma, a.nstep, [p](int i) { return p + i; }, r, d);
    a.rew_out[b] = r;
    a.disc_out[b] = d;
    return;
  }
  const int b = blockIdx.x;
  const long p = a.pos[b];
  if (p < 1 || p > a.R - a.nstep) return;           // the row is left as it was, nothing is read
  const int g = y / a.pieces, piece = y - g * a.pieces;
  const bool next = g >= 3;
  long s[3];
  ring_stack_slots(a.first, a.R, 1, next ? p + a.nstep - 1 : p - 1, s);
  const int f = next ? g - 3 : g;
  const uint4* src = reinterpret_cast<const uint4*>(a.frames + s[f] * a.frame_bytes);
  uint4* dst = reinterpret_cast<uint4*>((next ? a.next_obs : a.obs) + ((long)b * 3 + f) * a.frame_bytes);
  const long n16 = a.frame_bytes >> 4;
  const long i0 = (long)piece * (kFramePiece * 256) + threadIdx.x;
  uint4 v[kFramePiece];
#pragma unroll
  for (int u = 0; u < kFramePiece; ++u)
    if (i0 + u * 256 < n16) v[u] = src[i0 + u * 256];
#pragma unroll
  for (int u = 0; u < kFramePiece; ++u)
    if (i0 + u * 256 < n16) dst[i0 + u * 256] = v[u];
}

// ------------------------------------------------------------------------------------------------
// Replay sampling on the device (replay_buffer.py:142-160): batch row b is transition pos[b] of a flat store of
// steps (episodes contiguous): obs = frame[pos-1], next_obs = frame[pos+nstep-1], action = action[pos], and the
// n-step return in the reference's float32 order:  reward += discount*r[pos+i];  discount *= d[pos+i]*gamma
// (nstep_sum, replay_device.h).
// blockIdx.y = 0 / 1: obs / next_obs frame copy (16-byte pieces); blockIdx.y = 2: the scalars of 256 rows.
// ------------------------------------------------------------------------------------------------
struct NstepArgs {
  const uint8_t* frames;
  const float* action;
  const float* reward;
  const float* discount;
  const long* pos;
  uint8_t* obs;
  uint8_t* next_obs;
  float* act_out;
  float* rew_out;
  float* disc_out;
  long frame_bytes;   // multiple of 16
  int B, A, nstep;
  float gamma;
};

__global__ void nstep_gather_kernel(NstepArgs a) {
  const int which = a.obs ? blockIdx.y : 2;         // no output frames: the scalars only (grid.y == 1)
  if (which < 2) {
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const long p = a.pos[b] + (which == 0 ? -1 : (long)a.nstep - 1);
    const uint4* src = reinterpret_cast<const uint4*>(a.frames + p * a.frame_bytes);
    uint4* dst = reinterpret_cast<uint4*>((which == 0 ? a.obs : a.next_obs) + (long)b * a.frame_bytes);
    const long n16 = a.frame_bytes >> 4;
    for (long i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    return;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const long p = a.pos[b];
  for (int j = 0; j < a.A; ++j) a.act_out[(long)b * a.A + j] = a.action[p * a.A + j];
  float r, d;
  nstep_sum(a.reward, a.discount, a.gamma, a.nstep, [p](int i) { return p + i; }, r, d);
  a.rew_out[b] = r;
  a.disc_out[b] = d;
}

}  // namespace

// Device-side replay batch assembly (replay_buffer.py:142-160), see nstep_gather_kernel.
DRQ_API int drq_nstep_gather(const uint8_t* frames, const float* action, const float* reward, const float* discount,
                             const long* pos, int B, int A, long frame_bytes, int nstep, float gamma, uint8_t* obs,
                             float* act_out, float* rew_out, float* disc_out, uint8_t* next_obs, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!action || !reward || !discount || !pos || !act_out || !rew_out || !disc_out) return DRQ_EARG;
  if ((obs != nullptr) != (next_obs != nullptr)) return DRQ_EARG;
  if (obs && !frames) return DRQ_EARG;
  if (B <= 0 || A <= 0 || nstep <= 0 || frame_bytes <= 0 || frame_bytes % 16) return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)obs | (uintptr_t)next_obs) & 15) return DRQ_EARG;
  NstepArgs a{frames, action, reward, discount, pos, obs, next_obs, act_out, rew_out, disc_out, frame_bytes, B, A, nstep,
              gamma};
  // obs == next_obs == NULL: action rows and n-step reward / discount only (the frames stay in the store and the
  // update reads them through DrqStep.obs_index / next_obs_index)
  if (obs) hipLaunchKernelGGL(nstep_gather_kernel, dim3(B, 3), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(nstep_gather_kernel, dim3((B + 255) / 256, 1), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_nstep_gather_frames(const uint8_t* frames, const uint8_t* first, long R, const float* action,
                                    const float* reward, const float* discount, const long* pos, int B, int A,
                                    long frame_bytes, int nstep, float gamma, uint8_t* obs, float* act_out, float* rew_out,
                                    float* disc_out, uint8_t* next_obs, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!frames || !first || !action || !reward || !discount || !pos || !act_out || !rew_out || !disc_out) return DRQ_EARG;
  if ((obs != nullptr) != (next_obs != nullptr)) return DRQ_EARG;
  if (R <= 0 || B <= 0 || A <= 0 || nstep <= 0 || frame_bytes <= 0 || frame_bytes % 16) return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)obs | (uintptr_t)next_obs) & 15) return DRQ_EARG;
  if (((uintptr_t)action | (uintptr_t)reward | (uintptr_t)discount | (uintptr_t)act_out | (uintptr_t)rew_out |
       (uintptr_t)disc_out) & 3)
    return DRQ_EARG;
  if ((uintptr_t)pos & 7) return DRQ_EARG;
  const long pieces = ((frame_bytes >> 4) + kFramePiece * 256 - 1) / (kFramePiece * 256);
  if (6 * pieces + 1 > 65535) return DRQ_EARG;          // grid.y: frames beyond 85 MB
  NstepFramesArgs a{frames, first, action, reward, discount, pos, obs, next_obs, act_out, rew_out, disc_out, R,
                    frame_bytes, B, A, nstep, (int)pieces, gamma};
  if (obs) hipLaunchKernelGGL(nstep_gather_frames_kernel, dim3(B, 6 * (unsigned)pieces + 1), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(nstep_gather_frames_kernel, dim3((B + 255) / 256, 1), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

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
