// Episodes out of and into the step-major ring (contract: include/drqv2_hip.h, "episode files for the step-major ring").
// New functionality: the reference keeps every episode as a file of its own (replay_buffer.py:22-34); here the steps of
// N lockstep environments live in one ring in HBM, and these two launches are the bulk movements between that ring and
// episode-major staging.  The host plans (drqv2_amd/episodes.py), the device only copies.
//
// drq_vec_export_rows is one launch of M x G workgroups, G = 1 (a slot holds the whole observation) or 3 (a slot holds
// one frame): workgroup (m, g) copies frame g of output step m in 16-byte pieces, as vec_stack_gather_kernel
// (vecframes.hip) does; the source row of frame g follows from the table entry (t, e, t0) alone -- max(t - 2 + g, t0) --
// so no flag is read.  Workgroup (m, 0) also writes the step's action row, reward and discount, the canonical dummies
// where t == t0.  Every lane of a workgroup reads the same table entry: the loads are broadcast.
//
// drq_vec_fill is one launch of n x P workgroups: workgroup (i, j) copies pieces j * 256 + lane, + 256 P, ... of the
// N frame_bytes contiguous bytes of row T + i (source and ring row are both contiguous: slot = row * N + env) and
// workgroup (i, 0) writes the row's scalars with ring_add_scalars (replay_device.h) -- drq_vec_add's own code on the
// same sources, the rule for row 0 included.  n <= R, so no two rows of a launch share a ring row, whether or not the
// launch wraps the ring.
//
// Consecutive lanes move consecutive 16-byte pieces: every wave instruction is 1 KiB, contiguous and 16-byte aligned;
// the ragged tail (a frame is 1,323 pieces) is a shorter last trip of the loop.  Plain vector loads and stores, no LDS,
// no atomics, nothing crosses workgroups.
#include "common.h"
#include "replay_device.h"
#include "../../include/drqv2_hip.h"

namespace {

struct ExportArgs {
  const uint8_t* frames;
  const float* action;
  const float* reward;
  const float* discount;
  const int* table;       // [M][3]: t, e, t0
  uint8_t* obs;
  float* act_out;
  float* rew_out;
  float* disc_out;
  VecRing g;              // R and N only: no flag is read
  long frame_bytes;
  int M, A, groups;
};

__global__ __launch_bounds__(256) void vec_export_rows_kernel(ExportArgs a) {
  const long m = blockIdx.x;
  const int grp = blockIdx.y;
  if (m >= a.M) return;
  const long t = a.table[3 * m], e = a.table[3 * m + 1], t0 = a.table[3 * m + 2];
  if (e < 0 || e >= a.g.N || t0 < 0 || t < t0) return;     // no step of this ring: the row is left as it was
  // a one-frame ring: frames t-2, t-1, t of the episode that starts on row t0, oldest first, refilled from the reset row
  long ts = t - (a.groups - 1 - grp);
  if (ts < t0) ts = t0;
  const uint4* src = reinterpret_cast<const uint4*>(a.frames + ring_slot(a.g, ts, e) * a.frame_bytes);
  uint4* dst = reinterpret_cast<uint4*>(a.obs + (m * a.groups + grp) * a.frame_bytes);
  const long n16 = a.frame_bytes >> 4;
  for (long i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
  if (grp != 0) return;
  const long p = ring_slot(a.g, t, e);
  const bool reset = t == t0;                               // the file's dummy transition, whatever add() was handed
  for (int j = threadIdx.x; j < a.A; j += blockDim.x) a.act_out[m * a.A + j] = reset ? 0.f : a.action[p * a.A + j];
  if (threadIdx.x == 0) {
    a.rew_out[m] = reset ? 0.f : a.reward[p];
    a.disc_out[m] = reset ? 1.f : a.discount[p];
  }
}

constexpr int kFillBlocks = 1024;   // workgroups per row at most: beyond 4 MiB a row, a workgroup makes several trips

struct FillArgs {
  RingRowScalars s;       // row, the sources and force_first are set per row in the kernel
  uint8_t* frames;
  const uint8_t* src_frames;
  long R, T;
  long row16;             // N * frame_bytes / 16
  int n, blocks;          // rows, workgroups per row
};

__global__ __launch_bounds__(256) void vec_fill_kernel(FillArgs a) {
  const long i = blockIdx.x / a.blocks;                     // the row of this launch
  const int j = blockIdx.x - i * a.blocks;
  if (i >= a.n) return;
  const long t = a.T + i, row = t % a.R;
  const uint4* src = reinterpret_cast<const uint4*>(a.src_frames) + i * a.row16;
  uint4* dst = reinterpret_cast<uint4*>(a.frames) + row * a.row16;
  for (long k = (long)j * 256 + threadIdx.x; k < a.row16; k += 256L * a.blocks) dst[k] = src[k];
  if (j != 0) return;
  RingRowScalars s = a.s;
  const long N = s.N;
  s.src_action += i * N * s.A;
  s.src_reward += i * N;
  s.src_discount += i * N;
  s.src_first += i * N;
  s.row = row;
  s.force_first = t == 0 ? 1 : 0;
  ring_add_scalars(s, threadIdx.x, 256);
}

}  // namespace

DRQ_API int drq_vec_export_rows(const uint8_t* frames, const float* action, const float* reward, const float* discount,
                                long R, long N, int A, long frame_bytes, int stack, const int* table, int M, uint8_t* obs,
                                float* act_out, float* rew_out, float* disc_out, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!frames || !action || !reward || !discount || !table || !obs || !act_out || !rew_out || !disc_out) return DRQ_EARG;
  if (R <= 0 || N <= 0 || A <= 0 || M <= 0 || frame_bytes <= 0 || frame_bytes % 16) return DRQ_EARG;
  if (stack != 1 && stack != 3) return DRQ_EARG;
  if (N > INT32_MAX || R > INT64_MAX / N) return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)obs) & 15) return DRQ_EARG;
  if (((uintptr_t)action | (uintptr_t)reward | (uintptr_t)discount | (uintptr_t)table | (uintptr_t)act_out |
       (uintptr_t)rew_out | (uintptr_t)disc_out) & 3)
    return DRQ_EARG;
  ExportArgs a{frames, action, reward, discount, table, obs, act_out, rew_out, disc_out, VecRing{nullptr, R, N, 0, 0, 0},
               frame_bytes, M, A, stack};
  hipLaunchKernelGGL(vec_export_rows_kernel, dim3((unsigned)M, (unsigned)stack), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_fill(uint8_t* frames, float* action, float* reward, float* discount, uint8_t* first, long R, long N,
                         int A, long frame_bytes, long T, int n, const uint8_t* src_frames, const float* src_action,
                         const float* src_reward, const float* src_discount, const uint8_t* src_first,
                         drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!frames || !action || !reward || !discount || !first || !src_frames || !src_action || !src_reward ||
      !src_discount || !src_first)
    return DRQ_EARG;
  if (R <= 0 || N <= 0 || A <= 0 || frame_bytes <= 0 || frame_bytes % 16 || T < 0 || n <= 0 || n > R) return DRQ_EARG;
  if (N > INT32_MAX || frame_bytes > INT64_MAX / N || R > INT64_MAX / (N * frame_bytes) || T > INT64_MAX - n)
    return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)src_frames) & 15) return DRQ_EARG;
  if (((uintptr_t)action | (uintptr_t)reward | (uintptr_t)discount | (uintptr_t)src_action | (uintptr_t)src_reward |
       (uintptr_t)src_discount) & 3)
    return DRQ_EARG;
  const long row16 = N * (frame_bytes >> 4);
  const long want = (row16 + 255) / 256;
  const long blocks = want < kFillBlocks ? want : kFillBlocks;
  if (blocks * n > INT32_MAX) return DRQ_EARG;
  FillArgs a{RingRowScalars{action, reward, discount, first, src_action, src_reward, src_discount, src_first, 0, (int)N, A,
                            0},
             frames, src_frames, R, T, row16, n, (int)blocks};
  hipLaunchKernelGGL(vec_fill_kernel, dim3((unsigned)(blocks * n)), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
