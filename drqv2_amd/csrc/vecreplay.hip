// Step-major device replay for vectorised environments (contract: include/drqv2_hip.h, "step-major replay").  New
// functionality: the reference stores whole episodes of one environment (replay_buffer.py:76-118); here N environments
// write one row per step into a ring of R rows, and a batch is drawn, windowed and indexed on the device.
//
// drq_vec_add is one grid-stride copy: row t mod R of every array is contiguous (slot = row * N + env), the frames move
// in 16-byte pieces, the few scalars per environment in 4- and 1-byte ones.  drq_vec_sample is one launch shaped like
// nstep_gather_kernel (elementwise.hip): blockIdx.y = 2 does the scalars of 256 batch rows with one thread per row,
// blockIdx.y = 0 / 1 copy the obs / next_obs frame of batch row blockIdx.x.  A copy block needs the row's slots, which
// the scalar block of the same launch computes: instead of waiting for another workgroup it evaluates the (cheap,
// read-only) choice again -- every lane the same loads, so they are broadcast.  Plain vector stores, no atomics.
#include "common.h"
#include "../../include/drqv2_hip.h"

namespace {

struct VecAddArgs {
  uint8_t* frames;
  float* action;
  float* reward;
  float* discount;
  uint8_t* first;
  const uint8_t* src_obs;
  const float* src_action;
  const float* src_reward;
  const float* src_discount;
  const uint8_t* src_first;   // null = all 0
  long row;                   // t mod R
  long n16;                   // N * frame_bytes / 16
  long frame_bytes;
  int N, A, force_first;
};

__global__ __launch_bounds__(256) void vec_add_kernel(VecAddArgs a) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.x * blockDim.x;
  const long base = a.row * a.N;   // first slot of the row
  const uint4* src = reinterpret_cast<const uint4*>(a.src_obs);
  uint4* dst = reinterpret_cast<uint4*>(a.frames + base * a.frame_bytes);
  for (long i = tid; i < a.n16; i += step) dst[i] = src[i];
  const long na = (long)a.N * a.A;
  for (long i = tid; i < na; i += step) a.action[base * a.A + i] = a.src_action[i];
  for (long e = tid; e < a.N; e += step) {
    a.reward[base + e] = a.src_reward[e];
    a.discount[base + e] = a.src_discount[e];
    a.first[base + e] = (a.force_first || (a.src_first && a.src_first[e])) ? 1 : 0;
  }
}

struct VecSampleArgs {
  const uint8_t* first;
  const float* action;
  const float* reward;
  const float* discount;
  const double* u;
  const uint8_t* frames;
  long* idx_out;
  float* act_out;
  float* rew_out;
  float* disc_out;
  int* steps_out;
  uint8_t* obs_out;
  uint8_t* next_obs_out;
  long R, N, lo, hi, frame_bytes;
  int A, B, K, nstep;
  float gamma;
};

__device__ __forceinline__ long vec_slot(const VecSampleArgs& a, long t, long e) { return (t % a.R) * a.N + e; }

// The transition of batch row b: absolute row t and environment e; returns the window length k (1 .. nstep), or 0 when
// the environment of candidate 0 holds no drawable transition (then t, e are candidate 0's).
__device__ __forceinline__ int vec_choose(const VecSampleArgs& a, int b, long& t, long& e) {
  const long rows = a.hi - a.lo + 1;
  const long M = rows * a.N;
  long t0 = a.lo, e0 = 0;
  bool found = false;
  for (int j = 0; j < a.K && !found; ++j) {
    long c = (long)(a.u[(long)b * a.K + j] * (double)M);
    c = c < 0 ? 0 : (c > M - 1 ? M - 1 : c);     // u is in [0, 1): the lower clamp only keeps a bad table in range
    t = a.lo + c / a.N;
    e = c % a.N;
    if (j == 0) { t0 = t; e0 = e; }
    found = a.first[vec_slot(a, t, e)] == 0;
  }
  if (!found) {
    // every candidate is a reset row: walk candidate 0's environment t0+1 .. hi, lo .. t0-1
    e = e0;
    for (long i = 1; i < rows && !found; ++i) {
      t = a.lo + (t0 - a.lo + i) % rows;
      found = a.first[vec_slot(a, t, e)] == 0;
    }
    if (!found) {
      t = t0;
      return 0;
    }
  }
  int k = a.nstep;
  for (int i = 1; i < a.nstep; ++i)
    if (a.first[vec_slot(a, t + i, e)]) {
      k = i;
      break;
    }
  return k;
}

__global__ __launch_bounds__(256) void vec_sample_kernel(VecSampleArgs a) {
#pragma clang fp contract(off)
  const int which = a.obs_out ? blockIdx.y : 2;     // no output frames: the scalars only (grid.y == 1)
  if (which < 2) {
    const int b = blockIdx.x;
    if (b >= a.B) return;
    long t, e;
    const int k = vec_choose(a, b, t, e);
    const long p = k == 0 ? vec_slot(a, t, e) : vec_slot(a, which == 0 ? t - 1 : t + k - 1, e);
    const uint4* src = reinterpret_cast<const uint4*>(a.frames + p * a.frame_bytes);
    uint4* dst = reinterpret_cast<uint4*>((which == 0 ? a.obs_out : a.next_obs_out) + (long)b * a.frame_bytes);
    const long n16 = a.frame_bytes >> 4;
    for (long i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    return;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  long t, e;
  const int k = vec_choose(a, b, t, e);
  const long p = vec_slot(a, t, e);
  a.idx_out[b] = k == 0 ? p : vec_slot(a, t - 1, e);
  a.idx_out[(long)a.B + b] = k == 0 ? p : vec_slot(a, t + k - 1, e);
  a.idx_out[2L * a.B + b] = p;
  a.steps_out[b] = k;
  for (int j = 0; j < a.A; ++j) a.act_out[(long)b * a.A + j] = a.action[p * a.A + j];
  // nstep_gather_kernel's accumulation over k rows of the ring: one rounding per operation, the products pinned in
  // registers before the add / multiply that consumes them (see there)
  float r = 0.f, d = 1.f;
  for (int i = 0; i < k; ++i) {
    const long q = vec_slot(a, t + i, e);
    float x = d * a.reward[q];
    asm volatile("" : "+v"(x));
    r = r + x;
    float gd = a.discount[q] * a.gamma;
    asm volatile("" : "+v"(gd));
    d = d * gd;
  }
  a.rew_out[b] = r;
  a.disc_out[b] = k == 0 ? 0.f : d;
}

}  // namespace

DRQ_API int drq_vec_add(uint8_t* frames, float* action, float* reward, float* discount, uint8_t* first, long R, long N,
                        int A, long frame_bytes, long t, const uint8_t* src_obs, const float* src_action,
                        const float* src_reward, const float* src_discount, const uint8_t* src_first,
                        drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!frames || !action || !reward || !discount || !first || !src_obs || !src_action || !src_reward || !src_discount)
    return DRQ_EARG;
  if (R <= 0 || N <= 0 || A <= 0 || frame_bytes <= 0 || frame_bytes % 16 || t < 0) return DRQ_EARG;
  if (N > INT32_MAX) return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)src_obs) & 15) return DRQ_EARG;
  VecAddArgs a{frames, action, reward, discount, first, src_obs, src_action, src_reward, src_discount, src_first,
               t % R, N * (frame_bytes >> 4), frame_bytes, (int)N, A, t == 0 ? 1 : 0};
  const long want = (a.n16 + 255) / 256;
  const long cap = 8L * drq_num_cus();
  hipLaunchKernelGGL(vec_add_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_sample(const uint8_t* first, const float* action, const float* reward, const float* discount, long R,
                           long N, int A, long frame_bytes, long lo, long hi, const double* u, int B, int K, int nstep,
                           float gamma, long* idx_out, float* act_out, float* rew_out, float* disc_out, int* steps_out,
                           const uint8_t* frames, uint8_t* obs_out, uint8_t* next_obs_out, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!first || !action || !reward || !discount || !u || !idx_out || !act_out || !rew_out || !disc_out || !steps_out)
    return DRQ_EARG;
  if (R <= 0 || N <= 0 || A <= 0 || B <= 0 || K <= 0 || nstep <= 0 || frame_bytes <= 0 || frame_bytes % 16)
    return DRQ_EARG;
  if (lo < 1 || hi < lo || hi - lo + 1 + nstep > R) return DRQ_EARG;
  const int given = (frames != nullptr) + (obs_out != nullptr) + (next_obs_out != nullptr);
  if (given != 0 && given != 3) return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)obs_out | (uintptr_t)next_obs_out) & 15) return DRQ_EARG;
  VecSampleArgs a{first, action, reward, discount, u, frames, idx_out, act_out, rew_out, disc_out, steps_out, obs_out,
                  next_obs_out, R, N, lo, hi, frame_bytes, A, B, K, nstep, gamma};
  if (obs_out) hipLaunchKernelGGL(vec_sample_kernel, dim3(B, 3), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(vec_sample_kernel, dim3((B + 255) / 256, 1), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
