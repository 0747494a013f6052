// Episode statistics for vectorised collection (contract: include/drqv2_hip.h, "episode statistics").  The reference
// adds up episode_reward / episode_step on the host, one environment (train.py:133,186,189); with N lockstep
// environments on the device the same sums are kept here, from the reward and first tensors the ring's add() already
// takes, so that the host never reads a flag back.
//
// drq_vec_stats_step is ONE workgroup of 1,024 threads, the shape of the tree launches of per.hip / vecreplay.hip:
// nothing crosses workgroups, so there is no grid barrier, no agent-scope fence and no atomic.  It walks the N
// environments in chunks of 1,024, thread i of a chunk owning environment chunk + i in every pass:
//   scan     the "counted" flag of a chunk is scanned exclusively: inside a wave by one ballot (the lanes below mine that
//            are counted), across the 16 waves through their totals in LDS; `base`, carried from chunk to chunk, makes the
//            rank the number of counted environments with a smaller index -- the record numbers of a call ascend with e
//   records  record j lives at j mod W.  A call that counts more than W episodes names a log index more than once; the
//            newest record must stay.  Inside a chunk only the record that no later one OF THE CHUNK replaces is stored
//            (j + W >= the chunk's end), so no two threads of a chunk store to one index; a later chunk stores after the
//            barrier of its own scan, which every thread reaches behind its stores of the chunk before: __syncthreads()
//            orders the two stores to one address within the workgroup.  Hence the log is deterministic.
//   totals   min, max, length_sum and return_sum ride in registers through the chunks and are reduced once at the end,
//            by __shfl_xor inside the waves and through LDS across them; thread 0 then writes the header, last.
// All stores are plain vector stores.  drq_vec_stats_publish copies header and log to a pinned host mirror by the
// protocol of publish_sums_kernel (step.hip): the stores, __threadfence_system(), a barrier, then ONE lane's system-scope
// release store of the sequence word.
#include "internal.h"
#include "../../include/drqv2_hip.h"

#include <math.h>

namespace {

constexpr int kStatsThreads = 1024;
constexpr int kStatsWaves = kStatsThreads / 64;

struct VecStatsArgs {
  float* ret;
  int* len;
  int* done;
  VecStatsHeader* hdr;
  float* log_return;
  int* log_length;
  int* log_env;
  long* log_row;
  const float* reward;    // null only on row 0
  const uint8_t* first;   // null = no flags
  long N, W, row;
  int limit;
};

__global__ __launch_bounds__(kStatsThreads) void vec_stats_step_kernel(VecStatsArgs a) {
  __shared__ int s_cnt[2][kStatsWaves];     // the waves' counted totals of a chunk; two sets, so one barrier per chunk
  __shared__ float s_min[kStatsWaves], s_max[kStatsWaves];
  __shared__ long s_len[kStatsWaves];
  __shared__ double s_sum[kStatsWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long ep0 = a.hdr->episodes;         // read by every thread before the first barrier, written behind the last
  long base = 0;                            // episodes this call has counted in the chunks before
  float mn = INFINITY, mx = -INFINITY;
  long lsum = 0;
  double rsum = 0.0;
  int buf = 0;
  for (long c0 = 0; c0 < a.N; c0 += kStatsThreads, buf ^= 1) {
    const long e = c0 + threadIdx.x;
    bool f = false, counted = false;
    float r = 0.f;
    int l = 0;
    if (e < a.N) {
      f = a.row == 0 || (a.first && a.first[e]);
      r = a.ret[e];
      l = a.len[e];
      if (f && l >= 1) {                    // the running episode is finished
        const int d = a.done[e];
        counted = a.limit == 0 || d < a.limit;
        a.done[e] = d < INT32_MAX ? d + 1 : d;
      }
    }
    const unsigned long long m = __ballot(counted);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[buf][wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kStatsWaves; ++w) {
      const int c = s_cnt[buf][w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (counted) {
      const long k = base + before + below;           // rank within the call
      if (k + a.W >= base + total) {                  // no later record of this chunk takes the index
        const long i = (ep0 + k) % a.W;
        a.log_return[i] = r;
        a.log_length[i] = l;
        a.log_env[i] = (int)e;
        a.log_row[i] = a.row;
      }
      mn = fminf(mn, r);
      mx = fmaxf(mx, r);
      lsum += l;
      rsum += (double)r;
    }
    if (e < a.N) {
      a.ret[e] = f ? 0.f : r + a.reward[e];           // one float32 add per step, in step order
      a.len[e] = f ? 0 : l + 1;
    }
    base += total;
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o));
    mx = fmaxf(mx, __shfl_xor(mx, o));
    lsum += __shfl_xor(lsum, o);
    rsum += __shfl_xor(rsum, o);
  }
  if (lane == 0) {
    s_min[wave] = mn;
    s_max[wave] = mx;
    s_len[wave] = lsum;
    s_sum[wave] = rsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kStatsWaves; ++w) {
      mn = fminf(mn, s_min[w]);
      mx = fmaxf(mx, s_max[w]);
      lsum += s_len[w];
      rsum += s_sum[w];
    }
    VecStatsHeader h = *a.hdr;
    h.rows = a.row + 1;
    h.episodes = ep0 + base;
    h.length_sum += lsum;
    h.return_sum += rsum;
    h.min_return = fminf(h.min_return, mn);
    h.max_return = fmaxf(h.max_return, mx);
    *a.hdr = h;
  }
}

__global__ __launch_bounds__(kStatsThreads) void vec_stats_reset_kernel(float* ret, int* len, int* done,
                                                                         VecStatsHeader* hdr, float* log_return,
                                                                         int* log_length, int* log_env, long* log_row,
                                                                         long N, long W) {
  for (long e = threadIdx.x; e < N; e += kStatsThreads) {
    ret[e] = 0.f;
    len[e] = 0;
    done[e] = 0;
  }
  for (long i = threadIdx.x; i < W; i += kStatsThreads) {
    log_return[i] = 0.f;
    log_length[i] = 0;
    log_env[i] = 0;
    log_row[i] = 0;
  }
  if (threadIdx.x == 0) {
    VecStatsHeader h = {};
    h.min_return = INFINITY;
    h.max_return = -INFINITY;
    *hdr = h;
  }
}

// everything travels as 32-bit words; row_word = the word the int64 rows start on (an even one), the sequence word
// follows them
__global__ __launch_bounds__(kStatsThreads) void vec_stats_publish_kernel(const unsigned* hdr, const unsigned* log_return,
                                                                           const unsigned* log_length,
                                                                           const unsigned* log_env, const unsigned* log_row,
                                                                           long W, unsigned* host, long row_word,
                                                                           unsigned seq) {
  constexpr long H = sizeof(VecStatsHeader) / 4;
  if (threadIdx.x < H) host[threadIdx.x] = hdr[threadIdx.x];
  for (long i = threadIdx.x; i < W; i += kStatsThreads) {
    host[H + i] = log_return[i];
    host[H + W + i] = log_length[i];
    host[H + 2 * W + i] = log_env[i];
  }
  for (long i = threadIdx.x; i < 2 * W; i += kStatsThreads) host[row_word + i] = log_row[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store(host + row_word + 2 * W, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

inline bool stats_log_ok(const void* hdr, const float* log_return, const int* log_length, const int* log_env,
                         const long* log_row, long W) {
  return hdr && log_return && log_length && log_env && log_row && W >= 1 && !((uintptr_t)hdr & 7) && !((uintptr_t)log_row & 7);
}

}  // namespace

DRQ_API int drq_vec_stats_step(float* ret, int* len, int* done, void* header, float* log_return, int* log_length,
                               int* log_env, long* log_row, long N, long W, int limit, long row, const float* reward,
                               const uint8_t* first, drq_stream_t stream) {
  if (!ret || !len || !done || !stats_log_ok(header, log_return, log_length, log_env, log_row, W)) return DRQ_EARG;
  if (N < 1 || N > INT32_MAX || limit < 0 || row < 0 || (!reward && row > 0)) return DRQ_EARG;
  VecStatsArgs a{ret, len, done, (VecStatsHeader*)header, log_return, log_length, log_env, log_row, reward, first, N, W,
                 row, limit};
  hipLaunchKernelGGL(vec_stats_step_kernel, dim3(1), dim3(kStatsThreads), 0, (hipStream_t)stream, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_stats_publish(const void* header, const float* log_return, const int* log_length, const int* log_env,
                                  const long* log_row, long W, void* host_mirror, unsigned seq, drq_stream_t stream) {
  if (!stats_log_ok(header, log_return, log_length, log_env, log_row, W) || !host_mirror || ((uintptr_t)host_mirror & 7))
    return DRQ_EARG;
  const long row_word = (long)(sizeof(VecStatsHeader) / 4) + ((3 * W + 1) & ~1L);
  hipLaunchKernelGGL(vec_stats_publish_kernel, dim3(1), dim3(kStatsThreads), 0, (hipStream_t)stream,
                     (const unsigned*)header, (const unsigned*)log_return, (const unsigned*)log_length,
                     (const unsigned*)log_env, (const unsigned*)log_row, W, (unsigned*)host_mirror, row_word, seq);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_stats_reset(float* ret, int* len, int* done, void* header, float* log_return, int* log_length,
                                int* log_env, long* log_row, long N, long W, drq_stream_t stream) {
  if (!ret || !len || !done || !stats_log_ok(header, log_return, log_length, log_env, log_row, W)) return DRQ_EARG;
  if (N < 1 || N > INT32_MAX) return DRQ_EARG;
  hipLaunchKernelGGL(vec_stats_reset_kernel, dim3(1), dim3(kStatsThreads), 0, (hipStream_t)stream, ret, len, done,
                     (VecStatsHeader*)header, log_return, log_length, log_env, log_row, N, W);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
