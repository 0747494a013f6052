// Step-major device replay for vectorised environments (contract: include/drqv2_hip.h, "step-major replay").  New
// functionality: the reference stores whole episodes of one environment (replay_buffer.py:76-118); here N environments
// write one row per step into a ring of R rows, and a batch is drawn, windowed and indexed on the device.
//
// drq_vec_add is one grid-stride copy: row t mod R of every array is contiguous (slot = row * N + env), the frames move
// in 16-byte pieces, the few scalars per environment in 4- and 1-byte ones.  drq_vec_sample is one launch shaped like
// nstep_gather_kernel (vecframes.hip): blockIdx.y = 2 does the scalars of 256 batch rows with one thread per row,
// blockIdx.y = 0 / 1 copy the obs / next_obs frame of batch row blockIdx.x.  A copy block needs the row's slots, which
// the scalar block of the same launch computes: instead of waiting for another workgroup it evaluates the (cheap,
// read-only) choice again -- every lane the same loads, so they are broadcast.  Plain vector stores, no atomics.
//
// Prioritized sampling on the ring (contract: include/drqv2_hip.h, "prioritized step-major replay").  The sum tree is
// per.hip's -- double [2L], leaf of slot s at tree[L + s], every inner node recomputed as tree[2k] + tree[2k+1],
// tree[0] the largest leaf a priority update ever wrote -- and so is the shape of the three launches: ONE workgroup of
// 1,024 threads that walks the tree level by level with __syncthreads() between the levels (per.hip's header comment
// has the memory-ordering argument: nothing crosses workgroups, so no grid barrier and no agent-scope fence).
//   invariant  after every add(), with (lo, hi) the drawable rows: leaf(t, e) > 0 iff lo <= t <= hi and first[t, e] == 0;
//              every other leaf -- padding above R N, guard rows, head rows, reset rows -- is exactly 0
//   advance    an add() moves hi and lo by at most one row: the leaves of the row that entered become
//              first ? 0 : tree[0], those of the row that left 0, the ancestors of both ranges are recomputed
//   draw       the stratified descent to a slot p; e = p % N, ring row r = p / N, absolute row
//              t = T-1 - ((T-1-r) mod R); from there the uniform draw's window and batch row.  Weights
//              (n leaf / tree[1])^-beta / max_batch with the nominal n = (hi-lo+1) N, which cancels against the maximum
//   update     leaf(p) = (clamp(td_abs) + eps)^alpha only where p is still drawable (checked here from T, lo, hi and
//              first: the host never reads a flag); the highest row of a repeated position wins
// The host never learns whether the tree is empty (every drawable row a reset row): such a draw comes out as the
// uniform path's "no drawable transition" rows, all indices on slot(lo, 0), steps 0, reward 0, discount 0, weight 1.
//
// What the two draws share (ring geometry, window, batch row, n-step sum) and what the tree entries share with per.hip
// (descent, weight normalisation, priority update, ranged rebuild) is one copy each, in replay_device.h; so are the
// scalars of an added row, which drq_vec_add_render (vecrender.hip) writes as drq_vec_add does.
#include "common.h"
#include "replay_device.h"
#include "../../include/drqv2_hip.h"

namespace {

struct VecAddArgs {
  RingRowScalars s;           // the row's action, reward, discount and first (replay_device.h)
  uint8_t* frames;
  const uint8_t* src_obs;
  long n16;                   // N * frame_bytes / 16
  long frame_bytes;
};

__global__ __launch_bounds__(256) void vec_add_kernel(VecAddArgs a) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long step = (long)gridDim.x * blockDim.x;
  const long base = a.s.row * a.s.N;   // first slot of the row
  const uint4* src = reinterpret_cast<const uint4*>(a.src_obs);
  uint4* dst = reinterpret_cast<uint4*>(a.frames + base * a.frame_bytes);
  for (long i = tid; i < a.n16; i += step) dst[i] = src[i];
  ring_add_scalars(a.s, tid, step);
}

struct VecSampleArgs {
  RingBatch r;      // r.g.T is not known to this entry (0)
  const double* u;
  const uint8_t* frames;
  uint8_t* obs_out;
  uint8_t* next_obs_out;
  long frame_bytes;
  int K;
};

// The transition of batch row b: absolute row t and environment e; returns the window length k (1 .. nstep), or 0 when
// the environment of candidate 0 holds no drawable transition (then t, e are candidate 0's).
__device__ __forceinline__ int vec_choose(const VecSampleArgs& a, int b, long& t, long& e) {
  const VecRing& g = a.r.g;
  const long rows = g.hi - g.lo + 1;
  const long M = rows * g.N;
  long t0 = g.lo, e0 = 0;
  bool found = false;
  for (int j = 0; j < a.K && !found; ++j) {
    long c = (long)(a.u[(long)b * a.K + j] * (double)M);
    c = c < 0 ? 0 : (c > M - 1 ? M - 1 : c);     // u is in [0, 1): the lower clamp only keeps a bad table in range
    t = g.lo + c / g.N;
    e = c % g.N;
    if (j == 0) { t0 = t; e0 = e; }
    found = g.first[ring_slot(g, t, e)] == 0;
  }
  if (!found) {
    // every candidate is a reset row: walk candidate 0's environment t0+1 .. hi, lo .. t0-1
    e = e0;
    for (long i = 1; i < rows && !found; ++i) {
      t = g.lo + (t0 - g.lo + i) % rows;
      found = g.first[ring_slot(g, t, e)] == 0;
    }
    if (!found) {
      t = t0;
      return 0;
    }
  }
  return ring_window(g, t, e, a.r.nstep);
}

__global__ __launch_bounds__(256) void vec_sample_kernel(VecSampleArgs a) {
  const int which = a.obs_out ? blockIdx.y : 2;     // no output frames: the scalars only (grid.y == 1)
  if (which < 2) {
    const int b = blockIdx.x;
    if (b >= a.r.B) return;
    long t, e;
    const int k = vec_choose(a, b, t, e);
    const long p = ring_slot(a.r.g, k == 0 ? t : (which == 0 ? t - 1 : t + k - 1), e);
    const uint4* src = reinterpret_cast<const uint4*>(a.frames + p * a.frame_bytes);
    uint4* dst = reinterpret_cast<uint4*>((which == 0 ? a.obs_out : a.next_obs_out) + (long)b * a.frame_bytes);
    const long n16 = a.frame_bytes >> 4;
    for (long i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    return;
  }
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.r.B) return;
  long t, e;
  const int k = vec_choose(a, b, t, e);
  ring_emit_row(a.r, b, t, e, k);
}

// ---- the mixed draw: batch rows b < Bd from the demonstration partition, the others from the ring ------------------
// (contract: include/drqv2_hip.h, "demonstrations in the step-major replay")  Two geometries over ONE allocation: the
// ring's R rows, and behind them the partition's D rows, linear -- a VecRing of D rows whose drawable rows end nstep
// before the Td rows filled never takes the modulo.  `demo` is `live` with every store pointer moved R N slots on, so
// vec_choose, ring_window, ring_emit_row and the frame copy run on either as they stand; what a partition row has to
// add is the R N its three indices lack to index the whole allocation, which the thread that stored them puts on.
struct VecMixedArgs {
  VecSampleArgs live;   // the ring
  VecSampleArgs demo;   // the partition: the same u, outputs, B, K, nstep and gamma
  long base;            // R N: the partition's first slot
  int Bd;               // batch rows 0 .. Bd-1 come from the partition
};

__global__ __launch_bounds__(256) void vec_sample_mixed_kernel(VecMixedArgs m) {
  const int which = m.live.obs_out ? blockIdx.y : 2;   // no output frames: the scalars only (grid.y == 1)
  const int b = which < 2 ? blockIdx.x : blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m.live.r.B) return;
  const bool part = b < m.Bd;                          // uniform over a copy block
  const VecSampleArgs& a = part ? m.demo : m.live;
  long t, e;
  const int k = vec_choose(a, b, t, e);
  if (which < 2) {
    const long p = ring_slot(a.r.g, k == 0 ? t : (which == 0 ? t - 1 : t + k - 1), e);
    const uint4* src = reinterpret_cast<const uint4*>(a.frames + p * a.frame_bytes);
    uint4* dst = reinterpret_cast<uint4*>((which == 0 ? a.obs_out : a.next_obs_out) + (long)b * a.frame_bytes);
    const long n16 = a.frame_bytes >> 4;
    for (long i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    return;
  }
  ring_emit_row(a.r, b, t, e, k);
  if (part) {
    const long B = a.r.B;
    for (int q = 0; q < 3; ++q) a.r.idx_out[q * B + b] += m.base;   // this thread's own stores
  }
}

// ---- prioritized sampling: the sum tree over the ring's slots -----------------------------------------------------
__global__ __launch_bounds__(kPerThreads) void vec_per_advance_kernel(double* tree, long L, const uint8_t* first, long N,
                                                                      long enter_row, long leave_row) {
  const double v = tree[0];
  long a[2] = {-1, -1}, b[2] = {-1, -1};
  if (enter_row >= 0) {
    const long s0 = enter_row * N;
    for (long e = threadIdx.x; e < N; e += kPerThreads) tree[L + s0 + e] = first[s0 + e] ? 0.0 : v;
    a[0] = L + s0;
    b[0] = L + s0 + N - 1;
  }
  if (leave_row >= 0) {
    const long s0 = leave_row * N;
    for (long e = threadIdx.x; e < N; e += kPerThreads) tree[L + s0 + e] = 0.0;
    a[1] = L + s0;
    b[1] = L + s0 + N - 1;
  }
  per_rebuild_ranges(tree, L, a, b);
}

struct VecPerSampleArgs {
  RingBatch r;
  const double* tree;
  const double* u;
  float* weight_out;
  long L;
  double beta;
};

__global__ __launch_bounds__(kPerThreads) void vec_per_sample_kernel(VecPerSampleArgs a) {
  const VecRing& g = a.r.g;
  const double total = a.tree[1];
  const double n = (double)((g.hi - g.lo + 1) * g.N);     // nominal count, reset rows included: cancels in w / wmax
  double wmax = 0.0;
  for (int b = threadIdx.x; b < a.r.B; b += kPerThreads) {
    // row b draws from its own stratum of the total mass
    const long k = per_descend(a.tree, a.L, ((double)b + a.u[b]) / (double)a.r.B * total);
    long t = g.lo, e = 0;
    int steps = 0;
    // an empty tree (total == 0) draws nothing; with the invariant kept a positive root never ends on a slot that is
    // not drawable, and should one arrive all the same the row is the empty one too: nothing is read out of range
    if (total > 0.0 && ring_drawable(g, k - a.L, t)) {
      e = (k - a.L) % g.N;
      steps = ring_window(g, t, e, a.r.nstep);
    } else {
      t = g.lo;
    }
    ring_emit_row(a.r, b, t, e, steps);
    wmax = fmax(wmax, steps > 0 ? per_weight(a.tree[k], total, n, a.beta) : 1.0);
  }
  per_normalise(wmax, a.r.B, [&](int b) {
    const long pos = a.r.idx_out[2L * a.r.B + b];   // this thread's own stores
    return a.r.steps_out[b] > 0 ? per_weight(a.tree[a.L + pos], total, n, a.beta) : 1.0;
  }, a.weight_out);
}

__global__ __launch_bounds__(kPerThreads) void vec_per_update_kernel(double* tree, long L, VecRing g, const long* pos,
                                                                     const float* td_abs, int B, double alpha,
                                                                     double eps) {
  // only where the position is still drawable: its slot may have left the drawable rows since the batch was drawn
  per_update(tree, L, pos, td_abs, B, alpha, eps, [&g](long p) {
    long t;
    return ring_drawable(g, p, t);
  });
}

// the arguments every tree entry shares: the tree covers the ring's slots
inline bool ring_tree_ok(const double* tree, long L, const uint8_t* first, long R, long N) {
  return tree && first && pow2(L) && R > 0 && N > 0 && N <= INT32_MAX && R <= INT64_MAX / N && L >= R * N;
}

// drawable rows lo .. hi of a ring with T rows added whose windows are `span` rows long at least: rows lo-1 .. hi+span-1
// exist, are still in the ring and are distinct ring rows
inline bool ring_bounds_ok(long R, long T, long lo, long hi, long span) {
  return lo >= 1 && hi >= lo && hi - lo + 1 + span <= R && hi + span <= T && lo - 1 >= T - R;
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
  VecAddArgs a{RingRowScalars{action, reward, discount, first, src_action, src_reward, src_discount, src_first, t % R,
                              (int)N, A, t == 0 ? 1 : 0},
               frames, src_obs, N * (frame_bytes >> 4), frame_bytes};
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
  VecSampleArgs a{RingBatch{VecRing{first, R, N, 0, lo, hi}, action, reward, discount, idx_out, act_out, rew_out, disc_out,
                            steps_out, A, B, nstep, gamma},
                  u, frames, obs_out, next_obs_out, frame_bytes, K};
  if (obs_out) hipLaunchKernelGGL(vec_sample_kernel, dim3(B, 3), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(vec_sample_kernel, dim3((B + 255) / 256, 1), dim3(256), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_sample_mixed(const uint8_t* first, const float* action, const float* reward, const float* discount,
                                 long R, long D, long N, int A, long frame_bytes, long lo, long hi, long Td,
                                 const double* u, int B, int Bd, int K, int nstep, float gamma, long* idx_out,
                                 float* act_out, float* rew_out, float* disc_out, int* steps_out, const uint8_t* frames,
                                 uint8_t* obs_out, uint8_t* next_obs_out, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!first || !action || !reward || !discount || !u || !idx_out || !act_out || !rew_out || !disc_out || !steps_out)
    return DRQ_EARG;
  if (R <= 0 || N <= 0 || A <= 0 || B <= 0 || K <= 0 || nstep <= 0 || frame_bytes <= 0 || frame_bytes % 16)
    return DRQ_EARG;
  if (D <= 0 || Td < 0 || Td > D || Bd < 0 || Bd > B) return DRQ_EARG;
  // the slots of the whole allocation, times the widest row, stay inside a long
  if (N > INT32_MAX || R > INT64_MAX - D || R + D > INT64_MAX / N || frame_bytes > INT64_MAX / ((R + D) * N) ||
      A > INT64_MAX / ((R + D) * N))
    return DRQ_EARG;
  // the ring, if a row is drawn from it: drq_vec_sample's bounds
  if (Bd < B && (lo < 1 || hi < lo || hi - lo + 1 + nstep > R)) return DRQ_EARG;
  // the partition, if a row is drawn from it: rows 1 .. Td - nstep, whose windows end inside the Td rows filled
  if (Bd > 0 && Td - nstep < 1) return DRQ_EARG;
  const int given = (frames != nullptr) + (obs_out != nullptr) + (next_obs_out != nullptr);
  if (given != 0 && given != 3) return DRQ_EARG;
  if (((uintptr_t)frames | (uintptr_t)obs_out | (uintptr_t)next_obs_out) & 15) return DRQ_EARG;
  const long base = R * N;
  VecMixedArgs m{
      VecSampleArgs{RingBatch{VecRing{first, R, N, 0, lo, hi}, action, reward, discount, idx_out, act_out, rew_out,
                              disc_out, steps_out, A, B, nstep, gamma},
                    u, frames, obs_out, next_obs_out, frame_bytes, K},
      VecSampleArgs{RingBatch{VecRing{first + base, D, N, 0, 1, Td - nstep}, action + base * A, reward + base,
                              discount + base, idx_out, act_out, rew_out, disc_out, steps_out, A, B, nstep, gamma},
                    u, frames ? frames + base * frame_bytes : nullptr, obs_out, next_obs_out, frame_bytes, K},
      base, Bd};
  if (obs_out) hipLaunchKernelGGL(vec_sample_mixed_kernel, dim3(B, 3), dim3(256), 0, st, m);
  else hipLaunchKernelGGL(vec_sample_mixed_kernel, dim3((B + 255) / 256, 1), dim3(256), 0, st, m);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_per_advance(double* tree, long L, const uint8_t* first, long R, long N, long T, long enter_t,
                                long leave_t, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!ring_tree_ok(tree, L, first, R, N) || T <= 0) return DRQ_EARG;
  // a row outside [T - R, T) is not in the ring any more: its slots hold a newer one
  const long oldest = T - R > 0 ? T - R : 0;
  if (enter_t < -1 || enter_t >= T || leave_t < -1 || leave_t >= T) return DRQ_EARG;
  if ((enter_t >= 0 && enter_t < oldest) || (leave_t >= 0 && leave_t < oldest)) return DRQ_EARG;
  if (enter_t >= 0 && enter_t == leave_t) return DRQ_EARG;
  if (enter_t < 0 && leave_t < 0) return DRQ_OK;
  hipLaunchKernelGGL(vec_per_advance_kernel, dim3(1), dim3(kPerThreads), 0, st, tree, L, first, N,
                     enter_t < 0 ? -1 : enter_t % R, leave_t < 0 ? -1 : leave_t % R);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_per_sample(const double* tree, long L, const uint8_t* first, const float* action,
                               const float* reward, const float* discount, long R, long N, int A, long T, long lo, long hi,
                               const double* u, int B, int nstep, float gamma, double beta, long* idx_out, float* act_out,
                               float* rew_out, float* disc_out, int* steps_out, float* weight_out, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!action || !reward || !discount || !u || !idx_out || !act_out || !rew_out || !disc_out || !steps_out || !weight_out)
    return DRQ_EARG;
  if (!ring_tree_ok(tree, L, first, R, N) || A <= 0 || B <= 0 || nstep <= 0 || !(beta >= 0.0)) return DRQ_EARG;
  if (!ring_bounds_ok(R, T, lo, hi, nstep)) return DRQ_EARG;
  VecPerSampleArgs a{RingBatch{VecRing{first, R, N, T, lo, hi}, action, reward, discount, idx_out, act_out, rew_out,
                               disc_out, steps_out, A, B, nstep, gamma},
                     tree, u, weight_out, L, beta};
  hipLaunchKernelGGL(vec_per_sample_kernel, dim3(1), dim3(kPerThreads), 0, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_per_update(double* tree, long L, const uint8_t* first, long R, long N, long T, long lo, long hi,
                               const long* pos, const float* td_abs, int B, double alpha, double eps,
                               drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!pos || !td_abs || !ring_tree_ok(tree, L, first, R, N) || B <= 0 || !(alpha > 0.0) || !(eps >= 0.0)) return DRQ_EARG;
  if (!ring_bounds_ok(R, T, lo, hi, 1)) return DRQ_EARG;
  hipLaunchKernelGGL(vec_per_update_kernel, dim3(1), dim3(kPerThreads), 0, st, tree, L, VecRing{first, R, N, T, lo, hi},
                     pos, td_abs, B, alpha, eps);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
