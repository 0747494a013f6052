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
//   draw       per.hip's stratified descent to a slot p; e = p % N, ring row r = p / N, absolute row
//              t = T-1 - ((T-1-r) mod R); from there vec_sample_kernel's scalar block: window, indices, action,
//              n-step reward / discount in the same float32 order with the same pinned products.  Weights
//              (n leaf / tree[1])^-beta / max_batch with the nominal n = (hi-lo+1) N, which cancels against the maximum
//   update     leaf(p) = (clamp(td_abs) + eps)^alpha only where p is still drawable (checked here from T, lo, hi and
//              first: the host never reads a flag); the highest row of a repeated position wins
// The host never learns whether the tree is empty (every drawable row a reset row): such a draw comes out as the
// uniform path's "no drawable transition" rows, all indices on slot(lo, 0), steps 0, reward 0, discount 0, weight 1.
#include "common.h"
#include "per_tree.h"
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

// ---- prioritized sampling: the sum tree over the ring's slots -----------------------------------------------------
struct VecRing {
  const uint8_t* first;
  long R, N, T, lo, hi;
};

__device__ __forceinline__ long ring_slot(const VecRing& g, long t, long e) { return (t % g.R) * g.N + e; }

// the absolute row ring row r holds with T rows added: the newest t <= T-1 with t mod R == r (negative: never written)
__device__ __forceinline__ long ring_row_of(const VecRing& g, long r) {
  long d = (g.T - 1 - r) % g.R;
  if (d < 0) d += g.R;
  return g.T - 1 - d;
}

// slot p holds a drawable transition: inside the ring, its row t among lo .. hi, no reset row
__device__ __forceinline__ bool ring_drawable(const VecRing& g, long p, long& t) {
  if (p < 0 || p >= g.R * g.N) return false;
  t = ring_row_of(g, p / g.N);
  return t >= g.lo && t <= g.hi && g.first[p] == 0;
}

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
  // the ancestors of both ranges, level by level.  Where the ranges meet further up, two threads store the same sum of
  // the same children (as the rows of per_update_kernel that share a node do)
  for (long w = L; w > 1; w >>= 1) {
    __syncthreads();
    for (int q = 0; q < 2; ++q) {
      if (a[q] < 0) continue;
      a[q] >>= 1;
      b[q] >>= 1;
      for (long k = a[q] + threadIdx.x; k <= b[q]; k += kPerThreads) tree[k] = tree[2 * k] + tree[2 * k + 1];
    }
  }
}

struct VecPerSampleArgs {
  const double* tree;
  const float* action;
  const float* reward;
  const float* discount;
  const double* u;
  long* idx_out;
  float* act_out;
  float* rew_out;
  float* disc_out;
  int* steps_out;
  float* weight_out;
  VecRing g;
  long L;
  int A, B, nstep;
  float gamma;
  double beta;
};

__global__ __launch_bounds__(kPerThreads) void vec_per_sample_kernel(VecPerSampleArgs a) {
#pragma clang fp contract(off)
  __shared__ double sm[kPerThreads];
  const VecRing& g = a.g;
  const double total = a.tree[1];
  const double n = (double)((g.hi - g.lo + 1) * g.N);     // nominal count, reset rows included: cancels in w / wmax
  double wmax = 0.0;
  for (int b = threadIdx.x; b < a.B; b += kPerThreads) {
    // per_sample_kernel's descent: row b draws from its own stratum of the total mass
    double m = ((double)b + a.u[b]) / (double)a.B * total;
    long k = 1;
    while (k < a.L) {
      const double left = a.tree[2 * k], right = a.tree[2 * k + 1];
      if ((m < left && left > 0.0) || right == 0.0) {
        k = 2 * k;
      } else {
        m -= left;
        k = 2 * k + 1;
      }
    }
    long p = k - a.L, t = g.lo, e = 0;
    int steps = 0;
    // an empty tree (total == 0) draws nothing; with the invariant kept a positive root never ends on a slot that is
    // not drawable, and should one arrive all the same the row is the empty one too: nothing is read out of range
    if (total > 0.0 && ring_drawable(g, p, t)) {
      e = p % g.N;
      steps = a.nstep;
      for (int i = 1; i < a.nstep; ++i)
        if (g.first[ring_slot(g, t + i, e)]) {
          steps = i;
          break;
        }
    } else {
      t = g.lo;
      p = ring_slot(g, t, 0);
    }
    // from here vec_sample_kernel's scalar block
    a.idx_out[b] = steps == 0 ? p : ring_slot(g, t - 1, e);
    a.idx_out[(long)a.B + b] = steps == 0 ? p : ring_slot(g, t + steps - 1, e);
    a.idx_out[2L * a.B + b] = p;
    a.steps_out[b] = steps;
    for (int j = 0; j < a.A; ++j) a.act_out[(long)b * a.A + j] = a.action[p * a.A + j];
    float r = 0.f, d = 1.f;
    for (int i = 0; i < steps; ++i) {
      const long q = ring_slot(g, t + i, e);
      float x = d * a.reward[q];
      asm volatile("" : "+v"(x));
      r = r + x;
      float gd = a.discount[q] * a.gamma;
      asm volatile("" : "+v"(gd));
      d = d * gd;
    }
    a.rew_out[b] = r;
    a.disc_out[b] = steps == 0 ? 0.f : d;
    wmax = fmax(wmax, steps > 0 ? per_weight(a.tree[k], total, n, a.beta) : 1.0);
  }
  wmax = per_block_max(wmax, sm);
  // second pass: the same expression on the same operands gives the same bits, so the largest weight is exactly 1
  for (int b = threadIdx.x; b < a.B; b += kPerThreads) {
    const long pos = a.idx_out[2L * a.B + b];   // this thread's own stores
    const double w = a.steps_out[b] > 0 ? per_weight(a.tree[a.L + pos], total, n, a.beta) : 1.0;
    a.weight_out[b] = (float)(w / wmax);
  }
}

__global__ __launch_bounds__(kPerThreads) void vec_per_update_kernel(double* tree, long L, VecRing g, const long* pos,
                                                                     const float* td_abs, int B, double alpha,
                                                                     double eps) {
  __shared__ double sm[kPerThreads];
  __shared__ long sp[kPerThreads];
  double vmax = 0.0;
  // leaves, as per_update_kernel writes them (the highest row of a repeated position wins, whatever the schedule), but
  // only where the position is still drawable: its slot may have left the drawable rows since the batch was drawn
  for (int i0 = 0; i0 < B; i0 += kPerThreads) {
    const int i = i0 + threadIdx.x;
    const long my = i < B ? pos[i] : -1;
    long t = 0;
    bool win = i < B && ring_drawable(g, my, t);
    for (int j0 = i0; j0 < B; j0 += kPerThreads) {
      __syncthreads();
      sp[threadIdx.x] = j0 + (int)threadIdx.x < B ? pos[j0 + threadIdx.x] : -1;
      __syncthreads();
      const int n = min(kPerThreads, B - j0);
      for (int jj = 0; jj < n; ++jj)
        if (j0 + jj > i && sp[jj] == my) win = false;
    }
    if (win) {
      const double v = per_priority(td_abs[i], alpha, eps);
      tree[L + my] = v;
      vmax = fmax(vmax, v);
    }
  }
  // ancestors: every row whose position lies in the tree recomputes the node above its leaf at each level, a skipped
  // one too (its nodes get the sums they held); rows that share a node store the same sum
  for (int d = 1; (L >> d) >= 1; ++d) {
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += kPerThreads) {
      const long my = pos[i];
      if (my < 0 || my >= L) continue;
      const long k = (L + my) >> d;
      tree[k] = tree[2 * k] + tree[2 * k + 1];
    }
  }
  vmax = per_block_max(vmax, sm);
  if (threadIdx.x == 0) tree[0] = fmax(tree[0], vmax);
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
  VecPerSampleArgs a{tree, action, reward, discount, u, idx_out, act_out, rew_out, disc_out, steps_out, weight_out,
                     VecRing{first, R, N, T, lo, hi}, L, A, B, nstep, gamma, beta};
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
