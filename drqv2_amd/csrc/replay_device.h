// The device code the replay stores share: the n-step sum (vecframes.hip's flat stores, vecreplay.hip's ring), the
// priority sum tree (per.hip's episode store, vecreplay.hip's ring), the ring's geometry and batch rows (the uniform
// and the prioritized draw of vecreplay.hip), the scalars of an added row (vecreplay.hip's add, vecrender.hip's) and the
// frame stack of a single-frame ring (vecframes.hip's gather, conv1aug.hip's ring mode).  Layout and rules are the contract of include/drqv2_hip.h; the memory-ordering argument of
// the tree is per.hip's header comment: ONE workgroup of kPerThreads threads walks the levels with __syncthreads()
// between them, nothing crosses workgroups.
#pragma once
#include "common.h"

namespace {

// ---- n-step reward / discount -----------------------------------------------------------------------------------
// The reference's float32 order over the k steps whose store slots are slot_of(0 .. k-1):
//   r += d * reward[q];  d *= discount[q] * gamma
// One rounding per operation: each product is pinned in a register before the add / multiply that consumes it (the
// packed-math vectoriser otherwise emits v_pk_fma_f32 here, contract(off) notwithstanding).
template <class SlotOf>
__device__ __forceinline__ void nstep_sum(const float* reward, const float* discount, float gamma, int k, SlotOf slot_of,
                                          float& r, float& d) {
#pragma clang fp contract(off)
  r = 0.f;
  d = 1.f;
  for (int i = 0; i < k; ++i) {
    const long q = slot_of(i);
    float x = d * reward[q];
    asm volatile("" : "+v"(x));
    r = r + x;
    float gd = discount[q] * gamma;
    asm volatile("" : "+v"(gd));
    d = d * gd;
  }
}

// ---- the priority sum tree --------------------------------------------------------------------------------------
constexpr int kPerThreads = 1024;

inline bool pow2(long x) { return x > 0 && (x & (x - 1)) == 0; }

// tree[k] = tree[2k] + tree[2k+1] for the ancestors of the leaf nodes [a[q], b[q]] of every range q (a[q] < 0: no such
// range), level by level up to the root.  Where two ranges meet further up, two threads store the same sum of the
// same children.
template <int NR>
__device__ __forceinline__ void per_rebuild_ranges(double* tree, long L, long (&a)[NR], long (&b)[NR]) {
  for (long w = L; w > 1; w >>= 1) {
    __syncthreads();
    for (int q = 0; q < NR; ++q) {
      if (a[q] < 0) continue;
      a[q] >>= 1;
      b[q] >>= 1;
      for (long k = a[q] + threadIdx.x; k <= b[q]; k += kPerThreads) tree[k] = tree[2 * k] + tree[2 * k + 1];
    }
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

// the leaf node the mass m in [0, tree[1]) falls on
__device__ __forceinline__ long per_descend(const double* tree, long L, double m) {
  long k = 1;
  while (k < L) {
    const double left = tree[2 * k], right = tree[2 * k + 1];
    if ((m < left && left > 0.0) || right == 0.0) {
      k = 2 * k;
    } else {
      m -= left;
      k = 2 * k + 1;
    }
  }
  return k;
}

__device__ __forceinline__ double per_weight(double leaf, double total, double n_valid, double beta) {
  return pow(n_valid * leaf / total, -beta);
}

// The second pass of a draw.  wmax: this thread's largest weight of the first pass; weight_of(b): the weight of row b
// again, or 1 for an empty row.  The same expression on the same operands gives the same bits, so the largest weight
// of the batch comes out as exactly 1.
template <class WeightOf>
__device__ __forceinline__ void per_normalise(double wmax, int B, WeightOf weight_of, float* weight_out) {
  __shared__ double sm[kPerThreads];
  wmax = per_block_max(wmax, sm);
  for (int b = threadIdx.x; b < B; b += kPerThreads) weight_out[b] = (float)(weight_of(b) / wmax);
}

// A priority update: leaf(pos[i]) = (td_abs[i] + eps)^alpha where may_write(pos[i]); tree[0] keeps the largest leaf
// ever written.
template <class MayWrite>
__device__ __forceinline__ void per_update(double* tree, long L, const long* pos, const float* td_abs, int B,
                                           double alpha, double eps, MayWrite may_write) {
  __shared__ double sm[kPerThreads];
  __shared__ long sp[kPerThreads];
  double vmax = 0.0;
  // leaves.  Row i writes unless a row j > i names the same position: the highest row wins, whatever the schedule
  for (int i0 = 0; i0 < B; i0 += kPerThreads) {
    const int i = i0 + threadIdx.x;
    const long my = i < B ? pos[i] : -1;
    bool win = i < B && may_write(my);
    for (int j0 = i0; j0 < B; j0 += kPerThreads) {
      __syncthreads();
      sp[threadIdx.x] = j0 + (int)threadIdx.x < B ? pos[j0 + threadIdx.x] : -1;
      __syncthreads();
      const int n = min(kPerThreads, B - j0);
      for (int jj = 0; jj < n; ++jj)
        if (j0 + jj > i && sp[jj] == my) win = false;
    }
    if (win) {
      // a NaN or negative error counts as 0, an infinite one as the largest float, so the root stays finite
      double t = (double)td_abs[i];
      if (!(t >= 0.0)) t = 0.0;
      t = fmin(t, 3.4028234663852886e38);
      const double v = pow(t + eps, alpha);
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
      const long k = (L + my) >> d;   // the ancestor d levels above this row's leaf
      tree[k] = tree[2 * k] + tree[2 * k + 1];
    }
  }
  vmax = per_block_max(vmax, sm);
  if (threadIdx.x == 0) tree[0] = fmax(tree[0], vmax);
}

// ---- the step-major ring ----------------------------------------------------------------------------------------
// R rows of N environments, slot = row * N + env; absolute row t lives in ring row t mod R.  T rows added (the uniform
// draw does not know T and never asks for it), drawable rows lo .. hi.
struct VecRing {
  const uint8_t* first;
  long R, N, T, lo, hi;
};

__device__ __forceinline__ long ring_slot(const VecRing& g, long t, long e) { return (t % g.R) * g.N + e; }

// slot p holds a drawable transition: inside the ring, its row t among lo .. hi, no reset row
__device__ __forceinline__ bool ring_drawable(const VecRing& g, long p, long& t) {
  if (p < 0 || p >= g.R * g.N) return false;
  // the absolute row its ring row holds with T rows added: the newest t <= T-1 with t mod R == p / N (negative: never
  // written)
  long d = (g.T - 1 - p / g.N) % g.R;
  if (d < 0) d += g.R;
  t = g.T - 1 - d;
  return t >= g.lo && t <= g.hi && g.first[p] == 0;
}

// the length of the n-step window that starts at row t of environment e: it ends early at a reset row
__device__ __forceinline__ int ring_window(const VecRing& g, long t, long e, int nstep) {
  for (int i = 1; i < nstep; ++i)
    if (g.first[ring_slot(g, t + i, e)]) return i;
  return nstep;
}

// what a draw on the ring reads and writes per batch row, frames and weights aside
struct RingBatch {
  VecRing g;
  const float* action;
  const float* reward;
  const float* discount;
  long* idx_out;
  float* act_out;
  float* rew_out;
  float* disc_out;
  int* steps_out;
  int A, B, nstep;
  float gamma;
};

// The scalars of batch row b: the transition at row t of environment e with a window of `steps` rows; steps == 0 is
// the empty row (no drawable transition): all three indices on slot(t, e), reward 0, discount 0.
__device__ __forceinline__ void ring_emit_row(const RingBatch& a, int b, long t, long e, int steps) {
  const VecRing& g = a.g;
  const long p = ring_slot(g, t, e);
  a.idx_out[b] = steps == 0 ? p : ring_slot(g, t - 1, e);
  a.idx_out[(long)a.B + b] = steps == 0 ? p : ring_slot(g, t + steps - 1, e);
  a.idx_out[2L * a.B + b] = p;
  a.steps_out[b] = steps;
  for (int j = 0; j < a.A; ++j) a.act_out[(long)b * a.A + j] = a.action[p * a.A + j];
  float r, d;
  nstep_sum(a.reward, a.discount, a.gamma, steps, [&](int i) { return ring_slot(g, t + i, e); }, r, d);
  a.rew_out[b] = r;
  a.disc_out[b] = steps == 0 ? 0.f : d;
}

// ---- one row of an add: what is not the frame ---------------------------------------------------------------------
// (vecreplay.hip's drq_vec_add, vecrender.hip's drq_vec_add_render)  Ring row `row` of action, reward, discount and
// first from the sources of one step; thread tid of `step` threads, any grid.
struct RingRowScalars {
  float* action;
  float* reward;
  float* discount;
  uint8_t* first;
  const float* src_action;
  const float* src_reward;
  const float* src_discount;
  const uint8_t* src_first;   // null = all 0
  long row;                   // t mod R
  int N, A, force_first;      // force_first: t == 0, every environment starts an episode
};

__device__ __forceinline__ void ring_add_scalars(const RingRowScalars& a, long tid, long step) {
  const long base = a.row * a.N;   // first slot of the row
  const long na = (long)a.N * a.A;
  for (long i = tid; i < na; i += step) a.action[base * a.A + i] = a.src_action[i];
  for (long e = tid; e < a.N; e += step) {
    a.reward[base + e] = a.src_reward[e];
    a.discount[base + e] = a.src_discount[e];
    a.first[base + e] = (a.force_first || (a.src_first && a.src_first[e])) ? 1 : 0;
  }
}

// ---- single-frame rings: the frame stack is put together when it is read -------------------------------------------
// (contract: include/drqv2_hip.h, "single-frame step-major replay"; vecframes.hip's gather, conv1aug.hip's ring mode)
// The slots of the three frames of the stack whose newest frame lives in slot p0 (0 <= p0 < R N), oldest first: the
// rows one and two back of the same environment, ring rows modulo R, refilled from the reset row on (dmc.py:98-109).
// Every slot that is read or returned lies in [0, R N) whatever the flags hold; the second flag is read only where
// the first does not decide.
__device__ __forceinline__ void ring_stack_slots(const uint8_t* first, long R, long N, long p0, long (&s)[3]) {
  const long wrap = (R - 1) * N;
  const long p1 = p0 >= N ? p0 - N : p0 + wrap;
  const long p2 = p1 >= N ? p1 - N : p1 + wrap;
  s[2] = p0;
  if (first[p0]) {
    s[0] = s[1] = p0;
  } else if (first[p1]) {
    s[0] = s[1] = p1;
  } else {
    s[0] = p2;
    s[1] = p1;
  }
}

}  // namespace
