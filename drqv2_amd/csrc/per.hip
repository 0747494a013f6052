// Proportional prioritized replay (Schaul et al.) on the device store: a priority sum tree in HBM and the three
// launches that maintain it and draw from it (contract: include/drqv2_hip.h).  New functionality, the reference's
// replay is uniform.
//
// Every entry is ONE launch of ONE workgroup of 1,024 threads that walks the tree level by level with a workgroup
// barrier between the levels: the work is a few thousand nodes at most, and a single workgroup needs no grid barrier.
// A level reads what the level below it stored to GLOBAL memory.  __syncthreads() is a workgroup-scope release, the
// barrier and a workgroup-scope acquire: every wave drains its stores (vmcnt(0)) before it arrives, and all waves of a
// workgroup sit on one compute unit and share its vector L1, so the stores are visible to the loads behind the barrier.
// Nothing here talks to another workgroup; that would need agent scope.  Plain C++, vector stores, no atomics.
// An inner node is always recomputed as tree[2k] + tree[2k+1], never adjusted by a difference: it cannot drift.
#include "common.h"
#include "per_tree.h"
#include "../../include/drqv2_hip.h"

namespace {

__global__ __launch_bounds__(kPerThreads) void per_fill_kernel(double* tree, long L, long lo, long hi, int mode) {
  const double v = mode ? tree[0] : 0.0;
  for (long s = lo + threadIdx.x; s < hi; s += kPerThreads) tree[L + s] = v;
  per_rebuild_range(tree, L + lo, L + hi - 1);
}

__global__ __launch_bounds__(kPerThreads) void per_sample_kernel(const double* tree, long L, const double* u, int B,
                                                                 int nstep, double n_valid, double beta, long* idx_out,
                                                                 float* weight_out) {
  __shared__ double sm[kPerThreads];
  const double total = tree[1];
  double wmax = 0.0;
  for (int i = threadIdx.x; i < B; i += kPerThreads) {
    // row i draws from its own stratum of the total mass
    double m = ((double)i + u[i]) / (double)B * total;
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
    // an empty tree is refused by the host before the launch; should one arrive all the same, the row names slot 1
    // (inside every store) instead of slot 0, whose obs index would be -1
    const long pos = total > 0.0 ? k - L : 1;
    idx_out[i] = pos - 1;
    idx_out[(long)B + i] = pos + nstep - 1;
    idx_out[2L * B + i] = pos;
    wmax = fmax(wmax, total > 0.0 ? per_weight(tree[k], total, n_valid, beta) : 1.0);
  }
  wmax = per_block_max(wmax, sm);
  // second pass: the same expression on the same operands gives the same bits, so the largest weight is exactly 1
  for (int i = threadIdx.x; i < B; i += kPerThreads) {
    const long pos = idx_out[2L * B + i];   // this thread's own store
    const double w = total > 0.0 ? per_weight(tree[L + pos], total, n_valid, beta) : 1.0;
    weight_out[i] = (float)(w / wmax);
  }
}

__global__ __launch_bounds__(kPerThreads) void per_update_kernel(double* tree, long L, const long* pos,
                                                                 const float* td_abs, int B, double alpha, double eps) {
  __shared__ double sm[kPerThreads];
  __shared__ long sp[kPerThreads];
  double vmax = 0.0;
  // leaves.  Row i writes unless a row j > i names the same position: the highest row wins, whatever the schedule
  for (int i0 = 0; i0 < B; i0 += kPerThreads) {
    const int i = i0 + threadIdx.x;
    const long my = i < B ? pos[i] : -1;
    bool win = i < B && my >= 0 && my < L;
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
  // ancestors: every row recomputes the node above its leaf at each level; rows that share a node store the same sum
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

}  // namespace

DRQ_API int drq_per_fill(double* tree, long L, long lo, long hi, int mode, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tree || !pow2(L) || lo < 0 || hi < lo || hi > L || (mode != 0 && mode != 1)) return DRQ_EARG;
  if (lo == hi) return DRQ_OK;
  hipLaunchKernelGGL(per_fill_kernel, dim3(1), dim3(kPerThreads), 0, st, tree, L, lo, hi, mode);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_per_sample(const double* tree, long L, const double* u, int B, int nstep, long n_valid, double beta,
                           long* idx_out, float* weight_out, drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tree || !u || !idx_out || !weight_out || B <= 0 || !pow2(L) || nstep <= 0 || n_valid <= 0 || !(beta >= 0.0))
    return DRQ_EARG;
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(kPerThreads), 0, st, tree, L, u, B, nstep, (double)n_valid, beta,
                     idx_out, weight_out);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_per_update(double* tree, long L, const long* pos, const float* td_abs, int B, double alpha, double eps,
                           drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!tree || !pos || !td_abs || B <= 0 || !pow2(L) || !(alpha > 0.0) || !(eps >= 0.0)) return DRQ_EARG;
  hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(kPerThreads), 0, st, tree, L, pos, td_abs, B, alpha, eps);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
