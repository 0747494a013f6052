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
// The descent, the weight normalisation, the priority update and the ranged rebuild are replay_device.h's, shared with
// the step-major ring (vecreplay.hip); the kernels here keep what is the episode store's own.
#include "common.h"
#include "replay_device.h"
#include "../../include/drqv2_hip.h"

namespace {

__global__ __launch_bounds__(kPerThreads) void per_fill_kernel(double* tree, long L, long lo, long hi, int mode) {
  const double v = mode ? tree[0] : 0.0;
  for (long s = lo + threadIdx.x; s < hi; s += kPerThreads) tree[L + s] = v;
  long a[1] = {L + lo}, b[1] = {L + hi - 1};
  per_rebuild_ranges(tree, L, a, b);
}

__global__ __launch_bounds__(kPerThreads) void per_sample_kernel(const double* tree, long L, const double* u, int B,
                                                                 int nstep, double n_valid, double beta, long* idx_out,
                                                                 float* weight_out) {
  const double total = tree[1];
  double wmax = 0.0;
  for (int i = threadIdx.x; i < B; i += kPerThreads) {
    // row i draws from its own stratum of the total mass
    const long k = per_descend(tree, L, ((double)i + u[i]) / (double)B * total);
    // an empty tree is refused by the host before the launch; should one arrive all the same, the row names slot 1
    // (inside every store) instead of slot 0, whose obs index would be -1
    const long pos = total > 0.0 ? k - L : 1;
    idx_out[i] = pos - 1;
    idx_out[(long)B + i] = pos + nstep - 1;
    idx_out[2L * B + i] = pos;
    wmax = fmax(wmax, total > 0.0 ? per_weight(tree[k], total, n_valid, beta) : 1.0);
  }
  per_normalise(wmax, B, [&](int i) {
    const long pos = idx_out[2L * B + i];   // this thread's own store
    return total > 0.0 ? per_weight(tree[L + pos], total, n_valid, beta) : 1.0;
  }, weight_out);
}

__global__ __launch_bounds__(kPerThreads) void per_update_kernel(double* tree, long L, const long* pos,
                                                                 const float* td_abs, int B, double alpha, double eps) {
  per_update(tree, L, pos, td_abs, B, alpha, eps, [L](long p) { return p >= 0 && p < L; });
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
