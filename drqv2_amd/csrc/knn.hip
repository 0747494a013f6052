// k-NN exploration bonus on the device (contract: include/drqv2_hip.h, "k-NN bonus").  New functionality: the distance
// RE3 (Seo et al. 2021) takes the logarithm of -- for each of B drawn rows of a feature table, the distance to its k-th
// nearest neighbour among the rows the ring holds -- without the B x M matrix of distances ever existing.  Every squared
// distance is the contract's chain of single float32 operations in the written order (tests/knn_oracle.py restates it
// in numpy), so D is the same bits however the candidates are dealt to workgroups, and the k-th smallest of a multiset of
// exact values does not depend on the order they were met in.
//
// drq_explore_knn enqueues two launches:
//   partial  grid (G, ceil(B / 256)), 256 threads.  A LANE OWNS A QUERY: its row sits in 64 VGPRs (zeros past d: a zero
//            difference adds +0, which changes no bit of a sum that starts at +0 and only grows), beside the sorted list
//            of its 8 smallest D.  The candidates come in chunks of DRQ_KNN_CHUNK = 128 rows, chunk ch to workgroup
//            ch % G, staged in LDS once per 256 queries: [pair of candidates][element][2], zero-padded to a multiple of 4
//            elements, so that one 16-byte read gives two elements of two candidates.  Every lane of a wave reads the
//            SAME address (a broadcast: no bank can conflict), and the two candidates of a pair run as the two halves
//            of packed float32 instructions, each half one IEEE operation.  Two pairs are in flight per trip (two
//            independent chains of adds).  A candidate that is the query's own row, lies past the chunk's end or gave a
//            NaN counts as +inf; a D enters the list by 8 min/max steps, which a wave skips when no lane's D is below
//            its 8th (almost always, once the lists have settled).  Each lane stores its list to ws[b][g][8].
//   merge    one wave per query: lane l folds the lists of workgroups l, l + 64, ... into its own, six butterfly rounds
//            of __shfl_xor fold the 64 lists into one, lane 0 counts the candidates (arithmetic on live, stride, offset
//            and the slot: nothing is read for it) and stores sqrtf of the k-th, or 0.
// No atomics, no ticket, nothing float is combined across lanes but by min and max.
#include "common.h"
#include "../../include/drqv2_hip.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = DRQ_KNN_CHUNK;        // candidates per chunk
constexpr int kMaxD = DRQ_KNN_MAX_DIM;       // 64
constexpr int kList = DRQ_KNN_MAX_K;         // 8: every list holds 8, k picks among them
constexpr int kTargetGroups = 512;           // workgroups the partial launch aims at: two per CU, what 174 VGPRs admit
static_assert(kChunk % 4 == 0 && kMaxD % 4 == 0 && kList == 8, "the staging and the 32-byte list records assume it");

typedef float f32x2 __attribute__((ext_vector_type(2)));

// v into the ascending list l: 8 min/max steps; v is no NaN
__device__ __forceinline__ void knn_insert(float (&l)[kList], float v) {
#pragma unroll
  for (int m = 0; m < kList; ++m) {
    const float lo = fminf(l[m], v);
    v = fmaxf(l[m], v);
    l[m] = lo;
  }
}

// the lattice index of slot s, or -1 when s is no candidate: c = offset + j * stride
__device__ __forceinline__ long knn_lattice(long s, long stride, long offset) {
  if (s < offset) return -1;
  const long r = s - offset;
  return r % stride == 0 ? r / stride : -1;
}

__global__ __launch_bounds__(kThreads, 2) void knn_partial_kernel(const float* __restrict__ table, long live,
                                                                   const int64_t* __restrict__ slots, long B, int d,
                                                                   long stride, long offset, long ncand, long nchunks,
                                                                   float* __restrict__ ws) {
  __shared__ f32x4 s_x[kChunk * kMaxD / 4];      // 32 KB: [pair][element][2] floats, the element stride is dp
  float* const s_xf = reinterpret_cast<float*>(s_x);
  const int tid = threadIdx.x;
  const int G = gridDim.x, g = blockIdx.x;
  const long b = blockIdx.y * (long)kThreads + tid;
  const int dp = (d + 3) & ~3;

  long s = -1;
  if (b < B) s = slots[b];
  const bool valid = s >= 0 && s < live;
  const long self = valid ? knn_lattice(s, stride, offset) : -1;
  float q[kMaxD];
  {
    const float* row = table + (valid ? s : 0) * (long)d;      // never formed from a slot outside the live rows
#pragma unroll
    for (int i = 0; i < kMaxD; ++i) q[i] = valid && i < d ? row[i] : 0.0f;
  }
  float l[kList];
#pragma unroll
  for (int m = 0; m < kList; ++m) l[m] = INFINITY;
  const bool wave_has_query = __ballot(valid) != 0ull;

  for (long ch = g; ch < nchunks; ch += G) {
    const long j0 = ch * kChunk;
    const int n = (int)(ncand - j0 < kChunk ? ncand - j0 : kChunk);       // 1 .. kChunk candidates in this chunk
    __syncthreads();                              // the chunk before this one has been read by every wave
    for (int e = tid; e < kChunk * dp; e += kThreads) {
      const int jl = e / dp, i = e - jl * dp;
      float v = 0.0f;
      if (jl < n && i < d) v = table[(offset + (j0 + jl) * stride) * (long)d + i];      // a row below live: jl < n
      s_xf[((jl >> 1) * dp + i) * 2 + (jl & 1)] = v;
    }
    __syncthreads();
    if (!wave_has_query) continue;
    const long sj = self - j0;
    const int self_local = sj >= 0 && sj < kChunk ? (int)sj : -1;
    const int pairs = (n + 1) >> 1;
    for (int p = 0; p < pairs; p += 2) {          // pairs p and p + 1: the second may lie past the end (zeros)
      const f32x4* xa = s_x + (p * dp) / 2;       // (p * dp + i) * 2 floats = (p * dp + i) / 2 float4
      const f32x4* xb = xa + dp / 2;
      f32x2 acc_a = {0.0f, 0.0f}, acc_b = {0.0f, 0.0f};
#pragma unroll
      for (int i4 = 0; i4 < kMaxD / 4; ++i4) {
        if (i4 * 4 < d) {                         // the same in every lane
          const f32x4 a0 = xa[2 * i4], a1 = xa[2 * i4 + 1], b0 = xb[2 * i4], b1 = xb[2 * i4 + 1];
          const f32x2 xs_a[4] = {{a0.x, a0.y}, {a0.z, a0.w}, {a1.x, a1.y}, {a1.z, a1.w}};
          const f32x2 xs_b[4] = {{b0.x, b0.y}, {b0.z, b0.w}, {b1.x, b1.y}, {b1.z, b1.w}};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const f32x2 qq = {q[4 * i4 + r], q[4 * i4 + r]};
            const f32x2 ta = qq - xs_a[r], tb = qq - xs_b[r];
            acc_a = acc_a + ta * ta;              // no contraction: the file is built with -ffp-contract=off
            acc_b = acc_b + tb * tb;
          }
        }
      }
      const float D[4] = {acc_a.x, acc_a.y, acc_b.x, acc_b.y};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jl = 2 * p + r;
        float v = D[r];
        if (jl >= n || jl == self_local || v != v) v = INFINITY;
        if (__ballot(v < l[kList - 1]) != 0ull) knn_insert(l, v);
      }
    }
  }
  if (b < B) {
    f32x4* out = reinterpret_cast<f32x4*>(ws + (b * G + g) * kList);
    out[0] = f32x4{l[0], l[1], l[2], l[3]};
    out[1] = f32x4{l[4], l[5], l[6], l[7]};
  }
}

__global__ __launch_bounds__(kThreads) void knn_merge_kernel(const float* __restrict__ ws, int G, long live,
                                                             const int64_t* __restrict__ slots, long B, int k,
                                                             long stride, long offset, long ncand,
                                                             float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  const long b = blockIdx.x * (long)(kThreads / 64) + (threadIdx.x >> 6);      // the same in every lane of a wave
  if (b >= B) return;
  float l[kList];
#pragma unroll
  for (int m = 0; m < kList; ++m) l[m] = INFINITY;
  for (int g = lane; g < G; g += 64) {
    const f32x4* in = reinterpret_cast<const f32x4*>(ws + (b * G + g) * kList);
    const f32x4 lo = in[0], hi = in[1];
    const float v[kList] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int m = 0; m < kList; ++m)
      if (v[m] < l[kList - 1]) knn_insert(l, v[m]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    float other[kList];
#pragma unroll
    for (int m = 0; m < kList; ++m) other[m] = __shfl_xor(l[m], o);
#pragma unroll
    for (int m = 0; m < kList; ++m) knn_insert(l, other[m]);
  }
  if (lane != 0) return;
  const long s = slots[b];
  float out = 0.0f;
  if (s >= 0 && s < live) {
    const long others = ncand - (knn_lattice(s, stride, offset) >= 0 ? 1 : 0);
    if (others >= k) {
      float kth = l[0];
#pragma unroll
      for (int m = 1; m < kList; ++m) kth = m == k - 1 ? l[m] : kth;
      out = sqrtf(kth);                           // correctly rounded: -fhip-fp32-correctly-rounded-divide-sqrt
    }
  }
  dist[b] = out;
}

long knn_candidates(long live, long stride, long offset) {
  return live > offset ? (live - offset + stride - 1) / stride : 0;
}

// workgroups per tile of 256 queries: one per chunk, up to two per CU
long knn_groups(long B, long ncand) {
  const long nchunks = (ncand + kChunk - 1) / kChunk;
  const long tiles = (B + kThreads - 1) / kThreads;
  long cap = kTargetGroups / tiles;
  if (cap < 1) cap = 1;
  return nchunks < cap ? nchunks : cap;
}

bool knn_shape_ok(long B, long live, long stride, long offset) {
  return B >= 1 && B <= DRQ_KNN_MAX_QUERIES && live >= 0 && stride >= 1 && offset >= 0 && offset < stride;
}

}  // namespace

DRQ_API size_t drq_explore_knn_ws_bytes(long B, long live, long stride) {
  if (!knn_shape_ok(B, live, stride, 0)) return 0;
  return (size_t)B * (size_t)knn_groups(B, knn_candidates(live, stride, 0)) * kList * sizeof(float);
}

DRQ_API int drq_explore_knn(const float* table, long S, int d, long live, const int64_t* slots, long B, int k,
                            long stride, long offset, float* dist, float* ws, size_t ws_bytes, drq_stream_t stream) {
  if (!table || !slots || !dist) return DRQ_EARG;
  if (S < 1 || d < 1 || d > kMaxD || live > S || k < 1 || k > kList) return DRQ_EARG;
  if (!knn_shape_ok(B, live, stride, offset)) return DRQ_EARG;
  if (((uintptr_t)table | (uintptr_t)dist) & 3 || (uintptr_t)slots & 7 || (uintptr_t)ws & 15) return DRQ_EARG;
  const long ncand = knn_candidates(live, stride, offset);
  const long G = knn_groups(B, ncand);
  if (G > 0 && (!ws || ws_bytes < (size_t)B * (size_t)G * kList * sizeof(float))) return DRQ_EWS;
  hipStream_t st = (hipStream_t)stream;
  if (G > 0) {
    const long nchunks = (ncand + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(knn_partial_kernel, dim3((unsigned)G, (unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       st, table, live, slots, B, d, stride, offset, ncand, nchunks, ws);
    DRQ_LAUNCH_CHECK();
  }
  const int per_block = kThreads / 64;
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((B + per_block - 1) / per_block)), dim3(kThreads), 0, st, ws, (int)G,
                     live, slots, B, k, stride, offset, ncand, dist);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
