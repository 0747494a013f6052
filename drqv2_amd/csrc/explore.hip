// Count-based exploration bonus on the device (contract: include/drqv2_hip.h, "exploration bonus").  New functionality:
// the reference explores by the policy's own noise alone (drqv2.py:164-175); this is the count-based bonus of
// "#Exploration" (Tang et al. 2017) -- a SimHash of the frame, a table of counts, bonus = beta / sqrt(n) -- on the
// frames of N lockstep environments where they already are, without a download or a host wait.  Everything up to the
// count is integer arithmetic and exact; the bonus is one correctly rounded square root and one correctly rounded
// division (tests/simhash_oracle.py restates all of it in numpy).
//
// drq_explore_simhash_step enqueues two launches; the launch boundary between them is the grid-wide order "every
// increment before every read", so two environments with one code in one step both see the count after both increments.
//   hash and count   N workgroups of 256 threads, one per environment:
//     cells    a lane owns a cell of the 21 x 21 grid (441 cells: two rounds over the 256 lanes).  A frame row is 84
//              bytes = 21 dwords, so the four pixels of a cell row are ONE aligned dword: 3 channels x 4 rows = 12 loads
//              per cell, their 48 bytes summed by v_sad_u8.  Every byte of the frame is loaded exactly once.
//     centring the cell sums are added up inside the waves (__shfl_xor) and across them through LDS;
//              v = 441 s - sum goes to LDS (|v| <= 441 x 12,240: int32)
//     project  bit j belongs to wave j % 4.  A lane holds the v of its 7 cells (i = lane + 64 k) in registers, adds
//              +-v by the sign hash into an int64 and the wave adds the 64 partial sums up by __shfl_xor: every lane
//              then holds p_j and the wave ORs (p_j > 0) << j into its part of the code
//     count    thread 0 ORs the four parts, stores the code and, under `update`, does one atomicAdd on count[code]
//     Every trip count depends on `bits` alone, so it is the same in every workgroup and every wave.
//   bonus    ceil(N / 256) workgroups of 256 threads, one thread per environment: c = count[code], beta / sqrt(c) (beta
//            for c = 0), the optional reward add
#include "common.h"
#include "../../include/drqv2_hip.h"

namespace {

constexpr int kSide = 84;
constexpr int kRowDwords = kSide / 4;             // 21: a frame row
constexpr int kPlaneDwords = kSide * kRowDwords;  // 1,764: a channel plane
constexpr int kFrameDwords = 3 * kPlaneDwords;    // 5,292 = 21,168 bytes
constexpr int kGrid = 21;                         // cells per side
constexpr int kCells = kGrid * kGrid;             // 441
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kCellRounds = (kCells + kThreads - 1) / kThreads;   // 2
constexpr int kLaneCells = (kCells + 63) / 64;                    // 7

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void simhash_count_kernel(const unsigned* __restrict__ frame, int bits,
                                                                 unsigned seed, int update, int* count, int* code_out) {
  __shared__ int s_v[kCells];
  __shared__ int s_part[kWaves];
  __shared__ unsigned s_code[kWaves];
  const long e = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned* src = frame + e * (long)kFrameDwords;

  // cells: s of cell i = tid + 256 r, kept in a register until the total is known
  int s[kCellRounds];
  int part = 0;
#pragma unroll
  for (int r = 0; r < kCellRounds; ++r) {
    const int i = tid + r * kThreads;
    unsigned acc = 0u;
    if (i < kCells) {
      const int gy = i / kGrid, gx = i - gy * kGrid;
      const unsigned* p = src + 4 * gy * kRowDwords + gx;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc = __builtin_amdgcn_sad_u8(p[c * kPlaneDwords + y * kRowDwords], 0u, acc);
    }
    s[r] = (int)acc;
    part += (int)acc;                     // at most 441 x 12,240 over the whole workgroup
  }
  part = wave_sum(part);
  if (lane == 0) s_part[wave] = part;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) total += s_part[w];
#pragma unroll
  for (int r = 0; r < kCellRounds; ++r) {
    const int i = tid + r * kThreads;
    if (i < kCells) s_v[i] = kCells * s[r] - total;
  }
  __syncthreads();

  // projections: the lane's cells once into registers (0 past the end adds nothing), then one pass per bit of the wave
  int v[kLaneCells];
#pragma unroll
  for (int k = 0; k < kLaneCells; ++k) {
    const int i = lane + 64 * k;
    v[k] = i < kCells ? s_v[i] : 0;
  }
  unsigned code = 0u;
  const int rounds = (bits + kWaves - 1) / kWaves;
  for (int r = 0; r < rounds; ++r) {
    const int j = r * kWaves + wave;      // the same in all 64 lanes
    if (j < bits) {
      long long p = 0;
#pragma unroll
      for (int k = 0; k < kLaneCells; ++k) {
        const unsigned h = drq_fmix32(seed ^ (unsigned)(j * kCells + lane + 64 * k) * 0x9E3779B9u);
        p += (h & 1u) ? (long long)v[k] : -(long long)v[k];
      }
      p = wave_sum(p);
      code |= (unsigned)(p > 0) << j;
    }
  }
  if (lane == 0) s_code[wave] = code;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) code |= s_code[w];
    code_out[e] = (int)code;
    if (update) atomicAdd(count + code, 1);
  }
}

__global__ __launch_bounds__(kThreads) void simhash_bonus_kernel(const int* __restrict__ count,
                                                                 const int* __restrict__ code, long N, float beta,
                                                                 int* count_out, float* bonus_out,
                                                                 const float* __restrict__ reward, float* reward_out) {
  const long e = blockIdx.x * (long)kThreads + threadIdx.x;
  if (e >= N) return;
  const int c = count[code[e]];
  const float b = c == 0 ? beta : beta / sqrtf((float)c);
  count_out[e] = c;
  bonus_out[e] = b;
  if (reward) reward_out[e] = reward[e] + b;
}

}  // namespace

DRQ_API int drq_explore_simhash_step(const uint8_t* frame, long N, int bits, unsigned seed, float beta, int update,
                                     int* count, int* code_out, int* count_out, float* bonus_out, const float* reward,
                                     float* reward_out, drq_stream_t stream) {
  if (!frame || !count || !code_out || !count_out || !bonus_out) return DRQ_EARG;
  if (N < 1 || N > INT32_MAX || bits < 1 || bits > DRQ_SIMHASH_MAX_BITS) return DRQ_EARG;
  if (update != 0 && update != 1) return DRQ_EARG;
  if ((reward == nullptr) != (reward_out == nullptr)) return DRQ_EARG;
  if (((uintptr_t)frame | (uintptr_t)count | (uintptr_t)code_out | (uintptr_t)count_out | (uintptr_t)bonus_out |
       (uintptr_t)reward | (uintptr_t)reward_out) & 3)
    return DRQ_EARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(simhash_count_kernel, dim3((unsigned)N), dim3(kThreads), 0, st,
                     reinterpret_cast<const unsigned*>(frame), bits, seed, update, count, code_out);
  DRQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(simhash_bonus_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, count,
                     code_out, N, beta, count_out, bonus_out, reward, reward_out);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
