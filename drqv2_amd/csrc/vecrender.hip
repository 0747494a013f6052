// Renderer images into a single-frame step-major ring (contract: include/drqv2_hip.h, "renderer images").  New
// functionality: the reference's environments render 84 x 84 and its wrappers transpose on the host (dmc.py:87-109);
// here an add takes the uint8 [N][S][S][Cin] image a GPU renderer hands out, S = 84 .. 336, Cin = 3 or 4, and writes the
// 3 x 84 x 84 CHW frame of every environment into row t mod R: the exact area average of the contract, in integers.
//
// drq_vec_add_render is one launch of N x 21 workgroups of 256 threads: workgroup (e, b) makes output rows 4 b .. 4 b + 3
// of environment e, all three channels -- 336 bytes per channel plane, a multiple of 16 at a multiple of 16.
//   load      the input rows the band touches (at most 4 S / 84 + 2) are one contiguous byte range of the image; it goes
//             to LDS as it lies, in 16-byte pieces at 16-byte aligned addresses, consecutive lanes consecutive pieces.  A
//             piece that is not wholly inside the image (only the first and the last of the whole array can be) is put
//             together from guarded byte loads: nothing outside the image is read
//   across    one thread per (input row, output x): the at most 5 taps of the three channels -> int32 [row][c][84] in
//             LDS, each <= 255 S.  Cin = 4 reads a pixel as one dword (its address is a multiple of 4 because
//             src_image is) and never looks at its fourth byte; Cin = 3 reads bytes
//   down      252 threads, one per 4 consecutive output bytes of a channel: the at most 5 taps as 16-byte LDS reads,
//             sum <= 255 S^2 < 2^31, + S^2 / 2, / S^2, the four bytes packed into LDS
//   store     63 lanes, 16 bytes each
// The separable order is exact because everything is an integer; the rounding and the division happen once.  Weights
// and tap ranges are functions of (output index, S), computed where they are used; nothing is kept between calls.
// S = 84 takes the same path (one tap of weight 84 per axis, 84^2 / 84^2): no separate kernel has been measured against it.
// The scalars of the row are drq_vec_add's, the same device code (ring_add_scalars, replay_device.h), spread over the
// whole grid.  Plain vector loads and stores, no atomics, nothing crosses workgroups.
#include "common.h"
#include "replay_device.h"
#include "../../include/drqv2_hip.h"

namespace {

constexpr int kOut = 84;                    // the frame is 3 x kOut x kOut
constexpr int kBandRows = 4;                // output rows per workgroup: 4 x 84 = 336 bytes per plane = 21 x 16
constexpr int kBands = kOut / kBandRows;    // 21
constexpr int kPlane = kOut * kOut;         // 7,056 bytes = 441 x 16
constexpr int kBandBytes = kBandRows * kOut;
constexpr int kMinS = 84, kMaxS = 336;      // 255 * 336^2 + 336^2 / 2 = 28,844,928 < 2^31

// the input pixels output pixel o touches along one axis, first .. last (at most 5 for S <= 336; at most 4 for S <= 256)
__host__ __device__ __forceinline__ int tap_first(int o, int S) { return o * S / kOut; }
__host__ __device__ __forceinline__ int tap_last(int o, int S) { return ((o + 1) * S - 1) / kOut; }
// w(o, i), in units of 1/84 input pixel: the overlap of [S o, S (o + 1)) and [84 i, 84 (i + 1))
__device__ __forceinline__ int tap_weight(int o, int i, int S) {
  return min((o + 1) * S, kOut * (i + 1)) - max(o * S, kOut * i);
}

struct VecRenderArgs {
  RingRowScalars s;
  uint8_t* frames;
  const uint8_t* src;       // [N][S][S][Cin]
  long src_bytes;           // N S S Cin
  int S;
  int raw_bytes;            // LDS: the staged input rows (a multiple of 16), then the horizontal sums, then the band
  int max_rows;             // input rows a band touches at most
};

template <int CIN>
__global__ __launch_bounds__(256) void vec_add_render_kernel(VecRenderArgs a) {
  extern __shared__ uint4 smem[];
  uint8_t* raw = reinterpret_cast<uint8_t*>(smem);
  int* hs = reinterpret_cast<int*>(raw + a.raw_bytes);                           // [row][3][84]
  uint8_t* band = reinterpret_cast<uint8_t*>(hs + a.max_rows * 3 * kOut);        // [3][336]
  const int S = a.S, tid = threadIdx.x;
  const long e = blockIdx.x / kBands;
  const int b = blockIdx.x - (int)e * kBands;
  ring_add_scalars(a.s, (long)blockIdx.x * blockDim.x + tid, (long)gridDim.x * blockDim.x);

  // ---- load: input rows r0 .. r1 of environment e, bytes [g0, g1) of the image array
  const int y0 = b * kBandRows;
  const int r0 = tap_first(y0, S), r1 = tap_last(y0 + kBandRows - 1, S);
  const int rows = r1 - r0 + 1;                                                  // <= max_rows
  const long row_bytes = (long)S * CIN;
  const long g0 = (e * S + r0) * row_bytes, g1 = g0 + rows * row_bytes;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.src);
  const uintptr_t lo = (base + g0) & ~(uintptr_t)15;                             // LDS byte 0 is this address
  const int delta = (int)(base + g0 - lo);
  const int n16 = (int)((base + g1 - lo + 15) >> 4);                             // 16 n16 <= raw_bytes
  for (int i = tid; i < n16; i += 256) {
    const uintptr_t p = lo + 16 * (uintptr_t)i;
    uint4 v;
    if (p >= base && p + 16 <= base + a.src_bytes) {
      v = *reinterpret_cast<const uint4*>(p);
    } else {
      unsigned w[4] = {0, 0, 0, 0};
      for (int k = 0; k < 16; ++k)
        if (p + k >= base && p + k < base + a.src_bytes) w[k >> 2] |= (unsigned)*reinterpret_cast<const uint8_t*>(p + k) << (8 * (k & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    smem[i] = v;
  }
  __syncthreads();

  // ---- across: hs[r][c][x] = sum_j w(x, j) image[r0 + r][j][c]
  for (int i = tid; i < rows * kOut; i += 256) {
    const int r = i / kOut, x = i - r * kOut;
    const int j0 = tap_first(x, S), j1 = tap_last(x, S);
    const uint8_t* px = raw + delta + r * row_bytes + j0 * CIN;
    int s0 = 0, s1 = 0, s2 = 0;
    for (int j = j0; j <= j1; ++j, px += CIN) {
      const int w = tap_weight(x, j, S);
      if (CIN == 4) {
        const unsigned v = *reinterpret_cast<const unsigned*>(px);
        s0 += w * (int)(v & 255u);
        s1 += w * (int)((v >> 8) & 255u);
        s2 += w * (int)((v >> 16) & 255u);
      } else {
        s0 += w * px[0];
        s1 += w * px[1];
        s2 += w * px[2];
      }
    }
    int* h = hs + r * 3 * kOut + x;
    h[0] = s0;
    h[kOut] = s1;
    h[2 * kOut] = s2;
  }
  __syncthreads();

  // ---- down: four consecutive bytes of one channel of the band per thread
  if (tid < 3 * kBandBytes / 4) {
    const int c = tid / (kBandBytes / 4), q = tid - c * (kBandBytes / 4);
    const int yl = q / (kOut / 4), x = 4 * (q - yl * (kOut / 4));
    const int y = y0 + yl;
    const int i0 = tap_first(y, S), i1 = tap_last(y, S);
    int4 acc = make_int4(0, 0, 0, 0);
    for (int i = i0; i <= i1; ++i) {
      const int w = tap_weight(y, i, S);
      const int4 v = *reinterpret_cast<const int4*>(hs + ((i - r0) * 3 + c) * kOut + x);
      acc.x += w * v.x;
      acc.y += w * v.y;
      acc.z += w * v.z;
      acc.w += w * v.w;
    }
    const unsigned d = (unsigned)(S * S), half = d / 2;
    const unsigned o = ((unsigned)acc.x + half) / d | ((unsigned)acc.y + half) / d << 8 |
                       ((unsigned)acc.z + half) / d << 16 | ((unsigned)acc.w + half) / d << 24;
    reinterpret_cast<unsigned*>(band)[tid] = o;
  }
  __syncthreads();

  // ---- store: 21 pieces of 16 bytes per channel plane
  if (tid < 3 * kBandBytes / 16) {
    const int c = tid / (kBandBytes / 16), k = tid - c * (kBandBytes / 16);
    const long slot = a.s.row * a.s.N + e;
    uint8_t* dst = a.frames + slot * (3L * kPlane) + (long)c * kPlane + b * kBandBytes + 16 * k;
    *reinterpret_cast<uint4*>(dst) = reinterpret_cast<const uint4*>(band)[tid];
  }
}

}  // namespace

DRQ_API int drq_vec_add_render(uint8_t* frames, float* action, float* reward, float* discount, uint8_t* first, long R,
                               long N, int A, long t, const uint8_t* src_image, int S, int Cin, const float* src_action,
                               const float* src_reward, const float* src_discount, const uint8_t* src_first,
                               drq_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!frames || !action || !reward || !discount || !first || !src_image || !src_action || !src_reward || !src_discount)
    return DRQ_EARG;
  if (R <= 0 || N <= 0 || A <= 0 || t < 0) return DRQ_EARG;
  if (N > INT32_MAX / kBands) return DRQ_EARG;            // the grid: one workgroup per environment and band
  if (S < kMinS || S > kMaxS || (Cin != 3 && Cin != 4)) return DRQ_EARG;
  if (((uintptr_t)frames & 15) || ((uintptr_t)src_image & 3)) return DRQ_EARG;
  int max_rows = 0;
  for (int b = 0; b < kBands; ++b) {
    const int rows = tap_last(b * kBandRows + kBandRows - 1, S) - tap_first(b * kBandRows, S) + 1;
    max_rows = rows > max_rows ? rows : max_rows;
  }
  // the staged rows start up to 15 bytes into their first 16-byte piece and end inside their last
  const int raw_bytes = ((max_rows * S * Cin + 15) / 16 + 1) * 16;
  const size_t lds = (size_t)raw_bytes + (size_t)max_rows * 3 * kOut * sizeof(int) + 3 * kBandBytes;   // <= 41 KB
  VecRenderArgs a{RingRowScalars{action, reward, discount, first, src_action, src_reward, src_discount, src_first, t % R,
                                 (int)N, A, t == 0 ? 1 : 0},
                  frames, src_image, N * (long)S * S * Cin, S, raw_bytes, max_rows};
  const dim3 grid((unsigned)(N * kBands));
  if (Cin == 4) hipLaunchKernelGGL(vec_add_render_kernel<4>, grid, dim3(256), lds, st, a);
  else hipLaunchKernelGGL(vec_add_render_kernel<3>, grid, dim3(256), lds, st, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
