// Strong augmentations on uint8 frame stacks (contract: include/drqv2_hip.h, "strong augmentation").  New functionality:
// the reference's only augmentation is its random shift (drqv2.py:19-45, here fused into conv1).  These are the two that
// DMControl-GB's methods (SVEA, SODA, "DrQ + aug") are built from: random_overlay, the observation blended with an unrelated
// image, and random_conv, every frame passed through a random 3 x 3 convolution.  Both are stated to the bit and restated
// in numpy by tests/strongaug_oracle.py.  This file is compiled with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt (build.py): the convolution is single float32 operations in the written order,
// nothing is fused, and its one division is IEEE.
//
// drq_aug_overlay: a flat grid-stride walk over B x 3 x 441 items (sample, colour channel, piece of 16 pixels: a plane is 441
//   pieces, so a piece never crosses a channel).  An item loads its piece of the sample's bank image once and blends it
//   over the same piece of every one of the C / 3 frames: one 16-byte load and one 16-byte store per frame.  The blend is
//   two bytes per 32-bit operation: the even and the odd bytes of a dword sit in 16-bit halves, and
//   x (256 - a) + y a + 128 <= 255 x 256 + 128 < 2^16 never carries from one half into the other.  A lane reads a piece
//   of obs before it writes that piece of out and no other lane touches it, so out may be obs.
// drq_aug_random_conv: one workgroup of 256 threads per (sample, frame).
//   stage     the frame's three planes into LDS as they are, bytes, by aligned 16-byte loads; piece v of a plane sits at
//             dword 5 v, one dword of padding behind every 16 pixels, so that the lanes of a wave, a piece apart, are 5
//             dwords apart: every bank once, for the dword reads and for the byte reads of the neighbours alike
//             and the sample's 81 weights beside them
//   barrier   __syncthreads(): the planes and the weights are whole
//   weights   per quad of 4 pixels and input channel a lane reads that channel's 27 weights out of LDS as seven 16-byte
//             reads (one address for the whole wave: a broadcast): 84 reads per 16 pixels beside the 108 of the image.
//             All 81 held in vector registers for the whole kernel spilled to scratch at four waves per SIMD, and 81
//             scalar registers beside the kernel's own do not fit the scalar file
//   draw      441 pieces of 16 pixels, 1 or 2 per lane; a lane computes ALL THREE output channels of its 16 pixels, so
//             that the 27 inputs p of a pixel are converted and scaled once and not once per output channel, and stores
//             three pieces, one per channel plane.  A piece is four
//             quads of 4 pixels; a quad starts at a column that is a multiple of 4 and so never crosses a row (84 = 21 x
//             4) although a piece may.  Per quad and (ci, ky): one dword of LDS (columns j .. j + 3) and two bytes (columns
//             clamp(j - 1) and clamp(j + 4)) give the six inputs of the row; the accumulation order per output is the
//             contract's, ci then ky then kx.
// Both kernels store to global memory with 16-byte vector stores from plain C++; no atomics, nothing crosses workgroups.
#include "vecenv_common.h"      // the frame's geometry
#include "../../include/drqv2_hip.h"

namespace {

constexpr int kPlanePieces = kPlane / 16;                 // 441 pieces of 16 pixels
constexpr int kItems = 3 * kPlanePieces;                  // (channel, piece) items of one sample
constexpr int kPlaneLds = kPlane + 4 * kPlanePieces;      // bytes of a plane in LDS: pixel p at p + 4 (p >> 4)
constexpr int kQuadsPerRow = kSide / 4;

// ---------------------------------------------------------------------------------------------------- overlay
// the blend of four pixels: bytes 0 and 2 in one product, bytes 1 and 3 in the other
__device__ __forceinline__ unsigned blend4(unsigned x, unsigned y, unsigned a) {
  const unsigned m = 0x00FF00FFu, na = 256u - a;
  const unsigned even = ((x & m) * na + (y & m) * a + 0x00800080u) >> 8 & m;
  const unsigned odd = ((x >> 8 & m) * na + (y >> 8 & m) * a + 0x00800080u) >> 8 & m;
  return even | odd << 8;
}

__global__ __launch_bounds__(kThreads) void aug_overlay_kernel(const uint8_t* obs, const uint8_t* __restrict__ bank,
                                                               const int* __restrict__ idx, uint8_t* out, long B, int G,
                                                               int M, unsigned alpha) {
  const long total = B * kItems, stride = (long)gridDim.x * kThreads;
  const long sample_bytes = (long)G * kFrame;
  for (long item = (long)blockIdx.x * kThreads + threadIdx.x; item < total; item += stride) {
    const long b = item / kItems;
    const int rem = (int)(item - b * kItems);
    const int c = rem / kPlanePieces, v = rem - c * kPlanePieces;
    int m = idx[b];
    m = m < 0 ? 0 : (m > M - 1 ? M - 1 : m);               // no index reads outside the bank
    const uint4 y = *reinterpret_cast<const uint4*>(bank + (long)m * kFrame + c * kPlane + 16 * v);
    const long at = b * sample_bytes + c * kPlane + 16 * v;
    for (int g = 0; g < G; ++g) {
      const uint4 x = *reinterpret_cast<const uint4*>(obs + at + (long)g * kFrame);
      *reinterpret_cast<uint4*>(out + at + (long)g * kFrame) =
          make_uint4(blend4(x.x, y.x, alpha), blend4(x.y, y.y, alpha), blend4(x.z, y.z, alpha), blend4(x.w, y.w, alpha));
    }
  }
}

// ---------------------------------------------------------------------------------------------------- random conv
// the input of the contract for byte k of dword w: (float)byte * (1 / 255 rounded to float32), two operations
__device__ __forceinline__ float input_of(unsigned w, int k) { return (float)((w >> (8 * k)) & 255u) * 0.003921568859368563f; }

// steps 4 to 6 of the contract
__device__ __forceinline__ unsigned squash(float acc) {
  float q = acc / (1.0f + fabsf(acc));
  if (q != q) q = 0.0f;
  const float v = (0.5f + 0.5f * q) * 255.0f;
  return (unsigned)(int)(v + 0.5f);
}

__global__ __launch_bounds__(kThreads, 4) void aug_random_conv_kernel(const uint8_t* __restrict__ obs,
                                                                      const float* __restrict__ w,
                                                                      uint8_t* __restrict__ out, int G) {
  __shared__ unsigned s_image[3 * kPlaneLds / 4];
  __shared__ __attribute__((aligned(16))) float s_w[3 * 28];                            // [ci][co][ky][kx], 27 and a pad per input channel
  const int tid = threadIdx.x;
  const long b = blockIdx.x / G;
  const long frame = (long)blockIdx.x * kFrame;            // [B][G] frames lie back to back

  // ---- stage: piece v of plane c at dword c * (kPlaneLds / 4) + 5 v; the sample's 81 weights, input channel outermost
  for (int v = tid; v < kPieces; v += kThreads) {
    const int c = v / kPlanePieces, r = v - c * kPlanePieces;
    const uint4 f = *reinterpret_cast<const uint4*>(obs + frame + 16 * v);
    unsigned* dst = s_image + c * (kPlaneLds / 4) + 5 * r;
    dst[0] = f.x;
    dst[1] = f.y;
    dst[2] = f.z;
    dst[3] = f.w;
  }
  if (tid < 81) {
    const int co = tid / 27, ci = (tid / 9) % 3, tap = tid % 9;
    s_w[ci * 28 + co * 9 + tap] = w[b * 81 + tid];
  }
  __syncthreads();

  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(s_image);
  for (int v = tid; v < kPlanePieces; v += kThreads) {
    uint4 word[3];       // a shift register per output channel: after four quads (quad 0, quad 1, quad 2, quad 3)
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      const int quad = 4 * v + q;
      const int i = quad / kQuadsPerRow, j = 4 * (quad - i * kQuadsPerRow);
      const int jl = j > 0 ? j - 1 : 0, jr = j + 4 < kSide ? j + 4 : kSide - 1;
      float acc[3][4];                                     // output channel, pixel of the quad
#pragma unroll
      for (int co = 0; co < 3; ++co)
#pragma unroll
        for (int x = 0; x < 4; ++x) acc[co][x] = 0.0f;
#pragma unroll 1
      for (int ci = 0; ci < 3; ++ci) {
        float wt[28];                                      // (co, ky, kx) of this input channel: seven broadcast reads
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          const float4 w4 = *reinterpret_cast<const float4*>(s_w + ci * 28 + 4 * k);
          wt[4 * k] = w4.x, wt[4 * k + 1] = w4.y, wt[4 * k + 2] = w4.z, wt[4 * k + 3] = w4.w;
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          int si = i + ky - 1;
          si = si < 0 ? 0 : (si > kSide - 1 ? kSide - 1 : si);
          const int row = si * kSide;
          const int pm = row + j, pl = row + jl, pr = row + jr;
          const unsigned mid = s_image[ci * (kPlaneLds / 4) + (pm >> 2) + (pm >> 4)];
          float p[6];
          p[0] = (float)bytes[ci * kPlaneLds + pl + 4 * (pl >> 4)] * 0.003921568859368563f;
#pragma unroll
          for (int x = 0; x < 4; ++x) p[1 + x] = input_of(mid, x);
          p[5] = (float)bytes[ci * kPlaneLds + pr + 4 * (pr >> 4)] * 0.003921568859368563f;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int co = 0; co < 3; ++co)
#pragma unroll
              for (int x = 0; x < 4; ++x) acc[co][x] = acc[co][x] + wt[(co * 3 + ky) * 3 + kx] * p[x + kx];
          // the 36 products of a row are independent of the sums: unfenced, the scheduler forms all 108 of an input
          // channel before the first add and the kernel spills at four waves per SIMD
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int co = 0; co < 3; ++co) {
        const unsigned four = squash(acc[co][0]) | squash(acc[co][1]) << 8 | squash(acc[co][2]) << 16 | squash(acc[co][3]) << 24;
        word[co] = make_uint4(word[co].y, word[co].z, word[co].w, four);
      }
    }
#pragma unroll
    for (int co = 0; co < 3; ++co) *reinterpret_cast<uint4*>(out + frame + co * kPlane + 16 * v) = word[co];
  }
}

// what both entries refuse of the frames: B, C and the size of the batch
inline bool batch_ok(long B, int C) {
  if (B < 1 || (C != 3 && C != 6 && C != 9 && C != 12)) return false;
  return B <= (long)INT32_MAX / ((long)C * kPlane);       // B C 7,056 <= INT32_MAX
}

}  // namespace

DRQ_API int drq_aug_overlay(const uint8_t* obs, const uint8_t* bank, const int* idx, uint8_t* out, long B, int C, int M,
                            int alpha_q8, drq_stream_t stream) {
  if (!obs || !bank || !idx || !out) return DRQ_EARG;
  if (!batch_ok(B, C) || M < 1 || alpha_q8 < 0 || alpha_q8 > 256) return DRQ_EARG;
  if (((uintptr_t)obs | (uintptr_t)out | (uintptr_t)bank) & 15) return DRQ_EARG;
  if ((uintptr_t)idx & 3) return DRQ_EARG;
  const uintptr_t in = (uintptr_t)obs, o = (uintptr_t)out, bytes = (uintptr_t)B * C * kPlane;
  if (in != o && in < o + bytes && o < in + bytes) return DRQ_EARG;      // out is obs itself, or overlaps it nowhere
  const uintptr_t bk = (uintptr_t)bank, bank_bytes = (uintptr_t)M * kFrame;
  if (bk < o + bytes && o < bk + bank_bytes) return DRQ_EARG;             // the bank is only read
  hipLaunchKernelGGL(aug_overlay_kernel, dim3(drq_grid_for(B * kItems, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     obs, bank, idx, out, B, C / 3, M, (unsigned)alpha_q8);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_aug_random_conv(const uint8_t* obs, const float* w, uint8_t* out, long B, int C, drq_stream_t stream) {
  if (!obs || !w || !out) return DRQ_EARG;
  if (!batch_ok(B, C)) return DRQ_EARG;
  if (((uintptr_t)obs | (uintptr_t)out) & 15) return DRQ_EARG;
  if ((uintptr_t)w & 3) return DRQ_EARG;
  const uintptr_t in = (uintptr_t)obs, o = (uintptr_t)out, bytes = (uintptr_t)B * C * kPlane;
  if (in < o + bytes && o < in + bytes) return DRQ_EARG;                  // neighbours are read: out == obs included
  hipLaunchKernelGGL(aug_random_conv_kernel, dim3((unsigned)(B * (C / 3))), dim3(kThreads), 0, (hipStream_t)stream, obs, w,
                     out, C / 3);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
