// Evaluation of the vectorised loop (contract: include/drqv2_hip.h, "evaluation").  The reference builds the 9-channel
// observation of its one environment in a FrameStackWrapper on the host (dmc.py:87-109) and records evaluation episodes
// with video.py (train.py:98-122); for N lockstep environments whose frames live on the device both are one launch each
// here, and neither needs a replay ring.  Integer arithmetic only, no LDS, no atomics, nothing crosses workgroups.
//
// drq_vec_stack_push is the FrameStackWrapper rule for N environments: N x 4 workgroups of 256 threads, environment
// blockIdx.x, the 3,969 pieces of 16 bytes of its stack strided over the 1,024 threads of its four workgroups.  A stack is
// three frames of 1,323 pieces, so a piece never crosses a frame and every source piece is whole and aligned: piece v of
// next[e] is piece v + 1,323 of prev[e] (the two newer frames move down) or piece v - 2,646 of frame[e], and for a
// reset environment piece v mod 1,323 of frame[e].  The flag is one byte load per thread, the same in all of them.
//
// drq_vec_video_record writes one mosaic image, u8 [GH S][GW S][3], S = 84 k.  The image is walked as ONE flat byte
// array in pieces of PB bytes, 4 pieces per thread: its length GH GW 21,168 k^2 is a multiple of 16 whatever k is, so
// with `out` 16-byte aligned every piece is an aligned 16-byte store although a tile row (252 k bytes) is a multiple of 16
// for k = 4 only -- a piece simply runs across the seam between two tiles, or from the end of one image row into the
// next.  The launcher takes PB from the address it is given -- 16, else 4, else 1 -- and never from an assumption.  A
// thread decodes (image row, tile column, pixel, channel) from its flat offset once and then walks PB bytes; the tile
// (its environment, the dimming, the source row) is looked up again only where the walk enters another tile.  k is a
// template argument, so the decode divides by constants.  Source bytes come through the cache (a frame is 21 KB and
// is read k^2 times).
#include "common.h"
#include "../../include/drqv2_hip.h"

namespace {

constexpr int kSide = 84;
constexpr int kPlane = kSide * kSide;             // 7,056 bytes = 441 x 16
constexpr int kFrame = 3 * kPlane;                // 21,168 bytes = 1,323 x 16
constexpr int kFramePieces = kFrame / 16;
constexpr int kStackPieces = 3 * kFramePieces;    // 3,969
constexpr int kThreads = 256;
constexpr int kStackGridY = 4;
constexpr long kMaxTiles = 1L << 20;              // keeps every row and column index of a mosaic inside an int

__global__ __launch_bounds__(kThreads) void vec_stack_push_kernel(const uint4* __restrict__ prev, uint4* __restrict__ next,
                                                                  const uint4* __restrict__ frame,
                                                                  const uint8_t* __restrict__ first, int reset_all) {
  const long e = blockIdx.x;
  const bool reset = reset_all || (first && first[e]);
  const uint4* fr = frame + e * kFramePieces;
  uint4* dst = next + e * kStackPieces;
  if (reset) {
    for (int v = blockIdx.y * kThreads + threadIdx.x; v < kStackPieces; v += kStackGridY * kThreads)
      dst[v] = fr[v % kFramePieces];
  } else {
    const uint4* pv = prev + e * kStackPieces + kFramePieces;       // prev is not null here: the launcher checked
    for (int v = blockIdx.y * kThreads + threadIdx.x; v < kStackPieces; v += kStackGridY * kThreads)
      dst[v] = v < 2 * kFramePieces ? pv[v] : fr[v - 2 * kFramePieces];
  }
}

struct VideoArgs {
  const uint8_t* frame;   // [N][3][84][84]
  const int* envs;        // [M]
  const int* done;        // [N] or null
  uint8_t* out;           // [GH S][GW S][3]
  long pieces;            // of PB bytes
  long N;
  int M, limit, GW;
};

// the tile that holds image row Y, tile column gx: the source row of its environment (null = a zero tile) and the shift
template <int K>
__device__ __forceinline__ const uint8_t* video_tile(const VideoArgs& a, int Y, int gx, int& shift) {
  constexpr int S = kSide * K;
  const int gy = Y / S, y = Y - gy * S;
  const long m = (long)gy * a.GW + gx;
  shift = 0;
  if (m >= a.M) return nullptr;
  const int e = a.envs[m];
  if (e < 0 || e >= a.N) return nullptr;          // the host checks the table once; nothing is ever read outside frame
  if (a.done && a.limit > 0 && a.done[e] >= a.limit) shift = 2;
  return a.frame + e * (long)kFrame + (y / K) * kSide;
}

template <int K, int PB>
__global__ __launch_bounds__(kThreads) void vec_video_record_kernel(VideoArgs a) {
  constexpr int S = kSide * K, kTileRow = 3 * S;                    // 252 K bytes of one tile in one image row
  const int row_bytes = a.GW * kTileRow;
  for (long v = blockIdx.x * (long)kThreads + threadIdx.x; v < a.pieces; v += (long)gridDim.x * kThreads) {
    const long o = v * PB;
    int Y = (int)(o / row_bytes);
    const int xb = (int)(o - (long)Y * row_bytes);
    int gx = xb / kTileRow;
    const int tb = xb - gx * kTileRow;
    int x = tb / 3, c = tb - 3 * x;
    int shift;
    const uint8_t* src = video_tile<K>(a, Y, gx, shift);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < PB; ++b) {
      const unsigned p = src ? (unsigned)src[c * kPlane + x / K] >> shift : 0u;
      w[b >> 2] |= p << (8 * (b & 3));
      if (++c == 3) {
        c = 0;
        if (++x == S) {
          x = 0;
          if (++gx == a.GW) {
            gx = 0;
            ++Y;                                  // past the last row only behind the last byte of the image: unused
          }
          if (b + 1 < PB) src = video_tile<K>(a, Y, gx, shift);
        }
      }
    }
    if constexpr (PB == 16) reinterpret_cast<uint4*>(a.out)[v] = make_uint4(w[0], w[1], w[2], w[3]);
    else if constexpr (PB == 4) reinterpret_cast<unsigned*>(a.out)[v] = w[0];
    else a.out[v] = (uint8_t)w[0];
  }
}

template <int K>
void launch_video(int PB, dim3 grid, hipStream_t st, const VideoArgs& a) {
  if (PB == 16) hipLaunchKernelGGL((vec_video_record_kernel<K, 16>), grid, dim3(kThreads), 0, st, a);
  else if (PB == 4) hipLaunchKernelGGL((vec_video_record_kernel<K, 4>), grid, dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL((vec_video_record_kernel<K, 1>), grid, dim3(kThreads), 0, st, a);
}

inline bool overlap(const void* a, const void* b, long bytes_a, long bytes_b) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes_b && y < x + (uintptr_t)bytes_a;
}

}  // namespace

DRQ_API int drq_vec_stack_push(const uint8_t* prev, uint8_t* next, const uint8_t* frame, const uint8_t* first, long N,
                               int reset_all, drq_stream_t stream) {
  if (!next || !frame || N < 1 || N > INT32_MAX) return DRQ_EARG;
  if (reset_all != 0 && reset_all != 1) return DRQ_EARG;
  if (!prev && !reset_all) return DRQ_EARG;
  if (((uintptr_t)prev | (uintptr_t)next | (uintptr_t)frame) & 15) return DRQ_EARG;
  const long stack_bytes = N * 3L * kFrame, frame_bytes = N * (long)kFrame;
  if (prev && overlap(prev, next, stack_bytes, stack_bytes)) return DRQ_EARG;
  if (overlap(frame, next, frame_bytes, stack_bytes)) return DRQ_EARG;
  hipLaunchKernelGGL(vec_stack_push_kernel, dim3((unsigned)N, kStackGridY), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint4*>(prev), reinterpret_cast<uint4*>(next),
                     reinterpret_cast<const uint4*>(frame), first, reset_all);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_video_record(const uint8_t* frame, const int* envs, int M, const int* done, int limit, uint8_t* out,
                                 int GH, int GW, int k, long N, drq_stream_t stream) {
  if (!frame || !envs || !out || N < 1 || N > INT32_MAX) return DRQ_EARG;
  if (k < 1 || k > 4 || GH < 1 || GW < 1 || limit < 0) return DRQ_EARG;
  const long tiles = (long)GH * GW;
  if (tiles > kMaxTiles || M < 1 || M > tiles) return DRQ_EARG;
  if (((uintptr_t)envs | (uintptr_t)done) & 3) return DRQ_EARG;
  const long bytes = tiles * kFrame * k * k;                        // a multiple of 16
  const int PB = ((uintptr_t)out & 15) == 0 ? 16 : ((uintptr_t)out & 3) == 0 ? 4 : 1;
  VideoArgs a{frame, envs, done, out, bytes / PB, N, M, limit, GW};
  const long blocks = (a.pieces + 4 * kThreads - 1) / (4 * kThreads);
  const dim3 grid((unsigned)(blocks < 65536 ? blocks : 65536));
  hipStream_t st = (hipStream_t)stream;
  switch (k) {
    case 1: launch_video<1>(PB, grid, st, a); break;
    case 2: launch_video<2>(PB, grid, st, a); break;
    case 3: launch_video<3>(PB, grid, st, a); break;
    default: launch_video<4>(PB, grid, st, a); break;
  }
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
