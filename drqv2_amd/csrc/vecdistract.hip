// Distractions for the frames of N lockstep environments (contract: include/drqv2_hip.h, "distractions").  New
// functionality: the reference trains and evaluates on the clean frames of dm_control; the Distracting Control Suite and
// DMControl-GB ask whether a pixel agent still works when the image changes in ways that do not matter, and perturb
// exactly three things -- the background, the colours and the camera.  This does so where the frames already are: one
// launch per step, no download, no host wait.  Everything is integer arithmetic and exact (tests/vec_distract_oracle.py
// restates it in numpy).
//
// drq_vec_distract is one launch of N workgroups of 256 threads, one per environment:
//   state     every wave loads the two state words and the first flag of its environment through readfirstlane, so the
//             state step, the thirteen draws and every scalar derived from them (offsets, gains, velocities, clip and
//             frame) are wave-uniform: computed once, on the scalar unit, not per pixel
//   stage     441 pieces of 16 pixels, 1 or 2 per lane: three aligned 16-byte loads of the frame (and three of the key)
//             become 16 dwords r | g << 8 | b << 16 | background << 24 in LDS.  Pixel p sits at dword p + (p >> 4), so the
//             lanes of a wave, 16 pixels apart, are 17 dwords apart: every bank once.  In noise mode lanes 0 .. 80 hash
//             the 9 x 9 lattice points the window can touch, three channels packed into a dword each
//   barrier   __syncthreads(): the image and the lattice are whole; every wave holds the old state, so thread 0 may
//             replace it
//   draw      the same 441 pieces: per output pixel ONE LDS dword gives the three source bytes and the key test at the
//             camera's source pixel; the lattice corners are reread only when the pixel enters another cell (every 12
//             pixels); a bank frame comes in as three aligned 16-byte loads.  Three 16-byte stores, one per channel plane
// No atomics, nothing crosses workgroups; an environment's state is read and written by its own workgroup only.
#include "vecenv_common.h"      // the frame's geometry
#include "../../include/drqv2_hip.h"

namespace {

constexpr int kPlanePieces = kPlane / 16;                 // 441 pieces of 16 pixels
constexpr int kImageDwords = kPlane + kPlane / 16;        // pixel p at p + (p >> 4)
constexpr int kCell = 12, kLattice = 9;                   // 84 pixels from any phase touch at most 8 cells: 9 points

struct DistractArgs {
  const uint8_t* frame_in;    // [N][3][84][84]
  const uint8_t* first;       // [N] or null
  const uint8_t* key;         // [3][84][84] or null
  const uint8_t* bank;        // [M][F][3][84][84] or null
  unsigned* episode;          // [N]
  unsigned* t;                // [N]
  uint8_t* frame_out;         // [N][3][84][84]
  unsigned seed;
  int reset_all, hold, camera, camera_period, color, bg_mode, bg_alpha, dynamic, M, F;
};

__device__ __forceinline__ int tri(int v, int m) {
  if (m == 0) return 0;
  const int r = v % (2 * m);
  return r <= m ? r : 2 * m - r;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned byte_of(const uint4& q, int b) {
  const unsigned w = b < 4 ? q.x : (b < 8 ? q.y : (b < 12 ? q.z : q.w));
  return (w >> (8 * (b & 3))) & 255u;
}

__device__ __forceinline__ int floor_div(int a, int d) {
  const int q = a / d;
  return a % d < 0 ? q - 1 : q;
}

__global__ __launch_bounds__(kThreads) void vec_distract_kernel(DistractArgs a) {
  __shared__ unsigned s_image[kImageDwords];
  __shared__ unsigned s_lattice[kLattice * kLattice];
  const long e = blockIdx.x;
  const int tid = threadIdx.x;

  // ---- state and the episode's scalars: wave-uniform
  unsigned episode = __builtin_amdgcn_readfirstlane(a.episode[e]);
  unsigned t = __builtin_amdgcn_readfirstlane(a.t[e]);
  if (!a.hold) {
    const unsigned flag = a.first ? __builtin_amdgcn_readfirstlane((unsigned)a.first[e]) : 0u;
    if (a.reset_all || flag) {
      episode += 1u;
      t = 0u;
    } else {
      t += 1u;
    }
  }
  const int tau = a.dynamic ? (int)(t & 0xFFFFFu) : 0;
  const unsigned base = a.seed ^ (unsigned)e * 0x9E3779B9u ^ episode * 0x85EBCA6Bu;
  auto draw = [base](unsigned k) { return drq_fmix32(base ^ (256u + k) * 0xC2B2AE35u); };

  const int P = a.camera, C = a.color;
  const int travel = tau / a.camera_period;
  const int ox = tri((int)(draw(0) % (unsigned)(2 * P + 1)) + (int)(draw(2) % 3u) * travel, 2 * P) - P;
  const int oy = tri((int)(draw(1) % (unsigned)(2 * P + 1)) + (int)(draw(3) % 3u) * travel, 2 * P) - P;
  int gain[3], off[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gain[c] = 256 - C + (int)(draw(4u + c) % (unsigned)(2 * C + 1));
    off[c] = (int)(draw(7u + c) % (unsigned)(C + 1)) - (C >> 1);
  }
  const unsigned d10 = draw(10), d11 = draw(11);
  const int alpha = a.bg_alpha;
  // noise: the lattice cell and the phase of pixel (0, 0); pixel (i, j) is (fy0 + i, fx0 + j) further
  int gx0 = 0, gy0 = 0, fx0 = 0, fy0 = 0;
  const uint8_t* clip = nullptr;
  if (a.bg_mode == 1) {
    const int X0 = tau * ((int)(d11 % 5u) - 2), Y0 = tau * ((int)(draw(12) % 5u) - 2);
    gx0 = floor_div(X0, kCell);
    gy0 = floor_div(Y0, kCell);
    fx0 = X0 - kCell * gx0;
    fy0 = Y0 - kCell * gy0;
    if (tid < kLattice * kLattice) {
      const int ly = tid / kLattice, lx = tid - ly * kLattice;
      const unsigned h = d10 ^ (unsigned)(gy0 + ly) * 0x85EBCA6Bu ^ (unsigned)(gx0 + lx) * 0xC2B2AE35u;
      s_lattice[tid] = (drq_fmix32(h) >> 24) | (drq_fmix32(h ^ 0x9E3779B9u) >> 24) << 8 |
                       (drq_fmix32(h ^ 2u * 0x9E3779B9u) >> 24) << 16;
    }
  } else if (a.bg_mode == 2) {
    const long m = (long)(d10 % (unsigned)a.M);
    const long f = tri((int)(d11 % (unsigned)a.F) + tau, a.F - 1);
    clip = a.bank + (m * a.F + f) * (long)kFrame;
  }

  // ---- stage: the frame and the key test into LDS, a dword per pixel
  const uint8_t* src = a.frame_in + e * (long)kFrame;
  for (int v = tid; v < kPlanePieces; v += kThreads) {
    uint4 f[3], k[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      f[c] = *reinterpret_cast<const uint4*>(src + c * kPlane + 16 * v);
      if (a.key) k[c] = *reinterpret_cast<const uint4*>(a.key + c * kPlane + 16 * v);
    }
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const unsigned r = byte_of(f[0], b), g = byte_of(f[1], b), bl = byte_of(f[2], b);
      unsigned bg = 0u;
      if (a.key) bg = r == byte_of(k[0], b) && g == byte_of(k[1], b) && bl == byte_of(k[2], b);
      s_image[17 * v + b] = r | g << 8 | bl << 16 | bg << 24;
    }
  }
  __syncthreads();
  if (tid == 0 && !a.hold) {
    a.episode[e] = episode;
    a.t[e] = t;
  }

  // ---- draw
  uint8_t* dst = a.frame_out + e * (long)kFrame;
  for (int v = tid; v < kPlanePieces; v += kThreads) {
    const int p0 = 16 * v;
    int i = p0 / kSide, j = p0 - i * kSide;
    uint4 n4[3];
    if (clip) {
#pragma unroll
      for (int c = 0; c < 3; ++c) n4[c] = *reinterpret_cast<const uint4*>(clip + c * kPlane + p0);
    }
    unsigned w[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    int cell = -1;
    unsigned l00 = 0u, l01 = 0u, l10 = 0u, l11 = 0u;
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int si = clampi(i + oy, 0, kSide - 1), sj = clampi(j + ox, 0, kSide - 1);
      const int p = si * kSide + sj;
      const unsigned px = s_image[p + (p >> 4)];
      const bool background = (px >> 24) != 0u;
      int fx = 0, fy = 0;
      if (a.bg_mode == 1 && background) {
        const int ux = fx0 + j, uy = fy0 + i;               // 0 .. 94
        const int lx = ux / kCell, ly = uy / kCell;
        fx = ux - kCell * lx;
        fy = uy - kCell * ly;
        if (ly * kLattice + lx != cell) {
          cell = ly * kLattice + lx;
          l00 = s_lattice[cell];
          l01 = s_lattice[cell + 1];
          l10 = s_lattice[cell + kLattice];
          l11 = s_lattice[cell + kLattice + 1];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s = (int)((px >> (8 * c)) & 255u);
        int out;
        if (background) {
          int n = s;
          if (a.bg_mode == 1) {
            const int top = (int)((l00 >> (8 * c)) & 255u) * (kCell - fx) + (int)((l01 >> (8 * c)) & 255u) * fx;
            const int bot = (int)((l10 >> (8 * c)) & 255u) * (kCell - fx) + (int)((l11 >> (8 * c)) & 255u) * fx;
            n = (top * (kCell - fy) + bot * fy + 72) / 144;
          } else if (a.bg_mode == 2) {
            n = (int)byte_of(n4[c], b);
          }
          out = (alpha * n + (256 - alpha) * s + 128) >> 8;
        } else {
          out = clampi(((s * gain[c] + 128) >> 8) + off[c], 0, 255);
        }
        w[c][b >> 2] |= (unsigned)out << (8 * (b & 3));
      }
      if (++j == kSide) {
        j = 0;
        ++i;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<uint4*>(dst + c * kPlane + p0) = make_uint4(w[c][0], w[c][1], w[c][2], w[c][3]);
  }
}

}  // namespace

DRQ_API int drq_vec_distract(const uint8_t* frame_in, const uint8_t* first, const uint8_t* key, const uint8_t* bank,
                             unsigned* episode, unsigned* t, long N, unsigned seed, int reset_all, int hold, int camera,
                             int camera_period, int color, int bg_mode, int bg_alpha, int dynamic, int M, int F,
                             uint8_t* frame_out, drq_stream_t stream) {
  if (!frame_in || !frame_out || !episode || !t) return DRQ_EARG;
  if (N < 1 || N > INT32_MAX) return DRQ_EARG;
  if ((reset_all != 0 && reset_all != 1) || (hold != 0 && hold != 1) || (hold && reset_all)) return DRQ_EARG;
  if (dynamic != 0 && dynamic != 1) return DRQ_EARG;
  if (camera < 0 || camera > DRQ_DISTRACT_MAX_CAMERA || camera_period < 1) return DRQ_EARG;
  if (color < 0 || color > DRQ_DISTRACT_MAX_COLOR || bg_alpha < 0 || bg_alpha > 256) return DRQ_EARG;
  if (bg_mode < 0 || bg_mode > 2) return DRQ_EARG;
  if (bg_mode != 0 && !key) return DRQ_EARG;
  if (bg_mode == 2 && (!bank || M < 1 || M > DRQ_DISTRACT_MAX_BANK || F < 1 || F > DRQ_DISTRACT_MAX_BANK)) return DRQ_EARG;
  const uintptr_t in = (uintptr_t)frame_in, out = (uintptr_t)frame_out, bytes = (uintptr_t)N * kFrame;
  if (in < out + bytes && out < in + bytes) return DRQ_EARG;      // frame_out == frame_in, or any overlap
  if ((in | out | (uintptr_t)key | (uintptr_t)(bg_mode == 2 ? bank : nullptr)) & 15) return DRQ_EARG;
  if (((uintptr_t)episode | (uintptr_t)t) & 3) return DRQ_EARG;
  DistractArgs a{frame_in, first,  key,           bg_mode == 2 ? bank : nullptr,
                 episode,  t,      frame_out,     seed,
                 reset_all, hold,  camera,        camera_period,
                 color,    bg_mode, bg_alpha,     dynamic,
                 M,        F};
  hipLaunchKernelGGL(vec_distract_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
