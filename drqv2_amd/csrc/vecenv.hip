// A built-in device environment for vectorised collection (contract: include/drqv2_hip.h, "device environment").  New
// functionality: the reference steps one dm_control environment on the host (dmc.py, train.py:160-190); the rings of
// "step-major replay" take device tensors of N lockstep environments and nothing in the tree produced them.  "Reach" is
// a point in a square that must reach a target; it emits exactly what VecFrameReplay.add(), add_render() and
// VecEpisodeStats.step() take -- the 3 x 84 x 84 frame, reward, discount and first of every environment -- and is
// deterministic to the bit (tests/vec_env_oracle.py restates it in numpy).  It is no benchmark task.
//
// A second task, "pointmass", shares the square, the reset draws, the reward and the frame, and gives the point a velocity
// that no single frame shows: the smallest task that needs the three-frame stack.  drq_vec_task_step steps either task
// with `repeat` sub-steps per launch; drq_vec_reach_step is the same kernel with task reach and repeat 1.
//
// The macro step, the render kernel, the frame walker and the checks of the step entries are the skeleton's
// (vecenv_task.h); this file holds the square's policy -- its four (point mass: six) state words, its draws, its two rules
// of motion, its reward and its two discs -- one instantiation for both tasks, told apart by the launch argument `task`.
// It is compiled with -ffp-contract=off (build.py): the contract is single float32 operations in the written order, and
// hipcc's default would fuse a * 0.1f + pos and (x + 1) * 41.5f + 0.5f into one rounding.
//
// drq_vec_reach_image writes the renderer-shaped uint8 [N][S][S][C] image of frames, S = 84 k: every pixel k x k times,
// channels last, a fourth channel 255.  N x ceil(pieces / 1,024) workgroups of 256 threads, 16-byte stores, the source
// bytes through the cache (a frame is 21 KB); k and C are template arguments, so the decode divides by constants.
#include "vecenv_task.h"

namespace {

constexpr int kTargetR2 = 25, kAgentR2 = 16;

__device__ __forceinline__ int pixel_centre(float x) { return (int)floorf((x + 1.0f) * 41.5f + 0.5f); }

struct Square {
  struct Args {
    float* pos;             // [N][2]
    float* target;          // [N][2]
    float* vel;             // [N][2]; the point mass only (null for reach: neither read nor written)
    int task;
  };
  struct State { float px, py, tx, ty, vx, vy; };
  struct Action { float x, y; };

  static __device__ __forceinline__ State load(const Args& a, long e) {
    State s{a.pos[2 * e], a.pos[2 * e + 1], a.target[2 * e], a.target[2 * e + 1], 0.0f, 0.0f};
    if (a.task == DRQ_TASK_POINTMASS) {
      s.vx = a.vel[2 * e];
      s.vy = a.vel[2 * e + 1];
    }
    return s;
  }

  static __device__ __forceinline__ void reset(const Args&, State& s, unsigned seed, unsigned e, unsigned episode) {
    s.px = reach_draw(seed, e, episode, 0u);
    s.py = reach_draw(seed, e, episode, 1u);
    s.tx = reach_draw(seed, e, episode, 2u);
    s.ty = reach_draw(seed, e, episode, 3u);
    s.vx = s.vy = 0.0f;
  }

  static __device__ __forceinline__ Action sanitise(const float* row) { return {sanitise1(row[0]), sanitise1(row[1])}; }

  // the point mass: the velocity decays, takes the action and moves the point; a wall stops it
  static __device__ __forceinline__ void coast(float& p, float& v, float a) {
    v = v * 0.9f;
    v = v + a * 0.02f;
    const float q = p + v;
    if (q < -1.0f) {
      p = -1.0f;
      v = 0.0f;
    } else if (q > 1.0f) {
      p = 1.0f;
      v = 0.0f;
    } else {
      p = q;
    }
  }

  // reach ends its episode at the target, with discount 0; the point mass only at the time limit
  static __device__ __forceinline__ Sub substep(const Args& a, State& s, const Action& act) {
    const bool mass = a.task == DRQ_TASK_POINTMASS;
    if (mass) {
      coast(s.px, s.vx, act.x);
      coast(s.py, s.vy, act.y);
    } else {
      s.px = clamp1(s.px + act.x * 0.1f);
      s.py = clamp1(s.py + act.y * 0.1f);
    }
    const float dx = s.px - s.tx, dy = s.py - s.ty;
    const float d2 = dx * dx + dy * dy;
    const float r = 1.0f - d2;
    const bool reached = !mass && d2 <= 0.01f;
    return {r > 0.0f ? r : 0.0f, reached ? 0.0f : 1.0f, reached};
  }

  static __device__ __forceinline__ void store(const Args& a, long e, const State& s) {
    a.pos[2 * e] = s.px;
    a.pos[2 * e + 1] = s.py;
    a.target[2 * e] = s.tx;
    a.target[2 * e + 1] = s.ty;
    if (a.task == DRQ_TASK_POINTMASS) {
      a.vel[2 * e] = s.vx;
      a.vel[2 * e + 1] = s.vy;
    }
  }

  // the pixel rule: background, target disc, agent disc, in integers
  static __device__ __forceinline__ void frame(const State& s, uint8_t* frame) {
    const int acx = pixel_centre(s.px), acy = pixel_centre(s.py), tcx = pixel_centre(s.tx), tcy = pixel_centre(s.ty);
    draw_frame(frame, [=](int c, int i, int j) {
      unsigned p = frame_background(i, j);
      const int tdx = j - tcx, tdy = i - tcy, adx = j - acx, ady = i - acy;
      if (tdx * tdx + tdy * tdy <= kTargetR2) p = c == 1 ? 255u : 64u;
      if (adx * adx + ady * ady <= kAgentR2) p = c == 0 ? 255u : 64u;
      return p;
    });
  }
};

// image[e][y][x][ch] = frame[e][ch][y / K][x / K], ch < 3; 255 for ch == 3.  A piece is 16 consecutive bytes of the image
// of one environment (84^2 K^2 C is a multiple of 16).
template <int K, int C>
__global__ __launch_bounds__(kThreads) void vec_reach_image_kernel(const uint8_t* __restrict__ frame, uint8_t* image) {
  constexpr int S = kSide * K;
  constexpr int kBytes = S * S * C, kImagePieces = kBytes / 16;
  static_assert(kBytes % 16 == 0, "an image is whole 16-byte pieces");
  const long e = blockIdx.x;
  const uint8_t* src = frame + e * (long)kFrame;
  uint4* dst = reinterpret_cast<uint4*>(image + e * (long)kBytes);
  for (int v = blockIdx.y * kThreads + threadIdx.x; v < kImagePieces; v += gridDim.y * kThreads) {
    const int o = 16 * v;
    int pix = o / C, ch = o - pix * C;
    int y = pix / S, x = pix - y * S;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const unsigned p = ch == 3 ? 255u : (unsigned)src[ch * kPlane + (y / K) * kSide + x / K];
      w[b >> 2] |= p << (8 * (b & 3));
      if (++ch == C) {
        ch = 0;
        if (++x == S) {
          x = 0;
          ++y;
        }
      }
    }
    dst[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

template <int K>
void launch_image(int C, dim3 grid, hipStream_t st, const uint8_t* frame, uint8_t* image) {
  if (C == 4) hipLaunchKernelGGL((vec_reach_image_kernel<K, 4>), grid, dim3(kThreads), 0, st, frame, image);
  else hipLaunchKernelGGL((vec_reach_image_kernel<K, 3>), grid, dim3(kThreads), 0, st, frame, image);
}

// the square's own checks: pos and target always, vel where the task has one
int square_ok(const Square::Args& a) {
  if (!a.pos || !a.target || (a.task == DRQ_TASK_POINTMASS && !a.vel)) return 0;
  return !(((uintptr_t)a.pos | (uintptr_t)a.target | (uintptr_t)a.vel) & 3);
}

}  // namespace

DRQ_API int drq_vec_reach_step(float* pos, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                               const float* action, unsigned seed, int episode_length, int reset_all, uint8_t* frame,
                               float* reward, float* discount, uint8_t* first, drq_stream_t stream) {
  const Square::Args a{pos, target, nullptr, DRQ_TASK_REACH};
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, nullptr, seed, A, episode_length, 1, reset_all};
  if (!square_ok(a) || !env_io_ok(io, N, 2, false)) return DRQ_EARG;
  return launch_env_step<Square>(a, io, N, stream);
}

DRQ_API int drq_vec_task_step(int task, float* pos, float* target, float* vel, int* t, unsigned* episode, uint8_t* over,
                              long N, int A, const float* action, unsigned seed, int episode_length, int repeat,
                              int reset_all, uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps,
                              drq_stream_t stream) {
  if (task != DRQ_TASK_REACH && task != DRQ_TASK_POINTMASS) return DRQ_EARG;
  const Square::Args a{pos, target, task == DRQ_TASK_POINTMASS ? vel : nullptr, task};
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, substeps, seed, A, episode_length, repeat, reset_all};
  if (!square_ok(a) || !env_io_ok(io, N, 2)) return DRQ_EARG;
  return launch_env_step<Square>(a, io, N, stream);
}

DRQ_API int drq_vec_reach_render(const float* pos, const float* target, long N, uint8_t* frame, drq_stream_t stream) {
  const Square::Args a{const_cast<float*>(pos), const_cast<float*>(target), nullptr, DRQ_TASK_REACH};      // only loaded
  if (!square_ok(a)) return DRQ_EARG;
  return launch_env_render<Square>(a, N, frame, stream);
}

DRQ_API int drq_vec_reach_image(const uint8_t* frame, uint8_t* image, long N, int S, int C, drq_stream_t stream) {
  if (!frame || !image || N < 1 || N > INT32_MAX) return DRQ_EARG;
  if (S < kSide || S > 4 * kSide || S % kSide || (C != 3 && C != 4)) return DRQ_EARG;
  if (((uintptr_t)frame | (uintptr_t)image) & 15) return DRQ_EARG;
  const int K = S / kSide;
  const int pieces = S * S * C / 16;
  const dim3 grid((unsigned)N, (unsigned)((pieces + 4 * kThreads - 1) / (4 * kThreads)));      // at most 28 in y
  hipStream_t st = (hipStream_t)stream;
  switch (K) {
    case 1: launch_image<1>(C, grid, st, frame, image); break;
    case 2: launch_image<2>(C, grid, st, frame, image); break;
    case 3: launch_image<3>(C, grid, st, frame, image); break;
    default: launch_image<4>(C, grid, st, frame, image); break;
  }
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
