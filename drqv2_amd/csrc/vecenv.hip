// A built-in device environment for vectorised collection (contract: include/drqv2_hip.h, "device environment").  New
// functionality: the reference steps one dm_control environment on the host (dmc.py, train.py:160-190); the rings of
// "step-major replay" take device tensors of N lockstep environments and nothing in the tree produced them.  "Reach" is
// a point in a square that must reach a target; it emits exactly what VecFrameReplay.add(), add_render() and
// VecEpisodeStats.step() take -- the 3 x 84 x 84 frame, reward, discount and first of every environment -- and is
// deterministic to the bit (tests/vec_env_oracle.py restates it in numpy).  It is no benchmark task.
//
// A second task, "pointmass", shares the square, the reset draws, the reward and the frame, and gives the point a velocity
// that no single frame shows: the smallest task that needs the three-frame stack.  drq_vec_task_step steps either task
// with `repeat` sub-steps per launch (the ActionRepeatWrapper of dmc.py:35-50, inside the launch: lockstep environments
// cannot be wrapped from outside, since one that ends inside a repeat must stop there); drq_vec_reach_step is the same
// kernel with task reach and repeat 1.
//
// Either step entry is one launch of N workgroups of 256 threads, one per environment:
//   state     every thread loads the seven (point mass: nine) state words of its environment and computes the reset or
//             the macro step itself, in registers -- the same IEEE operations on the same operands in every lane, so all
//             256 agree, on the trip count of the sub-step loop too
//   barrier   __syncthreads(): every lane has read the old state before thread 0 stores the new one and the three scalars
//   frame     1,323 pieces of 16 bytes, 5 or 6 per lane, consecutive lanes consecutive pieces.  A lane decodes (c, i, j)
//             from its flat offset once (7,056 = 441 x 16: a piece never crosses a channel plane; 84 = 5 x 16 + 4: it may
//             cross a row), then walks 16 pixels: background, target disc, agent disc, in integers
// No LDS, no atomics, nothing crosses workgroups; an environment's state is read and written by its own workgroup only.
// This file is compiled with -ffp-contract=off (build.py): the contract is single float32 operations in the written
// order, and hipcc's default would fuse a * 0.1f + pos and (x + 1) * 41.5f + 0.5f into one rounding.
//
// drq_vec_reach_render draws the frames of the states as they are and changes nothing else: the frame part above alone, N
// workgroups of 256 threads, the same device function (reach_frame) -- what a restored environment shows before its next
// step, since a checkpoint holds the state and not the frames derived from it.
//
// drq_vec_reach_image writes the renderer-shaped uint8 [N][S][S][C] image of frames, S = 84 k: every pixel k x k times,
// channels last, a fourth channel 255.  N x ceil(pieces / 1,024) workgroups of 256 threads, 16-byte stores, the source
// bytes through the cache (a frame is 21 KB); k and C are template arguments, so the decode divides by constants.
#include "vecenv_common.h"      // the frame's geometry, reach_draw, clamp1: shared with veccartpole.hip
#include "../../include/drqv2_hip.h"

namespace {

constexpr int kTargetR2 = 25, kAgentR2 = 16;

__device__ __forceinline__ int pixel_centre(float x) { return (int)floorf((x + 1.0f) * 41.5f + 0.5f); }

// The pixel rule: the frame of the state (px, py, tx, ty) into the 21,168 bytes at `frame`, by the 256 threads of a
// workgroup -- 1,323 pieces of 16 bytes, consecutive lanes consecutive pieces.  The step and the render kernel share it.
__device__ __forceinline__ void reach_frame(float px, float py, float tx, float ty, uint8_t* frame) {
  const int acx = pixel_centre(px), acy = pixel_centre(py), tcx = pixel_centre(tx), tcy = pixel_centre(ty);
  uint4* dst = reinterpret_cast<uint4*>(frame);
  for (int v = threadIdx.x; v < kPieces; v += kThreads) {
    const int o = 16 * v;
    const int c = o / kPlane, rem = o - c * kPlane;
    int i = rem / kSide, j = rem - i * kSide;
    const unsigned target_colour = c == 1 ? 255u : 64u, agent_colour = c == 0 ? 255u : 64u;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      unsigned p = 32u + (unsigned)((i + j) >> 2);
      const int tdx = j - tcx, tdy = i - tcy, adx = j - acx, ady = i - acy;
      if (tdx * tdx + tdy * tdy <= kTargetR2) p = target_colour;
      if (adx * adx + ady * ady <= kAgentR2) p = agent_colour;
      w[b >> 2] |= p << (8 * (b & 3));
      if (++j == kSide) {
        j = 0;
        ++i;
      }
    }
    dst[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

struct TaskArgs {
  float* pos;             // [N][2]
  float* target;          // [N][2]
  float* vel;             // [N][2]; the point mass only (null for reach)
  int* t;
  unsigned* episode;
  uint8_t* over;
  const float* action;    // [N][A]; null only with reset_all
  uint8_t* frame;         // [N][3][84][84]
  float* reward;
  float* discount;
  uint8_t* first;
  int* substeps;          // [N]; null from drq_vec_reach_step, which has no such output
  unsigned seed;
  int task, A, episode_length, repeat, reset_all;
};

// One macro step of every environment: the reset row, or up to `repeat` sub-steps of the task folded by the wrapper rule
// (dmc.py:40-50).  task, repeat and reset_all are launch arguments and the state is the workgroup's own, so every branch
// and the trip count of the loop are uniform across the 256 lanes.
__global__ __launch_bounds__(kThreads) void vec_task_step_kernel(TaskArgs a) {
  const long e = blockIdx.x;
  const bool mass = a.task == DRQ_TASK_POINTMASS;
  float px = a.pos[2 * e], py = a.pos[2 * e + 1], tx = a.target[2 * e], ty = a.target[2 * e + 1];
  float vx = 0.0f, vy = 0.0f;
  if (mass) {
    vx = a.vel[2 * e];
    vy = a.vel[2 * e + 1];
  }
  int t = a.t[e];
  unsigned episode = a.episode[e];
  unsigned over = a.over[e];
  float reward = 0.0f, discount = 1.0f;
  unsigned first;
  int n = 0;
  if (a.reset_all || over) {
    episode += 1u;
    t = 0;
    over = 0u;
    px = reach_draw(a.seed, (unsigned)e, episode, 0u);
    py = reach_draw(a.seed, (unsigned)e, episode, 1u);
    tx = reach_draw(a.seed, (unsigned)e, episode, 2u);
    ty = reach_draw(a.seed, (unsigned)e, episode, 3u);
    vx = vy = 0.0f;
    first = 1u;
  } else {
    float ax = a.action[e * a.A], ay = a.action[e * a.A + 1];
    ax = ax != ax ? 0.0f : clamp1(ax);
    ay = ay != ay ? 0.0f : clamp1(ay);
    do {
      float d = 1.0f;
      if (mass) {
        vx = vx * 0.9f;
        vy = vy * 0.9f;
        vx = vx + ax * 0.02f;
        vy = vy + ay * 0.02f;
        const float qx = px + vx, qy = py + vy;
        if (qx < -1.0f) {
          px = -1.0f;
          vx = 0.0f;
        } else if (qx > 1.0f) {
          px = 1.0f;
          vx = 0.0f;
        } else {
          px = qx;
        }
        if (qy < -1.0f) {
          py = -1.0f;
          vy = 0.0f;
        } else if (qy > 1.0f) {
          py = 1.0f;
          vy = 0.0f;
        } else {
          py = qy;
        }
      } else {
        px = clamp1(px + ax * 0.1f);
        py = clamp1(py + ay * 0.1f);
      }
      t += 1;
      const float dx = px - tx, dy = py - ty;
      const float d2 = dx * dx + dy * dy;
      float r = 1.0f - d2;
      r = r > 0.0f ? r : 0.0f;
      if (!mass && d2 <= 0.01f) {
        d = 0.0f;
        over = 1u;
      } else if (t == a.episode_length) {
        over = 1u;
      }
      reward = reward + r * discount;
      discount = discount * d;
    } while (++n < a.repeat && !over);
    first = 0u;
  }
  __syncthreads();            // every lane holds the old state: thread 0 may now replace it
  if (threadIdx.x == 0) {
    a.pos[2 * e] = px;
    a.pos[2 * e + 1] = py;
    a.target[2 * e] = tx;
    a.target[2 * e + 1] = ty;
    if (mass) {
      a.vel[2 * e] = vx;
      a.vel[2 * e + 1] = vy;
    }
    a.t[e] = t;
    a.episode[e] = episode;
    a.over[e] = (uint8_t)over;
    a.reward[e] = reward;
    a.discount[e] = discount;
    a.first[e] = (uint8_t)first;
    if (a.substeps) a.substeps[e] = n;
  }

  reach_frame(px, py, tx, ty, a.frame + e * (long)kFrame);
}

// the checks both step entries share; vel and substeps are checked by drq_vec_task_step itself
int step_args_ok(const TaskArgs& a, long N) {
  if (!a.pos || !a.target || !a.t || !a.episode || !a.over || !a.frame || !a.reward || !a.discount || !a.first) return 0;
  if (N < 1 || N > INT32_MAX || a.A < 2 || a.episode_length < 1) return 0;
  if (a.reset_all != 0 && a.reset_all != 1) return 0;
  if (!a.action && !a.reset_all) return 0;
  if ((uintptr_t)a.frame & 15) return 0;
  if (((uintptr_t)a.pos | (uintptr_t)a.target | (uintptr_t)a.t | (uintptr_t)a.episode | (uintptr_t)a.reward |
       (uintptr_t)a.discount | (uintptr_t)a.action) & 3)
    return 0;
  return 1;
}

// the frames of the states as they are: the frame part of the step kernel alone, same launch shape
__global__ __launch_bounds__(kThreads) void vec_reach_render_kernel(const float* __restrict__ pos,
                                                                    const float* __restrict__ target, uint8_t* frame) {
  const long e = blockIdx.x;
  reach_frame(pos[2 * e], pos[2 * e + 1], target[2 * e], target[2 * e + 1], frame + e * (long)kFrame);
}

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

}  // namespace

DRQ_API int drq_vec_reach_step(float* pos, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                               const float* action, unsigned seed, int episode_length, int reset_all, uint8_t* frame,
                               float* reward, float* discount, uint8_t* first, drq_stream_t stream) {
  TaskArgs a{pos,      target, nullptr, t,    episode,        over, action,         frame, reward,
             discount, first,  nullptr, seed, DRQ_TASK_REACH, A,    episode_length, 1,     reset_all};
  if (!step_args_ok(a, N)) return DRQ_EARG;
  hipLaunchKernelGGL(vec_task_step_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_task_step(int task, float* pos, float* target, float* vel, int* t, unsigned* episode, uint8_t* over,
                              long N, int A, const float* action, unsigned seed, int episode_length, int repeat,
                              int reset_all, uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps,
                              drq_stream_t stream) {
  if (task != DRQ_TASK_REACH && task != DRQ_TASK_POINTMASS) return DRQ_EARG;
  if (repeat < 1 || repeat > DRQ_TASK_MAX_REPEAT || !substeps) return DRQ_EARG;
  if (task == DRQ_TASK_POINTMASS && !vel) return DRQ_EARG;
  if (task == DRQ_TASK_REACH) vel = nullptr;          // reach has no velocity: the array is neither read nor written
  if (((uintptr_t)vel | (uintptr_t)substeps) & 3) return DRQ_EARG;
  TaskArgs a{pos,      target, vel,      t,    episode, over, action,         frame,  reward,
             discount, first,  substeps, seed, task,    A,    episode_length, repeat, reset_all};
  if (!step_args_ok(a, N)) return DRQ_EARG;
  hipLaunchKernelGGL(vec_task_step_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_reach_render(const float* pos, const float* target, long N, uint8_t* frame, drq_stream_t stream) {
  if (!pos || !target || !frame || N < 1 || N > INT32_MAX) return DRQ_EARG;
  if ((uintptr_t)frame & 15) return DRQ_EARG;
  if (((uintptr_t)pos | (uintptr_t)target) & 3) return DRQ_EARG;
  hipLaunchKernelGGL(vec_reach_render_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, pos, target, frame);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
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
