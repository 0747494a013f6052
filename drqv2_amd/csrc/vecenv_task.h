// The skeleton of a device environment (contract: include/drqv2_hip.h, "device environment"): what a task does not decide.
// A task (vecenv.hip: the square of reach and the point mass; veccartpole.hip: the cartpole; vecreacher.hip: the reacher;
// vecmaze.hip: the maze; veccatch.hip: the catch; vecwalker.hip: the walker; vecfinger.hip: the finger) is a class of static
// device functions over Args (its state pointers and flags), State (one environment, in registers) and Action (what a sub-step
// reads of an action row):
//   State  load(const Args&, long e)
//   void   reset(const Args&, State&, unsigned seed, unsigned e, unsigned episode)      the draws of a new episode
//   Action sanitise(const float* row)                       NaN to 0, the clamp
//   Sub    substep(const Args&, State&, const Action&)      one simulator step; the time limit is the skeleton's
//   void   store(const Args&, long e, const State&)
//   void   frame(const State&, uint8_t* frame)              the pixel rule, through draw_frame below
// and gets the macro step, the render kernel, the frame walker and the argument checks of a step entry from here.
//
// Every file that instantiates the skeleton is compiled with -ffp-contract=off (build.py): the draw and the wrapper fold
// are single float32 operations in the written order, and a numpy oracle holds every task to them bit for bit.
#pragma once
#include "vecenv_common.h"
#include "../../include/drqv2_hip.h"

// draw k of episode `episode` of environment e: uniform on the 2^24 grid of [0, 1), then into [-0.9, 0.9]
__device__ __forceinline__ float reach_draw(unsigned seed, unsigned e, unsigned episode, unsigned k) {
  const unsigned h = drq_fmix32(seed ^ e * 0x9E3779B9u ^ episode * 0x85EBCA6Bu ^ k * 0xC2B2AE35u);
  const float u = (float)(h >> 8) * 5.9604644775390625e-8f;          // 2^-24: exact
  return (u * 2.0f - 1.0f) * 0.9f;
}

__device__ __forceinline__ float clamp1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// an action component as every task reads it
__device__ __forceinline__ float sanitise1(float v) { return v != v ? 0.0f : clamp1(v); }

// the background of every task's frame: a diagonal ramp, 32 .. 73
__device__ __forceinline__ unsigned frame_background(int i, int j) { return 32u + (unsigned)((i + j) >> 2); }

// The frame walker: the 21,168 bytes at `frame` by the 256 threads of a workgroup -- 1,323 pieces of 16 bytes, 5 or 6 per
// lane, consecutive lanes consecutive pieces.  A lane decodes (c, i, j) from its flat offset once (7,056 = 441 x 16: a
// piece never crosses a channel plane; 84 = 5 x 16 + 4: it may cross a row), then walks 16 pixels; pixel(c, i, j) is
// the byte of channel c, row i, column j.  c is fixed over a piece, so what a pixel rule derives from it alone is
// computed once per piece.
template <class Pixel>
__device__ __forceinline__ void draw_frame(uint8_t* frame, Pixel pixel) {
  uint4* dst = reinterpret_cast<uint4*>(frame);
  for (int v = threadIdx.x; v < kPieces; v += kThreads) {
    const int o = 16 * v;
    const int c = o / kPlane, rem = o - c * kPlane;
    int i = rem / kSide, j = rem - i * kSide;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      w[b >> 2] |= pixel(c, i, j) << (8 * (b & 3));
      if (++j == kSide) {
        j = 0;
        ++i;
      }
    }
    dst[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// what every step entry takes beside the task's own state
struct EnvIO {
  int* t;                 // [N], like every array here but action and frame
  unsigned* episode;
  uint8_t* over;
  const float* action;    // [N][A]; null only with reset_all
  uint8_t* frame;         // [N][3][84][84]
  float *reward, *discount;
  uint8_t* first;
  int* substeps;          // null only from drq_vec_reach_step, which has no such output
  unsigned seed;
  int A, episode_length, repeat, reset_all;
};

// The checks every step entry shares; a task's entry checks its own state pointers and flags.  min_A: the columns of
// an action row the task reads.
inline int env_io_ok(const EnvIO& io, long N, int min_A, bool has_substeps = true) {
  if (!io.t || !io.episode || !io.over || !io.frame || !io.reward || !io.discount || !io.first) return 0;
  if (has_substeps && !io.substeps) return 0;
  if (N < 1 || N > INT32_MAX || io.A < min_A || io.episode_length < 1) return 0;
  if (io.repeat < 1 || io.repeat > DRQ_TASK_MAX_REPEAT) return 0;
  if (io.reset_all != 0 && io.reset_all != 1) return 0;
  if (!io.action && !io.reset_all) return 0;
  if ((uintptr_t)io.frame & 15) return 0;
  if (((uintptr_t)io.t | (uintptr_t)io.episode | (uintptr_t)io.reward | (uintptr_t)io.discount | (uintptr_t)io.substeps |
       (uintptr_t)io.action) & 3)
    return 0;
  return 1;
}

// what a task's sub-step returns: its reward, its discount, and whether the task itself ended the episode
struct Sub {
  float r, d;
  bool ended;
};

// One macro step of every environment, one workgroup of 256 threads each: the reset row, or up to `repeat` sub-steps of
// the task folded by the wrapper rule (the ActionRepeatWrapper of dmc.py:40-50, inside the launch: lockstep environments
// cannot be wrapped from outside, since one that ends inside a repeat must stop there).
//   state     every thread loads the state words of its environment and computes the reset or the macro step itself, in
//             registers -- the same IEEE operations on the same operands in every lane, so all 256 agree
//   barrier   every lane has read the old state before thread 0 stores the new one and the scalars
//   frame     Task::frame of the new state
// Everything that decides a branch or the trip count is a launch argument or the workgroup's own state, so both are
// uniform across the 256 lanes.  No LDS, no atomics, nothing crosses workgroups.
template <class Task>
__global__ __launch_bounds__(kThreads) void vec_env_step_kernel(typename Task::Args a, EnvIO io) {
  const long e = blockIdx.x;
  typename Task::State s = Task::load(a, e);
  int t = io.t[e];
  unsigned episode = io.episode[e];
  unsigned over = io.over[e];
  float reward = 0.0f, discount = 1.0f;
  unsigned first;
  int n = 0;
  if (io.reset_all || over) {
    episode += 1u;
    t = 0;
    over = 0u;
    Task::reset(a, s, io.seed, (unsigned)e, episode);
    first = 1u;
  } else {
    const typename Task::Action act = Task::sanitise(io.action + e * io.A);
    do {
      const Sub sub = Task::substep(a, s, act);
      t += 1;
      if (sub.ended || t == io.episode_length) over = 1u;
      reward = reward + sub.r * discount;
      discount = discount * sub.d;
    } while (++n < io.repeat && !over);
    first = 0u;
  }
  __syncthreads();            // every lane holds the old state: thread 0 may now replace it
  if (threadIdx.x == 0) {
    Task::store(a, e, s);
    io.t[e] = t;
    io.episode[e] = episode;
    io.over[e] = (uint8_t)over;
    io.reward[e] = reward;
    io.discount[e] = discount;
    io.first[e] = (uint8_t)first;
    if (io.substeps) io.substeps[e] = n;
  }
  Task::frame(s, io.frame + e * (long)kFrame);
}

// the frames of the states as they are -- what a restored environment shows before its next step, since a checkpoint
// holds the state and not the frames derived from it: the frame part of the step kernel alone, same launch shape
template <class Task>
__global__ __launch_bounds__(kThreads) void vec_env_render_kernel(typename Task::Args a, uint8_t* frame) {
  const long e = blockIdx.x;
  Task::frame(Task::load(a, e), frame + e * (long)kFrame);
}

template <class Task>
int launch_env_step(const typename Task::Args& a, const EnvIO& io, long N, drq_stream_t stream) {
  hipLaunchKernelGGL(vec_env_step_kernel<Task>, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, a, io);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

// checks N and the frame; the task's entry has checked its own state pointers
template <class Task>
int launch_env_render(const typename Task::Args& a, long N, uint8_t* frame, drq_stream_t stream) {
  if (!frame || N < 1 || N > INT32_MAX || ((uintptr_t)frame & 15)) return DRQ_EARG;
  hipLaunchKernelGGL(vec_env_render_kernel<Task>, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, a, frame);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
