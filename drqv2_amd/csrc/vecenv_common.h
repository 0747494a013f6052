// What the device environments share (vecenv.hip: reach and the point mass; veccartpole.hip: the cartpole): the geometry
// of a frame and of the launch that writes it, the reset draw and the clamp of an action.  The contract of every one is
// spelled out in include/drqv2_hip.h ("device environment").  Every file that includes this is compiled with
// -ffp-contract=off (build.py): the draw is single float32 operations in the written order.
#pragma once
#include "common.h"

static constexpr int kSide = 84;
static constexpr int kPlane = kSide * kSide;             // 7,056 bytes = 441 x 16
static constexpr int kFrame = 3 * kPlane;                // 21,168 bytes = 1,323 x 16
static constexpr int kPieces = kFrame / 16;
static constexpr int kThreads = 256;

// draw k of episode `episode` of environment e: uniform on the 2^24 grid of [0, 1), then into [-0.9, 0.9]
__device__ __forceinline__ float reach_draw(unsigned seed, unsigned e, unsigned episode, unsigned k) {
  const unsigned h = drq_fmix32(seed ^ e * 0x9E3779B9u ^ episode * 0x85EBCA6Bu ^ k * 0xC2B2AE35u);
  const float u = (float)(h >> 8) * 5.9604644775390625e-8f;          // 2^-24: exact
  return (u * 2.0f - 1.0f) * 0.9f;
}

__device__ __forceinline__ float clamp1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }
