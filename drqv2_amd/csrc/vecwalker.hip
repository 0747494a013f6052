// The walker of the device environment (contract: include/drqv2_hip.h, "device environment", "Walker"): a planar legged
// runner -- a torso with a two-link leg at either end -- that moves through an unbounded world by pushing on a ground with
// friction, paid for standing (speed = 0) or for its forward speed (in the image of the reference's walker_stand /
// walker_walk / walker_run and cheetah_run, cfgs/task/: DMC's planar runners, not a port of them).  The first task here
// with ground contact, four actuators and a camera that follows the body.  New functionality: the reference steps one
// dm_control walker on the host.
//
// The body is six unit point masses under position-based dynamics: five rigid rods, four muscles that are distances
// across the joints, the ground.  A step is +, -, *, / and sqrt, each one correctly rounded float32 operation in the
// written order, so tests/vec_walker_oracle.py restates it in numpy to the bit.  This file is compiled with
// -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py): nothing is fused, and / and sqrt are IEEE.
//
// The macro step, the render kernel, the frame walker and the checks of the step entry are the skeleton's
// (vecenv_task.h); this file holds the walker's policy: its 24 state words, its five draws, its physics -- the advance,
// eight Gauss-Seidel sweeps over muscles with their limits, rods and the ground, written out constraint by constraint so
// that every particle stays in a register, the velocities, the wrap of the periodic world -- its reward and its pixel
// rule: per pixel the background, the striped ground and five capsules, in integers.
#include "vecenv_task.h"

namespace {

constexpr float kDt = 0.01f, kInvDt = 100.0f, kGravityDt = 0.1f, kDrag = 0.9f;      // gravity 10, times dt
constexpr float kFriction = 0.1f;                       // what the ground leaves of a particle's horizontal velocity
constexpr int kSweeps = 8, kForceSweeps = 4;            // the muscles pull in the first four; all eight hold the limits
constexpr float kMaxV = 2.0f, kMaxV2 = 4.0f, kMaxSpeed = 2.0f;
constexpr float kTorso = 0.4f, kLimb = 0.25f, kHalfTorso = 0.2f;
constexpr float kHipMid = 0.46f, kHipHalf = 0.1f, kHipLo = 0.3f, kHipHi = 0.6f, kHipJitter = 0.025f;
constexpr float kKneeMid = 0.34f, kKneeHalf = 0.06f, kKneeLo = 0.25f, kKneeHi = 0.43f, kKneeJitter = 0.015f;
constexpr float kStiff = 0.5f, kForce = 0.004f;
constexpr float kWorld = 4.0f, kHalfWorld = 2.0f;       // 8 periods of the ground's two stripes
constexpr float kTilt = 0.05f;
constexpr int kCapsuleR2 = 18 * 18, kGroundY = 1008, kStripe = 168, kPeriod = 336;

// particles: 0 shoulder, 1 hip, 2 front knee, 3 front foot, 4 back knee, 5 back foot
struct Body {
  float x[6], y[6], vx[6], vy[6];
};

// one distance constraint between particles i and j: the correction c (positive: too far apart) split equally
struct Pair {
  float d, nx, ny;
};

__device__ __forceinline__ Pair normal(const Body& b, int i, int j) {
  const float dx = b.x[j] - b.x[i], dy = b.y[j] - b.y[i];
  const float d2 = dx * dx + dy * dy;
  if (d2 == 0.0f) return {0.0f, 0.0f, 1.0f};            // the fixed normal of a zero distance
  const float d = sqrtf(d2);
  return {d, dx / d, dy / d};
}

__device__ __forceinline__ void move(Body& b, int i, int j, const Pair& n, float c) {
  const float h = c * 0.5f;
  const float hx = n.nx * h, hy = n.ny * h;
  b.x[i] = b.x[i] + hx;
  b.y[i] = b.y[i] + hy;
  b.x[j] = b.x[j] - hx;
  b.y[j] = b.y[j] - hy;
}

__device__ __forceinline__ void rod(Body& b, int i, int j, float length) {
  const Pair n = normal(b, i, j);
  move(b, i, j, n, n.d - length);
}

// a muscle and the limits of its joint: half the error towards the target, at most the force limit, while the muscles
// pull; then whatever it takes to stay inside [lo, hi]
__device__ __forceinline__ void muscle(Body& b, int i, int j, float target, bool pull, float lo, float hi) {
  const Pair n = normal(b, i, j);
  float c = 0.0f;
  if (pull) {
    c = (n.d - target) * kStiff;
    c = c < -kForce ? -kForce : (c > kForce ? kForce : c);
  }
  const float q = n.d - c;
  if (q < lo) {
    c = n.d - lo;
  } else if (q > hi) {
    c = n.d - hi;
  }
  move(b, i, j, n, c);
}

struct Drive {
  float a[4];      // front hip, front knee, back hip, back knee
};

// one simulator step under the sanitised action
__device__ __forceinline__ void walker_substep(Body& b, const Drive& act) {
  float ox[6], oy[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    b.vx[i] = b.vx[i] * kDrag;
    b.vy[i] = b.vy[i] * kDrag - kGravityDt;
    ox[i] = b.x[i];
    oy[i] = b.y[i];
    b.x[i] = b.x[i] + b.vx[i] * kDt;
    b.y[i] = b.y[i] + b.vy[i] * kDt;
  }
  const float t0 = kHipMid + act.a[0] * kHipHalf, t1 = kKneeMid + act.a[1] * kKneeHalf;
  const float t2 = kHipMid + act.a[2] * kHipHalf, t3 = kKneeMid + act.a[3] * kKneeHalf;
#pragma unroll 1
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    const bool pull = sweep < kForceSweeps;
    muscle(b, 1, 2, t0, pull, kHipLo, kHipHi);
    muscle(b, 0, 3, t1, pull, kKneeLo, kKneeHi);
    muscle(b, 0, 4, t2, pull, kHipLo, kHipHi);
    muscle(b, 1, 5, t3, pull, kKneeLo, kKneeHi);
    rod(b, 0, 1, kTorso);
    rod(b, 0, 2, kLimb);
    rod(b, 2, 3, kLimb);
    rod(b, 1, 4, kLimb);
    rod(b, 4, 5, kLimb);
#pragma unroll
    for (int i = 0; i < 6; ++i)
      if (b.y[i] < 0.0f) b.y[i] = 0.0f;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    float vx = (b.x[i] - ox[i]) * kInvDt, vy = (b.y[i] - oy[i]) * kInvDt;
    if (b.y[i] == 0.0f) vx = vx * kFriction;
    const float s2 = vx * vx + vy * vy;
    if (s2 > kMaxV2) {
      const float k = kMaxV / sqrtf(s2);
      vx = vx * k;
      vy = vy * k;
    }
    b.vx[i] = vx;
    b.vy[i] = vy;
  }
  // the periodic world: the torso's middle stays in [-2, 2)
  const float mid = (b.x[0] + b.x[1]) * 0.5f;
  if (mid >= kHalfWorld) {
#pragma unroll
    for (int i = 0; i < 6; ++i) b.x[i] = b.x[i] - kWorld;
  } else if (mid < -kHalfWorld) {
#pragma unroll
    for (int i = 0; i < 6; ++i) b.x[i] = b.x[i] + kWorld;
  }
}

__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__device__ __forceinline__ float walker_reward(const Body& b, float speed) {
  const float height = (b.y[0] + b.y[1]) * 0.5f;
  const float upright = (b.x[0] - b.x[1]) * 2.5f;
  const float stand = clamp01((height - 0.1f) * 10.0f) * clamp01((upright - 0.5f) * 2.5f);
  if (speed == 0.0f) return stand;
  const float v = (b.vx[0] + b.vx[1]) * 0.5f;
  return stand * (1.0f + 5.0f * clamp01(v / speed)) / 6.0f;
}

// the knee of a leg that hangs from (bx, by): `dist` from the torso's other end, which lies along (dx, dy); (px, py) is
// the torso's normal, downwards
__device__ __forceinline__ void place_knee(float bx, float by, float dx, float dy, float px, float py, float dist, float& kx,
                                           float& ky) {
  const float al = (kLimb * kLimb - dist * dist + kTorso * kTorso) / 0.8f;
  const float h = sqrtf(kLimb * kLimb - al * al);
  kx = bx + al * dx + h * px;
  ky = by + al * dy + h * py;
}

// the foot: `dist` from (bx, by), behind the thigh's line
__device__ __forceinline__ void place_foot(float bx, float by, float kx, float ky, float dist, float& fx, float& fy) {
  const float wx = (kx - bx) / kLimb, wy = (ky - by) / kLimb;
  const float dd = dist * dist;
  const float al = dd / 0.5f;
  const float h = sqrtf(dd - al * al);
  fx = bx + al * wx + h * wy;
  fy = by + al * wy - h * wx;
}

struct Capsule {
  int ax, ay, bx, by, sx, sy, ss;
  long edge;
};

__device__ __forceinline__ Capsule capsule_of(int ax, int ay, int bx, int by) {
  const int sx = bx - ax, sy = by - ay;
  const int ss = sx * sx + sy * sy;
  return {ax, ay, bx, by, sx, sy, ss, (long)kCapsuleR2 * ss};
}

// the cartpole's capsule test
__device__ __forceinline__ bool inside(const Capsule& c, int px, int py) {
  const int vx = px - c.ax, vy = py - c.ay;
  const int dot = vx * c.sx + vy * c.sy;
  if (dot <= 0) return vx * vx + vy * vy <= kCapsuleR2;
  if (dot >= c.ss) {
    const int qx = px - c.bx, qy = py - c.by;
    return qx * qx + qy * qy <= kCapsuleR2;
  }
  const long cross = (long)vx * c.sy - (long)vy * c.sx;
  return cross * cross <= c.edge;
}

// The walker's policy.  speed is a launch argument, like everything else that decides a branch (vecenv_task.h).
struct Walker {
  struct Args {
    float* phys;            // [N][24]: x, y, vx, vy of each of the six particles
    float speed;
  };
  using State = Body;
  using Action = Drive;

  static __device__ __forceinline__ State load(const Args& a, long e) {
    const float* ph = a.phys + 24 * e;
    State b;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      b.x[i] = ph[4 * i];
      b.y[i] = ph[4 * i + 1];
      b.vx[i] = ph[4 * i + 2];
      b.vy[i] = ph[4 * i + 3];
    }
    return b;
  }

  // a standing pose around x = 0: the torso a little tilted, the four joint distances near the muscles' middles
  static __device__ __forceinline__ void reset(const Args&, State& b, unsigned seed, unsigned e, unsigned episode) {
    const float tilt = reach_draw(seed, e, episode, 0u) * kTilt;
    const float n = sqrtf(tilt * tilt + 1.0f);
    const float ux = 1.0f / n, uy = tilt / n;
    const float d0 = kHipMid + reach_draw(seed, e, episode, 1u) * kHipJitter;
    const float d1 = kKneeMid + reach_draw(seed, e, episode, 2u) * kKneeJitter;
    const float d2 = kHipMid + reach_draw(seed, e, episode, 3u) * kHipJitter;
    const float d3 = kKneeMid + reach_draw(seed, e, episode, 4u) * kKneeJitter;
    b.x[0] = ux * kHalfTorso;
    b.y[0] = uy * kHalfTorso;
    b.x[1] = -b.x[0];
    b.y[1] = -b.y[0];
    const float px = uy, py = -ux;
    place_knee(b.x[0], b.y[0], -ux, -uy, px, py, d0, b.x[2], b.y[2]);
    place_foot(b.x[0], b.y[0], b.x[2], b.y[2], d1, b.x[3], b.y[3]);
    place_knee(b.x[1], b.y[1], ux, uy, px, py, d2, b.x[4], b.y[4]);
    place_foot(b.x[1], b.y[1], b.x[4], b.y[4], d3, b.x[5], b.y[5]);
    float low = b.y[3] < b.y[5] ? b.y[3] : b.y[5];            // the lowest knee or foot on the ground
    low = b.y[2] < low ? b.y[2] : low;
    low = b.y[4] < low ? b.y[4] : low;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      b.y[i] = b.y[i] - low;
      b.vx[i] = 0.0f;
      b.vy[i] = 0.0f;
    }
  }

  static __device__ __forceinline__ Action sanitise(const float* row) {
    return {{sanitise1(row[0]), sanitise1(row[1]), sanitise1(row[2]), sanitise1(row[3])}};
  }

  // The task never ends an episode itself and every d is 1 (veccartpole.hip): a fallen body lies there until the limit.
  static __device__ __forceinline__ Sub substep(const Args& a, State& b, const Action& act) {
    walker_substep(b, act);
    return {walker_reward(b, a.speed), 1.0f, false};
  }

  static __device__ __forceinline__ void store(const Args& a, long e, const State& b) {
    float* ph = a.phys + 24 * e;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      ph[4 * i] = b.x[i];
      ph[4 * i + 1] = b.y[i];
      ph[4 * i + 2] = b.vx[i];
      ph[4 * i + 3] = b.vy[i];
    }
  }

  // The pixel rule: the frame of the twelve coordinates.  1/16 pixel, 672 to the unit, y upwards, the ground line y = 0 at
  // 1008; pixel (i, j) has its centre at (16 j + 8, 16 i + 8).  The camera's x is the torso's middle, as the integer
  // C = floor(mid * 672): a particle is at X = floor(x * 672 + 0.5) - C + 672, and the pixel at px shows the world's
  // px - 672 + C, which decides the stripe.  Draw order: ground, back thigh, back shin, torso, front thigh, front shin.
  static __device__ __forceinline__ void frame(const State& b, uint8_t* frame) {
    const int C = (int)floorf((b.x[0] + b.x[1]) * 0.5f * 672.0f);
    int X[6], Y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      X[i] = (int)floorf(b.x[i] * 672.0f + 0.5f) - C + 672;
      Y[i] = (int)floorf(1008.5f - b.y[i] * 672.0f);
    }
    const Capsule back_thigh = capsule_of(X[1], Y[1], X[4], Y[4]), back_shin = capsule_of(X[4], Y[4], X[5], Y[5]);
    const Capsule torso = capsule_of(X[0], Y[0], X[1], Y[1]);
    const Capsule front_thigh = capsule_of(X[0], Y[0], X[2], Y[2]), front_shin = capsule_of(X[2], Y[2], X[3], Y[3]);
    const int phase = ((C - 672) % kPeriod + kPeriod) % kPeriod;      // of the world's x at px = 0; in 0 .. 335
    draw_frame(frame, [=](int ch, int i, int j) {
      unsigned p = frame_background(i, j);
      const int px = 16 * j + 8, py = 16 * i + 8;
      if (py > kGroundY) {      // the ground: stripes of 0.25, green and blue, fixed to the world
        p = (px + phase) % kPeriod < kStripe ? (ch == 1 ? 255u : 64u) : (ch == 2 ? 255u : 64u);
      }
      if (inside(back_thigh, px, py) || inside(back_shin, px, py)) p = ch == 1 ? 64u : 255u;        // the back leg: magenta
      if (inside(torso, px, py)) p = ch == 0 ? 255u : 64u;                                          // the torso: red
      if (inside(front_thigh, px, py) || inside(front_shin, px, py)) p = ch == 0 ? 64u : 255u;      // the front leg: cyan
      return p;
    });
  }
};

// a NaN passes neither comparison
inline bool speed_ok(float s) { return s >= 0.0f && s <= kMaxSpeed; }

}  // namespace

DRQ_API int drq_vec_walker_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                                unsigned seed, int episode_length, int repeat, int reset_all, float speed, uint8_t* frame,
                                float* reward, float* discount, uint8_t* first, int* substeps, drq_stream_t stream) {
  if (!phys || ((uintptr_t)phys & 3)) return DRQ_EARG;
  if (!speed_ok(speed)) return DRQ_EARG;
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, substeps, seed, A, episode_length, repeat, reset_all};
  if (!env_io_ok(io, N, 4)) return DRQ_EARG;
  return launch_env_step<Walker>({phys, speed}, io, N, stream);
}

DRQ_API int drq_vec_walker_render(const float* phys, long N, uint8_t* frame, drq_stream_t stream) {
  if (!phys || ((uintptr_t)phys & 3)) return DRQ_EARG;
  return launch_env_render<Walker>({const_cast<float*>(phys), 0.0f}, N, frame, stream);      // only loaded
}
