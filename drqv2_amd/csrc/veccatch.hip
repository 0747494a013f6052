// The catch of the device environment (contract: include/drqv2_hip.h, "device environment", "Catch"): a cup driven in the
// plane, a ball tied to it by a string that is either slack or taut, and the ball must be swung up and caught.  sparse = 1
// pays 1 while the ball's centre is inside the cup and 0 otherwise (in the image of the reference's cup_catch,
// cfgs/task/cup_catch.yaml: DMC's ball-in-cup, not a port of it); sparse = 0 pays a dense shaping of the distance to the
// cup's interior.  The first task here with a unilateral constraint, contacts between moving bodies and dynamics that
// switch regime inside an episode.  New functionality: the reference steps one dm_control ball_in_cup on the host.
//
// A step is +, -, *, / and sqrt, each one correctly rounded float32 operation in the written order, so
// tests/vec_catch_oracle.py restates it in numpy to the bit.  This file is compiled with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt (build.py): nothing is fused, and / and sqrt are IEEE.
//
// The macro step, the render kernel, the frame walker and the checks of the step entry are the skeleton's
// (vecenv_task.h); this file holds the catch's policy: its eight state words, its three draws, its physics -- the cup, the
// ball's free flight, the tether, the three capsules of the cup one after the other -- its reward and its pixel rule: per
// pixel the background, the tether's capsule (int64 where its cross product is squared), the cup's three axis-aligned
// capsules and the ball's disc, in integers.
#include "vecenv_task.h"

namespace {

constexpr float kDt = 0.01f, kGravityDt = 0.04f, kDrag = 0.9f, kGain = 0.3f;      // gravity 4, times dt
constexpr float kMaxCupV = 1.5f, kMaxBallV = 4.0f, kMaxBallV2 = 16.0f;
constexpr float kRange = 0.4f, kTether = 0.5f, kTether2 = 0.25f, kWall = 0.15f;
constexpr float kCapsuleR = 0.02f, kTouch = 0.07f, kTouch2 = 0.0049f;             // the ball's radius is 0.05: 0.07 is touching
constexpr float kMidY = 0.085f;                                                    // the interior's centre above cy
constexpr float kMinWidth = 0.16f, kMaxWidth = 0.4f;
constexpr int kCupR2 = 13 * 13, kBallR2 = 34 * 34, kTetherR2 = 10 * 10;

struct Cup {
  float cx, cy, vcx, vcy;      // the cup: the middle of its floor's segment, its velocity
  float bx, by, vbx, vby;      // the ball's centre, its velocity
  float hw;                    // half the launch's cup_width
};

// one axis of the cup: the point mass's momentum, a clamp on the speed, a stop at either end of the range
__device__ __forceinline__ void cup_axis(float& c, float& v, float a) {
  const float w = v * kDrag + a * kGain;
  v = w < -kMaxCupV ? -kMaxCupV : (w > kMaxCupV ? kMaxCupV : w);
  const float q = c + v * kDt;
  if (q < -kRange) {
    c = -kRange;
    v = 0.0f;
  } else if (q > kRange) {
    c = kRange;
    v = 0.0f;
  } else {
    c = q;
  }
}

// the ball against the capsule whose segment's closest point to it is (tx, ty): out along the normal to touching, the
// approaching part of the relative normal velocity removed (restitution 0); a centre on the segment is pushed upwards
__device__ __forceinline__ void contact(Cup& p, float tx, float ty) {
  const float ex = p.bx - tx, ey = p.by - ty;
  const float e2 = ex * ex + ey * ey;
  if (!(e2 < kTouch2)) return;
  float nx = 0.0f, ny = 1.0f;
  if (e2 != 0.0f) {
    const float e = sqrtf(e2);
    nx = ex / e;
    ny = ey / e;
  }
  p.bx = tx + nx * kTouch;
  p.by = ty + ny * kTouch;
  const float vn = (p.vbx - p.vcx) * nx + (p.vby - p.vcy) * ny;
  if (vn < 0.0f) {
    p.vbx = p.vbx - vn * nx;
    p.vby = p.vby - vn * ny;
  }
}

// one simulator step under the sanitised action
__device__ __forceinline__ void catch_substep(Cup& p, float a1, float a2) {
  cup_axis(p.cx, p.vcx, a1);
  cup_axis(p.cy, p.vcy, a2);
  // free flight: semi-implicit Euler, the speed clamped
  p.vby = p.vby - kGravityDt;
  const float s2 = p.vbx * p.vbx + p.vby * p.vby;
  if (s2 > kMaxBallV2) {
    const float k = kMaxBallV / sqrtf(s2);
    p.vbx = p.vbx * k;
    p.vby = p.vby * k;
  }
  p.bx = p.bx + p.vbx * kDt;
  p.by = p.by + p.vby * kDt;
  // the tether: beyond its length back onto the circle, the outward part of the relative velocity removed
  const float ay = p.cy + kCapsuleR;
  const float dx = p.bx - p.cx, dy = p.by - ay;
  const float d2 = dx * dx + dy * dy;
  if (d2 > kTether2) {
    const float d = sqrtf(d2);
    const float nx = dx / d, ny = dy / d;
    p.bx = p.cx + nx * kTether;
    p.by = ay + ny * kTether;
    const float vn = (p.vbx - p.vcx) * nx + (p.vby - p.vcy) * ny;
    if (vn > 0.0f) {
      p.vbx = p.vbx - vn * nx;
      p.vby = p.vby - vn * ny;
    }
  }
  // the contacts: left wall, right wall, floor, each with the ball as the one before left it
  const float xl = p.cx - p.hw, xr = p.cx + p.hw, top = p.cy + kWall;
  contact(p, xl, p.by < p.cy ? p.cy : (p.by > top ? top : p.by));
  contact(p, xr, p.by < p.cy ? p.cy : (p.by > top ? top : p.by));
  contact(p, p.bx < xl ? xl : (p.bx > xr ? xr : p.bx), p.cy);
}

__device__ __forceinline__ float catch_reward(const Cup& p, int sparse) {
  const float ux = p.bx - p.cx;
  if (sparse) {
    const float inner = p.hw - kCapsuleR;
    return (ux >= -inner && ux <= inner && p.by >= p.cy + kCapsuleR && p.by <= p.cy + kWall) ? 1.0f : 0.0f;
  }
  const float uy = p.by - (p.cy + kMidY);
  const float d2 = ux * ux + uy * uy;
  return 1.0f / (1.0f + 4.0f * d2);
}

struct Drive {
  float a1, a2;
};

// The catch's policy.  cup_width and sparse are launch arguments, like everything else that decides a branch
// (vecenv_task.h).
struct Catch {
  struct Args {
    float* phys;            // [N][8]: cx, cy, vcx, vcy, bx, by, vbx, vby
    float width;
    int sparse;
  };
  using State = Cup;
  using Action = Drive;

  static __device__ __forceinline__ State load(const Args& a, long e) {
    const float* ph = a.phys + 8 * e;
    return {ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], ph[7], a.width * 0.5f};
  }

  static __device__ __forceinline__ void reset(const Args&, State& p, unsigned seed, unsigned e, unsigned episode) {
    p.cx = reach_draw(seed, e, episode, 0u) * 0.4f;
    p.cy = reach_draw(seed, e, episode, 1u) * 0.4f;
    const float ay = p.cy + kCapsuleR;
    const float o = reach_draw(seed, e, episode, 2u) * 0.25f;      // the hanging ball a little off the vertical
    const float n = sqrtf(o * o + 1.0f);
    p.bx = p.cx + (o / n) * kTether;
    p.by = ay - (1.0f / n) * kTether;
    p.vcx = 0.0f;
    p.vcy = 0.0f;
    p.vbx = 0.0f;
    p.vby = 0.0f;
  }

  static __device__ __forceinline__ Action sanitise(const float* row) { return {sanitise1(row[0]), sanitise1(row[1])}; }

  // The task never ends an episode itself and every d is 1, so the macro step's reward is the plain sum of the r and the
  // discount stays 1 (veccartpole.hip); in the sparse form that sum is an exact small integer.
  static __device__ __forceinline__ Sub substep(const Args& a, State& p, const Action& act) {
    catch_substep(p, act.a1, act.a2);
    return {catch_reward(p, a.sparse), 1.0f, false};
  }

  static __device__ __forceinline__ void store(const Args& a, long e, const State& p) {
    float* ph = a.phys + 8 * e;
    ph[0] = p.cx;
    ph[1] = p.cy;
    ph[2] = p.vcx;
    ph[3] = p.vcy;
    ph[4] = p.bx;
    ph[5] = p.by;
    ph[6] = p.vbx;
    ph[7] = p.vby;
  }

  // The pixel rule: the frame of (cx, cy, bx, by, hw).  Coordinates are 1/16 pixel, 672 to the unit, y upwards: the frame is
  // the world; pixel (i, j) has its centre at (16 j + 8, 16 i + 8).  The cup (0.4 + 0.2 + 0.02 <= 1) and the ball
  // (0.4 + 0.02 + 0.5 + 0.05 <= 1) stay inside it.
  static __device__ __forceinline__ void frame(const State& st, uint8_t* frame) {
    const int LX = (int)floorf((st.cx - st.hw) * 672.0f + 672.5f), RX = (int)floorf((st.cx + st.hw) * 672.0f + 672.5f);
    const int CY = (int)floorf(672.5f - st.cy * 672.0f), TY = (int)floorf(672.5f - (st.cy + kWall) * 672.0f);
    const int AX = (int)floorf(st.cx * 672.0f + 672.5f), AY = (int)floorf(672.5f - (st.cy + kCapsuleR) * 672.0f);
    const int BX = (int)floorf(st.bx * 672.0f + 672.5f), BY = (int)floorf(672.5f - st.by * 672.0f);
    const int sx = BX - AX, sy = BY - AY;      // the tether, from the anchor
    const int ss = sx * sx + sy * sy;
    const long sedge = (long)kTetherR2 * ss;
    draw_frame(frame, [=](int ch, int i, int j) {
      unsigned p = frame_background(i, j);
      const int px = 16 * j + 8, py = 16 * i + 8;
      // the tether: the cartpole's capsule, radius 10
      const int vx = px - AX, vy = py - AY;
      const int dot = vx * sx + vy * sy;
      bool in;
      if (dot <= 0) {
        in = vx * vx + vy * vy <= kTetherR2;
      } else if (dot >= ss) {
        const int qx = px - BX, qy = py - BY;
        in = qx * qx + qy * qy <= kTetherR2;
      } else {
        const long cross = (long)vx * sy - (long)vy * sx;
        in = cross * cross <= sedge;
      }
      if (in) p = ch == 0 ? 64u : 255u;                                     // cyan
      // the cup: axis-aligned capsules of radius 13, the distance to the clamped point (TY <= CY: y points down here)
      const int wy = py - (py < TY ? TY : (py > CY ? CY : py));
      const int lx = px - LX, rx = px - RX;
      if (lx * lx + wy * wy <= kCupR2) p = ch == 2 ? 255u : 64u;            // the left wall: blue
      if (rx * rx + wy * wy <= kCupR2) p = ch == 1 ? 64u : 255u;            // the right wall: magenta
      const int fx = px - (px < LX ? LX : (px > RX ? RX : px)), fy = py - CY;
      if (fx * fx + fy * fy <= kCupR2) p = ch == 1 ? 255u : 64u;            // the floor: green
      const int qx = px - BX, qy = py - BY;
      if (qx * qx + qy * qy <= kBallR2) p = ch == 2 ? 64u : 255u;           // the ball: yellow
      return p;
    });
  }
};

// a NaN passes neither comparison
inline bool width_ok(float w) { return w >= kMinWidth && w <= kMaxWidth; }

}  // namespace

DRQ_API int drq_vec_catch_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                               unsigned seed, int episode_length, int repeat, int reset_all, float cup_width, int sparse,
                               uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps,
                               drq_stream_t stream) {
  if (!phys || ((uintptr_t)phys & 3)) return DRQ_EARG;
  if (!width_ok(cup_width) || (sparse != 0 && sparse != 1)) return DRQ_EARG;
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, substeps, seed, A, episode_length, repeat, reset_all};
  if (!env_io_ok(io, N, 2)) return DRQ_EARG;
  return launch_env_step<Catch>({phys, cup_width, sparse}, io, N, stream);
}

DRQ_API int drq_vec_catch_render(const float* phys, long N, float cup_width, uint8_t* frame, drq_stream_t stream) {
  if (!phys || ((uintptr_t)phys & 3) || !width_ok(cup_width)) return DRQ_EARG;
  return launch_env_render<Catch>({const_cast<float*>(phys), cup_width, 0}, N, frame, stream);      // only loaded
}
