// The cartpole of the device environment (contract: include/drqv2_hip.h, "device environment", "Cartpole"): a cart on a
// rail carries a free pole; swing_up = 1 starts with the pole hanging (DMC's cartpole_swingup), 0 with it near upright
// (cartpole_balance).  The first task here whose action acts through second-order coupled dynamics with an unstable
// equilibrium.  New functionality: the reference steps one dm_control cartpole on the host (cfgs/task/easy.yaml).
//
// The pole's angle is held as the unit vector (c, s) = (cos, sin) of the angle from upright, rotated by omega dt and
// renormalised every step: the whole step is +, -, *, / and sqrt, each one correctly rounded float32 operation in the
// written order, so tests/vec_cartpole_oracle.py restates it in numpy to the bit.  This file is compiled with
// -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py): nothing is fused, and / and sqrt are IEEE.
//
// The macro step, the render kernel, the frame walker and the checks of the step entry are the skeleton's
// (vecenv_task.h); this file holds the cartpole's policy: its five state words, its two draws, its physics, its reward
// and its pixel rule -- per pixel the background, the rail, the cart and the pole's capsule, in integers (int64 where the
// capsule's cross product is squared).
#include "vecenv_task.h"

namespace {

constexpr float kDt = 0.01f, kForce = 10.0f, kGravity = 9.8f, kHalfLength = 0.5f;
constexpr float kPoleMassLength = 0.05f, kPoleMass = 0.1f, kTotalMass = 1.1f, kFourThirds = 1.3333334f;
constexpr float kRail = 1.8f, kMaxXdot = 16.0f, kMaxOmega = 32.0f;
constexpr int kCentre = 672;                       // 42 pixels in 1/16: the middle of the frame, the pivot's row
constexpr int kRailRow = 42, kRailHalf = 576;      // 1.8 x 320
constexpr int kCartHalfW = 96, kCartHalfH = 48, kPoleR2 = 24 * 24;

struct Pole {
  float x, xdot, c, s, omega;
};

__device__ __forceinline__ float clamp_to(float v, float m) { return v < -m ? -m : (v > m ? m : v); }

// a * a as an unevaluated sum p + err, exactly, from +, - and * alone: Veltkamp's split of a into two halves of 12 bits,
// whose products are exact, then Dekker's error term of the rounded square
__device__ __forceinline__ void exact_square(float a, float& p, float& err) {
  const float t = a * 4097.0f;
  const float hi = t - (t - a);
  const float lo = a - hi;
  p = a * a;
  const float q = hi * lo;
  err = ((hi * hi - p) + (q + q)) + lo * lo;
}

// (c, s) / |(c, s)|: two multiplies, an add, a square root and two divisions leave c^2 + s^2 within 3 ulp of 1; one
// correction by the defect d = 1 - c^2 - s^2, computed exactly up to its own last bits, leaves c and s the float32
// nearest to the unit vector's components (c (1 + d / 2) = c / sqrt(1 - d) up to d^2): c^2 + s^2 within 1 ulp of 1
__device__ __forceinline__ void normalise(float& c, float& s) {
  const float n = sqrtf(c * c + s * s);
  c = c / n;
  s = s / n;
  float pc, ec, ps, es;
  exact_square(c, pc, ec);
  exact_square(s, ps, es);
  float d = pc >= ps ? (1.0f - pc) - ps : (1.0f - ps) - pc;      // the larger square first: both subtractions are exact
  d = d - (ec + es);
  const float g = d * 0.5f;
  c = c + c * g;
  s = s + s * g;
}

// one simulator step under the sanitised action a
__device__ __forceinline__ void cartpole_substep(Pole& p, float a) {
  const float force = a * kForce;
  float t1 = p.omega * p.omega;
  t1 = kPoleMassLength * t1;
  t1 = t1 * p.s;
  const float temp = (force + t1) / kTotalMass;
  const float num = kGravity * p.s - p.c * temp;
  float q = p.c * p.c;
  q = kPoleMass * q;
  q = q / kTotalMass;
  float den = kFourThirds - q;
  den = kHalfLength * den;
  const float thacc = num / den;
  float r = kPoleMassLength * thacc;
  r = r * p.c;
  r = r / kTotalMass;
  const float xacc = temp - r;
  p.omega = clamp_to(p.omega + thacc * kDt, kMaxOmega);
  p.xdot = clamp_to(p.xdot + xacc * kDt, kMaxXdot);
  const float xq = p.x + p.xdot * kDt;
  if (xq < -kRail) {
    p.x = -kRail;
    p.xdot = 0.0f;
  } else if (xq > kRail) {
    p.x = kRail;
    p.xdot = 0.0f;
  } else {
    p.x = xq;
  }
  const float h = p.omega * kDt;
  const float c1 = p.c - p.s * h, s1 = p.s + p.c * h;
  p.c = c1;
  p.s = s1;
  normalise(p.c, p.s);
}

__device__ __forceinline__ float cartpole_reward(const Pole& p, float a) {
  const float upright = (p.c + 1.0f) * 0.5f;
  float centred = 1.0f / (1.0f + p.x * p.x);
  centred = (1.0f + centred) * 0.5f;
  const float control = (4.0f + (1.0f - a * a)) / 5.0f;
  const float w = p.omega / 5.0f;
  float slow = 1.0f / (1.0f + w * w);
  slow = (1.0f + slow) * 0.5f;
  return ((upright * centred) * control) * slow;
}

// The cartpole's policy.  swing_up is a launch argument, like everything else that decides a branch (vecenv_task.h).
struct Cartpole {
  struct Args {
    float* phys;            // [N][5]: x, xdot, c, s, omega
    int swing_up;
  };
  using State = Pole;
  using Action = float;

  static __device__ __forceinline__ State load(const Args& a, long e) {
    const float* ph = a.phys + 5 * e;
    return {ph[0], ph[1], ph[2], ph[3], ph[4]};
  }

  static __device__ __forceinline__ void reset(const Args& a, State& p, unsigned seed, unsigned e, unsigned episode) {
    p.x = reach_draw(seed, e, episode, 0u) * 0.1f;
    p.xdot = 0.0f;
    p.c = a.swing_up ? -1.0f : 1.0f;
    p.s = reach_draw(seed, e, episode, 1u) * 0.05f;
    normalise(p.c, p.s);
    p.omega = 0.0f;
  }

  static __device__ __forceinline__ Action sanitise(const float* row) { return sanitise1(row[0]); }

  // The task never ends an episode itself and every d is 1, so the wrapper rule's r * discount is r * 1 = r and its
  // discount * d is 1 * 1 = 1, both exact in float32 for every r: the macro step's reward is the plain sum of the r, and
  // the discount stays 1.
  static __device__ __forceinline__ Sub substep(const Args&, State& p, Action act) {
    cartpole_substep(p, act);
    return {cartpole_reward(p, act), 1.0f, false};
  }

  static __device__ __forceinline__ void store(const Args& a, long e, const State& p) {
    float* out = a.phys + 5 * e;
    out[0] = p.x;
    out[1] = p.xdot;
    out[2] = p.c;
    out[3] = p.s;
    out[4] = p.omega;
  }

  // The pixel rule: the frame of (x, c, s).  Coordinates are 1/16 pixel; pixel (i, j) has its centre at (16 j + 8,
  // 16 i + 8).  Shapes that leave the frame are clipped by the walker itself: it visits the frame's pixels only.
  static __device__ __forceinline__ void frame(const State& st, uint8_t* frame) {
    const float xs = st.x * 320.0f;
    const int X0 = (int)floorf(xs + 672.5f);
    const int X1 = (int)floorf((xs + st.s * 320.0f) + 672.5f);
    const int Y1 = (int)floorf(672.5f - st.c * 320.0f);
    const int dx = X1 - X0, dy = Y1 - kCentre;
    const int dd = dx * dx + dy * dy;
    const long edge = (long)kPoleR2 * dd;
    draw_frame(frame, [=](int ch, int i, int j) {
      unsigned p = frame_background(i, j);
      const int px = 16 * j + 8, py = 16 * i + 8;
      const int rx = px - kCentre, vx = px - X0, vy = py - kCentre;
      if (i == kRailRow && rx >= -kRailHalf && rx <= kRailHalf) p = ch == 2 ? 255u : 64u;
      if (vx >= -kCartHalfW && vx <= kCartHalfW && vy >= -kCartHalfH && vy <= kCartHalfH) p = ch == 1 ? 255u : 64u;
      const int dot = vx * dx + vy * dy;
      bool in;
      if (dot <= 0) {
        in = vx * vx + vy * vy <= kPoleR2;
      } else if (dot >= dd) {
        const int ux = px - X1, uy = py - Y1;
        in = ux * ux + uy * uy <= kPoleR2;
      } else {
        const long cross = (long)vx * dy - (long)vy * dx;
        in = cross * cross <= edge;
      }
      return in ? (ch == 0 ? 255u : 64u) : p;
    });
  }
};

}  // namespace

DRQ_API int drq_vec_cartpole_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                                  unsigned seed, int episode_length, int repeat, int reset_all, int swing_up,
                                  uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps,
                                  drq_stream_t stream) {
  if (!phys || ((uintptr_t)phys & 3) || (swing_up != 0 && swing_up != 1)) return DRQ_EARG;
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, substeps, seed, A, episode_length, repeat, reset_all};
  if (!env_io_ok(io, N, 1)) return DRQ_EARG;
  return launch_env_step<Cartpole>({phys, swing_up}, io, N, stream);
}

DRQ_API int drq_vec_cartpole_render(const float* phys, long N, uint8_t* frame, drq_stream_t stream) {
  if (!phys || ((uintptr_t)phys & 3)) return DRQ_EARG;
  return launch_env_render<Cartpole>({const_cast<float*>(phys), 0}, N, frame, stream);      // only loaded
}
