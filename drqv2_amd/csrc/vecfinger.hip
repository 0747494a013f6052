// The finger of the device environment (contract: include/drqv2_hip.h, "device environment", "Finger"): the reacher's arm
// of two links, torque-driven at both joints, above a rod that turns freely on a hinge.  The agent is paid for the motion
// of the rod, which it can only influence through contact: mode 0 (spin) pays while the rod turns anticlockwise at
// kSpinSpeed or faster, mode 1 (turn) while the rod's tip is inside a target disc on its circle -- in the image of the
// reference's finger_spin / finger_turn_easy / finger_turn_hard (cfgs/task), not a port of them.  The first task here of
// manipulation.  New functionality: the reference steps one dm_control finger on the host.
//
// Only the fingertip's disc collides, against the rod's capsule; the finger's two links pass over the rod, the hinge and
// each other.  A contact is two parts: an impulse along the normal, before the advance, that leaves the two bodies no more
// approaching speed than closes the gap between them in this step (restitution 0; shared by effective mass, the arm's from
// the 2x2 mass matrix the drive already inverts, the rod's (r x n)^2 / I: at the hinge end the rod has no lever and the
// finger alone is stopped, by the same formula); and a separation, after the advance, that turns the shoulder and the rod
// -- never the elbow, so the mass matrix and with it the kinetic energy stay as they are -- until the two touch again.
// kSkin = 0.011 is the most a sub-step may leave the fingertip's centre closer to the rod's axis than touching.
//
// Reset: the draws 0 .. 3 are the two joint directions, the rod's and the target's.  A fingertip closer than kClear2 to the
// rod's axis turns the rod to point away from it; one that close to the hinge itself puts the finger straight up.  The
// target's direction is the rod's turned by at least 45 degrees, so no episode starts rewarded.
//
// The whole step is +, -, *, / and sqrt, each one correctly rounded float32 operation in the written order, so
// tests/vec_finger_oracle.py restates it in numpy to the bit.  This file is compiled with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt (build.py): nothing is fused, and / and sqrt are IEEE.
//
// The macro step, the render kernel, the frame walker and the checks of the step entry are the skeleton's
// (vecenv_task.h); this file holds the finger's policy: its eleven state words, its four draws, its physics, its rewards
// and its pixel rule, in integers (int64 where a capsule's cross product is squared).
#include "vecenv_task.h"

namespace {

constexpr float kDt = 0.01f, kTorque = 2.0f, kDamping = 0.5f, kMaxW = 6.0f, kMaxWs = 10.0f, kKeep = 0.97f;
constexpr float kL1 = 0.4f, kL2 = 0.3f, kLs = 0.3f, kDrop = 0.4f;      // the links, the rod, the root above the hinge
constexpr float kTouch = 0.11f, kTouch2 = 0.0121f, kNear2 = 0.0441f, kClear2 = 0.0169f;
constexpr float kInvI = 20.0f, kInvA = 2.5f, kMinDen = 0.01f;          // 1 / the rod's inertia; the shoulder's weight in a separation
constexpr float kSpinSpeed = 2.0f;
constexpr float kMinRadius = 0.02f, kMaxRadius = 0.2f;
constexpr int kCentre = 672, kRootY = 538, kHingeY = 806;              // 1/16 pixel: the world's origin, y of root and hinge
constexpr int kLinkR2 = 20 * 20, kTipR2 = 40 * 40, kRodR2 = 34 * 34, kHingeR2 = 44 * 44;

struct Hand {
  float c1, s1, w1, c2, s2, w2;      // the finger: the reacher's six words
  float cs, ss, ws;                  // the rod's unit vector and angular velocity
  float gx, gy;                      // the unit vector of the target's angle
};

__device__ __forceinline__ float clamp_to(float v, float m) { return v < -m ? -m : (v > m ? m : v); }

// exact_square, normalise and direction are vecreacher.hip's, word for word, a third copy: veccartpole.hip must keep its
// own (its test reads the file for them), so the copies are unified only after a change to tests/test_cpu_vec_cartpole.py.
// a * a as an unevaluated sum p + err, exactly, from +, - and * alone: Veltkamp's split, Dekker's error term
__device__ __forceinline__ void exact_square(float a, float& p, float& err) {
  const float t = a * 4097.0f;
  const float hi = t - (t - a);
  const float lo = a - hi;
  p = a * a;
  const float q = hi * lo;
  err = ((hi * hi - p) + (q + q)) + lo * lo;
}

// (c, s) / |(c, s)|, then one correction by the exactly computed defect 1 - c^2 - s^2: c^2 + s^2 within 1 ulp of 1
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

// the unit vector of a draw v in [-0.9, 0.9]: u walks the diamond |x| + |y| = 1 once, the point on it is normalised
__device__ __forceinline__ void direction(float v, float& c, float& s) {
  const float u = clamp1(v * 1.1111112f);
  const float x = 1.0f - 2.0f * fabsf(u);
  float y = 1.0f - fabsf(x);
  if (u < 0.0f) y = -y;
  if (x * x + y * y < 0.25f) {
    c = 1.0f;
    s = 0.0f;
    return;
  }
  c = x;
  s = y;
  normalise(c, s);
}

// a unit vector turned by k; k == 0 keeps it to the bit
__device__ __forceinline__ void rotate(float& c, float& s, float k) {
  if (k == 0.0f) return;
  const float c1 = c - s * k, s1 = s + c * k;
  c = c1;
  s = s1;
  normalise(c, s);
}

// what a contact reads of the positions: the fingertip relative to the root (t) and to the hinge (q), the forearm (f), the
// closest point of the rod's axis (r), the squared distance to it, and, once normal() has run, the distance, the normal
// from the rod to the fingertip and the three levers
struct Touch {
  float fx, fy, tx, ty, qx, qy, rx, ry, e2, e, nx, ny, j1, j2, js;
};

__device__ __forceinline__ Touch closest(const Hand& p) {
  Touch g;
  const float c12 = p.c1 * p.c2 - p.s1 * p.s2;
  const float s12 = p.s1 * p.c2 + p.c1 * p.s2;
  g.fx = kL2 * c12;
  g.fy = kL2 * s12;
  g.tx = kL1 * p.c1 + g.fx;
  g.ty = kL1 * p.s1 + g.fy;
  g.qx = g.tx;
  g.qy = g.ty + kDrop;
  const float proj = g.qx * p.cs + g.qy * p.ss;
  const float u = proj < 0.0f ? 0.0f : (proj > kLs ? kLs : proj);
  g.rx = p.cs * u;
  g.ry = p.ss * u;
  const float dx = g.qx - g.rx, dy = g.qy - g.ry;
  g.e2 = dx * dx + dy * dy;
  g.e = 0.0f;
  g.nx = dx;      // normal() divides them
  g.ny = dy;
  return g;
}

// a centre exactly on the axis takes the fixed normal (0, 1), as the catch does
__device__ __forceinline__ void normal(Touch& g) {
  if (g.e2 != 0.0f) {
    g.e = sqrtf(g.e2);
    g.nx = g.nx / g.e;
    g.ny = g.ny / g.e;
  } else {
    g.nx = 0.0f;
    g.ny = 1.0f;
  }
  g.j1 = g.ny * g.tx - g.nx * g.ty;
  g.j2 = g.ny * g.fx - g.nx * g.fy;
  g.js = g.rx * g.ny - g.ry * g.nx;
}

// one simulator step under the sanitised torques: unit point masses at the elbow and the tip, no gravity
__device__ __forceinline__ void finger_substep(Hand& p, float a1, float a2) {
  // 1 the drive: the reacher's, with these links
  const float m11 = 0.41f + 0.24f * p.c2;
  const float m12 = 0.09f + 0.12f * p.c2;
  const float h = 0.12f * p.s2;
  const float cor = (2.0f * p.w1) * p.w2 + p.w2 * p.w2;
  const float tau1 = (a1 * kTorque - kDamping * p.w1) + h * cor;
  const float tau2 = (a2 * kTorque - kDamping * p.w2) - h * (p.w1 * p.w1);
  const float det = m11 * 0.09f - m12 * m12;                 // 0.0288 - 0.0144 c2^2 >= 0.0144
  const float al1 = (0.09f * tau1 - m12 * tau2) / det;
  const float al2 = (m11 * tau2 - m12 * tau1) / det;
  p.w1 = clamp_to(p.w1 + al1 * kDt, kMaxW);
  p.w2 = clamp_to(p.w2 + al2 * kDt, kMaxW);
  p.ws = p.ws * kKeep;
  // 2 the impulse, at the positions as they are: no more approach than closes the gap in this step
  Touch g = closest(p);
  if (g.e2 < kNear2) {
    normal(g);
    const float gap = g.e - kTouch;
    const float lim = -((gap < 0.0f ? 0.0f : gap) * 100.0f);
    const float vn = (g.j1 * p.w1 + g.j2 * p.w2) - g.js * p.ws;
    const float u1 = (0.09f * g.j1 - m12 * g.j2) / det;
    const float u2 = (m11 * g.j2 - m12 * g.j1) / det;
    const float den = (g.j1 * u1 + g.j2 * u2) + (g.js * g.js) * kInvI;
    if (vn < lim && den > 0.0f) {
      const float lam = (lim - vn) / den;
      p.w1 = p.w1 + u1 * lam;
      p.w2 = p.w2 + u2 * lam;
      p.ws = p.ws - (g.js * kInvI) * lam;
    }
  }
  // 3 the clamps
  p.w1 = clamp_to(p.w1, kMaxW);
  p.w2 = clamp_to(p.w2, kMaxW);
  p.ws = clamp_to(p.ws, kMaxWs);
  // 4 the advance
  rotate(p.c1, p.s1, p.w1 * kDt);
  rotate(p.c2, p.s2, p.w2 * kDt);
  rotate(p.cs, p.ss, p.ws * kDt);
  // 5 the separation, at the new positions: the shoulder and the rod turn until the two touch; without a lever, nothing
  g = closest(p);
  if (g.e2 < kTouch2) {
    normal(g);
    const float den = (g.j1 * g.j1) * kInvA + (g.js * g.js) * kInvI;
    if (den >= kMinDen) {
      const float mu = (kTouch - g.e) / den;
      rotate(p.c1, p.s1, (g.j1 * kInvA) * mu);
      rotate(p.cs, p.ss, -((g.js * kInvI) * mu));
    }
  }
}

__device__ __forceinline__ float finger_reward(const Hand& p, int mode, float radius, int sparse) {
  if (mode == 0) {
    if (sparse) return p.ws >= kSpinSpeed ? 1.0f : 0.0f;
    const float v = p.ws / kSpinSpeed;
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  }
  const float dx = kLs * p.cs - kLs * p.gx;
  const float dy = kLs * p.ss - kLs * p.gy;
  const float d2 = dx * dx + dy * dy;
  if (sparse) return d2 <= radius * radius ? 1.0f : 0.0f;
  return 1.0f / (1.0f + 4.0f * d2);
}

struct Torques {
  float a1, a2;
};

// The finger's policy.  mode, target_radius and sparse are launch arguments, like everything else that decides a branch
// (vecenv_task.h).
struct Finger {
  struct Args {
    float* phys;            // [N][9]: c1, s1, w1, c2, s2, w2, cs, ss, ws
    float* target;          // [N][2]: the unit vector of the target's angle, drawn in both modes
    int mode;
    float radius;
    int sparse;
  };
  struct State {
    Hand p;
    int mode;               // the launch's, beside the state they are drawn with
    float radius;
  };
  using Action = Torques;

  static __device__ __forceinline__ State load(const Args& a, long e) {
    const float* ph = a.phys + 9 * e;
    const float* tg = a.target + 2 * e;
    return {{ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6], ph[7], ph[8], tg[0], tg[1]}, a.mode, a.radius};
  }

  static __device__ __forceinline__ void reset(const Args&, State& st, unsigned seed, unsigned e, unsigned episode) {
    Hand& p = st.p;
    direction(reach_draw(seed, e, episode, 0u), p.c1, p.s1);
    direction(reach_draw(seed, e, episode, 1u), p.c2, p.s2);
    direction(reach_draw(seed, e, episode, 2u), p.cs, p.ss);
    p.w1 = 0.0f;
    p.w2 = 0.0f;
    p.ws = 0.0f;
    const Touch g = closest(p);
    if (g.e2 < kClear2) {
      if (g.qx * g.qx + g.qy * g.qy >= kClear2) {      // the rod points away from the fingertip
        p.cs = -g.qx;
        p.ss = -g.qy;
        normalise(p.cs, p.ss);
      } else {                                         // the finger straight up, far from everything
        p.c1 = 0.0f;
        p.s1 = 1.0f;
        p.c2 = 1.0f;
        p.s2 = 0.0f;
      }
    }
    float v = reach_draw(seed, e, episode, 3u);
    v = v < 0.0f ? v * 0.75f - 0.225f : v * 0.75f + 0.225f;      // at least 45 degrees from the rod
    float ax, ay;
    direction(v, ax, ay);
    p.gx = p.cs * ax - p.ss * ay;
    p.gy = p.ss * ax + p.cs * ay;
    normalise(p.gx, p.gy);
  }

  static __device__ __forceinline__ Action sanitise(const float* row) { return {sanitise1(row[0]), sanitise1(row[1])}; }

  // The task never ends an episode itself and every d is 1, so the macro step's reward is the plain sum of the r and the
  // discount stays 1 (veccartpole.hip); in the sparse forms that sum is an exact small integer.
  static __device__ __forceinline__ Sub substep(const Args& a, State& st, const Action& act) {
    finger_substep(st.p, act.a1, act.a2);
    return {finger_reward(st.p, a.mode, a.radius, a.sparse), 1.0f, false};
  }

  static __device__ __forceinline__ void store(const Args& a, long e, const State& st) {
    const Hand& p = st.p;
    float* ph = a.phys + 9 * e;
    float* tg = a.target + 2 * e;
    ph[0] = p.c1;
    ph[1] = p.s1;
    ph[2] = p.w1;
    ph[3] = p.c2;
    ph[4] = p.s2;
    ph[5] = p.w2;
    ph[6] = p.cs;
    ph[7] = p.ss;
    ph[8] = p.ws;
    tg[0] = p.gx;
    tg[1] = p.gy;
  }

  // The pixel rule: the frame of (c1, s1, c2, s2, cs, ss, target, mode, radius).  Coordinates are 1/16 pixel, 672 to the
  // unit, y upwards: the frame is the world; pixel (i, j) has its centre at (16 j + 8, 16 i + 8).  The finger
  // (0.2 + 0.7 + 0.06 <= 1), the rod (0.2 + 0.3 + 0.05 <= 1) and the target's disc (0.2 + 0.3 + 0.2 <= 1) stay inside it.
  static __device__ __forceinline__ void frame(const State& st, uint8_t* frame) {
    const Hand& p = st.p;
    const float c12 = p.c1 * p.c2 - p.s1 * p.s2;
    const float s12 = p.s1 * p.c2 + p.c1 * p.s2;
    const float ax = p.c1 * 268.8f, ay = p.s1 * 268.8f;
    const int EX = (int)floorf(ax + 672.5f), EY = (int)floorf(672.5f - (ay + 134.4f));
    const int TX = (int)floorf((ax + c12 * 201.6f) + 672.5f), TY = (int)floorf(672.5f - ((ay + s12 * 201.6f) + 134.4f));
    const int SX = (int)floorf(p.cs * 201.6f + 672.5f), SY = (int)floorf(672.5f - (p.ss * 201.6f - 134.4f));
    const int GX = (int)floorf(p.gx * 201.6f + 672.5f), GY = (int)floorf(672.5f - (p.gy * 201.6f - 134.4f));
    const int GR = (int)floorf(st.radius * 672.0f + 0.5f);
    const int GR2 = st.mode == 1 ? GR * GR : -1;                  // spin draws no target
    const int rx = SX - kCentre, ry = SY - kHingeY;               // the rod, the upper link, the forearm
    const int ux = EX - kCentre, uy = EY - kRootY, fx = TX - EX, fy = TY - EY;
    const int rr = rx * rx + ry * ry, uu = ux * ux + uy * uy, ff = fx * fx + fy * fy;
    // inside the capsule of squared radius r2 around the segment from P - v along d (dd = d.d)
    auto capsule = [](int vx, int vy, int dx, int dy, int dd, int r2) {
      const int dot = vx * dx + vy * dy;
      if (dot <= 0) return vx * vx + vy * vy <= r2;
      if (dot >= dd) {
        const int qx = vx - dx, qy = vy - dy;
        return qx * qx + qy * qy <= r2;
      }
      const long cross = (long)vx * dy - (long)vy * dx;
      return cross * cross <= (long)r2 * dd;
    };
    draw_frame(frame, [=](int ch, int i, int j) {
      unsigned px_ = frame_background(i, j);
      const int px = 16 * j + 8, py = 16 * i + 8;
      const int gx = px - GX, gy = py - GY;
      if (gx * gx + gy * gy <= GR2) px_ = ch == 1 ? 255u : 64u;                                   // the target: green
      const int hx = px - kCentre, hy = py - kHingeY;
      if (hx * hx + hy * hy <= kHingeR2) px_ = ch == 2 ? 255u : 64u;                              // the hinge: blue
      if (capsule(hx, hy, rx, ry, rr, kRodR2)) px_ = ch == 1 ? 64u : 255u;                        // the rod: magenta
      const int sx = px - SX, sy = py - SY;
      if (sx * sx + sy * sy <= kRodR2) px_ = ch == 2 ? 255u : 64u;                                // the rod's tip: blue
      if (capsule(px - kCentre, py - kRootY, ux, uy, uu, kLinkR2)) px_ = ch == 0 ? 255u : 64u;    // the upper link: red
      if (capsule(px - EX, py - EY, fx, fy, ff, kLinkR2)) px_ = ch == 0 ? 64u : 255u;             // the forearm: cyan
      const int qx = px - TX, qy = py - TY;
      if (qx * qx + qy * qy <= kTipR2) px_ = ch == 2 ? 64u : 255u;                                // the fingertip: yellow
      return px_;
    });
  }
};

// a NaN passes neither comparison
inline bool finger_ok(const float* phys, const float* target, int mode, float radius) {
  if (!phys || !target || (((uintptr_t)phys | (uintptr_t)target) & 3)) return false;
  return (mode == 0 || mode == 1) && radius >= kMinRadius && radius <= kMaxRadius;
}

}  // namespace

DRQ_API int drq_vec_finger_step(float* phys, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                                const float* action, unsigned seed, int episode_length, int repeat, int reset_all, int mode,
                                float target_radius, int sparse, uint8_t* frame, float* reward, float* discount,
                                uint8_t* first, int* substeps, drq_stream_t stream) {
  if (!finger_ok(phys, target, mode, target_radius) || (sparse != 0 && sparse != 1)) return DRQ_EARG;
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, substeps, seed, A, episode_length, repeat, reset_all};
  if (!env_io_ok(io, N, 2)) return DRQ_EARG;
  return launch_env_step<Finger>({phys, target, mode, target_radius, sparse}, io, N, stream);
}

DRQ_API int drq_vec_finger_render(const float* phys, const float* target, long N, int mode, float target_radius,
                                  uint8_t* frame, drq_stream_t stream) {
  if (!finger_ok(phys, target, mode, target_radius)) return DRQ_EARG;
  return launch_env_render<Finger>({const_cast<float*>(phys), const_cast<float*>(target), mode, target_radius, 0}, N, frame,
                                   stream);      // only loaded
}
