// The reacher of the device environment (contract: include/drqv2_hip.h, "device environment", "Reacher"): a planar arm of
// two links seen from above, torque-driven at the shoulder and the elbow, whose fingertip must be brought into a target
// disc.  sparse = 1 pays 1 while the fingertip is inside the disc and 0 otherwise (in the image of the reference's
// reacher_easy / reacher_hard, cfgs/task: target_radius about 0.15 / 0.05); sparse = 0 pays a dense shaping of the
// same distance.  The first task here with a sparse reward and the first body with two coupled joints.  New
// functionality: the reference steps one dm_control reacher on the host.
//
// Both joint angles are held as unit vectors (c, s), rotated by w dt and renormalised every step, as the cartpole's pole
// is: the whole step is +, -, *, / and sqrt, each one correctly rounded float32 operation in the written order, so
// tests/vec_reacher_oracle.py restates it in numpy to the bit.  This file is compiled with -ffp-contract=off
// -fhip-fp32-correctly-rounded-divide-sqrt (build.py): nothing is fused, and / and sqrt are IEEE.
//
// The macro step, the render kernel, the frame walker and the checks of the step entry are the skeleton's
// (vecenv_task.h); this file holds the reacher's policy: its eight state words, its four draws, its physics, its reward
// and its pixel rule -- per pixel the background, the target's disc, the two capsules of the arm and the fingertip's
// disc, in integers (int64 where a capsule's cross product is squared).
#include "vecenv_task.h"

namespace {

constexpr float kDt = 0.01f, kTorque = 2.0f, kDamping = 0.5f, kMaxW = 16.0f;
constexpr float kMinRadius = 0.02f, kMaxRadius = 0.3f;
constexpr int kCentre = 672;                       // 42 pixels in 1/16: the middle of the frame, the shoulder
constexpr int kArmR2 = 24 * 24, kTipR2 = 32 * 32;

struct Arm {
  float c1, s1, w1, c2, s2, w2;      // the shoulder's unit vector and angular velocity, the elbow's (relative to the upper arm)
  float tx, ty;                      // the target's centre
  float radius;                      // the launch's target_radius, beside the state it is drawn with
};

__device__ __forceinline__ float clamp_to(float v, float m) { return v < -m ? -m : (v > m ? m : v); }

// exact_square and normalise are veccartpole.hip's, word for word: that file must keep its own (its test reads the file
// for them), so the two copies are unified only after a change to tests/test_cpu_vec_cartpole.py.
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

// the unit vector of a draw v in [-0.9, 0.9]: u walks the diamond |x| + |y| = 1 once, the point on it is normalised.
// On the diamond x^2 + y^2 >= 0.5; the threshold keeps the division safe for whatever pair is handed in.
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

// a joint's unit vector turned by w dt; a joint at rest keeps its vector to the bit
__device__ __forceinline__ void rotate(float& c, float& s, float w) {
  const float k = w * kDt;
  if (k == 0.0f) return;
  const float c1 = c - s * k, s1 = s + c * k;
  c = c1;
  s = s1;
  normalise(c, s);
}

// one simulator step under the sanitised torques: two point masses of 1 at the ends of two links of 0.5, no gravity
__device__ __forceinline__ void reacher_substep(Arm& p, float a1, float a2) {
  const float m11 = 0.75f + 0.5f * p.c2;
  const float m12 = 0.25f + 0.25f * p.c2;
  const float h = 0.25f * p.s2;
  const float cor = (2.0f * p.w1) * p.w2 + p.w2 * p.w2;
  const float tau1 = (a1 * kTorque - kDamping * p.w1) + h * cor;
  const float tau2 = (a2 * kTorque - kDamping * p.w2) - h * (p.w1 * p.w1);
  const float det = m11 * 0.25f - m12 * m12;                 // 0.125 - 0.0625 c2^2 >= 0.0625
  const float al1 = (0.25f * tau1 - m12 * tau2) / det;
  const float al2 = (m11 * tau2 - m12 * tau1) / det;
  p.w1 = clamp_to(p.w1 + al1 * kDt, kMaxW);
  p.w2 = clamp_to(p.w2 + al2 * kDt, kMaxW);
  rotate(p.c1, p.s1, p.w1);
  rotate(p.c2, p.s2, p.w2);
}

__device__ __forceinline__ float reacher_reward(const Arm& p, int sparse) {
  const float c12 = p.c1 * p.c2 - p.s1 * p.s2;
  const float s12 = p.s1 * p.c2 + p.c1 * p.s2;
  const float dx = (0.5f * p.c1 + 0.5f * c12) - p.tx;
  const float dy = (0.5f * p.s1 + 0.5f * s12) - p.ty;
  const float d2 = dx * dx + dy * dy;
  if (sparse) return d2 <= p.radius * p.radius ? 1.0f : 0.0f;
  return 1.0f / (1.0f + 4.0f * d2);
}

struct Torques {
  float a1, a2;
};

// The reacher's policy.  target_radius and sparse are launch arguments, like everything else that decides a branch
// (vecenv_task.h).
struct Reacher {
  struct Args {
    float* phys;            // [N][6]: c1, s1, w1, c2, s2, w2
    float* target;          // [N][2]
    float radius;
    int sparse;
  };
  using State = Arm;
  using Action = Torques;

  static __device__ __forceinline__ State load(const Args& a, long e) {
    const float* ph = a.phys + 6 * e;
    const float* tg = a.target + 2 * e;
    return {ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], tg[0], tg[1], a.radius};
  }

  static __device__ __forceinline__ void reset(const Args& a, State& p, unsigned seed, unsigned e, unsigned episode) {
    direction(reach_draw(seed, e, episode, 0u), p.c1, p.s1);
    direction(reach_draw(seed, e, episode, 1u), p.c2, p.s2);
    p.w1 = 0.0f;
    p.w2 = 0.0f;
    float gx, gy;
    direction(reach_draw(seed, e, episode, 2u), gx, gy);
    const float f = 0.5f + reach_draw(seed, e, episode, 3u) * 0.5f;      // 0.05 .. 0.95
    const float rho = (1.0f - a.radius) * f;                              // the whole disc within reach: rho + radius < 1
    p.tx = rho * gx;
    p.ty = rho * gy;
  }

  static __device__ __forceinline__ Action sanitise(const float* row) { return {sanitise1(row[0]), sanitise1(row[1])}; }

  // The task never ends an episode itself and every d is 1, so the macro step's reward is the plain sum of the r and the
  // discount stays 1 (veccartpole.hip); in the sparse form that sum is an exact small integer.
  static __device__ __forceinline__ Sub substep(const Args& a, State& p, const Action& act) {
    reacher_substep(p, act.a1, act.a2);
    return {reacher_reward(p, a.sparse), 1.0f, false};
  }

  static __device__ __forceinline__ void store(const Args& a, long e, const State& p) {
    float* ph = a.phys + 6 * e;
    float* tg = a.target + 2 * e;
    ph[0] = p.c1;
    ph[1] = p.s1;
    ph[2] = p.w1;
    ph[3] = p.c2;
    ph[4] = p.s2;
    ph[5] = p.w2;
    tg[0] = p.tx;
    tg[1] = p.ty;
  }

  // The pixel rule: the frame of (c1, s1, c2, s2, target, radius).  Coordinates are 1/16 pixel, 576 to the unit, y
  // upwards; pixel (i, j) has its centre at (16 j + 8, 16 i + 8).  The arm's reach (576) and its fingertip's radius stay
  // inside the frame (672 - 576 - 32 >= 0), and so does the target's disc (|target| + radius < 1).
  static __device__ __forceinline__ void frame(const State& st, uint8_t* frame) {
    const float c12 = st.c1 * st.c2 - st.s1 * st.s2;
    const float s12 = st.s1 * st.c2 + st.c1 * st.s2;
    const float ax = st.c1 * 288.0f, ay = st.s1 * 288.0f;
    const int EX = (int)floorf(ax + 672.5f), EY = (int)floorf(672.5f - ay);
    const int TX = (int)floorf((ax + c12 * 288.0f) + 672.5f), TY = (int)floorf(672.5f - (ay + s12 * 288.0f));
    const int GX = (int)floorf(st.tx * 576.0f + 672.5f), GY = (int)floorf(672.5f - st.ty * 576.0f);
    const int GR = (int)floorf(st.radius * 576.0f + 0.5f);
    const int GR2 = GR * GR;
    const int ux = EX - kCentre, uy = EY - kCentre, fx = TX - EX, fy = TY - EY;      // the upper arm, the forearm
    const int uu = ux * ux + uy * uy, ff = fx * fx + fy * fy;
    const long uedge = (long)kArmR2 * uu, fedge = (long)kArmR2 * ff;
    // inside the capsule of radius 24 around the segment from P - v along d (dd = d.d, edge = 576 dd)
    auto capsule = [](int vx, int vy, int dx, int dy, int dd, long edge) {
      const int dot = vx * dx + vy * dy;
      if (dot <= 0) return vx * vx + vy * vy <= kArmR2;
      if (dot >= dd) {
        const int qx = vx - dx, qy = vy - dy;
        return qx * qx + qy * qy <= kArmR2;
      }
      const long cross = (long)vx * dy - (long)vy * dx;
      return cross * cross <= edge;
    };
    draw_frame(frame, [=](int ch, int i, int j) {
      unsigned p = frame_background(i, j);
      const int px = 16 * j + 8, py = 16 * i + 8;
      const int gx = px - GX, gy = py - GY;
      if (gx * gx + gy * gy <= GR2) p = ch == 1 ? 255u : 64u;                                  // the target: green
      if (capsule(px - kCentre, py - kCentre, ux, uy, uu, uedge)) p = ch == 2 ? 255u : 64u;    // the upper arm: blue
      const int vx = px - EX, vy = py - EY;
      if (capsule(vx, vy, fx, fy, ff, fedge)) p = ch == 0 ? 255u : 64u;                        // the forearm: red
      const int qx = px - TX, qy = py - TY;
      if (qx * qx + qy * qy <= kTipR2) p = ch == 2 ? 64u : 255u;                               // the fingertip: yellow
      return p;
    });
  }
};

// a NaN passes neither comparison
inline bool radius_ok(float r) { return r >= kMinRadius && r <= kMaxRadius; }

}  // namespace

DRQ_API int drq_vec_reacher_step(float* phys, float* target, int* t, unsigned* episode, uint8_t* over, long N, int A,
                                 const float* action, unsigned seed, int episode_length, int repeat, int reset_all,
                                 float target_radius, int sparse, uint8_t* frame, float* reward, float* discount,
                                 uint8_t* first, int* substeps, drq_stream_t stream) {
  if (!phys || !target || (((uintptr_t)phys | (uintptr_t)target) & 3)) return DRQ_EARG;
  if (!radius_ok(target_radius) || (sparse != 0 && sparse != 1)) return DRQ_EARG;
  const EnvIO io{t, episode, over, action, frame, reward, discount, first, substeps, seed, A, episode_length, repeat, reset_all};
  if (!env_io_ok(io, N, 2)) return DRQ_EARG;
  return launch_env_step<Reacher>({phys, target, target_radius, sparse}, io, N, stream);
}

DRQ_API int drq_vec_reacher_render(const float* phys, const float* target, long N, float target_radius, uint8_t* frame,
                                   drq_stream_t stream) {
  if (!phys || !target || (((uintptr_t)phys | (uintptr_t)target) & 3) || !radius_ok(target_radius)) return DRQ_EARG;
  return launch_env_render<Reacher>({const_cast<float*>(phys), const_cast<float*>(target), target_radius, 0}, N, frame,
                                    stream);      // only loaded
}
