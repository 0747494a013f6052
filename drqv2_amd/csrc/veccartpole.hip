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
// drq_vec_cartpole_step is one launch of N workgroups of 256 threads, one per environment, the shape of
// vec_task_step_kernel (vecenv.hip):
//   state     every thread loads the eight state words of its environment and computes the reset or the macro step
//             itself, in registers -- the same IEEE operations on the same operands in every lane, so all 256 agree, on
//             the trip count of the sub-step loop too
//   barrier   __syncthreads(): every lane has read the old state before thread 0 stores the new one and the scalars
//   frame     1,323 pieces of 16 bytes, 5 or 6 per lane, consecutive lanes consecutive pieces; per pixel the background,
//             the rail, the cart and the pole's capsule, in integers (int64 where the capsule's cross product is squared)
// No LDS, no atomics, nothing crosses workgroups.  drq_vec_cartpole_render is the frame part alone.
#include "vecenv_common.h"
#include "../../include/drqv2_hip.h"

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

// The pixel rule: the frame of (x, c, s) into the 21,168 bytes at `frame`, by the 256 threads of a workgroup -- 1,323
// pieces of 16 bytes, consecutive lanes consecutive pieces.  Coordinates are 1/16 pixel; pixel (i, j) has its centre at
// (16 j + 8, 16 i + 8).  Shapes that leave the frame are clipped by the loop itself: it visits the frame's pixels only.
__device__ __forceinline__ void cartpole_frame(float x, float c, float s, uint8_t* frame) {
  const float xs = x * 320.0f;
  const int X0 = (int)floorf(xs + 672.5f);
  const int X1 = (int)floorf((xs + s * 320.0f) + 672.5f);
  const int Y1 = (int)floorf(672.5f - c * 320.0f);
  const int dx = X1 - X0, dy = Y1 - kCentre;
  const int dd = dx * dx + dy * dy;
  const long edge = (long)kPoleR2 * dd;
  uint4* dst = reinterpret_cast<uint4*>(frame);
  for (int v = threadIdx.x; v < kPieces; v += kThreads) {
    const int o = 16 * v;
    const int ch = o / kPlane, rem = o - ch * kPlane;
    int i = rem / kSide, j = rem - i * kSide;
    const unsigned pole_colour = ch == 0 ? 255u : 64u, cart_colour = ch == 1 ? 255u : 64u, rail_colour = ch == 2 ? 255u : 64u;
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      unsigned p = 32u + (unsigned)((i + j) >> 2);
      const int px = 16 * j + 8, py = 16 * i + 8;
      const int rx = px - kCentre, vx = px - X0, vy = py - kCentre;
      if (i == kRailRow && rx >= -kRailHalf && rx <= kRailHalf) p = rail_colour;
      if (vx >= -kCartHalfW && vx <= kCartHalfW && vy >= -kCartHalfH && vy <= kCartHalfH) p = cart_colour;
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
      if (in) p = pole_colour;
      w[b >> 2] |= p << (8 * (b & 3));
      if (++j == kSide) {
        j = 0;
        ++i;
      }
    }
    dst[v] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

struct CartpoleArgs {
  float* phys;            // [N][5]: x, xdot, c, s, omega
  int* t;
  unsigned* episode;
  uint8_t* over;
  const float* action;    // [N][A]; null only with reset_all
  uint8_t* frame;         // [N][3][84][84]
  float* reward;
  float* discount;
  uint8_t* first;
  int* substeps;
  unsigned seed;
  int A, episode_length, repeat, reset_all, swing_up;
};

// One macro step of every environment: the reset row, or up to `repeat` sub-steps folded by the wrapper rule
// (dmc.py:40-50).  repeat, reset_all and swing_up are launch arguments and the state is the workgroup's own, so every
// branch and the trip count of the loop are uniform across the 256 lanes.
__global__ __launch_bounds__(kThreads) void vec_cartpole_step_kernel(CartpoleArgs a) {
  const long e = blockIdx.x;
  const float* ph = a.phys + 5 * e;
  Pole p{ph[0], ph[1], ph[2], ph[3], ph[4]};
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
    p.x = reach_draw(a.seed, (unsigned)e, episode, 0u) * 0.1f;
    p.xdot = 0.0f;
    p.c = a.swing_up ? -1.0f : 1.0f;
    p.s = reach_draw(a.seed, (unsigned)e, episode, 1u) * 0.05f;
    normalise(p.c, p.s);
    p.omega = 0.0f;
    first = 1u;
  } else {
    float act = a.action[e * a.A];
    act = act != act ? 0.0f : clamp1(act);
    do {
      cartpole_substep(p, act);
      t += 1;
      const float r = cartpole_reward(p, act);
      if (t == a.episode_length) over = 1u;
      reward = reward + r;          // the wrapper rule with every d_i = 1: r * 1 = r, and the discount stays 1
    } while (++n < a.repeat && !over);
    first = 0u;
  }
  __syncthreads();            // every lane holds the old state: thread 0 may now replace it
  if (threadIdx.x == 0) {
    float* out = a.phys + 5 * e;
    out[0] = p.x;
    out[1] = p.xdot;
    out[2] = p.c;
    out[3] = p.s;
    out[4] = p.omega;
    a.t[e] = t;
    a.episode[e] = episode;
    a.over[e] = (uint8_t)over;
    a.reward[e] = reward;
    a.discount[e] = discount;
    a.first[e] = (uint8_t)first;
    a.substeps[e] = n;
  }

  cartpole_frame(p.x, p.c, p.s, a.frame + e * (long)kFrame);
}

// the frames of the states as they are: the frame part of the step kernel alone, same launch shape
__global__ __launch_bounds__(kThreads) void vec_cartpole_render_kernel(const float* __restrict__ phys, uint8_t* frame) {
  const long e = blockIdx.x;
  cartpole_frame(phys[5 * e], phys[5 * e + 2], phys[5 * e + 3], frame + e * (long)kFrame);
}

}  // namespace

DRQ_API int drq_vec_cartpole_step(float* phys, int* t, unsigned* episode, uint8_t* over, long N, int A, const float* action,
                                  unsigned seed, int episode_length, int repeat, int reset_all, int swing_up,
                                  uint8_t* frame, float* reward, float* discount, uint8_t* first, int* substeps,
                                  drq_stream_t stream) {
  if (!phys || !t || !episode || !over || !frame || !reward || !discount || !first || !substeps) return DRQ_EARG;
  if (N < 1 || N > INT32_MAX || A < 1 || episode_length < 1) return DRQ_EARG;
  if (repeat < 1 || repeat > DRQ_TASK_MAX_REPEAT) return DRQ_EARG;
  if ((reset_all != 0 && reset_all != 1) || (swing_up != 0 && swing_up != 1)) return DRQ_EARG;
  if (!action && !reset_all) return DRQ_EARG;
  if ((uintptr_t)frame & 15) return DRQ_EARG;
  if (((uintptr_t)phys | (uintptr_t)t | (uintptr_t)episode | (uintptr_t)reward | (uintptr_t)discount |
       (uintptr_t)substeps | (uintptr_t)action) & 3)
    return DRQ_EARG;
  CartpoleArgs a{phys,     t,     episode,  over, action, frame,          reward,
                 discount, first, substeps, seed, A,      episode_length, repeat, reset_all, swing_up};
  hipLaunchKernelGGL(vec_cartpole_step_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, a);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}

DRQ_API int drq_vec_cartpole_render(const float* phys, long N, uint8_t* frame, drq_stream_t stream) {
  if (!phys || !frame || N < 1 || N > INT32_MAX) return DRQ_EARG;
  if (((uintptr_t)frame & 15) || ((uintptr_t)phys & 3)) return DRQ_EARG;
  hipLaunchKernelGGL(vec_cartpole_render_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, phys, frame);
  DRQ_LAUNCH_CHECK();
  return DRQ_OK;
}
