"""numpy restatement of the device environment's walker (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("device environment", "Walker"), stated here once more with float32 scalars, one rounding per
operation in the written order (every operand below is a numpy float32, so every operation rounds to float32), and Python
integers for the frame.  The hash and the draws are those of tests/vec_env_oracle.py; the capsules are the cartpole's
(tests/vec_cartpole_oracle.py).

  body       six unit point masses: 0 shoulder, 1 hip, 2 front knee, 3 front foot, 4 back knee, 5 back foot; RODS hold them,
             MUSCLES are the distances across the four joints
  state      per environment e: phys[24], phys[4 i : 4 i + 4] = (x, y, vx, vy) of particle i; t int32; episode uint32; over uint8
  reset      reset_state(): a standing pose from five draws, built with sqrt alone; every velocity 0
  sub-step   substep(): drag and gravity, the advance, eight sweeps (muscles with their limits, rods, ground), the velocity
             from the displacement with the ground's friction and the clamp, the wrap of the periodic world
  reward     stand = clamp01((height - 0.1) 10) clamp01((upright - 0.5) 2.5); speed == 0: stand; otherwise
             stand (1 + 5 clamp01(v / speed)) / 6
  macro step the skeleton's (tests/vec_skeleton_oracle.py); a_0 .. a_3 = action[e, 0:4] sanitised once; d_i = 1, and the task
             never ends an episode
  frame      in 1/16 pixel, 672 to the unit, the camera on the torso's middle, the ground line at 1008 (render below)

substep_many() is the same step on arrays, one row per environment, for the searches and the long runs of the CPU test,
which holds it equal to substep() bit for bit.

Beside the rule: the runs, poses and refused argument lists the CPU and the GPU tests share, and gait(), the scripted
open-loop controller that makes the body run: a_m(t) = clamp(A_m sin(2 pi (f t 0.01 + phase_m)) + B_m, -1, 1) with the
constants GAIT_F, GAIT_A, GAIT_PHASE, GAIT_B.  They are the best of 2,048 candidates of a random search over 1,000 steps
on substep_many(), numpy.random.RandomState(7): f uniform in 0.5 .. 4, A in 0.3 .. 1, phase in 0 .. 1, B in -0.5 .. 0.5."""
import numpy as np

from tests.vec_cartpole_oracle import capsule
from tests import vec_skeleton_oracle as S
from tests.vec_env_oracle import BACKGROUND, F, SIDE, draw
from tests.vec_skeleton_oracle import sanitise

NAMES = ("shoulder", "hip", "front_knee", "front_foot", "back_knee", "back_foot")
DT, INV_DT, GDT, DRAG, FRICTION = F(0.01), F(100), F(0.1), F(0.9), F(0.1)
SWEEPS, FORCE_SWEEPS = 8, 4
MAX_V, MAX_V2 = F(2), F(4)
TORSO, LIMB, HALF_TORSO = F(0.4), F(0.25), F(0.2)
L2, T2, TWO_TORSO, TWO_LIMB = F(0.0625), F(F(0.4) * F(0.4)), F(0.8), F(0.5)
RODS = ((0, 1, TORSO), (0, 2, LIMB), (2, 3, LIMB), (1, 4, LIMB), (4, 5, LIMB))
ROD_NAMES = ("torso", "front_thigh", "front_shin", "back_thigh", "back_shin")
MUSCLES = ((1, 2), (0, 3), (0, 4), (1, 5))
MUSCLE_NAMES = ("front_hip", "front_knee", "back_hip", "back_knee")
MID = (F(0.46), F(0.34), F(0.46), F(0.34))
HALF = (F(0.1), F(0.06), F(0.1), F(0.06))
LO = (F(0.3), F(0.25), F(0.3), F(0.25))                  # what a sweep projects a muscle's distance into
HI = (F(0.6), F(0.43), F(0.6), F(0.43))
SKIN = 0.005                                             # the hard limits of a joint are [LO - SKIN, HI + SKIN]
JITTER = (F(0.025), F(0.015), F(0.025), F(0.015))
STIFF, FORCE = F(0.5), F(0.004)
WORLD, HALF_WORLD = F(4), F(2)
TILT = F(0.05)
MAX_SPEED, WALK_SPEED, RUN_SPEED = 2.0, 0.3, 0.6
STAND_LOW, STAND_SCALE, UPRIGHT_LOW, UPRIGHT_SCALE = F(0.1), F(10), F(0.5), F(2.5)
STAND_HEIGHT = 0.2                                       # stand's height term is 1 from here
ZERO, ONE, HALF_, FIVE, SIX = F(0), F(1), F(0.5), F(5), F(6)
UNIT, GROUND_Y, STRIPE, PERIOD, CAPSULE_R = 672, 1008, 168, 336, 18
TORSO_RGB, FRONT_RGB, BACK_RGB, STRIPE_A_RGB, STRIPE_B_RGB = (255, 64, 64), (64, 255, 255), (255, 64, 255), (64, 255, 64), (64, 64, 255)
_II, _JJ = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
_PX, _PY = (16 * _JJ + 8).astype(np.int64), (16 * _II + 8).astype(np.int64)

GAIT_F = 2.93843566
GAIT_A = (0.82920531, 0.95223464, 0.57681681, 0.59532281)
GAIT_PHASE = (0.47073255, 0.01950197, 0.67365478, 0.74374457)
GAIT_B = (0.49031962, -0.1706505, 0.43998909, 0.01151752)

EVENTS = tuple("ground_" + n for n in NAMES) + tuple("lower_" + n for n in MUSCLE_NAMES) + tuple("upper_" + n for n in MUSCLE_NAMES) + (
    "force_clamp", "speed_clamp", "degenerate", "wrap_forward", "wrap_backward", "fallen", "stand_partial",
    "move_zero", "move_inside", "move_one")


def gait(t):
    """the action (four float32) of the scripted open-loop gait at simulator step t"""
    a = [A * np.sin(2 * np.pi * (GAIT_F * t * 0.01 + ph)) + B for A, ph, B in zip(GAIT_A, GAIT_PHASE, GAIT_B)]
    return np.clip(np.array(a), -1, 1).astype(F)


# ---- the rule on float32 scalars -------------------------------------------------------------------------------------------
def _normal(x, y, i, j, ev):
    dx, dy = x[j] - x[i], y[j] - y[i]
    d2 = dx * dx + dy * dy
    if d2 == 0:
        ev["degenerate"] += 1
        return ZERO, ZERO, ONE
    d = np.sqrt(d2)
    return d, dx / d, dy / d


def _move(x, y, i, j, nx, ny, c):
    h = c * HALF_
    hx, hy = nx * h, ny * h
    x[i] = x[i] + hx
    y[i] = y[i] + hy
    x[j] = x[j] - hx
    y[j] = y[j] - hy


def substep(p, a, ev=None):
    """one simulator step of the state p (24 float32 scalars) under the sanitised action a (four); counts what happened in
    the dict ev.  Returns the new state and ev"""
    if ev is None:
        ev = dict.fromkeys(EVENTS, 0)
    x, y, vx, vy = list(p[0::4]), list(p[1::4]), list(p[2::4]), list(p[3::4])
    ox, oy = [None] * 6, [None] * 6
    for i in range(6):
        vx[i] = vx[i] * DRAG
        vy[i] = vy[i] * DRAG - GDT
        ox[i], oy[i] = x[i], y[i]
        x[i] = x[i] + vx[i] * DT
        y[i] = y[i] + vy[i] * DT
    target = [MID[m] + a[m] * HALF[m] for m in range(4)]
    for sweep in range(SWEEPS):
        for m, (i, j) in enumerate(MUSCLES):
            d, nx, ny = _normal(x, y, i, j, ev)
            c = ZERO
            if sweep < FORCE_SWEEPS:
                c = (d - target[m]) * STIFF
                if c < -FORCE or c > FORCE:
                    c = -FORCE if c < -FORCE else FORCE
                    ev["force_clamp"] += 1
            q = d - c
            if q < LO[m]:
                c = d - LO[m]
                ev["lower_" + MUSCLE_NAMES[m]] += 1
            elif q > HI[m]:
                c = d - HI[m]
                ev["upper_" + MUSCLE_NAMES[m]] += 1
            _move(x, y, i, j, nx, ny, c)
        for i, j, length in RODS:
            d, nx, ny = _normal(x, y, i, j, ev)
            _move(x, y, i, j, nx, ny, d - length)
        for i in range(6):
            if y[i] < 0:
                y[i] = ZERO
    for i in range(6):
        wx, wy = (x[i] - ox[i]) * INV_DT, (y[i] - oy[i]) * INV_DT
        if y[i] == 0:
            wx = wx * FRICTION
            ev["ground_" + NAMES[i]] += 1
        s2 = wx * wx + wy * wy
        if s2 > MAX_V2:
            k = MAX_V / np.sqrt(s2)
            wx, wy = wx * k, wy * k
            ev["speed_clamp"] += 1
        vx[i], vy[i] = wx, wy
    mid = (x[0] + x[1]) * HALF_
    if mid >= HALF_WORLD:
        x = [v - WORLD for v in x]
        ev["wrap_forward"] += 1
    elif mid < -HALF_WORLD:
        x = [v + WORLD for v in x]
        ev["wrap_backward"] += 1
    if y[0] == 0 and y[1] == 0:
        ev["fallen"] += 1
    out = [None] * 24
    out[0::4], out[1::4], out[2::4], out[3::4] = x, y, vx, vy
    return tuple(out), ev


def clamp01(v):
    return ZERO if v < 0 else (ONE if v > 1 else v)


def stand_of(p):
    height, upright = (p[1] + p[5]) * HALF_, (p[0] - p[4]) * UPRIGHT_SCALE
    return clamp01((height - STAND_LOW) * STAND_SCALE) * clamp01((upright - UPRIGHT_LOW) * UPRIGHT_SCALE)


def move_of(p, speed):
    return clamp01((p[2] + p[6]) * HALF_ / F(speed))


def reward_of(p, speed):
    stand = stand_of(p)
    if F(speed) == 0:
        return stand
    return stand * (ONE + FIVE * move_of(p, speed)) / SIX


# ---- the reset: the same expressions serve scalars and arrays -----------------------------------------------------------------
def _knee(bx, by, dx, dy, px, py, dist):
    al = (L2 - dist * dist + T2) / TWO_TORSO
    h = np.sqrt(L2 - al * al)
    return bx + al * dx + h * px, by + al * dy + h * py


def _foot(bx, by, kx, ky, dist):
    wx, wy = (kx - bx) / LIMB, (ky - by) / LIMB
    dd = dist * dist
    al = dd / TWO_LIMB
    h = np.sqrt(dd - al * al)
    return bx + al * wx + h * wy, by + al * wy - h * wx


def pose_of(v):
    """the standing pose of the five draws v (float32 scalars, or arrays): x[6], y[6]"""
    tilt = v[0] * TILT
    n = np.sqrt(tilt * tilt + ONE)
    ux, uy = ONE / n, tilt / n
    d = [MID[m] + v[1 + m] * JITTER[m] for m in range(4)]
    sx, sy = ux * HALF_TORSO, uy * HALF_TORSO
    hx, hy = -sx, -sy
    px, py = uy, -ux
    fkx, fky = _knee(sx, sy, -ux, -uy, px, py, d[0])
    ffx, ffy = _foot(sx, sy, fkx, fky, d[1])
    bkx, bky = _knee(hx, hy, ux, uy, px, py, d[2])
    bfx, bfy = _foot(hx, hy, bkx, bky, d[3])
    low = np.minimum(np.minimum(ffy, bfy), np.minimum(fky, bky))
    return [sx, hx, fkx, ffx, bkx, bfx], [y - low for y in (sy, hy, fky, ffy, bky, bfy)]


def reset_state(seed, e, ep):
    """phys of episode ep of environment e"""
    x, y = pose_of([draw(seed, e, ep, k) for k in range(5)])
    out = [ZERO] * 24
    out[0::4], out[1::4] = x, y
    assert all(v.dtype == np.float32 for v in out)
    return tuple(out)


def reset_states(seed, envs, ep=1):
    """float32 [len(envs), 24]"""
    return np.array([reset_state(seed, e, ep) for e in envs], F)


# ---- the rule on arrays: one row per environment -------------------------------------------------------------------------------
def _normal_many(x, y, i, j):
    dx, dy = x[j] - x[i], y[j] - y[i]
    d2 = dx * dx + dy * dy
    zero = d2 == 0
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        nx, ny = np.where(zero, ZERO, dx / d), np.where(zero, ONE, dy / d)
    return d, nx, ny


def substep_many(phys, a):
    """substep() of every row of phys, float32 [n, 24], under the sanitised actions a, float32 [n, 4]: the new states and
    the shift of the wrap per row (+-4 or 0)"""
    assert phys.dtype == np.float32 and a.dtype == np.float32
    x, y, vx, vy = (list(phys[:, k::4].T) for k in range(4))
    ox, oy = [None] * 6, [None] * 6
    for i in range(6):
        vx[i] = vx[i] * DRAG
        vy[i] = vy[i] * DRAG - GDT
        ox[i], oy[i] = x[i], y[i]
        x[i] = x[i] + vx[i] * DT
        y[i] = y[i] + vy[i] * DT
    target = [MID[m] + a[:, m] * HALF[m] for m in range(4)]
    for sweep in range(SWEEPS):
        for m, (i, j) in enumerate(MUSCLES):
            d, nx, ny = _normal_many(x, y, i, j)
            if sweep < FORCE_SWEEPS:
                c = (d - target[m]) * STIFF
                c = np.where(c < -FORCE, -FORCE, np.where(c > FORCE, FORCE, c))
            else:
                c = np.zeros_like(d)
            q = d - c
            c = np.where(q < LO[m], d - LO[m], np.where(q > HI[m], d - HI[m], c))
            _move(x, y, i, j, nx, ny, c)
        for i, j, length in RODS:
            d, nx, ny = _normal_many(x, y, i, j)
            _move(x, y, i, j, nx, ny, d - length)
        for i in range(6):
            y[i] = np.where(y[i] < 0, ZERO, y[i])
    for i in range(6):
        wx, wy = (x[i] - ox[i]) * INV_DT, (y[i] - oy[i]) * INV_DT
        wx = np.where(y[i] == 0, wx * FRICTION, wx)
        s2 = wx * wx + wy * wy
        with np.errstate(all="ignore"):
            k = MAX_V / np.sqrt(s2)
            vx[i], vy[i] = np.where(s2 > MAX_V2, wx * k, wx), np.where(s2 > MAX_V2, wy * k, wy)
    mid = (x[0] + x[1]) * HALF_
    shift = np.where(mid >= HALF_WORLD, -WORLD, np.where(mid < -HALF_WORLD, WORLD, ZERO))
    x = [v + shift for v in x]                          # v - 4 and v + (-4) are the same float32 operation
    out = np.empty_like(phys)
    for i in range(6):
        out[:, 4 * i], out[:, 4 * i + 1], out[:, 4 * i + 2], out[:, 4 * i + 3] = x[i], y[i], vx[i], vy[i]
    assert out.dtype == np.float32
    return out, shift


def sanitise_many(a):
    """S.sanitise of every element"""
    a = np.asarray(a, F)
    return np.clip(np.where(np.isnan(a), ZERO, a), F(-1), F(1)).astype(F)


# ---- the frame ----------------------------------------------------------------------------------------------------------
def _px(v):
    return int(np.floor(v))


def points(phys):
    """the integers of a frame, each rounded once: the camera's C, then X and Y of the six particles"""
    x, y = [F(v) for v in phys[0::4]], [F(v) for v in phys[1::4]]
    C = _px((x[0] + x[1]) * HALF_ * F(UNIT))
    X = [_px(v * F(UNIT) + HALF_) - C + UNIT for v in x]
    Y = [_px(F(1008.5) - v * F(UNIT)) for v in y]
    return C, X, Y


def masks(phys):
    """the shapes in their draw order, each with its colour: the ground's two stripes, the back leg, the torso, the front leg"""
    C, X, Y = points(phys)
    below = _PY > GROUND_Y
    stripe = (_PX - UNIT + C) % PERIOD < STRIPE          # Python's %: the floor modulo
    cap = lambda i, j: capsule(X[i], Y[i], X[j], Y[j], CAPSULE_R)
    return ((below & stripe, STRIPE_A_RGB), (below & ~stripe, STRIPE_B_RGB), (cap(1, 4) | cap(4, 5), BACK_RGB),
            (cap(0, 1), TORSO_RGB), (cap(0, 2) | cap(2, 3), FRONT_RGB))


def render(phys):
    """the frame of one state"""
    frame = np.stack([BACKGROUND] * 3)
    for m, rgb in masks(phys):
        for ch in range(3):
            frame[ch][m] = rgb[ch]
    return frame


# ---- what holds for every state the rule produces from a reset ---------------------------------------------------------------
ROD_TOLERANCE = 0.01            # of the rod's length
LIMIT_SLACK = 0.0               # the hard limits [LO - SKIN, HI + SKIN] hold as the header states them; the issue allows 0.0025
# Stays in the frame.  A particle is joined to the torso's middle by half the torso and at most two limbs, so it is within
# (0.2 + 0.25 + 0.25) * 1.01 = 0.707 < 1 of the camera, the frame's half width; and no higher above the lowest particle
# than the longest chain, foot to foot, (0.25 + 0.25 + 0.4 + 0.25 + 0.25) * 1.01 = 1.414 < 1.5, the frame's top above the
# ground -- if some particle is within FRAME_TOP - 1.414 of the ground, which the runs are held to beside the rest.
FRAME_HALF_WIDTH, FRAME_TOP, REACH, CHAIN = 1.0, 1.5, 0.7 * 1.01, 1.4 * 1.01


def lengths(phys):
    """float64 [n, 5] rod lengths and [n, 4] muscle distances of the states phys [n, 24]"""
    p = np.asarray(phys, np.float64).reshape(-1, 6, 4)
    dist = lambda i, j: np.hypot(p[:, j, 0] - p[:, i, 0], p[:, j, 1] - p[:, i, 1])
    return np.stack([dist(i, j) for i, j, _ in RODS], 1), np.stack([dist(i, j) for i, j in MUSCLES], 1)


def joint_signs(phys):
    """the signs of the four joints' cross products, [n, 4]: thigh x shin of either leg, torso x thigh at either end"""
    p = np.asarray(phys, np.float64).reshape(-1, 6, 4)
    cross = lambda a, b, c, d: (p[:, b, 0] - p[:, a, 0]) * (p[:, d, 1] - p[:, c, 1]) - (p[:, b, 1] - p[:, a, 1]) * (p[:, d, 0] - p[:, c, 0])
    return np.sign(np.stack([cross(0, 2, 2, 3), cross(1, 4, 4, 5), cross(1, 0, 0, 2), cross(0, 1, 1, 4)], 1))


def check_states(phys, signs=None):
    """the conditions of a body that holds together, on the states phys [n, 24]"""
    phys = np.asarray(phys)
    assert np.isfinite(phys).all() and (phys[:, 1::4] >= 0).all()
    rods, muscles = lengths(phys)
    nominal = np.array([float(r[2]) for r in RODS])
    assert (np.abs(rods / nominal - 1) <= ROD_TOLERANCE).all(), rods
    lo, hi = np.array([float(v) for v in LO]) - SKIN, np.array([float(v) for v in HI]) + SKIN
    assert (muscles >= lo - LIMIT_SLACK).all() and (muscles <= hi + LIMIT_SLACK).all(), muscles
    x, y = phys[:, 0::4].astype(np.float64), phys[:, 1::4].astype(np.float64)
    cam = (x[:, 0] + x[:, 1]) / 2
    assert (np.abs(x - cam[:, None]) <= REACH).all() and REACH < FRAME_HALF_WIDTH
    assert (y.max(1) - y.min(1) <= CHAIN).all() and (y.max(1) < FRAME_TOP).all() and CHAIN < FRAME_TOP
    assert (np.abs(cam) <= float(HALF_WORLD)).all()
    if signs is not None:
        assert (joint_signs(phys) == signs).all()


class WalkerOracle(S.SkeletonOracle):
    WORDS = (("phys", (24,), F),)

    def __init__(self, num_envs, episode_length=1000, seed=0, repeat=1, speed=WALK_SPEED, frames=True, checked=True):
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.speed, self.checked = F(speed), checked       # checked: states from a reset hold together (not hand-set ones)
        self.events = dict.fromkeys(EVENTS, 0)

    def new_episode(self, e, ep):
        self.phys[e] = reset_state(self.seed, e, ep)

    def sanitise(self, row):
        return tuple(sanitise(row[m]) for m in range(4))

    def frame(self, e):
        return render(self.phys[e])

    def substep(self, e, a):
        p, _ = substep(tuple(self.phys[e]), a, self.events)
        if self.checked:
            check_states(np.array([p]))
        stand = stand_of(p)
        self.events["stand_partial"] += bool(0 < stand < 1)
        if self.speed > 0:
            move = move_of(p, self.speed)
            self.events["move_zero" if move == 0 else ("move_one" if move == 1 else "move_inside")] += 1
        self.phys[e] = p
        return reward_of(p, self.speed), ONE, False


_SEEN = ("events", "cut_by_limit", "full", "reset_rows")

# ---- the driven run the CPU and the GPU tests share ---------------------------------------------------------------
STEPS, EPISODE_LENGTH, SEED = 40, 7, 5
DRIVEN = tuple((N, A, k, speed) for (N, A) in ((3, 4), (5, 6)) for k in (1, 2, 16) for speed in (0.0, WALK_SPEED))


def driven_run(N, A, repeat, speed, seed=SEED, steps=STEPS, episode_length=EPISODE_LENGTH, frames=True):
    """the oracle driven for `steps` macro steps by S.wild_actions from the staggered reset (S.stagger)"""
    r = np.random.RandomState(seed * 100003 + N * 101 + A * 17 + repeat * 3 + int(speed > 0))
    o = WalkerOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, speed=speed, frames=frames)
    o.reset()
    S.stagger(o)
    return S.record(o, steps, lambda s: S.wild_actions(r, N, A), _SEEN)


# The physics drive: seven simulator steps from a standing pose meet the ground under the feet and the force clamp and
# little else.  These runs are one long episode of five environments, started from hand-set states ("state0" holds them; a
# user of the class writes them through load_state_dict()):
#   0  the reset pose just behind the seam at +2, shoved forwards and then driven by gait(): the wrap forwards, a body
#      that moves at and above the speed asked for
#   1  the reset pose just in front of the seam at -2, thrown backwards at more than the speed clamp: the wrap backwards,
#      the clamp, move = 0; then shaken by +-1 flips
#   2  the reset pose upside down, 0.3 above the ground: falls on its back, the torso on the ground, legs waving
#   3  a crumpled body: every muscle distance below its lower limit, the front foot exactly on the shoulder (the
#      degenerate normal)
#   4  a body stretched out on one line 0.3 above the ground: every muscle distance above its upper limit; falls flat, so
#      every particle meets the ground
PHYSICS = tuple((5, 4, 16, speed, 60, 2000) for speed in (0.0, WALK_SPEED))      # N, A, repeat, speed, steps, episode_length


def _state(x, y, vx=0.0, vy=0.0):
    out = np.zeros(24, F)
    out[0::4], out[1::4], out[2::4], out[3::4] = x, y, vx, vy
    return out


def physics_start(seed=SEED):
    base = [np.array(reset_state(seed, e, 1), F) for e in range(5)]
    s0 = _state(base[0][0::4] + F(1.9), base[0][1::4], 1.5)
    s1 = _state(base[1][0::4] - F(1.9), base[1][1::4], -3.0, 0.5)
    s2 = _state(base[2][0::4], F(0.6) - base[2][1::4])
    s3 = _state([0.2, -0.2, -0.05, 0.2, 0.05, -0.2], [0.3, 0.3, 0.2, 0.3, 0.2, 0.2])
    s4 = _state([0.2, -0.2, 0.45, 0.7, -0.45, -0.7], [0.3] * 6)
    return {0: s0, 1: s1, 2: s2, 3: s3, 4: s4}


def physics_actions(N, A, s):
    a = np.zeros((N, A), F)
    a[0, :4] = gait(16 * s)
    a[1, :4] = (1, -1, -1, 1) if (s // 2) % 2 == 0 else (-1, 1, 1, -1)
    a[2, :4] = (1.5, -1.5, -1.5, 1.5) if (s // 3) % 2 == 0 else (-1.5, 1.5, 1.5, -1.5)      # beyond the action's clamp
    return a


def physics_run(N, A, repeat, speed, steps, episode_length, seed=SEED, frames=True):
    o = WalkerOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, speed=speed, frames=frames, checked=False)
    o.reset()
    for e, p in physics_start(seed).items():
        o.phys[e] = p
    return S.record(o, steps, lambda s: physics_actions(N, A, s), _SEEN)


def run(cfg, frames=True):
    """the run of a configuration of DRIVEN or PHYSICS"""
    return driven_run(*cfg, frames=frames) if len(cfg) == 4 else physics_run(*cfg, frames=frames)


# ---- the poses the frame is compared at ----------------------------------------------------------------------------------
def _standing(dx=0.0):
    p = np.array(reset_state(SEED, 0, 1), F)
    p[0::4] += F(dx)
    p[2::4], p[3::4] = 0.25, -0.5                        # the velocities are in no frame
    return p


POSES = (
    _standing(),                                                                         # upright, both feet near y = 0
    _state([0.2, -0.2, 0.45, 0.7, -0.45, -0.7], [0.0] * 6),                               # lying flat: every particle at y = 0
    _state([0.2, -0.2, 0.2, 0.2, -0.2, -0.45], [0.25, 0.25, 0.0, 0.0, 0.0, 0.0]),         # the torso exactly horizontal, both thighs
                                                                                         # exactly vertical, knee and foot at one point
    _standing(1.99), _standing(-2.0),                                                    # either side of the seam
    _standing(-0.7),                                                                     # a negative camera offset
    _state([0.7, 0.3, 0.7, 0.6, 0.3, 0.2], [0.3, 0.3, 0.05, 0.0, 0.1, 0.0]),              # the camera at 0.5: C = 336, one period
    _state([-0.3, -0.7, -0.3, -0.4, -0.7, -0.8], [0.3, 0.3, 0.05, 0.0, 0.1, 0.0]),        # ... and at -0.5: C = -336
    _state([0.1, -0.2, 0.3, 0.5, -0.3, -0.1], [0.5, 0.2, 0.4, 0.6, 0.4, 0.1]),            # oblique, a foot above the torso
)


# ---- the argument lists drq_vec_walker_step refuses: shared by the CPU and the GPU test -------------------------------------
_BAD_SPEEDS = (-0.001, 2.001, float("nan"), float("inf"), -1.0)


def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_walker_step must refuse, around one well-formed list over the four given base addresses
    (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     phys t          episode     over        N  A  action seed L repeat reset speed frame
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, 5, 4, ACT, 7, 9, 2, 0, 0.3, FR,
          SC, SC + 0x100, SC + 0x200, SC + 0x300]                          # reward discount first substeps
    return S.refused_steps(ok, "w w w b N A action - L repeat reset - frame w w b w", {11: _BAD_SPEEDS})


def refused_renders(S0, FR):
    """the argument lists drq_vec_walker_render must refuse: (phys, N, frame)"""
    return S.refused_reads([S0, 3, FR], "w N frame", {})
