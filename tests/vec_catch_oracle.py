"""numpy restatement of the device environment's catch (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("device environment", "Catch"), stated here once more with float32 scalars, one rounding per operation
in the written order, and Python integers (exact, so wider than the contract's int64) for the frame.  The hash and the
draws are those of tests/vec_env_oracle.py; the tether's capsule is the cartpole's (tests/vec_cartpole_oracle.py).

  state      per environment e: phys[8] = (cx, cy, vcx, vcy, bx, by, vbx, vby) float32; t int32; episode uint32; over uint8
  reset      episode += 1, t = 0, over = 0; cx = draw_0 0.4; cy = draw_1 0.4; ay = cy + 0.02; o = draw_2 0.25;
             n = sqrt(o o + 1); bx = cx + (o / n) 0.5; by = ay - (1 / n) 0.5; every velocity 0
  sub-step   hw = cup_width 0.5.
             cup, x then y: v = clamp(v 0.9 + a 0.3, 1.5); q = c + v 0.01; beyond +-0.4 the stop: c = +-0.4, v = 0
             ball: vby = vby - 0.04; s2 = vbx vbx + vby vby; s2 > 16: k = 4 / sqrt(s2), vb = vb k; b = b + vb 0.01
             tether: ay = cy + 0.02; d = b - (cx, ay); d2 = dx dx + dy dy; d2 > 0.25: n = d / sqrt(d2); b = (cx, ay) + n 0.5;
                     vn = (vbx - vcx) nx + (vby - vcy) ny; vn > 0: vb = vb - vn n
             contacts, left wall, right wall, floor: T = the closest point of the segment (a clamp); e = b - T;
                     e2 = ex ex + ey ey; e2 < 0.0049: n = e / sqrt(e2), or (0, 1) for e2 == 0; b = T + n 0.07;
                     vn = (vbx - vcx) nx + (vby - vcy) ny; vn < 0: vb = vb - vn n
             t += 1; over at the limit
  reward     ux = bx - cx; sparse: -(hw - 0.02) <= ux <= hw - 0.02 and cy + 0.02 <= by <= cy + 0.15 ? 1 : 0;
             dense: uy = by - (cy + 0.085); 1 / (1 + 4 (ux ux + uy uy))
  macro step the skeleton's (tests/vec_skeleton_oracle.py); ax, ay = action[e, 0:2] sanitised once; d_i = 1, and the task
             never ends an episode
  frame      in 1/16 pixel, 672 to the unit, the world's centre at (672, 672), y upwards (render below)

Beside the rule: the runs, poses and refused argument lists the CPU and the GPU tests share, and expert(), the scripted
controller that makes the task solvable."""
import numpy as np

from tests.vec_cartpole_oracle import capsule, clamp_to
from tests import vec_skeleton_oracle as S
from tests.vec_env_oracle import BACKGROUND, F, SIDE, draw
from tests.vec_skeleton_oracle import sanitise

DT, GDT, DRAG, GAIN = F(0.01), F(0.04), F(0.9), F(0.3)            # GDT: gravity 4 times dt
MAX_CUP_V, MAX_BALL_V, MAX_BALL_V2 = F(1.5), F(4), F(16)
RANGE, TETHER, TETHER2, WALL = F(0.4), F(0.5), F(0.25), F(0.15)
CAPSULE_R, BALL_R, TOUCH, TOUCH2 = F(0.02), F(0.05), F(0.07), F(0.0049)
MID_Y = F(0.085)                                                  # the interior's centre above cy: (0.02 + 0.15) / 2
RESET_XY, RESET_OFFSET = F(0.4), F(0.25)
MIN_WIDTH, MAX_WIDTH, WIDTH, HARD_WIDTH = 0.16, 0.4, 0.3, 0.18
CENTRE, CUP_R, BALL_PIX, TETHER_R = 672, 13, 34, 10
TETHER_RGB, LEFT_RGB, RIGHT_RGB, FLOOR_RGB, BALL_RGB = (64, 255, 255), (64, 64, 255), (255, 64, 255), (64, 255, 64), (255, 255, 64)
_II, _JJ = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
_PX, _PY = (16 * _JJ + 8).astype(np.int64), (16 * _II + 8).astype(np.int64)

EVENTS = ("taut", "slack", "left_inside", "left_outside", "right_inside", "right_outside", "floor", "degenerate",
          "stop_x_lo", "stop_x_hi", "stop_y_lo", "stop_y_hi", "clamp_cup_x", "clamp_cup_y", "clamp_ball")


def half_width(width):
    return F(F(width) * F(0.5))


def _axis(c, v, a, ev, name):
    q = F(F(v * DRAG) + F(a * GAIN))
    v = clamp_to(q, MAX_CUP_V)
    if v != q:
        ev["clamp_cup_" + name] += 1
    q = F(c + F(v * DT))
    if q < -RANGE:
        ev["stop_" + name + "_lo"] += 1
        return F(-RANGE), F(0)
    if q > RANGE:
        ev["stop_" + name + "_hi"] += 1
        return RANGE, F(0)
    return q, v


def _contact(tx, ty, bx, by, vbx, vby, vcx, vcy, ev):
    """the ball against the capsule whose segment's closest point is (tx, ty); returns the ball and the normal's x (None
    without contact)"""
    ex, ey = F(bx - tx), F(by - ty)
    e2 = F(F(ex * ex) + F(ey * ey))
    if not e2 < TOUCH2:
        return bx, by, vbx, vby, None
    if e2 == 0:
        nx, ny = F(0), F(1)
        ev["degenerate"] += 1
    else:
        e = np.sqrt(e2)
        nx, ny = F(ex / e), F(ey / e)
    bx, by = F(tx + F(nx * TOUCH)), F(ty + F(ny * TOUCH))
    vn = F(F(F(vbx - vcx) * nx) + F(F(vby - vcy) * ny))
    if vn < 0:
        vbx, vby = F(vbx - F(vn * nx)), F(vby - F(vn * ny))
    return bx, by, vbx, vby, ex


def substep(p, a1, a2, hw, ev=None):
    """one simulator step of the state p = (cx, cy, vcx, vcy, bx, by, vbx, vby), float32 scalars, under the sanitised
    action and the half width hw; counts what happened in the dict ev"""
    if ev is None:
        ev = dict.fromkeys(EVENTS, 0)
    cx, cy, vcx, vcy, bx, by, vbx, vby = p
    cx, vcx = _axis(cx, vcx, a1, ev, "x")
    cy, vcy = _axis(cy, vcy, a2, ev, "y")
    vby = F(vby - GDT)
    s2 = F(F(vbx * vbx) + F(vby * vby))
    if s2 > MAX_BALL_V2:
        k = F(MAX_BALL_V / np.sqrt(s2))
        vbx, vby = F(vbx * k), F(vby * k)
        ev["clamp_ball"] += 1
    bx, by = F(bx + F(vbx * DT)), F(by + F(vby * DT))
    ay = F(cy + CAPSULE_R)
    dx, dy = F(bx - cx), F(by - ay)
    d2 = F(F(dx * dx) + F(dy * dy))
    if d2 > TETHER2:
        d = np.sqrt(d2)
        nx, ny = F(dx / d), F(dy / d)
        bx, by = F(cx + F(nx * TETHER)), F(ay + F(ny * TETHER))
        vn = F(F(F(vbx - vcx) * nx) + F(F(vby - vcy) * ny))
        if vn > 0:
            vbx, vby = F(vbx - F(vn * nx)), F(vby - F(vn * ny))
        ev["taut"] += 1
    else:
        ev["slack"] += 1
    xl, xr, top = F(cx - hw), F(cx + hw), F(cy + WALL)
    clampy = lambda y: cy if y < cy else (top if y > top else y)
    bx, by, vbx, vby, ex = _contact(xl, clampy(by), bx, by, vbx, vby, vcx, vcy, ev)
    if ex is not None:
        ev["left_inside" if ex > 0 else "left_outside"] += 1
    bx, by, vbx, vby, ex = _contact(xr, clampy(by), bx, by, vbx, vby, vcx, vcy, ev)
    if ex is not None:
        ev["right_inside" if ex < 0 else "right_outside"] += 1
    tx = xl if bx < xl else (xr if bx > xr else bx)
    bx, by, vbx, vby, ex = _contact(tx, cy, bx, by, vbx, vby, vcx, vcy, ev)
    if ex is not None:
        ev["floor"] += 1
    return (cx, cy, vcx, vcy, bx, by, vbx, vby), ev


def in_cup(p, hw):
    cx, cy, bx, by = p[0], p[1], p[4], p[5]
    ux, inner = F(bx - cx), F(hw - CAPSULE_R)
    return bool(ux >= -inner and ux <= inner and by >= F(cy + CAPSULE_R) and by <= F(cy + WALL))


def reward_of(p, hw, sparse):
    if sparse:
        return F(1) if in_cup(p, hw) else F(0)
    ux, uy = F(p[4] - p[0]), F(p[5] - F(p[1] + MID_Y))
    d2 = F(F(ux * ux) + F(uy * uy))
    return F(F(1) / F(F(1) + F(F(4) * d2)))


def reset_state(seed, e, ep):
    """phys of episode ep of environment e"""
    cx, cy = F(draw(seed, e, ep, 0) * RESET_XY), F(draw(seed, e, ep, 1) * RESET_XY)
    ay = F(cy + CAPSULE_R)
    o = F(draw(seed, e, ep, 2) * RESET_OFFSET)
    n = np.sqrt(F(F(o * o) + F(1)))
    bx = F(cx + F(F(o / n) * TETHER))
    by = F(ay - F(F(F(1) / n) * TETHER))
    return (cx, cy, F(0), F(0), bx, by, F(0), F(0))


def _px(v):
    return int(np.floor(v))


def points(phys, width):
    """the integer coordinates of a frame, each rounded once: the walls' x, the floor's y, the rim's y, the anchor's x and
    y, the ball"""
    cx, cy, _, _, bx, by = phys[:6]
    hw = half_width(width)
    X = lambda x: _px(F(F(x * F(672)) + F(672.5)))
    Y = lambda y: _px(F(F(672.5) - F(y * F(672))))
    return X(F(cx - hw)), X(F(cx + hw)), Y(cy), Y(F(cy + WALL)), X(cx), Y(F(cy + CAPSULE_R)), X(bx), Y(by)


def upright(X, Y_top, Y_bottom, r=CUP_R):
    """the capsule around the vertical segment (X, Y_top) -- (X, Y_bottom), Y_top <= Y_bottom (y points down in the frame)"""
    qy = _PY - np.clip(_PY, Y_top, Y_bottom)
    return (_PX - X) ** 2 + qy ** 2 <= r * r


def level(X_left, X_right, Y, r=CUP_R):
    qx = _PX - np.clip(_PX, X_left, X_right)
    return qx ** 2 + (_PY - Y) ** 2 <= r * r


def disc(X, Y, r):
    return (_PX - X) ** 2 + (_PY - Y) ** 2 <= r * r


def masks(phys, width):
    """the five shapes in their draw order, each with its colour"""
    LX, RX, CY, TY, AX, AY, BX, BY = points(phys, width)
    return ((capsule(AX, AY, BX, BY, TETHER_R), TETHER_RGB), (upright(LX, TY, CY), LEFT_RGB), (upright(RX, TY, CY), RIGHT_RGB),
            (level(LX, RX, CY), FLOOR_RGB), (disc(BX, BY, BALL_PIX), BALL_RGB))


def render(phys, width):
    """the frame of one state"""
    frame = np.stack([BACKGROUND] * 3)
    for m, rgb in masks(phys, width):
        for ch in range(3):
            frame[ch][m] = rgb[ch]
    return frame


def check_state(p, hw):
    """what holds for every state the rule produces: the ball within the tether's length of the anchor, up to the
    rounding of the projection, and inside the world; the cup inside its range.  The slack: the projected ball is
    anchor + n * 0.5 with n = d / sqrt(d2); d2 carries two roundings and a half (the two squares, the sum), the square
    root halves their sum and adds one, the quotient and the product add one each: |n * 0.5| <= 0.5 (1 + 2^-24)^4.25.  The
    final add rounds a number below 1 by at most 2^-25 per axis.  Together 0.5 * 4.25 * 2^-24 + sqrt(2) * 2^-25 < 2 * 2^-23;
    a ball left alone because d2 <= 0.25 as computed is within 0.5 (1 + 2^-24)^1.25.  The anchor's y is the float32 the rule
    uses, and the distance is evaluated in float64."""
    cx, cy, _, _, bx, by = (float(v) for v in p[:6])
    ay = float(F(p[1] + CAPSULE_R))
    assert np.hypot(bx - cx, by - ay) <= 0.5 + 2 * 2.0 ** -23, p
    assert abs(bx) + float(BALL_R) <= 1 and abs(by) + float(BALL_R) <= 1, p
    assert abs(cx) <= float(RANGE) and abs(cy) <= float(RANGE), p
    assert abs(cx) + float(hw) + float(CAPSULE_R) <= 1, p


class CatchOracle(S.SkeletonOracle):
    WORDS = (("phys", (8,), F),)

    def __init__(self, num_envs, episode_length=1000, seed=0, repeat=1, cup_width=WIDTH, sparse=True, frames=True):
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.width, self.sparse = F(cup_width), bool(sparse)
        self.hw = half_width(self.width)
        # what a run met: the events of substep(), sub-steps with and without reward, the longest run of consecutive
        # sub-steps with the ball on the floor
        self.events = dict.fromkeys(EVENTS, 0)
        self.rewarded = self.unrewarded = self.longest_rest = 0
        self._rest = np.zeros(self.N, np.int64)

    def new_episode(self, e, ep):
        self.phys[e] = reset_state(self.seed, e, ep)
        check_state(self.phys[e], self.hw)

    def sanitise(self, row):
        return sanitise(row[0]), sanitise(row[1])

    def frame(self, e):
        return render(self.phys[e], self.width)

    def substep(self, e, a):
        floor = self.events["floor"]
        p, _ = substep(tuple(self.phys[e]), *a, self.hw, self.events)
        check_state(p, self.hw)
        self._rest[e] = self._rest[e] + 1 if self.events["floor"] > floor else 0
        self.longest_rest = max(self.longest_rest, int(self._rest[e]))
        hit = in_cup(p, self.hw)
        self.rewarded += hit
        self.unrewarded += not hit
        self.phys[e] = p
        return reward_of(p, self.hw, self.sparse), F(1), False


_SEEN = ("events", "rewarded", "unrewarded", "longest_rest", "cut_by_limit", "full", "reset_rows")

# ---- the driven run the CPU and the GPU tests share ---------------------------------------------------------------
STEPS, EPISODE_LENGTH, SEED = 40, 7, 5
DRIVEN = tuple((N, A, k, sparse) for (N, A) in ((3, 2), (5, 4)) for k in (1, 2, 16) for sparse in (True, False))


def driven_run(N, A, repeat, sparse, seed=SEED, steps=STEPS, episode_length=EPISODE_LENGTH, frames=True):
    """the oracle driven for `steps` macro steps by S.wild_actions from the staggered reset (S.stagger): the actions it was
    given, everything it returned (the frames only if asked for) and the state after every step"""
    r = np.random.RandomState(seed * 100003 + N * 101 + A * 17 + repeat * 3 + int(sparse))
    o = CatchOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, sparse=sparse, frames=frames)
    o.reset()
    S.stagger(o)
    return S.record(o, steps, lambda s: S.wild_actions(r, N, A), _SEEN)


# The physics drive: seven simulator steps from a hanging ball at rest meet a slack or a taut tether and nothing else.  These
# runs are one long episode of five environments, started from hand-set states ("state0" holds them; a user of the class
# writes them through load_state_dict()):
#   0  the reset state, the cup driven into all four stops at full action: the stops, the cup's clamps, a tether that is
#      taut while the ball is dragged and slack while the cup comes back over it
#   1  the ball on the floor of a cup that is shaken from side to side: both walls from the inside, the floor
#   2  a still cup and a ball that the first step's gravity puts exactly on the floor's segment: the degenerate normal, then
#      rest on the floor for the rest of the run, in the cup
#   3  a ball thrown at the left wall from outside at more than the ball's clamp; 4 the same at the right wall
PHYSICS = tuple((5, 2, 16, sparse, 60, 2000) for sparse in (True, False))         # N, A, repeat, sparse, steps, episode_length
_ON_THE_SEGMENT = -F(F(0) - GDT) * DT                                             # by with by + (0 - 0.04) 0.01 == 0


def physics_start():
    assert F(_ON_THE_SEGMENT + F(F(F(0) - GDT) * DT)) == 0
    return {1: (0, 0, 0, 0, 0, 0.07, 0, 0), 2: (0, 0, 0, 0, 0.05, _ON_THE_SEGMENT, 0, 0),
            3: (0, 0, 0, 0, -0.4, 0.1, 5, 0.5), 4: (0, 0, 0, 0, 0.4, 0.1, -5, 0.5)}


def physics_actions(N, A, s):
    a = np.zeros((N, A), F)
    a[0] = (F(1.5), F(1.5)) if s < 15 else ((F(-1.5), F(-1.5)) if s < 35 else (F(1), F(-0.5)))   # beyond the action's clamp
    a[1, 0] = F(1) if (s // 2) % 2 == 0 else F(-1)
    return a


def physics_run(N, A, repeat, sparse, steps, episode_length, seed=SEED, frames=True):
    o = CatchOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, sparse=sparse, frames=frames)
    o.reset()
    for e, p in physics_start().items():
        o.phys[e] = p
    return S.record(o, steps, lambda s: physics_actions(N, A, s), _SEEN)


def run(cfg, frames=True):
    """the run of a configuration of DRIVEN or PHYSICS"""
    return driven_run(*cfg, frames=frames) if len(cfg) == 4 else physics_run(*cfg, frames=frames)


# ---- the poses the frame is compared at: (phys, cup_width) ------------------------------------------------------------------
def _pose(cx, cy, bx, by, width=WIDTH):
    return np.array([cx, cy, 0.25, -0.5, bx, by, 1, -2], F), width      # the velocities are in no frame


_HW = 0.15
POSES = (
    _pose(0, 0, 0.03, 0.07),                       # the ball on the floor
    _pose(0.1, -0.1, 0.1 - _HW + 0.07, -0.02),     # touching the left wall from inside
    _pose(0.1, -0.1, 0.1 + _HW - 0.07, -0.02),     # touching the right wall from inside
    _pose(-0.2, 0.1, -0.2 + _HW + 0.07, 0.2),      # touching the right wall from outside
    _pose(0, 0, _HW, 0.15 + 0.07),                 # over the rim: on top of the right wall
    _pose(0, 0, 0.5, 0.02),                        # the tether horizontal
    _pose(0, 0, 0, 0.02 - 0.5),                    # the tether vertical: the ball hanging
    _pose(0, 0, 0, 0.02),                          # the tether at zero length: the ball's centre on the anchor
    _pose(0.4, 0.4, 0.4, 0.92, MAX_WIDTH),         # the four corners of the cup's range, the ball at its farthest reach
    _pose(-0.4, 0.4, -0.9, 0.42, MAX_WIDTH),
    _pose(0.4, -0.4, 0.9, -0.38, MIN_WIDTH),
    _pose(-0.4, -0.4, -0.4, -0.88, HARD_WIDTH),
    _pose(0.3, 0.2, -0.05, -0.13),                 # an oblique tether
)


# ---- the scripted controller: what makes the task solvable, and what the constants were chosen for ------------------------
def expert(state, cup_width=WIDTH):
    """the action (two float32) of a scripted controller for the state words (cx, cy, vcx, vcy, bx, by, vbx, vby), in
    float64.  Three modes, chosen from the state alone.  Swing: near the top of its range the cup is accelerated against the
    ball's horizontal velocity relative to it -- the sign that feeds energy into a pendulum through its pivot -- and pulled
    back towards the middle.  Catch: once the ball is no more than 0.25 below the anchor and no longer rising it is at the
    top of a swing, almost at rest; the cup, which is much faster than a ball that has just begun to fall, drops beside
    it until the rim is below the ball and then slides under it.  Hold: with the ball between the walls, the cup brakes."""
    cx, cy, vcx, vcy, bx, by, vbx, vby = (float(v) for v in state)
    hw = float(cup_width) * 0.5
    brake = lambda v: float(np.clip(-3.0 * v, -1, 1))                      # v 0.9 + a 0.3 == 0
    to = lambda goal, c, v, kp=20.0, kd=3.0: float(np.clip(kp * (goal - c) - kd * v, -1, 1))
    ay, rim = cy + 0.02, cy + 0.15
    ux = bx - cx
    if abs(ux) <= hw - 0.02 and ay <= by <= rim + 0.05:
        return F(brake(vcx)), F(brake(vcy))
    clear = cy + 0.17 < by - 0.05
    if clear or (by > ay - 0.25 and vby < 0.1):
        side = 1.0 if ux >= 0 else -1.0
        goal = bx + vbx * 0.1 if clear else bx - side * (hw + 0.1)
        return F(to(float(np.clip(goal, -0.4, 0.4)), cx, vcx)), F(to(max(by - 0.3, -0.4), cy, vcy))
    rel = vbx - vcx
    push = -np.sign(rel) if abs(rel) > 0.02 else (1.0 if ux >= 0 else -1.0)
    return F(float(np.clip(push - 2.5 * cx, -1, 1))), F(to(0.38, cy, vcy, 4.0))


def episode(seed, e, ep, policy, steps=1000, cup_width=WIDTH, sparse=True):
    """episode ep of environment e under policy(state, step) -> (a1, a2): the return and, per step, whether the ball was
    in the cup"""
    p, hw = reset_state(seed, e, ep), half_width(cup_width)
    total, inside = 0.0, []
    for i in range(steps):
        a1, a2 = policy(p, i)
        p, _ = substep(p, sanitise(F(a1)), sanitise(F(a2)), hw)
        check_state(p, hw)
        total += float(reward_of(p, hw, sparse))
        inside.append(in_cup(p, hw))
    return total, inside


# ---- the argument lists drq_vec_catch_step refuses: shared by the CPU and the GPU test -------------------------------------
_BAD_WIDTHS = (0.1599, 0.401, float("nan"), 0.0, -0.3, float("inf"))


def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_catch_step must refuse, around one well-formed list over the four given base addresses
    (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     phys t          episode     over        N  A  action seed L repeat reset width sparse frame
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, 5, 2, ACT, 7, 9, 2, 0, 0.3, 1, FR,
          SC, SC + 0x100, SC + 0x200, SC + 0x300]                          # reward discount first substeps
    bad = S.refused_steps(ok, "w w w b N A action - L repeat reset - - frame w w b w", {11: _BAD_WIDTHS, 12: (2, -1)})
    assert len(bad) == 10 + 22 + 3 + 7
    return bad


def refused_renders(S0, FR):
    """the argument lists drq_vec_catch_render must refuse: (phys, N, cup_width, frame)"""
    return S.refused_reads([S0, 3, 0.3, FR], "w N - frame", {2: (0.1599, 0.401, float("nan"), float("inf"))})
