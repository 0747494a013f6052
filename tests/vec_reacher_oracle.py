"""numpy restatement of the device environment's reacher (a helper module: not collected).  The contract is the comment
of include/drqv2_hip.h ("device environment", "Reacher"), stated here once more with float32 scalars, one rounding per
operation in the written order, and Python integers (exact, so wider than the contract's int64) for the capsules.  The
hash and the draws are those of tests/vec_env_oracle.py, normalise() is the cartpole's (tests/vec_cartpole_oracle.py).

  state      per environment e: phys[6] = (c1, s1, w1, c2, s2, w2), target[2] float32; t int32; episode uint32; over uint8
  direction  of a draw v: u = clamp(v 1.1111112, 1); x = 1 - 2 |u|; y = 1 - |x|, negated for u < 0; x x + y y < 0.25: (1, 0);
             otherwise normalise(x, y)
  reset      episode += 1, t = 0, over = 0; (c1, s1) = direction(draw_0); (c2, s2) = direction(draw_1); w1 = w2 = 0;
             (gx, gy) = direction(draw_2); f = 0.5 + draw_3 0.5; rho = (1 - radius) f; target = (rho gx, rho gy)
  sub-step   M11 = 0.75 + 0.5 c2; M12 = 0.25 + 0.25 c2; h = 0.25 s2; cor = (2 w1) w2 + w2 w2;
             tau1 = (a1 K - B w1) + h cor; tau2 = (a2 K - B w2) - h (w1 w1); det = M11 0.25 - M12 M12;
             al1 = (0.25 tau1 - M12 tau2) / det; al2 = (M11 tau2 - M12 tau1) / det; w = clamp(w + al 0.01, 16) for both;
             per joint k = w 0.01; k != 0: (c, s) = normalise(c - s k, s + c k); t += 1; over at the limit
  reward     c12 = c1 c2 - s1 s2; s12 = s1 c2 + c1 s2; tip = (0.5 c1 + 0.5 c12, 0.5 s1 + 0.5 s12); d = tip - target;
             d2 = dx dx + dy dy; sparse: d2 <= radius radius ? 1 : 0; dense: 1 / (1 + 4 d2)
  macro step the skeleton's (tests/vec_skeleton_oracle.py); a1, a2 = action[e, 0:2] sanitised once; d_i = 1, and the task
             never ends an episode
  frame      in 1/16 pixel, 576 to the unit, the shoulder at (672, 672), y upwards (render below)
"""
import numpy as np

from tests.vec_cartpole_oracle import capsule, clamp_to, normalise
from tests import vec_skeleton_oracle as S
from tests.vec_env_oracle import BACKGROUND, F, SIDE, clamp1, draw
from tests.vec_skeleton_oracle import sanitise

K, B = F(2), F(0.5)
DT, MAX_W = F(0.01), F(16)
CENTRE, ARM_R, TIP_R = 672, 24, 32
TARGET_RGB, UPPER_RGB, FORE_RGB, TIP_RGB = (64, 255, 64), (64, 64, 255), (255, 64, 64), (255, 255, 64)
_II, _JJ = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
_PX, _PY = (16 * _JJ + 8).astype(np.int64), (16 * _II + 8).astype(np.int64)


def direction(v):
    """the unit vector of a draw: the diamond |x| + |y| = 1 walked once by u in [-1, 1], then normalised"""
    u = clamp1(F(v * F(1.1111112)))
    x = F(F(1) - F(F(2) * np.abs(u)))
    y = F(F(1) - np.abs(x))
    if u < 0:
        y = F(-y)
    if F(F(x * x) + F(y * y)) < F(0.25):
        return F(1), F(0)
    return normalise(x, y)


def rotate(c, s, w):
    k = F(w * DT)
    if k == 0:
        return c, s
    return normalise(F(c - F(s * k)), F(s + F(c * k)))


def substep(p, a1, a2):
    """one simulator step of the state p = (c1, s1, w1, c2, s2, w2), float32 scalars, under the sanitised torques;
    returns the new state and how many of w1, w2 the clamp cut"""
    c1, s1, w1, c2, s2, w2 = p
    m11 = F(F(0.75) + F(F(0.5) * c2))
    m12 = F(F(0.25) + F(F(0.25) * c2))
    h = F(F(0.25) * s2)
    cor = F(F(F(F(2) * w1) * w2) + F(w2 * w2))
    tau1 = F(F(F(a1 * K) - F(B * w1)) + F(h * cor))
    tau2 = F(F(F(a2 * K) - F(B * w2)) - F(h * F(w1 * w1)))
    det = F(F(m11 * F(0.25)) - F(m12 * m12))
    al1 = F(F(F(F(0.25) * tau1) - F(m12 * tau2)) / det)
    al2 = F(F(F(m11 * tau2) - F(m12 * tau1)) / det)
    q1, q2 = F(w1 + F(al1 * DT)), F(w2 + F(al2 * DT))
    w1, w2 = clamp_to(q1, MAX_W), clamp_to(q2, MAX_W)
    c1, s1 = rotate(c1, s1, w1)
    c2, s2 = rotate(c2, s2, w2)
    return (c1, s1, w1, c2, s2, w2), int(w1 != q1) + int(w2 != q2)


def tip_of(p):
    c1, s1, _, c2, s2, _ = p
    c12 = F(F(c1 * c2) - F(s1 * s2))
    s12 = F(F(s1 * c2) + F(c1 * s2))
    return F(F(F(0.5) * c1) + F(F(0.5) * c12)), F(F(F(0.5) * s1) + F(F(0.5) * s12))


def distance2(p, target):
    x, y = tip_of(p)
    dx, dy = F(x - target[0]), F(y - target[1])
    return F(F(dx * dx) + F(dy * dy))


def reward_of(p, target, radius, sparse):
    d2 = distance2(p, target)
    if sparse:
        return F(1) if d2 <= F(radius * radius) else F(0)
    return F(F(1) / F(F(1) + F(F(4) * d2)))


def reset_state(seed, e, ep, radius):
    """(phys, target) of episode ep of environment e"""
    c1, s1 = direction(draw(seed, e, ep, 0))
    c2, s2 = direction(draw(seed, e, ep, 1))
    gx, gy = direction(draw(seed, e, ep, 2))
    f = F(F(0.5) + F(draw(seed, e, ep, 3) * F(0.5)))
    rho = F(F(F(1) - radius) * f)
    return (c1, s1, F(0), c2, s2, F(0)), (F(rho * gx), F(rho * gy))


def _px(v):
    return int(np.floor(v))


def points(phys, target, radius):
    """the integer coordinates of a frame, each rounded once: elbow, tip, target centre, target radius"""
    c1, s1, _, c2, s2, _ = phys
    c12 = F(F(c1 * c2) - F(s1 * s2))
    s12 = F(F(s1 * c2) + F(c1 * s2))
    ax, ay = F(c1 * F(288)), F(s1 * F(288))
    EX, EY = _px(F(ax + F(672.5))), _px(F(F(672.5) - ay))
    TX, TY = _px(F(F(ax + F(c12 * F(288))) + F(672.5))), _px(F(F(672.5) - F(ay + F(s12 * F(288)))))
    GX, GY = _px(F(F(target[0] * F(576)) + F(672.5))), _px(F(F(672.5) - F(target[1] * F(576))))
    GR = _px(F(F(radius * F(576)) + F(0.5)))
    return EX, EY, TX, TY, GX, GY, GR


def disc(X, Y, r):
    return (_PX - X) ** 2 + (_PY - Y) ** 2 <= r * r


def render(phys, target, radius):
    """the frame of one state"""
    EX, EY, TX, TY, GX, GY, GR = points(phys, target, F(radius))
    frame = np.stack([BACKGROUND] * 3)
    for m, rgb in ((disc(GX, GY, GR), TARGET_RGB), (capsule(CENTRE, CENTRE, EX, EY, ARM_R), UPPER_RGB),
                   (capsule(EX, EY, TX, TY, ARM_R), FORE_RGB), (disc(TX, TY, TIP_R), TIP_RGB)):
        for ch in range(3):
            frame[ch][m] = rgb[ch]
    return frame


def quadrant(c, s):
    return (0 if c >= 0 else 1) if s >= 0 else (3 if c >= 0 else 2)


class ReacherOracle(S.SkeletonOracle):
    WORDS = (("phys", (6,), F), ("target", (2,), F))

    def __init__(self, num_envs, episode_length=1000, seed=0, repeat=1, target_radius=0.15, sparse=True, frames=True):
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.radius, self.sparse = F(target_radius), bool(sparse)
        # what a run met: sub-steps with and without reward, clamps of w, the quadrants either joint's vector was in
        self.rewarded = self.unrewarded = self.clamped = 0
        self.quadrants = (set(), set())

    def new_episode(self, e, ep):
        self.phys[e], self.target[e] = reset_state(self.seed, e, ep, self.radius)

    def sanitise(self, row):
        return sanitise(row[0]), sanitise(row[1])

    def frame(self, e):
        return render(self.phys[e], self.target[e], self.radius)

    def substep(self, e, a):
        p, cut = substep(tuple(self.phys[e]), *a)
        self.clamped += cut
        self.quadrants[0].add(quadrant(p[0], p[1]))
        self.quadrants[1].add(quadrant(p[3], p[4]))
        r = reward_of(p, tuple(self.target[e]), self.radius, self.sparse)
        self.rewarded += r > 0 if self.sparse else 0
        self.unrewarded += r == 0
        self.phys[e] = p
        return r, F(1), False


_SEEN = ("rewarded", "unrewarded", "clamped", "quadrants", "cut_by_limit", "full", "reset_rows")

# ---- the driven run the CPU and the GPU tests share ---------------------------------------------------------------
STEPS, EPISODE_LENGTH, SEED = 40, 7, 5
DRIVEN_RADIUS = 0.3         # the largest: in episodes of seven steps a fingertip is on the target only if it starts there
DRIVEN = tuple((N, A, k, sparse) for (N, A) in ((3, 2), (5, 4)) for k in (1, 2, 16) for sparse in (True, False))


def driven_run(N, A, repeat, sparse, seed=SEED, steps=STEPS, episode_length=EPISODE_LENGTH, frames=True):
    """the oracle driven for `steps` macro steps by S.wild_actions from the staggered reset (S.stagger): the actions it was
    given, everything it returned (the frames only if asked for) and the state after every step"""
    r = np.random.RandomState(seed * 100003 + N * 101 + A * 17 + repeat * 3 + int(sparse))
    o = ReacherOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, target_radius=DRIVEN_RADIUS, sparse=sparse,
                      frames=frames)
    o.reset()
    S.stagger(o)
    return S.record(o, steps, lambda s: S.wild_actions(r, N, A), _SEEN)


# The physics drive: in seven simulator steps from rest no joint leaves its quadrant and no velocity comes near the
# clamp.  These runs are one long episode: environments 0 and 1 are driven round from the reset state by torques that hold
# their sign (opposite signs in the two, both joints through all four quadrants); environments 2 and 3 start spinning at
# w = +-15.9 with the elbow at a right angle, where the centrifugal term throws w2 into the clamp in the first sub-step.
# "state0" holds the start; a user of the class writes it through load_state_dict().
PHYSICS_RADIUS = 0.15
PHYSICS = tuple((4, 2, 16, sparse, 60, 2000) for sparse in (True, False))         # N, A, repeat, sparse, steps, episode_length


def physics_actions(N, A, s):
    a = np.zeros((N, A), F)
    sign = np.where(np.arange(N) % 2 == 0, F(1), F(-1))
    a[:, 0] = sign * F(1.5)                                                     # beyond the clamp of the action
    a[:, 1] = sign * (F(1.25) if s < 40 else F(-0.75))                          # round one way, then back
    return a


def physics_run(N, A, repeat, sparse, steps, episode_length, seed=SEED, frames=True):
    o = ReacherOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, target_radius=PHYSICS_RADIUS, sparse=sparse,
                      frames=frames)
    o.reset()
    for e, sgn in ((2, F(1)), (3, F(-1))):
        o.phys[e] = (F(1), F(0), F(15.9) * sgn, F(0), -sgn, F(15.9) * sgn)
    return S.record(o, steps, lambda s: physics_actions(N, A, s), _SEEN)


def run(cfg, frames=True):
    """the run of a configuration of DRIVEN or PHYSICS"""
    return driven_run(*cfg, frames=frames) if len(cfg) == 4 else physics_run(*cfg, frames=frames)


# ---- the poses the frame is compared at: (phys, target, target_radius) ----------------------------------------------------
def _pose(c1, s1, c2, s2, target, radius):
    return np.array([c1, s1, 0.25, c2, s2, -0.5], F), np.array(target, F), radius      # the velocities are in no frame


_D = tuple(float(v) for v in normalise(F(0.6), F(0.8)))
POSES = (
    _pose(1, 0, 1, 0, (-0.5, 0.3), 0.15),           # stretched (c2 = 1) along +x: the tip touches the reach circle
    _pose(0, 1, 1, 0, (0.3, -0.5), 0.05),           # along +y
    _pose(-1, 0, 1, 0, (0.2, 0.6), 0.3),            # along -x, the largest target
    _pose(0, -1, 1, 0, (-0.6, -0.2), 0.02),         # along -y, the smallest
    _pose(1, 0, -1, 0, (0.4, 0.4), 0.15),           # folded back on itself (c2 = -1): the tip over the shoulder
    _pose(0, 1, 0, -1, (0.5, 0.5), 0.15),           # the fingertip over the target: the elbow bent to the right
    _pose(_D[0], _D[1], 0, 1, (0.12, 0.2), 0.15),   # the target partly under the upper arm
    _pose(_D[0], -_D[1], -_D[0], _D[1], (0.85, 0.0), 0.15),    # oblique capsules; the target's disc reaches the reach circle
)


# ---- the scripted controller: what makes the task solvable, and what K and B were chosen for ------------------------------
def joint_angles_for(target):
    """the joint angles (float64) that put the fingertip on `target`, elbow to the left: |target|^2 = 0.5 + 0.5 cos q2"""
    x, y = float(target[0]), float(target[1])
    q2 = np.arccos(np.clip(2.0 * (x * x + y * y) - 1.0, -1.0, 1.0))
    return np.arctan2(y, x) - 0.5 * q2, q2


def controller_action(p, goal, kp=4.0, kd=2.0):
    """a PD law on the joint angles: the float32 torques for the state p towards the joint angles `goal`"""
    out = []
    for (c, s, w), q in zip((p[0:3], p[3:6]), goal):
        err = np.arctan2(np.sin(q - np.arctan2(float(s), float(c))), np.cos(q - np.arctan2(float(s), float(c))))
        out.append(F(np.clip(kp * err - kd * float(w), -1.0, 1.0)))
    return out


def controlled_episode(seed, e, radius, steps=1000, controlled=True, sparse=True):
    """the return of episode 1 of environment e under the controller (or under zero action), and the first rewarded step"""
    p, target = reset_state(seed, e, 1, F(radius))
    goal = joint_angles_for(target)
    total, first = 0.0, None
    for i in range(steps):
        a1, a2 = controller_action(p, goal) if controlled else (F(0), F(0))
        p, _ = substep(p, a1, a2)
        r = reward_of(p, target, F(radius), sparse)
        total += float(r)
        if r > 0 and first is None:
            first = i
    return total, first


# ---- the argument lists drq_vec_reacher_step refuses: shared by the CPU and the GPU test ----------------------------------
def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_reacher_step must refuse, around one well-formed list over the four given base
    addresses (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     phys target     t           episode     over        N  A  action seed L repeat reset radius sparse frame
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, S0 + 0x400, 5, 2, ACT, 7, 9, 2, 0, 0.15, 1, FR,
          SC, SC + 0x100, SC + 0x200, SC + 0x300]                         # reward discount first substeps
    bad = S.refused_steps(ok, "w w w w b N A action - L repeat reset - - frame w w b w",
                          {12: (0.0199, 0.301, float("nan"), 0.0, -0.15, float("inf")), 13: (2, -1)})      # radius, sparse
    assert len(bad) == 11 + 22 + 3 + 8
    return bad


def refused_renders(S0, FR):
    """the argument lists drq_vec_reacher_render must refuse: (phys, target, N, target_radius, frame)"""
    return S.refused_reads([S0, S0 + 0x100, 3, 0.15, FR], "w w N - frame", {3: (0.0199, 0.301, float("nan"))})
