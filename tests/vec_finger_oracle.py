"""numpy restatement of the device environment's finger (a helper module: not collected).  The contract is the comment
of include/drqv2_hip.h ("device environment", "Finger"), stated here once more in float32, one rounding per operation in
the written order, and Python integers (exact, so wider than the contract's int64) for the capsules.  The hash and the
draws are those of tests/vec_env_oracle.py, direction() is the reacher's (tests/vec_reacher_oracle.py).  The rule is
written once, over float32 arrays of one value per environment: the skeleton oracle calls it with arrays of length 1, the
property tests of tests/test_cpu_vec_finger.py with many environments at once; numpy rounds every array operation
elementwise exactly as it rounds the scalar one.

  world      [-1, 1]^2, y up, no gravity.  The finger: the reacher's arm with links of 0.4 and 0.3 and unit point masses at
             the elbow and the tip, rooted at (0, 0.2); its tip is a disc of radius 0.06.  The spinner: a rod of length 0.3
             and radius 0.05 on a hinge at (0, -0.2), inertia 0.05.  Touching is a distance of 0.11 between the fingertip's
             centre and the rod's axis.  Only the fingertip collides; the links pass over everything.
  state      per environment e: phys[9] = (c1, s1, w1, c2, s2, w2, cs, ss, ws), target[2] (the unit vector of the target's
             angle) float32; t int32; episode uint32; over uint8
  geometry   c12 = c1 c2 - s1 s2; s12 = s1 c2 + c1 s2; f = (0.3 c12, 0.3 s12); tip - root: t = (0.4 c1 + fx, 0.4 s1 + fy);
             tip - hinge: q = (tx, ty + 0.4); u = clamp(qx cs + qy ss, 0, 0.3); r = (cs u, ss u); d = q - r; e2 = dx dx + dy dy;
             e2 == 0: e = 0, n = (0, 1); otherwise e = sqrt(e2), n = d / e.  j1 = ny tx - nx ty; j2 = ny fx - nx fy;
             js = rx ny - ry nx
  reset      (c1, s1) = direction(draw_0); (c2, s2) = direction(draw_1); (cs, ss) = direction(draw_2); every w = 0;
             geometry: e2 < 0.0169 (closer than 0.13): q.q >= 0.0169: (cs, ss) = normalise(-qx, -qy) (the rod points away from
             the fingertip); otherwise (c1, s1, c2, s2) = (0, 1, 1, 0) (the finger straight up).  v = draw_3;
             v' = v 0.75 + 0.225, or v 0.75 - 0.225 for v < 0; (ax, ay) = direction(v');
             target = normalise(cs ax - ss ay, ss ax + cs ay): at least 45 degrees from the rod
  sub-step   1 drive: M11 = 0.41 + 0.24 c2; M12 = 0.09 + 0.12 c2; h = 0.12 s2; cor = (2 w1) w2 + w2 w2;
               tau1 = (a1 2 - 0.5 w1) + h cor; tau2 = (a2 2 - 0.5 w2) - h (w1 w1); det = M11 0.09 - M12 M12;
               al1 = (0.09 tau1 - M12 tau2) / det; al2 = (M11 tau2 - M12 tau1) / det; w1 = clamp(w1 + al1 0.01, 6);
               w2 = clamp(w2 + al2 0.01, 6); ws = ws 0.97
             2 impulse, at the positions as they are: geometry; e2 < 0.0441: g = max(e - 0.11, 0); lim = -(g 100);
               vn = (j1 w1 + j2 w2) - js ws; u1 = (0.09 j1 - M12 j2) / det; u2 = (M11 j2 - M12 j1) / det;
               den = (j1 u1 + j2 u2) + (js js) 20; vn < lim and den > 0: lam = (lim - vn) / den; w1 = w1 + u1 lam;
               w2 = w2 + u2 lam; ws = ws - (js 20) lam
             3 clamps: w1, w2 to 6, ws to 10
             4 advance: rotate(c1, s1, w1 0.01); rotate(c2, s2, w2 0.01); rotate(cs, ss, ws 0.01), with
               rotate(c, s, k): k == 0: unchanged; otherwise normalise(c - s k, s + c k)
             5 separation, at the new positions: geometry; e2 < 0.0121: den = (j1 j1) 2.5 + (js js) 20; den >= 0.01:
               mu = (0.11 - e) / den; rotate(c1, s1, (j1 2.5) mu); rotate(cs, ss, -((js 20) mu))
  reward     mode 0: sparse ws >= 2 ? 1 : 0; dense clamp(ws / 2, 0, 1).  mode 1: dx = 0.3 cs - 0.3 gx; dy = 0.3 ss - 0.3 gy;
             d2 = dx dx + dy dy; sparse d2 <= radius radius ? 1 : 0; dense 1 / (1 + 4 d2)
  macro step the skeleton's (tests/vec_skeleton_oracle.py); a1, a2 = action[e, 0:2] sanitised once; d_i = 1, and the task
             never ends an episode
  frame      in 1/16 pixel, 672 to the unit, the world's origin at (672, 672), y upwards (render below)
"""
import numpy as np

from tests import vec_skeleton_oracle as S
from tests.vec_cartpole_oracle import capsule
from tests.vec_env_oracle import BACKGROUND, F, SIDE, draw
from tests.vec_reacher_oracle import direction
from tests.vec_skeleton_oracle import sanitise

L1, L2, LS = F(0.4), F(0.3), F(0.3)
ROOT_Y, HINGE_Y, DROP = F(0.2), F(-0.2), F(0.4)            # the root above the hinge by DROP
TIP_RADIUS, ROD_RADIUS = 0.06, 0.05
TOUCH, TOUCH2, NEAR2, CLEAR2 = F(0.11), F(0.0121), F(0.0441), F(0.0169)
SKIN = 0.011                                               # a tenth of TOUCH: the most a sub-step may leave the tip inside
K, B, DT = F(2), F(0.5), F(0.01)
MAX_W, MAX_WS = F(6), F(10)
INV_I, INV_A, KEEP, MIN_DEN = F(20), F(2.5), F(0.97), F(0.01)
INERTIA = 0.05
SPIN_SPEED, TURN_EASY_RADIUS, TURN_HARD_RADIUS = 2.0, 0.1, 0.04
MIN_RADIUS, MAX_RADIUS = 0.02, 0.2
ROOT_PY, HINGE_PY, CENTRE = 538, 806, 672
LINK_R, TIP_R, ROD_R, HINGE_R = 20, 40, 34, 44
TARGET_RGB, HINGE_RGB, ROD_RGB, END_RGB = (64, 255, 64), (64, 64, 255), (255, 64, 255), (64, 64, 255)
UPPER_RGB, FORE_RGB, TIP_RGB = (255, 64, 64), (64, 255, 255), (255, 255, 64)
_II, _JJ = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
_PX, _PY = (16 * _JJ + 8).astype(np.int64), (16 * _II + 8).astype(np.int64)

EVENTS = ("side", "cap", "hinge_end", "degenerate", "impulse", "separation", "separation_skipped", "clamp_w1", "clamp_w2",
          "clamp_ws", "spinner_rest", "spin_0", "spin_1", "spin_dense_inside", "turn_inside", "turn_outside")


# ---- the rule over arrays -------------------------------------------------------------------------------------------------
def _where(m, a, b):
    return np.where(m, a, b).astype(F)


def clamp_many(v, m):
    return _where(v < -m, -m, _where(v > m, m, v))


def exact_square_many(a):
    t = a * F(4097)
    hi = t - (t - a)
    lo = a - hi
    p = a * a
    q = hi * lo
    return p, ((hi * hi - p) + (q + q)) + lo * lo


def normalise_many(c, s):
    """tests/vec_cartpole_oracle.normalise, elementwise"""
    n = np.sqrt(c * c + s * s)
    c, s = c / n, s / n
    (pc, ec), (ps, es) = exact_square_many(c), exact_square_many(s)
    d = _where(pc >= ps, (F(1) - pc) - ps, (F(1) - ps) - pc)
    d = d - (ec + es)
    g = d * F(0.5)
    return c + c * g, s + s * g


def rotate_many(c, s, k):
    """(c, s) turned by k; k == 0 keeps the vector to the bit"""
    with np.errstate(all="ignore"):
        nc, ns = normalise_many(c - s * k, s + c * k)
    still = k == 0
    return _where(still, c, nc), _where(still, s, ns)


def geometry(p):
    """what the impulse and the separation read of the positions of p [n, 9]: a dict of float32 [n] arrays"""
    c1, s1, c2, s2, cs, ss = p[:, 0], p[:, 1], p[:, 3], p[:, 4], p[:, 6], p[:, 7]
    c12 = c1 * c2 - s1 * s2
    s12 = s1 * c2 + c1 * s2
    fx, fy = L2 * c12, L2 * s12
    tx, ty = L1 * c1 + fx, L1 * s1 + fy
    qx, qy = tx, ty + DROP
    proj = qx * cs + qy * ss
    u = _where(proj < 0, F(0), _where(proj > LS, LS, proj))
    rx, ry = cs * u, ss * u
    dx, dy = qx - rx, qy - ry
    e2 = dx * dx + dy * dy
    zero = e2 == 0
    with np.errstate(all="ignore"):
        e = _where(zero, F(0), np.sqrt(e2))
        nx, ny = _where(zero, F(0), dx / e), _where(zero, F(1), dy / e)
    return dict(fx=fx, fy=fy, tx=tx, ty=ty, qx=qx, qy=qy, proj=proj, u=u, rx=rx, ry=ry, e2=e2, e=e, nx=nx, ny=ny, zero=zero,
                j1=ny * tx - nx * ty, j2=ny * fx - nx * fy, js=rx * ny - ry * nx)


def _count(events, name, mask):
    if events is not None:
        events[name] += int(np.count_nonzero(mask))


def _where_it_touches(events, g, mask):
    _count(events, "hinge_end", mask & (g["proj"] <= 0))
    _count(events, "cap", mask & (g["proj"] >= LS))
    _count(events, "side", mask & (g["proj"] > 0) & (g["proj"] < LS))


def substep_many(p, a, events=None, trace=None):
    """one simulator step of the states p [n, 9] under the sanitised actions a [n, 2] -> the new states.  events: a dict of
    counters to add to.  trace: a dict that receives the states around the two contact parts ("before_impulse",
    "after_impulse", "before_separation", "after_separation") and the masks "impulse" and "separation" """
    with np.errstate(all="ignore"):                      # the branch not taken divides by zero here and there
        return _substep_many(np.array(p, F), a, events, trace)


def _substep_many(p, a, events, trace):
    c1, s1, w1, c2, s2, w2, cs, ss, ws = (p[:, k].copy() for k in range(9))
    a1, a2 = a[:, 0], a[:, 1]
    rest = ws == 0
    # 1 drive
    m11 = F(0.41) + F(0.24) * c2
    m12 = F(0.09) + F(0.12) * c2
    h = F(0.12) * s2
    cor = (F(2) * w1) * w2 + w2 * w2
    tau1 = (a1 * K - B * w1) + h * cor
    tau2 = (a2 * K - B * w2) - h * (w1 * w1)
    det = m11 * F(0.09) - m12 * m12
    al1 = (F(0.09) * tau1 - m12 * tau2) / det
    al2 = (m11 * tau2 - m12 * tau1) / det
    q1, q2 = w1 + al1 * DT, w2 + al2 * DT
    w1, w2 = clamp_many(q1, MAX_W), clamp_many(q2, MAX_W)
    cut1, cut2 = w1 != q1, w2 != q2
    ws = ws * KEEP
    # 2 the impulse
    g = geometry(p)
    near = g["e2"] < NEAR2
    gap = g["e"] - TOUCH
    lim = -(_where(gap < 0, F(0), gap) * F(100))
    vn = (g["j1"] * w1 + g["j2"] * w2) - g["js"] * ws
    u1 = (F(0.09) * g["j1"] - m12 * g["j2"]) / det
    u2 = (m11 * g["j2"] - m12 * g["j1"]) / det
    den = (g["j1"] * u1 + g["j2"] * u2) + (g["js"] * g["js"]) * INV_I
    hit = near & (vn < lim) & (den > 0)
    with np.errstate(all="ignore"):
        lam = (lim - vn) / den
    if trace is not None:
        trace["before_impulse"] = np.stack([c1, s1, w1, c2, s2, w2, cs, ss, ws], 1)
    w1 = _where(hit, w1 + u1 * lam, w1)
    w2 = _where(hit, w2 + u2 * lam, w2)
    ws = _where(hit, ws - (g["js"] * INV_I) * lam, ws)
    if trace is not None:
        trace["after_impulse"], trace["impulse"] = np.stack([c1, s1, w1, c2, s2, w2, cs, ss, ws], 1), hit
    _count(events, "impulse", hit)
    _where_it_touches(events, g, hit)
    _count(events, "degenerate", near & g["zero"])
    # 3 the clamps
    q1, q2, q3 = w1, w2, ws
    w1, w2, ws = clamp_many(q1, MAX_W), clamp_many(q2, MAX_W), clamp_many(q3, MAX_WS)
    _count(events, "clamp_w1", cut1 | (w1 != q1))
    _count(events, "clamp_w2", cut2 | (w2 != q2))
    _count(events, "clamp_ws", ws != q3)
    # 4 the advance
    c1, s1 = rotate_many(c1, s1, w1 * DT)
    c2, s2 = rotate_many(c2, s2, w2 * DT)
    ncs, nss = rotate_many(cs, ss, ws * DT)
    _count(events, "spinner_rest", rest & (ws == 0) & (ncs.view(np.uint32) == cs.view(np.uint32)) & (nss.view(np.uint32) == ss.view(np.uint32)) & ~near)
    cs, ss = ncs, nss
    # 5 the separation
    new = np.stack([c1, s1, w1, c2, s2, w2, cs, ss, ws], 1)
    g = geometry(new)
    inside = g["e2"] < TOUCH2
    den = (g["j1"] * g["j1"]) * INV_A + (g["js"] * g["js"]) * INV_I
    apart = inside & (den >= MIN_DEN)
    with np.errstate(all="ignore"):
        mu = (TOUCH - g["e"]) / den
    k1 = _where(apart, (g["j1"] * INV_A) * mu, F(0))
    ks = _where(apart, -((g["js"] * INV_I) * mu), F(0))
    c1, s1 = rotate_many(c1, s1, k1)
    cs, ss = rotate_many(cs, ss, ks)
    out = np.stack([c1, s1, w1, c2, s2, w2, cs, ss, ws], 1)
    if trace is not None:
        trace["before_separation"], trace["after_separation"], trace["separation"] = new, out, apart
    _count(events, "separation", apart)
    _count(events, "separation_skipped", inside & ~apart)
    _where_it_touches(events, g, inside)
    _count(events, "degenerate", inside & g["zero"])
    return out


def distance2_many(p, target):
    dx = LS * p[:, 6] - LS * target[:, 0]
    dy = LS * p[:, 7] - LS * target[:, 1]
    return dx * dx + dy * dy


def reward_many(p, target, mode, radius, sparse):
    if mode == 0:
        ws = p[:, 8]
        if sparse:
            return _where(ws >= F(SPIN_SPEED), F(1), F(0))
        v = ws / F(SPIN_SPEED)
        return _where(v < 0, F(0), _where(v > 1, F(1), v))
    d2 = distance2_many(p, target)
    if sparse:
        return _where(d2 <= F(radius) * F(radius), F(1), F(0))
    return F(1) / (F(1) + F(4) * d2)


def gap_many(p):
    """float64: the distance of the fingertip's centre from the rod's axis (the segment hinge -- tip), and on which side"""
    p = np.asarray(p, np.float64)
    c12, s12 = p[:, 0] * p[:, 3] - p[:, 1] * p[:, 4], p[:, 1] * p[:, 3] + p[:, 0] * p[:, 4]
    qx, qy = 0.4 * p[:, 0] + 0.3 * c12, 0.4 * p[:, 1] + 0.3 * s12 + 0.4
    proj = qx * p[:, 6] + qy * p[:, 7]
    u = np.clip(proj, 0, 0.3)
    return np.hypot(qx - p[:, 6] * u, qy - p[:, 7] * u), np.sign(p[:, 6] * qy - p[:, 7] * qx), proj


def energy_many(p):
    """float64: 0.5 w^T M w + 0.5 I ws^2"""
    p = np.asarray(p, np.float64)
    m11, m12 = 0.41 + 0.24 * p[:, 3], 0.09 + 0.12 * p[:, 3]
    return 0.5 * (m11 * p[:, 2] ** 2 + 2 * m12 * p[:, 2] * p[:, 5] + 0.09 * p[:, 5] ** 2) + 0.5 * INERTIA * p[:, 8] ** 2


# ---- the reset --------------------------------------------------------------------------------------------------------
def reset_state(seed, e, ep, counts=None):
    """(phys, target) of episode ep of environment e; counts: a dict whose "away" / "upright" count the two shifts"""
    c1, s1 = direction(draw(seed, e, ep, 0))
    c2, s2 = direction(draw(seed, e, ep, 1))
    cs, ss = direction(draw(seed, e, ep, 2))
    g = geometry(np.array([[c1, s1, 0, c2, s2, 0, cs, ss, 0]], F))
    if g["e2"][0] < CLEAR2:
        qx, qy = g["qx"][0], g["qy"][0]
        if F(F(qx * qx) + F(qy * qy)) >= CLEAR2:
            cs, ss = (v[0] for v in normalise_many(np.array([-qx], F), np.array([-qy], F)))
            if counts is not None:
                counts["away"] += 1
        else:
            c1, s1, c2, s2 = F(0), F(1), F(1), F(0)
            if counts is not None:
                counts["upright"] += 1
    v = draw(seed, e, ep, 3)
    v = F(F(v * F(0.75)) - F(0.225)) if v < 0 else F(F(v * F(0.75)) + F(0.225))
    ax, ay = direction(v)
    gx, gy = normalise_many(np.array([F(F(cs * ax) - F(ss * ay))], F), np.array([F(F(ss * ax) + F(cs * ay))], F))
    return np.array([c1, s1, 0, c2, s2, 0, cs, ss, 0], F), np.array([gx[0], gy[0]], F)


def reset_states(seed, envs, ep=1):
    both = [reset_state(seed, e, ep) for e in envs]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


# ---- the frame ----------------------------------------------------------------------------------------------------------
def _px(v):
    return int(np.floor(v))


def points(phys, target, radius):
    """the integer coordinates of a frame, each rounded once: elbow, tip, the spinner's tip, the target's centre and radius"""
    c1, s1, _, c2, s2, _, cs, ss, _ = (F(v) for v in phys)
    c12 = F(F(c1 * c2) - F(s1 * s2))
    s12 = F(F(s1 * c2) + F(c1 * s2))
    ax, ay = F(c1 * F(268.8)), F(s1 * F(268.8))
    EX, EY = _px(F(ax + F(672.5))), _px(F(F(672.5) - F(ay + F(134.4))))
    TX = _px(F(F(ax + F(c12 * F(201.6))) + F(672.5)))
    TY = _px(F(F(672.5) - F(F(ay + F(s12 * F(201.6))) + F(134.4))))
    SX, SY = _px(F(F(cs * F(201.6)) + F(672.5))), _px(F(F(672.5) - F(F(ss * F(201.6)) - F(134.4))))
    GX = _px(F(F(F(target[0]) * F(201.6)) + F(672.5)))
    GY = _px(F(F(672.5) - F(F(F(target[1]) * F(201.6)) - F(134.4))))
    GR = _px(F(F(F(radius) * F(672)) + F(0.5)))
    return EX, EY, TX, TY, SX, SY, GX, GY, GR


def disc(X, Y, r):
    return (_PX - X) ** 2 + (_PY - Y) ** 2 <= r * r


def masks(pose):
    """(mask, colour) of every shape of the pose (phys, target, mode, radius), in the draw order"""
    phys, target, mode, radius = pose
    EX, EY, TX, TY, SX, SY, GX, GY, GR = points(phys, target, radius)
    out = [(disc(GX, GY, GR), TARGET_RGB)] if mode == 1 else []
    return out + [(disc(CENTRE, HINGE_PY, HINGE_R), HINGE_RGB), (capsule(CENTRE, HINGE_PY, SX, SY, ROD_R), ROD_RGB),
                  (disc(SX, SY, ROD_R), END_RGB), (capsule(CENTRE, ROOT_PY, EX, EY, LINK_R), UPPER_RGB),
                  (capsule(EX, EY, TX, TY, LINK_R), FORE_RGB), (disc(TX, TY, TIP_R), TIP_RGB)]


def render(pose):
    """the frame of one pose (phys, target, mode, radius)"""
    frame = np.stack([BACKGROUND] * 3)
    for m, rgb in masks(pose):
        for ch in range(3):
            frame[ch][m] = rgb[ch]
    return frame


# ---- the oracle -----------------------------------------------------------------------------------------------------------
class FingerOracle(S.SkeletonOracle):
    WORDS = (("phys", (9,), F), ("target", (2,), F))

    def __init__(self, num_envs, episode_length=1000, seed=0, repeat=1, mode=0, target_radius=TURN_EASY_RADIUS, sparse=True,
                 frames=True):
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.mode, self.radius, self.sparse = int(mode), F(target_radius), bool(sparse)
        self.events = dict.fromkeys(EVENTS, 0)

    def new_episode(self, e, ep):
        self.phys[e], self.target[e] = reset_state(self.seed, e, ep)

    def sanitise(self, row):
        return np.array([[sanitise(row[0]), sanitise(row[1])]], F)

    def frame(self, e):
        return render((self.phys[e], self.target[e], self.mode, self.radius))

    def substep(self, e, a):
        p = substep_many(self.phys[e:e + 1], a, self.events)
        self.phys[e] = p[0]
        ev, tg = self.events, self.target[e:e + 1]
        if self.mode == 0:                                   # what the reward met, whichever form is paid
            ws = p[0, 8]
            ev["spin_1"] += ws >= F(SPIN_SPEED)
            ev["spin_0"] += ws < F(SPIN_SPEED)
            ev["spin_dense_inside"] += F(0) < F(ws / F(SPIN_SPEED)) < F(1)
        else:
            inside = distance2_many(p, tg)[0] <= F(self.radius * self.radius)
            ev["turn_inside"] += inside
            ev["turn_outside"] += not inside
        return reward_many(p, tg, self.mode, self.radius, self.sparse)[0], F(1), False


_SEEN = ("events", "cut_by_limit", "full", "reset_rows")

# ---- the driven run the CPU and the GPU tests share ---------------------------------------------------------------
STEPS, EPISODE_LENGTH, SEED = 40, 7, 5
CUT = 9                      # macro steps of the spin physics run after which environment 0 is in contact and in motion
#                  N, A, repeat, mode, radius, sparse
DRIVEN = tuple((N, A, k, mode, TURN_EASY_RADIUS, sparse) for (N, A) in ((3, 2), (5, 4)) for k in (1, 2, 16) for mode in (0, 1)
               for sparse in (True, False))


def driven_run(N, A, repeat, mode, radius, sparse, seed=SEED, steps=STEPS, episode_length=EPISODE_LENGTH, frames=True):
    """the oracle driven for `steps` macro steps by S.wild_actions from the staggered reset (S.stagger)"""
    r = np.random.RandomState(seed * 100003 + N * 101 + A * 17 + repeat * 3 + 2 * mode + int(sparse))
    o = FingerOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, mode=mode, target_radius=radius, sparse=sparse,
                     frames=frames)
    o.reset()
    S.stagger(o)
    return S.record(o, steps, lambda s: S.wild_actions(r, N, A), _SEEN)


# The physics drive: seven steps from rest meet no contact.  These runs are one long episode of five hand-set environments:
#   0  the fingertip beside a rod that points up, driven by flick(): contacts on the rod's side, the spin reward 0, inside
#      and 1
#   1  the fingertip beyond the tip of a rod that points along +x, pulled towards the hinge along the rod's axis: the cap;
#      then flick()
#   2  the finger folded with its tip's centre exactly on the axis of a rod that points up: the degenerate normal, with no
#      lever at all (the separation is skipped); then the elbow is driven to and fro
#   3  the shoulder thrown into its clamp by the centrifugal term; the elbow and the rod, handed over faster than their
#      clamps, cut
#      to them; then the fingertip is pulled to a point behind the hinge: the hinge end
#   4  a reset pose under the zero action for the first 20 macro steps (the rod untouched and at rest), then turn_to()
# "state0" holds the start; a user of the class writes it through load_state_dict().
PHYSICS_RADIUS = TURN_EASY_RADIUS
#           N, A, repeat, mode, radius, sparse, steps, episode_length
PHYSICS = ((5, 2, 16, 0, PHYSICS_RADIUS, True, 60, 2000), (5, 2, 16, 1, PHYSICS_RADIUS, False, 60, 2000))


def _unit(angle):
    c, s = normalise_many(np.array([np.cos(angle)], F), np.array([np.sin(angle)], F))
    return c[0], s[0]


def _pose_for(tip, bend, w=(0.0, 0.0)):
    """(c1, s1, w1, c2, s2, w2) that put the tip at `tip` relative to the root, the elbow bent to the side `bend`"""
    x, y = tip
    q2 = bend * np.arccos(np.clip((x * x + y * y - 0.25) / 0.24, -1, 1))
    q1 = np.arctan2(y, x) - np.arctan2(0.3 * np.sin(q2), 0.4 + 0.3 * np.cos(q2))
    return _unit(q1) + (w[0],) + _unit(q2) + (w[1],)


def physics_start():
    """the hand-set states of environments 0 .. 3 (4 keeps its reset): phys rows"""
    return np.array([_pose_for((-0.125, 0.15 - 0.4), 1) + (0, 1, 0),
                     _pose_for((0.3 + 0.125, 0.02 - 0.4), -1) + (1, 0, 0),
                     (0, -1, 0, -1, 0, 0, 0, 1, 0),
                     (1, 0, 5.9, 0, 1, 9, -1, 0, 12)], F)


def physics_actions(o, A, s):
    a = np.zeros((o.N, A), F)
    a[0] = flick(o.phys[0])
    a[1] = _towards(o.phys[1], (0.0, 0.0)) if s < 20 else flick(o.phys[1])
    a[2] = (F(0), F(1.5)) if s % 20 < 10 else (F(0), F(-1))
    a[3] = (F(1.5), F(1.5)) if s < 10 else _towards(o.phys[3], (-0.05 * o.phys[3, 6], -0.05 * o.phys[3, 7]))
    a[4] = (F(0), F(0)) if s < 20 else turn_to(o.phys[4], o.target[4])
    return a


def physics_run(N, A, repeat, mode, radius, sparse, steps, episode_length, seed=SEED, frames=True):
    o = FingerOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, mode=mode, target_radius=radius, sparse=sparse,
                     frames=frames)
    o.reset()
    o.phys[:4] = physics_start()
    return S.record(o, steps, lambda s: physics_actions(o, A, s), _SEEN)


def run(cfg, frames=True):
    """the run of a configuration of DRIVEN or PHYSICS"""
    return driven_run(*cfg, frames=frames) if len(cfg) == 6 else physics_run(*cfg, frames=frames)


# ---- the poses the frame is compared at: (phys, target, mode, target_radius) ------------------------------------------------
def _pose(c1, s1, c2, s2, cs, ss, target, mode, radius):
    return np.array([c1, s1, 0.25, c2, s2, -0.5, cs, ss, 2.0], F), np.array(target, F), mode, radius   # no velocity is in a frame


_D = tuple(float(v[0]) for v in normalise_many(np.array([0.6], F), np.array([0.8], F)))
_OVER_HINGE = _pose_for((0.0, -0.4), 1)         # the fingertip over the hinge
_OVER_END = _pose_for((0.3, -0.4), -1)          # the fingertip over the tip of a spinner that points along +x
POSES = (
    _pose(1, 0, 1, 0, 0, 1, (1, 0), 0, 0.1),                # the finger horizontal along +x, the spinner up; spin: no target
    _pose(0, 1, 1, 0, 1, 0, (0, -1), 1, MIN_RADIUS),        # the finger vertical, the spinner along +x, the smallest target
    _pose(-1, 0, 0, 1, 0, -1, (-1, 0), 1, MAX_RADIUS),      # upper link along -x, forearm vertical; spinner down; the largest
    _pose(0, -1, 0, 1, -1, 0, (0, 1), 1, 0.1),              # upper link down over the spinner's hinge side, spinner along -x
    _pose(_OVER_HINGE[0], _OVER_HINGE[1], _OVER_HINGE[3], _OVER_HINGE[4], _D[0], _D[1], (_D[0], _D[1]), 1, 0.1),
    _pose(_OVER_END[0], _OVER_END[1], _OVER_END[3], _OVER_END[4], 1, 0, (_D[0], -_D[1]), 1, 0.1),
    _pose(0, 0, 1, 0, 0, 0, (0, 0), 1, 0.1),                # zero-length projected segments: upper link, rod, target at the hinge
    _pose(_D[0], -_D[1], -_D[0], _D[1], -_D[0], _D[1], (-_D[0], _D[1]), 1, 0.04),      # oblique; the target under the spinner's tip
)


# ---- the scripted controllers: what makes the task solvable, and what the constants were chosen for ------------------------
ORBIT, LEAD, KP, KD = 0.18, 1.3, 40.0, 0.6
TURN_LEAD, TURN_KD, CATCH_UP, COAST, SPEED_CAP = 0.4, 0.6, 1.0, 2.4, 3.0


def _towards(p, point, kd=KD):
    """the float32 torques of a PD law that pulls the fingertip towards `point` (relative to the hinge): J^T of the error"""
    p = np.asarray(p, np.float64)
    c12, s12 = p[0] * p[3] - p[1] * p[4], p[1] * p[3] + p[0] * p[4]
    fx, fy = 0.3 * c12, 0.3 * s12
    tx, ty = 0.4 * p[0] + fx, 0.4 * p[1] + fy
    ex, ey = point[0] - tx, point[1] - (ty + 0.4)
    t1, t2 = -ty * ex + tx * ey, -fy * ex + fx * ey
    unfold = 0.5 * (1.0 if p[4] >= 0 else -1.0) * (1.0 if p[3] < 0 else -1.0) if abs(p[4]) < 0.3 else 0.0      # away from the singular elbow
    return np.array([np.clip(KP * t1 - kd * p[2], -1, 1), np.clip(KP * t2 - kd * p[5] + unfold, -1, 1)], F)


def _finger_angle(p):
    p = np.asarray(p, np.float64)
    c12, s12 = p[0] * p[3] - p[1] * p[4], p[1] * p[3] + p[0] * p[4]
    return np.arctan2(0.4 * p[1] + 0.3 * s12 + 0.4, 0.4 * p[0] + 0.3 * c12)


def flick(p, lead=LEAD):
    """spin: the fingertip circles the hinge anticlockwise at a radius of ORBIT, `lead` radians ahead of where it is, and
    sweeps the rod along with it"""
    phi = _finger_angle(p) + lead
    return _towards(p, (ORBIT * np.cos(phi), ORBIT * np.sin(phi)))


def turn_to(p, target, hold=0.03):
    """turn: the fingertip circles anticlockwise behind the rod and pushes it no faster than the rod can coast to a stop
    in the angle it has left (2.4 rad/s per radian, at most 3); it waits while the rod is faster than that, and stays where
    it is once the rod is at the target's angle"""
    theta, goal, phi = np.arctan2(float(p[7]), float(p[6])), np.arctan2(float(target[1]), float(target[0])), _finger_angle(p)
    left = (goal - theta + hold) % (2 * np.pi) - hold                # what the rod has left to turn, anticlockwise
    behind = (theta - phi) % (2 * np.pi)                             # how far the finger is behind the rod
    touching = np.arcsin(min(1.0, 0.11 / ORBIT))
    wanted = min(SPEED_CAP, COAST * left)
    if left <= hold or float(p[8]) > wanted:
        lead = 0.0
    else:
        lead = min(LEAD, TURN_LEAD * wanted + CATCH_UP * max(0.0, behind - touching - 0.05))
    phi += lead
    return _towards(p, (ORBIT * np.cos(phi), ORBIT * np.sin(phi)), kd=TURN_KD)


def episode_returns(seed, envs, mode, radius, policy, steps=1000, sparse=True):
    """the returns of episode 1 of the environments `envs` over `steps` simulator steps under policy(phys, target, s) ->
    float32 [n, 2] actions"""
    phys, target = reset_states(seed, envs)
    total = np.zeros(len(phys))
    for s in range(steps):
        phys = substep_many(phys, policy(phys, target, s))
        total += reward_many(phys, target, mode, radius, sparse)
    return total


def scripted(mode):
    if mode == 0:
        return lambda phys, target, s: np.stack([flick(p) for p in phys])
    return lambda phys, target, s: np.stack([turn_to(p, g) for p, g in zip(phys, target)])


# ---- the argument lists drq_vec_finger_step refuses: shared by the CPU and the GPU test ------------------------------------
_BAD_RADIUS = (0.0199, 0.201, float("nan"), 0.0, -0.1, float("inf"))


def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_finger_step must refuse, around one well-formed list over the four given base addresses
    (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     phys target     t           episode     over        N  A  action seed L repeat reset mode radius sparse frame
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, S0 + 0x400, 5, 2, ACT, 7, 9, 2, 0, 1, 0.1, 1, FR,
          SC, SC + 0x100, SC + 0x200, SC + 0x300]                         # reward discount first substeps
    bad = S.refused_steps(ok, "w w w w b N A action - L repeat reset - - - frame w w b w",
                          {12: (2, -1), 13: _BAD_RADIUS, 14: (2, -1)})      # mode, radius, sparse
    assert len(bad) == 11 + 24 + 3 + 8
    return bad


def refused_renders(S0, FR):
    """the argument lists drq_vec_finger_render must refuse: (phys, target, N, mode, target_radius, frame)"""
    return S.refused_reads([S0, S0 + 0x100, 3, 1, 0.1, FR], "w w N - - frame", {3: (2, -1), 4: _BAD_RADIUS[:3]})
