"""numpy restatement of the device environment's cartpole (a helper module: not collected).  The contract is the comment
of include/drqv2_hip.h ("device environment", "Cartpole"), stated here once more with float32 scalars, one rounding per
operation in the written order, and Python integers (exact, so wider than the contract's int64) for the capsule.  The
hash and the draws are those of tests/vec_env_oracle.py.

  state      per environment e: phys[5] = (x, xdot, c, s, omega) float32; t int32; episode uint32; over uint8
  normalise  n = sqrt(c c + s s); c = c / n; s = s / n; then one correction by the exact defect of the length:
             split(a): t = a 4097; hi = t - (t - a); lo = a - hi.  square(a): p = a a; q = hi lo;
             err = ((hi hi - p) + (q + q)) + lo lo.  (pc, ec) = square(c); (ps, es) = square(s);
             d = (1 - pc) - ps if pc >= ps else (1 - ps) - pc; d = d - (ec + es); g = d 0.5; c = c + c g; s = s + s g
  reset      episode += 1, t = 0, over = 0; x = draw_0 * 0.1; xdot = omega = 0; c = -1 (swing-up) or 1 (balance);
             s = draw_1 * 0.05; normalise.  first = 1, reward = 0, discount = 1, substeps = 0; the action is not read
  sub-step   F = a * 10; t1 = omega omega; t1 = 0.05 t1; t1 = t1 s; temp = (F + t1) / 1.1; num = 9.8 s - c temp;
             q = c c; q = 0.1 q; q = q / 1.1; den = 1.3333334 - q; den = 0.5 den; thacc = num / den;
             r = 0.05 thacc; r = r c; r = r / 1.1; xacc = temp - r;
             omega = clamp(omega + thacc 0.01, 32); xdot = clamp(xdot + xacc 0.01, 16); p = x + xdot 0.01; beyond +-1.8 the
             rail end: x = +-1.8, xdot = 0; h = omega 0.01; (c, s) = normalise(c - s h, s + c h); t += 1; over at the limit
  reward     up = (c + 1) 0.5; ce = (1 + 1 / (1 + x x)) 0.5; co = (4 + (1 - a a)) / 5; w = omega / 5;
             sl = (1 + 1 / (1 + w w)) 0.5; r = ((up ce) co) sl
  macro step the skeleton's (tests/vec_skeleton_oracle.py); a = action[e, 0] sanitised once (NaN -> 0, clamp to [-1, 1]);
             d_i = 1, and the task never ends an episode
  frame      in 1/16 pixel, pixel (i, j) centred at (16 j + 8, 16 i + 8): X0 = floor(x 320 + 672.5), X1 = floor((x 320 + s 320)
             + 672.5), Y1 = floor(672.5 - c 320); background, rail, cart, the pole's capsule of radius 24 (render below)
"""
import numpy as np

from tests import vec_skeleton_oracle as S
from tests.vec_env_oracle import BACKGROUND, F, SIDE, clamp1, draw  # noqa: F401  (clamp1: for the property tests)

RAIL, MAX_XDOT, MAX_OMEGA = F(1.8), F(16), F(32)
DT = F(0.01)
CENTRE, RAIL_ROW, RAIL_HALF, CART_HALF_W, CART_HALF_H, POLE_R = 672, 42, 576, 96, 48, 24
POLE_RGB, CART_RGB, RAIL_RGB = (255, 64, 64), (64, 255, 64), (64, 64, 255)
_II, _JJ = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
_PX, _PY = (16 * _JJ + 8).astype(np.int64), (16 * _II + 8).astype(np.int64)


def clamp_to(v, m):
    if v < -m:
        return F(-m)
    if v > m:
        return m
    return F(v)


def exact_square(a):
    """(p, err) with p + err = a * a exactly: Veltkamp's split, Dekker's error term, in +, - and * alone"""
    t = F(a * F(4097))
    hi = F(t - F(t - a))
    lo = F(a - hi)
    p = F(a * a)
    q = F(hi * lo)
    err = F(F(F(F(hi * hi) - p) + F(q + q)) + F(lo * lo))
    return p, err


def normalise(c, s):
    n = np.sqrt(F(F(c * c) + F(s * s)))
    c, s = F(c / n), F(s / n)
    (pc, ec), (ps, es) = exact_square(c), exact_square(s)
    d = F(F(F(1) - pc) - ps) if pc >= ps else F(F(F(1) - ps) - pc)
    d = F(d - F(ec + es))
    g = F(d * F(0.5))
    return F(c + F(c * g)), F(s + F(s * g))


def substep(p, a):
    """one simulator step of the state p = (x, xdot, c, s, omega), float32 scalars, under the sanitised action a"""
    x, xdot, c, s, omega = p
    force = F(a * F(10))
    t1 = F(omega * omega)
    t1 = F(F(0.05) * t1)
    t1 = F(t1 * s)
    temp = F(F(force + t1) / F(1.1))
    num = F(F(F(9.8) * s) - F(c * temp))
    q = F(c * c)
    q = F(F(0.1) * q)
    q = F(q / F(1.1))
    den = F(F(1.3333334) - q)
    den = F(F(0.5) * den)
    thacc = F(num / den)
    r = F(F(0.05) * thacc)
    r = F(r * c)
    r = F(r / F(1.1))
    xacc = F(temp - r)
    omega = clamp_to(F(omega + F(thacc * DT)), MAX_OMEGA)
    xdot = clamp_to(F(xdot + F(xacc * DT)), MAX_XDOT)
    xq = F(x + F(xdot * DT))
    hit = 0
    if xq < -RAIL:
        x, xdot, hit = F(-RAIL), F(0), -1
    elif xq > RAIL:
        x, xdot, hit = RAIL, F(0), 1
    else:
        x = xq
    h = F(omega * DT)
    c, s = normalise(F(c - F(s * h)), F(s + F(c * h)))
    return (x, xdot, c, s, omega), hit


def reward_of(p, a):
    x, _, c, _, omega = p
    up = F(F(c + F(1)) * F(0.5))
    ce = F(F(1) / F(F(1) + F(x * x)))
    ce = F(F(F(1) + ce) * F(0.5))
    co = F(F(F(4) + F(F(1) - F(a * a))) / F(5))
    w = F(omega / F(5))
    sl = F(F(1) / F(F(1) + F(w * w)))
    sl = F(F(F(1) + sl) * F(0.5))
    return F(F(F(up * ce) * co) * sl)


def end_points(x, c, s):
    """(X0, X1, Y1): the pivot's and the tip's coordinates in 1/16 pixel, each rounded once"""
    xs = F(x * F(320))
    X0 = int(np.floor(F(xs + F(672.5))))
    X1 = int(np.floor(F(F(xs + F(s * F(320))) + F(672.5))))
    Y1 = int(np.floor(F(F(672.5) - F(c * F(320)))))
    return X0, X1, Y1


def capsule(X0, Y0, X1, Y1, r=POLE_R):
    """the mask of the pixels inside the capsule of radius r around the segment (X0, Y0) -- (X1, Y1), by the integer rule"""
    dx, dy = X1 - X0, Y1 - Y0
    dd = dx * dx + dy * dy
    vx, vy = _PX - X0, _PY - Y0
    dot = vx * dx + vy * dy
    cross = vx * dy - vy * dx                       # int64: cross * cross reaches about 10^12
    assert int(np.abs(cross).max()) ** 2 < 2 ** 62
    near_pivot = vx * vx + vy * vy <= r * r
    near_tip = (_PX - X1) ** 2 + (_PY - Y1) ** 2 <= r * r
    beside = cross * cross <= r * r * dd
    return np.where(dot <= 0, near_pivot, np.where(dot >= dd, near_tip, beside))


def render(phys):
    """the frame of one state"""
    X0, X1, Y1 = end_points(phys[0], phys[2], phys[3])
    frame = np.stack([BACKGROUND] * 3)
    rail = (_II == RAIL_ROW) & (np.abs(_PX - CENTRE) <= RAIL_HALF)
    cart = (np.abs(_PX - X0) <= CART_HALF_W) & (np.abs(_PY - CENTRE) <= CART_HALF_H)
    for m, rgb in ((rail, RAIL_RGB), (cart, CART_RGB), (capsule(X0, CENTRE, X1, Y1), POLE_RGB)):
        for ch in range(3):
            frame[ch][m] = rgb[ch]
    return frame


class CartpoleOracle(S.SkeletonOracle):
    WORDS = (("phys", (5,), F),)

    def __init__(self, num_envs, episode_length=1000, seed=0, repeat=1, swing_up=True, frames=True):
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.swing_up = bool(swing_up)
        # what a run met: hits of either rail end, sign changes of s while hanging (c < 0) and while upright (c > 0)
        self.hit_left = self.hit_right = self.through_hanging = self.through_upright = 0

    def new_episode(self, e, ep):
        c, s = normalise(F(-1) if self.swing_up else F(1), F(draw(self.seed, e, ep, 1) * F(0.05)))
        self.phys[e] = (F(draw(self.seed, e, ep, 0) * F(0.1)), 0, c, s, 0)

    def sanitise(self, row):
        return S.sanitise(row[0])

    def frame(self, e):
        return render(self.phys[e])

    def substep(self, e, a):
        s_before = self.phys[e, 3]
        p, hit = substep(tuple(self.phys[e]), a)
        self.hit_left += hit < 0
        self.hit_right += hit > 0
        if (s_before < 0) != (p[3] < 0) and s_before != 0 and p[3] != 0:
            if p[2] < 0:
                self.through_hanging += 1
            else:
                self.through_upright += 1
        self.phys[e] = p
        return reward_of(p, a), F(1), False


_SEEN = ("hit_left", "hit_right", "through_hanging", "through_upright", "cut_by_limit", "full", "reset_rows")

# ---- the driven run the CPU and the GPU tests share ---------------------------------------------------------------
STEPS, EPISODE_LENGTH, SEED = 40, 7, 5
DRIVEN = tuple((N, A, k, swing) for (N, A) in ((3, 1), (5, 3)) for k in (1, 2, 16) for swing in (True, False))


def driven_run(N, A, repeat, swing_up, seed=SEED, steps=STEPS, episode_length=EPISODE_LENGTH, frames=True):
    """the oracle driven for `steps` macro steps by S.wild_actions from the staggered reset (S.stagger): the actions it was
    given, everything it returned (the frames only if asked for) and the state after every step"""
    r = np.random.RandomState(seed * 100003 + N * 101 + A * 17 + repeat * 3 + int(swing_up))
    o = CartpoleOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, swing_up=swing_up, frames=frames)
    o.reset()
    S.stagger(o)
    return S.record(o, steps, lambda s: S.wild_actions(r, N, A), _SEEN)


# The physics drive: the driven runs above have episodes of seven simulator steps, in which no cart reaches a rail end
# and no pole swings through the vertical.  These runs do, under a pattern of actions that holds one sign for long:
# environment e pushes with sign (-1)^e for `hold` macro steps, then alternates in blocks of `swing` macro steps, which
# pumps the hanging pole through the bottom and lets the near-upright pole fall through the top in its first blocks.
PHYSICS = tuple((4, 1, 16, swing, 60, 2000) for swing in (True, False))         # N, A, repeat, swing_up, steps, episode_length


def physics_actions(N, A, s, swing_up):
    a = np.zeros((N, A), F)
    sign = np.where(np.arange(N) % 2 == 0, F(1), F(-1))
    if swing_up:
        a[:, 0] = sign * (F(1.5) if (s // 4) % 2 == 0 else F(-1.5))          # 64 simulator steps a side: the pole is pumped
        if s >= 30:
            a[:, 0] = sign * F(2)                                             # then into the rail end
    else:
        a[:, 0] = sign * (F(0.25) if s % 2 == 0 else F(-0.25)) if s < 6 else sign * F(2)
    return a


def physics_run(N, A, repeat, swing_up, steps, episode_length, seed=SEED, frames=True):
    o = CartpoleOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, swing_up=swing_up, frames=frames)
    o.reset()
    return S.record(o, steps, lambda s: physics_actions(N, A, s, swing_up), _SEEN)


def run(cfg, frames=True):
    """the run of a configuration of DRIVEN or PHYSICS"""
    return driven_run(*cfg, frames=frames) if len(cfg) == 4 else physics_run(*cfg, frames=frames)


# ---- the argument lists drq_vec_cartpole_step refuses: shared by the CPU and the GPU test ------------------------------
def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_cartpole_step must refuse, around one well-formed list over the four given base
    addresses (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     phys t          episode     over        N  A  action seed L repeat reset swing frame
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, 5, 1, ACT, 7, 9, 2, 0, 1, FR,
          SC, SC + 0x100, SC + 0x200, SC + 0x300]                         # reward discount first substeps
    bad = S.refused_steps(ok, "w w w b N A action - L repeat reset - frame w w b w", {11: (2, -1)})      # swing_up
    assert len(bad) == 10 + 15 + 3 + 7
    return bad


def refused_renders(S0, FR):
    """the argument lists drq_vec_cartpole_render must refuse: (phys, N, frame)"""
    return S.refused_reads([S0, 3, FR], "w N frame", {})
