"""numpy restatement of the device environment (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("device environment"), stated here once more with float32 scalars, one rounding per operation in
the written order, and uint32 hashing in Python integers:

  state   per environment e: pos[2], target[2] float32; t int32; episode uint32; over uint8
  reset   episode += 1, t = 0, over = 0; draws k = 0 .. 3 -> pos.x, pos.y, target.x, target.y:
          h = fmix32(seed ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ k * 0xC2B2AE35); u = float(h >> 8) * 2^-24;
          v = (u * 2 - 1) * 0.9.   Outputs first = 1, reward = 0, discount = 1, the frame; the action is not read
  step    a = action[e, 0:2], NaN -> 0, else clamped to [-1, 1]; pos = clamp(pos + a * 0.1, -1, 1); t += 1;
          d2 = dx dx + dy dy; reward = max(0, 1 - d2); d2 <= 0.01: discount 0, over; else t == episode_length: discount 1,
          over; else discount 1.  first = 0.  An environment whose last step set `over` is reset instead
  frame   uint8 [3, 84, 84]: 32 + ((i + j) >> 2); target disc (j-cx)^2 + (i-cy)^2 <= 25 in (64, 255, 64); agent disc <= 16 in
          (255, 64, 64) over it; cx = int(floor((x + 1) * 41.5 + 0.5)), cy from y
"""
import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
SIDE = 84
TARGET_RGB, AGENT_RGB = (64, 255, 64), (255, 64, 64)
_II, _JJ = np.meshgrid(np.arange(SIDE), np.arange(SIDE), indexing="ij")
BACKGROUND = (32 + ((_II + _JJ) >> 2)).astype(np.uint8)


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    h ^= h >> 16
    return h


def draw(seed, e, episode, k):
    h = fmix32((seed & M32) ^ (e * 0x9E3779B9 & M32) ^ (episode * 0x85EBCA6B & M32) ^ (k * 0xC2B2AE35 & M32))
    u = F(F(h >> 8) * F(2.0 ** -24))
    return F(F(F(u * F(2)) - F(1)) * F(0.9))


def clamp1(v):
    if v < F(-1):
        return F(-1)
    if v > F(1):
        return F(1)
    return F(v)


def centre(x):
    return int(np.floor(F(F(F(x + F(1)) * F(41.5)) + F(0.5))))


def disc(cx, cy, r2):
    """the mask of the pixels (i, j) with (j - cx)^2 + (i - cy)^2 <= r2"""
    return (_JJ - cx) ** 2 + (_II - cy) ** 2 <= r2


def render(pos, target):
    """the frame of one state"""
    frame = np.stack([BACKGROUND] * 3)
    for (x, y), r2, rgb in ((target, 25, TARGET_RGB), (pos, 16, AGENT_RGB)):
        m = disc(centre(x), centre(y), r2)
        for c in range(3):
            frame[c][m] = rgb[c]
    return frame


def replicate(frames, size, channels):
    """the renderer-shaped image of frames [N, 3, 84, 84]: uint8 [N, size, size, channels], every pixel size / 84 times in
    both directions, channels last, a fourth channel 255"""
    k = size // SIDE
    assert size == SIDE * k and 1 <= k <= 4 and channels in (3, 4)
    img = np.repeat(np.repeat(frames.transpose(0, 2, 3, 1), k, axis=1), k, axis=2)
    if channels == 4:
        img = np.concatenate([img, np.full(img.shape[:3] + (1,), 255, np.uint8)], axis=3)
    return np.ascontiguousarray(img)


class ReachOracle:
    def __init__(self, num_envs, episode_length=250, seed=0):
        self.N, self.episode_length, self.seed = int(num_envs), int(episode_length), int(seed) & M32
        self.pos = np.zeros((self.N, 2), F)
        self.target = np.zeros((self.N, 2), F)
        self.t = np.zeros(self.N, np.int32)
        self.episode = np.zeros(self.N, np.uint32)
        self.over = np.zeros(self.N, np.uint8)
        self.reached = self.timed_out = 0       # terminations of either kind so far

    def _reset_one(self, e):
        ep = (int(self.episode[e]) + 1) & M32
        self.episode[e], self.t[e], self.over[e] = ep, 0, 0
        v = [draw(self.seed, e, ep, k) for k in range(4)]
        self.pos[e], self.target[e] = v[:2], v[2:]

    def _outputs(self, reward, discount, first):
        frame = np.stack([render(self.pos[e], self.target[e]) for e in range(self.N)])
        return frame, reward, discount, first

    def reset(self):
        for e in range(self.N):
            self._reset_one(e)
        return self._outputs(np.zeros(self.N, F), np.ones(self.N, F), np.ones(self.N, np.uint8))[0]

    def step(self, action):
        """action: float32 [N, A], A >= 2 -> (frame, reward, discount, first)"""
        action = np.asarray(action, F)
        reward, discount, first = np.zeros(self.N, F), np.ones(self.N, F), np.zeros(self.N, np.uint8)
        for e in range(self.N):
            if self.over[e]:
                self._reset_one(e)
                first[e] = 1
                continue
            for k in range(2):
                a = action[e, k]
                a = F(0) if np.isnan(a) else clamp1(a)
                self.pos[e, k] = clamp1(F(self.pos[e, k] + F(a * F(0.1))))
            self.t[e] += 1
            dx, dy = F(self.pos[e, 0] - self.target[e, 0]), F(self.pos[e, 1] - self.target[e, 1])
            d2 = F(F(dx * dx) + F(dy * dy))
            r = F(F(1) - d2)
            reward[e] = r if r > 0 else F(0)
            if d2 <= F(0.01):
                discount[e], self.over[e] = 0, 1
                self.reached += 1
            elif self.t[e] == self.episode_length:
                self.over[e] = 1
                self.timed_out += 1
        return self._outputs(reward, discount, first)

    def state(self):
        return {"pos": self.pos.copy(), "target": self.target.copy(), "t": self.t.copy(), "episode": self.episode.copy(),
                "over": self.over.copy()}
