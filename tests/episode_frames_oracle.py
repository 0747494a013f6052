"""numpy restatement of the single-frame episode store (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("single frames in the episode store"); stated here once more, each on its own:

  stack_slots   the slot rule on a flat store of R slots: p1 = p0 - 1, p2 = p0 - 2, modulo R,
                first[p0] -> (p0, p0, p0); else first[p1] -> (p1, p1, p0); else (p2, p1, p0)
  stack_at      the bytes of that stack: three single frames, oldest first
  episode       the simulator: an episode as the reference's environment hands it over -- FrameStackWrapper (dmc.py:87-109,
                restated in tests/vec_frames_oracle.py) run over random frames: reset on step 0, one step per further row
  Layout        DeviceReplay's placement restated (contiguous, wrap to slot 0 when the tail is too short, evict what the
                range overlaps) over host arrays: the stacked observations a stacked store would hold, and the single
                frames and flags a single-frame store holds -- stale frames and flags of evicted episodes left in place
"""
import numpy as np

from tests.vec_frames_oracle import FrameStack


def stack_slots(first, p0):
    R = len(first)
    p1, p2 = (p0 - 1) % R, (p0 - 2) % R
    if first[p0]:
        return p0, p0, p0
    if first[p1]:
        return p1, p1, p0
    return p2, p1, p0


def stack_at(frames, first, p0):
    """frames [R, ...] single frames by slot -> the stack whose newest frame is slot p0, flat"""
    return np.concatenate([frames[q].reshape(-1) for q in stack_slots(first, p0)])


def episode(r, n, A, frame_shape=(3, 84, 84)):
    """an episode of n steps (n = T + 1, index 0 the dummy reset transition) as a dict like the reference's npz, plus
    "frames": the single frames [n, *frame_shape] the stacks were built from"""
    frames = r.randint(0, 256, (n,) + tuple(frame_shape)).astype(np.uint8)
    w = FrameStack()
    obs = np.stack([w.reset(frames[0])] + [w.step(frames[t]) for t in range(1, n)])
    return {"observation": obs, "frames": frames,
            "action": r.uniform(-1, 1, (n, A)).astype(np.float32),
            "reward": r.standard_normal((n, 1)).astype(np.float32),
            "discount": np.where(r.uniform(size=(n, 1)) < 0.15, 0.0, 1.0).astype(np.float32)}


def npz_fields(ep):
    """the episode without the simulator's extra"""
    return {k: v for k, v in ep.items() if k != "frames"}


class Layout:
    def __init__(self, capacity, A, frame_shape=(3, 84, 84), seed=None):
        self.R, self.A = capacity, A
        fb = int(np.prod(frame_shape))
        # slots no episode was ever placed on: garbage frames and garbage flags (seed) or zeros, as the store allocates
        g = np.random.RandomState(seed) if seed is not None else None
        self.frames = g.randint(0, 256, (capacity, fb)).astype(np.uint8) if g else np.zeros((capacity, fb), np.uint8)
        self.first = g.randint(0, 2, capacity).astype(np.uint8) if g else np.zeros(capacity, np.uint8)
        self.stacked = np.zeros((capacity, 3 * fb), np.uint8)
        self.action = np.zeros((capacity, A), np.float32)
        self.reward = np.zeros(capacity, np.float32)
        self.discount = np.ones(capacity, np.float32)
        self.episodes, self.head = [], 0

    def add(self, ep):
        n = ep["frames"].shape[0]
        assert n <= self.R
        start = self.head if self.head + n <= self.R else 0
        end = start + n
        clear = lambda e: e[0] + e[1] <= start or e[0] >= end
        evicted = [e for e in self.episodes if not clear(e)]
        self.episodes = [e for e in self.episodes if clear(e)] + [[start, n]]
        self.head = end
        sl = slice(start, end)
        self.frames[sl] = ep["frames"].reshape(n, -1)
        self.stacked[sl] = ep["observation"].reshape(n, -1)
        self.first[sl] = 0
        self.first[start] = 1
        self.action[sl], self.reward[sl], self.discount[sl] = ep["action"], ep["reward"].reshape(n), ep["discount"].reshape(n)
        return start, evicted

    def live_slots(self):
        return [q for s, n in self.episodes for q in range(s, s + n)]

    def drawable(self, nstep):
        """every position a draw can name: start+1 .. start+n-nstep of the episodes at least nstep long"""
        return [q for s, n in self.episodes if n - 1 >= nstep for q in range(s + 1, s + n - nstep + 1)]
