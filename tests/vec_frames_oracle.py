"""numpy restatement of the single-frame step-major replay (a helper module: not collected).  The contract is the comment
of include/drqv2_hip.h ("single-frame step-major replay"); three things are stated here once more, each on its own:

  FrameStack    the reference's FrameStackWrapper (dmc.py:87-109) per environment: a deque(maxlen=3) of frames; reset()
                appends the episode's first frame three times (:98-103), step() appends the new frame once (:105-109),
                the observation is the deque concatenated along the channel axis, oldest first (:87-88)
  stack_slots   the slot rule: with p0 = slot(t, e), p1 = slot(t-1, e), p2 = slot(t-2, e), rows modulo R,
                first[p0] -> (p0, p0, p0); else first[p1] -> (p1, p1, p0); else (p2, p1, p0)
  FrameStream   from a stream of single frames and flags, the stacked rows a VecDeviceReplay would have been fed, and the
                ring of single frames a device store must hold

bounds: hi = T - nstep, lo = max(1, T - R + 1 + guard_rows + 2).
"""
from collections import deque

import numpy as np


def bounds(T, R, nstep, guard_rows):
    return max(1, T - R + 1 + guard_rows + 2), T - nstep


class FrameStack:
    """dmc.py:87-109 for one environment; frames are arrays whose axis 0 is the channel axis"""

    def __init__(self, num_frames=3):
        self._num_frames = num_frames
        self._frames = deque([], maxlen=num_frames)

    def reset(self, frame):
        for _ in range(self._num_frames):
            self._frames.append(frame)
        return self.observation()

    def step(self, frame):
        self._frames.append(frame)
        return self.observation()

    def observation(self):
        assert len(self._frames) == self._num_frames
        return np.concatenate(list(self._frames), axis=0)


def stack_slots(first, R, N, p0):
    """the slots of the three frames of the stack whose newest frame is slot p0, oldest first; first: flags by slot"""
    row, e = divmod(p0, N)
    p1 = ((row - 1) % R) * N + e
    p2 = ((row - 2) % R) * N + e
    if first[p0]:
        return p0, p0, p0
    if first[p1]:
        return p1, p1, p0
    return p2, p1, p0


class FrameStream:
    """rows of single frames [N, c, h, w] and reset flags [N] -> stacks[t] uint8 [N, 3c, h, w]: what a FrameStackWrapper
    per environment returns after step t.  Row 0 is a reset row for every environment whatever the flags say."""

    def __init__(self, R, N):
        self.R, self.N = R, N
        self.frames, self.first, self.stacks = [], [], []
        self._wrappers = [FrameStack() for _ in range(N)]

    @property
    def T(self):
        return len(self.frames)

    def add(self, frame, first=None):
        N = self.N
        f = np.zeros(N, np.uint8) if first is None else (np.asarray(first).reshape(N) != 0).astype(np.uint8)
        if self.T == 0:
            f[:] = 1
        frame = np.asarray(frame, np.uint8).copy()
        self.frames.append(frame)
        self.first.append(f)
        self.stacks.append(np.stack([self._wrappers[e].reset(frame[e]) if f[e] else self._wrappers[e].step(frame[e])
                                     for e in range(N)]))
        return self.stacks[-1]

    def ring(self):
        """(frames by slot [R N, frame bytes], flags by slot [R N]) as a device ring holds them after T adds; slots never
        written: frames 0, flag 1 (the stores' initial value)"""
        R, N = self.R, self.N
        fb = self.frames[0][0].size
        fr, fl = np.zeros((R * N, fb), np.uint8), np.ones(R * N, np.uint8)
        for t in range(max(0, self.T - R), self.T):
            s = slice((t % R) * N, (t % R) * N + N)
            fr[s], fl[s] = self.frames[t].reshape(N, fb), self.first[t]
        return fr, fl

    def has_drawable(self, lo, hi):
        """every environment holds a non-reset row among lo .. hi: the stores' precondition for a draw"""
        return all(any(not self.first[t][e] for t in range(lo, hi + 1)) for e in range(self.N))
