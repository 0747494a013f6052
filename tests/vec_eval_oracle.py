"""numpy restatement of the evaluation launches and of the order of evaluate() (a helper module: not collected).  The
contract is the comment of include/drqv2_hip.h ("evaluation") and the docstring of drqv2_amd.evaluate.evaluate(); three
things are stated here once more, each on its own:

  stack_push    the FrameStackWrapper rule (dmc.py:87-109) on arrays: a reset environment holds its frame three times,
                every other one drops its oldest frame and appends the new one
  StackOracle   the object around it: the first push after construction or reset() resets every environment
  mosaic        one image of the clip: tile m at (m // GW, m % GW) shows environment envs[m], every pixel k x k times,
                channels last, >> 2 where done[e] >= limit > 0, zero tiles past M
  EvalOrder     the rows of one evaluation in the order evaluate() keeps: push, then the statistics' `done` rule, then the
                image of that row with the counters as they stand AFTER it

Everything is integer arithmetic: every comparison against these is exact.
"""
import numpy as np


def stack_push(prev, frame, first=None, reset_all=False):
    """prev uint8 [N, 9, h, w] (not read where an environment is reset; None with reset_all), frame uint8 [N, 3, h, w],
    first [N] or None -> the new stacks uint8 [N, 9, h, w]"""
    frame = np.asarray(frame, np.uint8)
    N = frame.shape[0]
    f = np.ones(N, bool) if reset_all else (np.zeros(N, bool) if first is None else np.asarray(first).reshape(N) != 0)
    out = np.empty((N, 9) + frame.shape[2:], np.uint8)
    for e in range(N):
        if f[e]:
            out[e] = np.concatenate([frame[e]] * 3, axis=0)
        else:
            out[e, :6] = prev[e, 3:]
            out[e, 6:] = frame[e]
    return out


class StackOracle:
    def __init__(self, N):
        self.N, self.obs = N, None

    def reset(self):
        self.obs = None

    def push(self, frame, first=None):
        self.obs = stack_push(self.obs, frame, first, reset_all=self.obs is None)
        return self.obs


def mosaic(frame, envs, grid, k, done=None, limit=0):
    """frame uint8 [N, 3, 84, 84] -> uint8 [GH S, GW S, 3], S = 84 k"""
    frame = np.asarray(frame, np.uint8)
    GH, GW = grid
    side = frame.shape[2]
    S = side * k
    assert 1 <= len(envs) <= GH * GW and frame.shape[2] == frame.shape[3]
    out = np.zeros((GH * S, GW * S, 3), np.uint8)
    for m, e in enumerate(envs):
        gy, gx = divmod(m, GW)
        tile = np.empty((S, S, 3), np.uint8)
        for y in range(S):
            for c in range(3):
                tile[y, :, c] = frame[e, c, y // k, np.arange(S) // k]
        if done is not None and limit > 0 and done[e] >= limit:
            tile = tile >> 2
        out[gy * S:(gy + 1) * S, gx * S:(gx + 1) * S] = tile
    return out


class EvalOrder:
    """one evaluation, row by row: row(frame, first) is what evaluate() does with the outputs of env.reset() (row 0) or
    env.step(): stack.push -> stats.step (here only its per-environment counters: a flagged row with a running length
    >= 1 closes an episode; row 0 is a reset row for every environment) -> video.record with the counters after the row"""

    def __init__(self, N, envs, grid, k, limit):
        self.N, self.envs, self.grid, self.k, self.limit = N, list(envs), grid, k, limit
        self.stack = StackOracle(N)
        self.len = np.zeros(N, np.int64)
        self.done = np.zeros(N, np.int32)
        self.rows = 0
        self.clip, self.dones, self.frames = [], [], []

    def row(self, frame, first=None):
        N = self.N
        f = np.zeros(N, bool) if first is None else np.asarray(first).reshape(N) != 0
        if self.rows == 0:
            f[:] = True
        obs = self.stack.push(frame, f)
        for e in range(N):
            if f[e]:
                if self.len[e] >= 1:
                    self.done[e] += 1
                self.len[e] = 0
            else:
                self.len[e] += 1
        self.rows += 1
        self.dones.append(self.done.copy())
        self.frames.append(np.asarray(frame, np.uint8).copy())
        self.clip.append(mosaic(frame, self.envs, self.grid, self.k, self.done, self.limit))
        return obs
