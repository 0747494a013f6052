"""numpy restatement of the episode statistics (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("episode statistics"), stated here once more:

  state     per environment e: ret[e] float32, len[e], done[e]; totals rows, episodes, length_sum, return_sum, min_return
            (+inf), max_return (-inf); a log of the newest W records (return, length, env, row)
  step      call number t = rows, for every e: f = t == 0 or first[e].  f and len[e] >= 1: the running episode is finished;
            it is counted if limit == 0 or done[e] < limit; done[e] += 1 either way.  f: ret[e] = len[e] = 0 (the reward of
            a reset row is not read); else ret[e] = float32(ret[e] + reward[e]), len[e] += 1
  records   the episodes one call counts are numbered in ascending e behind those counted before; record j at j mod W
  totals    return_sum here is math.fsum over every counted float32 return: the exact sum, rounded once

Every counted episode is kept (tests are small), so a snapshot can name what the log has lost.
"""
import math

import numpy as np

RECORD = np.dtype([("return", np.float32), ("length", np.int32), ("env", np.int32), ("row", np.int64)])


class Snapshot:
    def __init__(self, o):
        self.rows, self.episodes = o.rows, len(o.counted)
        rets = [float(r[0]) for r in o.counted]
        self.length_sum = sum(int(r[1]) for r in o.counted)
        self.return_sum = math.fsum(rets)
        self.abs_return_sum = math.fsum(abs(r) for r in rets)      # what the bound on return_sum is made of
        self.min_return = float(np.float32(min(rets))) if rets else float("inf")
        self.max_return = float(np.float32(max(rets))) if rets else float("-inf")
        self.records = np.array(o.counted[-o.W:] if o.counted else [], dtype=RECORD)
        self.lost = max(0, self.episodes - o.W)
        self.complete = o.limit > 0 and self.episodes == o.limit * o.N
        self.mean_return = self.return_sum / self.episodes if self.episodes else float("nan")
        self.mean_length = self.length_sum / self.episodes if self.episodes else float("nan")

    def since(self, prev_episodes):
        prev = max(0, int(prev_episodes))
        oldest = self.episodes - len(self.records)
        return self.records[max(0, prev - oldest):], max(0, oldest - prev)


class StatsOracle:
    def __init__(self, N, W=1024, limit=0):
        self.N, self.W, self.limit = int(N), int(W), int(limit)
        self.reset()

    def reset(self):
        self.ret = np.zeros(self.N, np.float32)
        self.len = np.zeros(self.N, np.int32)
        self.done = np.zeros(self.N, np.int32)
        self.rows = 0
        self.counted = []           # (return, length, env, row) of every counted episode, in the order (row, env)

    def step(self, reward, first=None):
        t = self.rows
        reward = None if reward is None else np.asarray(reward, np.float32).reshape(self.N)
        flags = np.zeros(self.N, bool) if first is None else np.asarray(first).reshape(self.N) != 0
        for e in range(self.N):
            if t == 0 or flags[e]:
                if self.len[e] >= 1:
                    if self.limit == 0 or self.done[e] < self.limit:
                        self.counted.append((self.ret[e], self.len[e], e, t))
                    self.done[e] += 1
                self.ret[e], self.len[e] = np.float32(0), 0
            else:
                self.ret[e] = np.float32(self.ret[e] + reward[e])      # one float32 add
                self.len[e] += 1
        self.rows += 1

    def log(self):
        """the four log arrays as the device holds them: record j at j mod W; and the mask of the indices written"""
        out = np.zeros(self.W, RECORD)
        written = np.zeros(self.W, bool)
        for j in range(max(0, len(self.counted) - self.W), len(self.counted)):
            out[j % self.W] = self.counted[j]
            written[j % self.W] = True
        return out, written

    def snapshot(self):
        return Snapshot(self)
