"""numpy restatement of the step-major replay (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("step-major replay"), stated here once more:

  ring      R rows x N environments; absolute row t (= number of add() calls before it) of environment e lives in slot
            (t mod R) N + e.  first == 1: the dummy reset transition of a new episode; row 0 always is one
  bounds    with T rows added: hi = T - nstep, lo = max(1, T - R + 1 + guard_rows)
  choose    M = (hi - lo + 1) N; candidate j of batch row b: c = min(int(u[b, j] M), M - 1), t = lo + c // N, e = c % N
            (float64 product, truncated); the first candidate that is no reset row; if all are, candidate 0 walked
            cyclically through t+1 .. hi, lo .. t-1 of its environment; if that finds none: steps 0
  window    k = nstep, or the first i > 0 with first[t+i, e] == 1

The n-step arithmetic is NOT restated: sample() cuts the environment's current episode out of the history and calls
oracle.nstep_sample(episode, t - start, k, gamma), so the reference-pinned function stays the yardstick.

The oracle keeps every row ever added (tests are small), which is what lets it name the episode of a transition after
the ring has wrapped; ring() gives the R rows a device store must hold, slot by slot.
"""
from collections import Counter

import numpy as np

from oracle import drq_oracle as O


def bounds(T, R, nstep, guard_rows):
    return max(1, T - R + 1 + guard_rows), T - nstep


def slot(t, e, R, N):
    return (t % R) * N + e


class VecOracle:
    def __init__(self, R, N, A, frame_bytes, nstep, gamma, guard_rows=8):
        self.R, self.N, self.A, self.fb = R, N, A, frame_bytes
        self.nstep, self.gamma, self.guard = nstep, gamma, guard_rows
        self.obs, self.action, self.reward, self.discount, self.first = [], [], [], [], []

    @property
    def T(self):
        return len(self.obs)

    def add(self, obs, action, reward, discount, first=None):
        N = self.N
        f = np.zeros(N, np.uint8) if first is None else (np.asarray(first).reshape(N) != 0).astype(np.uint8)
        if self.T == 0:
            f[:] = 1
        self.obs.append(np.asarray(obs, np.uint8).reshape(N, self.fb).copy())
        self.action.append(np.asarray(action, np.float32).reshape(N, self.A).copy())
        self.reward.append(np.asarray(reward, np.float32).reshape(N).copy())
        self.discount.append(np.asarray(discount, np.float32).reshape(N).copy())
        self.first.append(f)

    def bounds(self):
        return bounds(self.T, self.R, self.nstep, self.guard)

    def slot(self, t, e):
        return slot(t, e, self.R, self.N)

    def ring(self):
        """what the device arrays hold for the rows still in the ring: dict name -> array indexed by slot, and the mask
        of the slots that have been written"""
        R, N = self.R, self.N
        out = {"frames": np.zeros((R * N, self.fb), np.uint8), "action": np.zeros((R * N, self.A), np.float32),
               "reward": np.zeros(R * N, np.float32), "discount": np.zeros(R * N, np.float32),
               "first": np.zeros(R * N, np.uint8)}
        written = np.zeros(R * N, bool)
        for t in range(max(0, self.T - R), self.T):
            s = slice((t % R) * N, (t % R) * N + N)
            out["frames"][s], out["action"][s] = self.obs[t], self.action[t]
            out["reward"][s], out["discount"][s], out["first"][s] = self.reward[t], self.discount[t], self.first[t]
            written[s] = True
        return out, written

    # ---- the draw ------------------------------------------------------------------------
    def choose(self, u_row):
        """(t, e, k, case) of one batch row; case names how the row came about: accept0 .. accept<K-1>, walk, walk_wrap
        or empty (k = 0, t and e candidate 0's)"""
        lo, hi = self.bounds()
        rows, N = hi - lo + 1, self.N
        M = rows * N
        cands = []
        for uj in u_row:
            c = min(int(np.float64(uj) * np.float64(M)), M - 1)
            cands.append((lo + c // N, c % N))
        for j, (t, e) in enumerate(cands):
            if not self.first[t][e]:
                return t, e, self.window(t, e), f"accept{j}"
        t0, e = cands[0]
        for i in range(1, rows):
            t = lo + (t0 - lo + i) % rows
            if not self.first[t][e]:
                return t, e, self.window(t, e), "walk_wrap" if t < t0 else "walk"
        return t0, e, 0, "empty"

    def window(self, t, e):
        for i in range(1, self.nstep):
            if self.first[t + i][e]:
                return i
        return self.nstep

    def episode(self, t, e):
        """(start row, episode dict) of the episode of environment e that holds row t, as far as it has been added"""
        s = t
        while not self.first[s][e]:
            s -= 1
        end = s + 1
        while end < self.T and not self.first[end][e]:
            end += 1
        col = lambda rows_: np.stack([r[e] for r in rows_[s:end]])
        return s, {"observation": col(self.obs), "action": col(self.action), "reward": col(self.reward)[:, None],
                   "discount": col(self.discount)[:, None]}

    def sample(self, u):
        """u float64 [B][K] -> dict: idx int64 [3][B], steps int32 [B], action [B][A], reward / discount float32 [B],
        obs / next_obs uint8 [B][frame_bytes], rows [(t, e)], and tally, the Counter of the cases met (the choice cases
        of choose(), and per drawn transition full or cut<k>)"""
        u = np.asarray(u, np.float64)
        B = u.shape[0]
        idx, steps = np.zeros((3, B), np.int64), np.zeros(B, np.int32)
        act, rew, disc = np.zeros((B, self.A), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        obs, nxt = np.zeros((B, self.fb), np.uint8), np.zeros((B, self.fb), np.uint8)
        tally, rows = Counter(), []
        for b in range(B):
            t, e, k, case = self.choose(u[b])
            tally[case] += 1
            rows.append((t, e))
            steps[b] = k
            if k == 0:
                idx[:, b] = self.slot(t, e)
                act[b], obs[b], nxt[b] = self.action[t][e], self.obs[t][e], self.obs[t][e]
                continue
            tally["full" if k == self.nstep else f"cut{k}"] += 1
            idx[:, b] = self.slot(t - 1, e), self.slot(t + k - 1, e), self.slot(t, e)
            s, ep = self.episode(t, e)
            o, a, r, d, n = O.nstep_sample(ep, t - s, k, self.gamma)
            obs[b], act[b], rew[b], disc[b], nxt[b] = o, a, r[0], d[0], n
        return dict(idx=idx, steps=steps, action=act, reward=rew, discount=disc, obs=obs, next_obs=nxt, rows=rows,
                    tally=tally)
