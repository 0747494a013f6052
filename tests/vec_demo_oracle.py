"""numpy restatement of the mixed draw of the step-major replay (a helper module: not collected).  The contract is the
comment of include/drqv2_hip.h ("demonstrations in the step-major replay"), stated here once more:

  storage   one allocation of (R + D) N slots.  Rows 0 .. R-1 are the ring of tests/vec_oracle.py; rows R .. R+D-1 are the
            demonstration partition: linear, demonstration row d of lane e in slot (R + d) N + e, Td <= D rows filled,
            row 0 a reset row for every lane
  bounds    ring: vec_oracle's (lo, hi); partition: (1, Td - nstep)
  draw      batch rows b < Bd from the partition, rows b >= Bd from the ring; every row is vec_oracle's choose() and
            window on its own geometry from its own u[b]; a partition row's three indices are R N + its slots in the
            partition

Nothing of the draw is restated: the partition IS a VecOracle of D rows that never wraps (guard_rows 0: with T <= D its
lower bound is 1), and both halves of a batch come out of VecOracle.sample(), so oracle.nstep_sample stays the yardstick
for every window.  What this module adds is the split, the offset and the book-keeping of which branch of the choice the
partition rows took: MixedOracle.demo_tally counts them over all draws, and require_branches() is what a test calls to
know that its partition rows met every one -- it does not rest on the test's luck.
"""
from collections import Counter

import numpy as np

from tests import vec_oracle as V


class MixedOracle:
    def __init__(self, R, D, N, A, frame_bytes, nstep, gamma, guard_rows=8):
        self.R, self.D, self.N, self.A, self.fb, self.nstep = R, D, N, A, frame_bytes, nstep
        self.live = V.VecOracle(R, N, A, frame_bytes, nstep, gamma, guard_rows)
        self.demo = V.VecOracle(D, N, A, frame_bytes, nstep, gamma, guard_rows=0)
        self.demo_tally = Counter()

    @property
    def base(self):
        return self.R * self.N

    @property
    def Td(self):
        return self.demo.T

    def add(self, *row):
        self.live.add(*row)

    def add_demo(self, obs, action, reward, discount, first):
        """one row of the partition; row 0 is a reset row whatever `first` says, as in the ring"""
        assert self.demo.T < self.D, "the partition never wraps"
        self.demo.add(obs, action, reward, discount, first)

    def demo_bounds(self):
        lo, hi = self.demo.bounds()
        assert lo == 1 and hi == self.Td - self.nstep
        return lo, hi

    def whole(self):
        """the five arrays of the whole allocation, slot by slot; slots never written hold what the store's constructor
        puts there (frames, action, reward 0; discount, first 1)"""
        out = {}
        (ring, rw), (part, pw) = self.live.ring(), self.demo.ring()
        for n in ring:
            for a, w in ((ring[n], rw), (part[n], pw)):
                if n in ("discount", "first"):
                    a[~w] = 1
            out[n] = np.concatenate([ring[n], part[n]])
        return out

    def sample(self, u, Bd):
        """u float64 [B][K], Bd rows from the partition -> the dict of VecOracle.sample() for the mixed batch (rows: (t, e)
        in the geometry the row was drawn from), with demo_cases, the choice case of every partition row"""
        u = np.asarray(u, np.float64)
        B = u.shape[0]
        assert 0 <= Bd <= B
        if Bd:
            lo, hi = self.demo_bounds()
            assert hi >= lo, "no drawable demonstration row"
        if Bd < B:
            lo, hi = self.live.bounds()
            assert hi >= lo, "no drawable ring row"
        d, l = self.demo.sample(u[:Bd]), self.live.sample(u[Bd:])
        d["idx"] = d["idx"] + self.base
        out = {k: np.concatenate([d[k], l[k]], axis=1 if k == "idx" else 0)
               for k in ("idx", "steps", "action", "reward", "discount", "obs", "next_obs")}
        out["rows"] = d["rows"] + l["rows"]
        out["tally"] = d["tally"] + l["tally"]
        out["demo_cases"] = Counter({c: n for c, n in d["tally"].items() if c.startswith(("accept", "walk", "empty"))})
        self.demo_tally += d["tally"]
        # the geometry of the indices: a partition row never names a ring slot, a ring row never a partition slot
        assert (out["idx"][:, :Bd] >= self.base).all() and (out["idx"][:, :Bd] < self.base + self.D * self.N).all()
        assert (out["idx"][:, Bd:] >= 0).all() and (out["idx"][:, Bd:] < self.base).all()
        return out

    def require_branches(self, empty):
        """the partition rows drawn so far took every branch of the choice: a candidate accepted, the walk along
        candidate 0's lane, and (empty: a lane of nothing but reset rows exists) the steps-0 row; also a window that a
        reset row cut, when nstep > 1"""
        t = self.demo_tally
        got = {"accept": any(c.startswith("accept") for c in t), "walk": any(c.startswith("walk") for c in t),
               "empty": "empty" in t, "cut": any(c.startswith("cut") for c in t)}
        need = {"accept", "walk"} | ({"empty"} if empty else set()) | ({"cut"} if self.nstep > 1 else set())
        missing = sorted(k for k in need if not got[k])
        assert not missing, f"the partition rows never took: {missing} (tally {dict(t)})"


# the reset flags of the partition's lanes, rows 0 .. 7 (Td = 8 of D = 9: one row stays unfilled)
#   lane 0  an episode of length 1, a reset row, an episode of length 2, trailing pad rows: windows end early, and a row
#           whose candidates are the reset rows 2 and 3 walks to row 4
#   lane 1  reset rows 0 .. 3, then three steps: candidates on rows 1 .. 3 are all reset rows while row 4 is not -- the walk
#   lane 2  nothing but reset rows: the steps-0 row
LANES = ([1, 0, 1, 1, 0, 0, 1, 1], [1, 1, 1, 1, 0, 0, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1])
TD = len(LANES[0])


def fill_partition(mo, seed):
    """writes the TD rows of LANES (the first N lanes) into mo's partition, with random frames, actions, rewards and a
    few terminal discounts"""
    r = np.random.RandomState(seed)
    N = mo.N
    assert N <= len(LANES) and mo.D >= TD
    for t in range(TD):
        first = np.array([LANES[e][t] for e in range(N)], np.uint8)
        disc = np.where(r.uniform(size=N) < 0.2, 0.0, 1.0).astype(np.float32)
        mo.add_demo(r.randint(0, 256, (N, mo.fb)), r.uniform(-1, 1, (N, mo.A)), r.standard_normal(N), disc, first)


def crafted_rows(mo, K=4):
    """u rows that send a partition row down each branch of the choice, for the partition of fill_partition(): a
    candidate accepted at once (its window cut by the pad rows when nstep > 1), one accepted third after two reset rows
    (window cut after one step), the walk, and for N = 3 the lane of reset rows"""
    lo, hi = mo.demo_bounds()
    N = mo.N
    M = (hi - lo + 1) * N
    cell = lambda t, e: (((t - lo) * N + e) + 0.5) / M
    assert hi >= 4 and K == 4
    w = 1 if N == 3 else 0                                         # the lane the walk runs along
    rows = [[cell(4, 0)] * K,
            [cell(2, 0), cell(3, 0), cell(1, 0), cell(2, 0)],
            [cell(1, w) if N == 3 else cell(2, w), cell(2, w), cell(3, w), cell(3, w)]]
    if N == 3:
        rows.append([cell(2, 2), cell(1, 2), cell(3, 2), cell(4, 2)])
    return rows
