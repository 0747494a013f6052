"""numpy restatement of prioritized sampling on the step-major ring (a helper module: not collected).  Composed from
tests/vec_oracle.py (rows, bounds, slots, windows, and through it oracle.nstep_sample) and tests/per_oracle.py (rebuild,
descend, weights, update); the contract is the comment of include/drqv2_hip.h ("prioritized step-major replay").  What is
new here, stated once more:

  tree      per_oracle's, over the R N slots of the ring: L = leaves_of(R N), all leaves 0, tree[0] = 1
  invariant after every add, (lo, hi) = bounds: leaf(slot(t, e)) > 0 iff lo <= t <= hi and first[t][e] == 0; all others 0
  advance   after the add that makes T rows: (lo, hi) = bounds(T); enter = hi if hi >= lo else none; leave = lo - 1 if
            lo >= 2 else none (lo moved iff it left 1).  The N leaves of row enter <- 0 where first else tree[0], those of
            row leave <- 0, ancestors of both rebuilt
  row_of    slot p lies in ring row r = p // N, which holds the absolute row T-1 - ((T-1-r) mod R)
  drawable  0 <= p < R N, lo <= row_of(p) <= hi, first == 0
  draw      descend -> p; e = p % N, t = row_of(p); window and n-step sums as VecOracle.sample; weights with the nominal
            n = (hi - lo + 1) N.  tree[1] == 0: every batch row is the empty one -- all indices slot(lo, 0), its action
            row, steps 0, reward 0, discount 0, weight 1
  update    td clamped (NaN / negative -> 0, inf -> FLT_MAX); rows whose position is not drawable NOW are dropped, the
            rest is per_oracle.update; the ancestors of every named position inside the tree are rebuilt all the same
"""
import numpy as np

from oracle import drq_oracle as O
from tests import per_oracle as P
from tests import vec_oracle as V

FLT_MAX = np.float64(np.finfo(np.float32).max)


def entering_leaving(T, R, nstep, guard_rows):
    """(enter_t, leave_t) of the add that made T rows, -1 = none: from the counters alone"""
    lo, hi = V.bounds(T, R, nstep, guard_rows)
    return (hi if hi >= lo else -1), (lo - 1 if lo >= 2 else -1)


def advance(tree, R, N, enter_t, leave_t, first_of_enter):
    """first_of_enter: the N flags of row enter_t (ignored when enter_t is -1)"""
    L = tree.size // 2
    nodes = []
    if enter_t >= 0:
        s = (enter_t % R) * N
        tree[L + s:L + s + N] = np.where(np.asarray(first_of_enter) != 0, 0.0, tree[0])
        nodes.append(np.arange(L + s, L + s + N))
    if leave_t >= 0:
        s = (leave_t % R) * N
        tree[L + s:L + s + N] = 0.0
        nodes.append(np.arange(L + s, L + s + N))
    if nodes:
        P.rebuild(tree, np.concatenate(nodes))


def row_of(p, T, R, N):
    return T - 1 - ((T - 1 - p // N) % R)


def clamp_td(td_abs):
    t = np.asarray(td_abs, np.float32).astype(np.float64)
    t = np.where(t >= 0.0, t, 0.0)                  # NaN compares false: 0
    return np.minimum(t, FLT_MAX).astype(np.float32)


class VecPEROracle:
    def __init__(self, R, N, A, frame_bytes, nstep, gamma, guard_rows=8, alpha=0.6, beta=0.4, eps=1e-6):
        self.vo = V.VecOracle(R, N, A, frame_bytes, nstep, gamma, guard_rows)
        self.alpha, self.beta, self.eps = alpha, beta, eps
        self.tree = P.new_tree(R * N)
        self.L = self.tree.size // 2

    @property
    def T(self):
        return self.vo.T

    def bounds(self):
        return self.vo.bounds()

    def add(self, obs, action, reward, discount, first=None):
        vo = self.vo
        vo.add(obs, action, reward, discount, first)
        enter, leave = entering_leaving(vo.T, vo.R, vo.nstep, vo.guard)
        advance(self.tree, vo.R, vo.N, enter, leave, vo.first[enter] if enter >= 0 else None)

    def drawable(self, p):
        vo = self.vo
        if not 0 <= p < vo.R * vo.N:
            return False
        lo, hi = vo.bounds()
        t = row_of(p, vo.T, vo.R, vo.N)
        return lo <= t <= hi and not vo.first[t][p % vo.N]

    def expected_leaf_mask(self):
        """bool [L]: where the invariant wants a positive leaf"""
        return np.array([self.drawable(p) for p in range(self.L)])

    def sample(self, u):
        """u float64 [B] -> dict like VecOracle.sample's (no frames), plus weights float64 [B] and pos int64 [B]"""
        vo = self.vo
        u = np.asarray(u, np.float64)
        B = u.shape[0]
        lo, hi = vo.bounds()
        idx, steps = np.zeros((3, B), np.int64), np.zeros(B, np.int32)
        act, rew, disc = np.zeros((B, vo.A), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        if self.tree[1] == 0:
            idx[:] = vo.slot(lo, 0)
            act[:] = vo.action[lo][0]
            return dict(idx=idx, steps=steps, action=act, reward=rew, discount=disc, weights=np.ones(B), pos=idx[2].copy(),
                        rows=[(lo, 0)] * B)
        pos = P.descend(self.tree, u)
        w = P.weights(self.tree, pos, (hi - lo + 1) * vo.N, self.beta)
        rows = []
        for b, p in enumerate(pos.tolist()):
            assert self.drawable(p), (b, p)
            t, e = row_of(p, vo.T, vo.R, vo.N), p % vo.N
            k = vo.window(t, e)
            rows.append((t, e))
            steps[b] = k
            idx[:, b] = vo.slot(t - 1, e), vo.slot(t + k - 1, e), p
            s, ep = vo.episode(t, e)
            _, a, r, d, _ = O.nstep_sample(ep, t - s, k, vo.gamma)
            act[b], rew[b], disc[b] = a, r[0], d[0]
        return dict(idx=idx, steps=steps, action=act, reward=rew, discount=disc, weights=w, pos=pos, rows=rows)

    def update(self, pos, td_abs):
        """returns {position: leaf written}"""
        pos = np.asarray(pos, np.int64)
        td = clamp_td(td_abs)
        keep = np.array([self.drawable(p) for p in pos.tolist()], bool)
        written = P.update(self.tree, pos[keep], td[keep], self.alpha, self.eps) if keep.any() else {}
        inside = pos[(pos >= 0) & (pos < self.L)]
        if inside.size:
            P.rebuild(self.tree, self.L + inside)
        return written
