"""The k-NN bonus in numpy (a helper module: not collected): the contract of include/drqv2_hip.h, "k-NN bonus", restated
with float32 array operations in the contract's order, and the slot arithmetic and offset draws of
drqv2_amd.explore.KnnBonus.  tests/test_cpu_knn.py holds this file to a scalar loop; tests/test_hip_knn.py holds the
kernel and the class to this file, bit for bit.

  knn_dist(table, live, slots, k, stride, offset)   dist float32 [B]
  knn_dist_fused(...)                                the same with t * t + acc rounded ONCE (what a contracted build would
                                                     compute), emulated in float64: for the "teeth" check only
  KnnOracle                                          observe / lattice / apply of KnnBonus
  entry_inputs(...)                                  the tables and slots the GPU tests of the raw entry use
"""
import numpy as np

F = np.float32
MAX_DIM, MAX_K, CHUNK = 64, 8, 128


def _accumulate(q, x, fused=False):
    """D [B, M]: acc = 0, then for i in order t = q[i] - x[i], acc = acc + t * t, every operation one float32 operation"""
    B, M, d = q.shape[0], x.shape[0], q.shape[1]
    acc = np.zeros((B, M), F)
    with np.errstate(all="ignore"):
        for i in range(d):
            t = q[:, i:i + 1] - x[None, :, i]
            assert t.dtype == F
            if fused:
                acc = (t.astype(np.float64) * t.astype(np.float64) + acc.astype(np.float64)).astype(F)
            else:
                acc = acc + t * t
            assert acc.dtype == F
    return acc


def candidates(live, stride=1, offset=0):
    return np.arange(offset, live, stride, dtype=np.int64)


def knn_dist(table, live, slots, k, stride=1, offset=0, fused=False):
    table, slots = np.asarray(table), np.asarray(slots, np.int64)
    assert table.dtype == F and table.ndim == 2 and 1 <= table.shape[1] <= MAX_DIM
    assert 0 <= live <= table.shape[0] and 1 <= k <= MAX_K and stride >= 1 and 0 <= offset < stride
    B = slots.shape[0]
    out = np.zeros(B, F)
    cand = candidates(live, stride, offset)
    valid = (slots >= 0) & (slots < live)
    if not valid.any() or len(cand) == 0:
        return out
    q = table[np.where(valid, slots, 0)]            # a row of its own for the slots outside: never used below
    D = _accumulate(q, table[cand], fused)          # rows below live only
    D[np.isnan(D)] = np.inf
    own = cand[None, :] == slots[:, None]
    D[own] = np.inf                                 # excluded by index; counted out below
    others = len(cand) - own.sum(axis=1)
    for b in range(B):
        if valid[b] and others[b] >= k:
            with np.errstate(all="ignore"):
                out[b] = np.sqrt(np.partition(D[b], k - 1)[k - 1])
    assert out.dtype == F
    return out


def knn_dist_fused(table, live, slots, k, stride=1, offset=0):
    return knn_dist(table, live, slots, k, stride, offset, fused=True)


class KnnOracle:
    """KnnBonus on the host: the feature table beside a ring of R rows x N environments, the lattice draws, the bonus"""

    def __init__(self, R, N, dim, k, beta, candidates=None, seed=0):
        self.R, self.N, self.dim, self.k, self.beta, self.candidates = R, N, dim, k, beta, candidates
        self.table = np.zeros((R * N, dim), F)
        self.rows = 0
        self.rng = np.random.RandomState(seed & 0xFFFFFFFF)

    @property
    def live(self):
        return min(self.rows, self.R) * self.N

    def observe(self, y, T):
        assert T == self.rows + 1 and y.shape == (self.N, self.dim) and y.dtype == F
        lo = ((T - 1) % self.R) * self.N
        self.table[lo:lo + self.N] = y
        self.rows = T

    def lattice(self):
        if self.candidates is None:
            return 1, 0
        stride = max(1, -(-self.live // self.candidates))
        return stride, int(self.rng.randint(0, stride))

    def apply(self, slots, reward):
        """(dist [B], bonus [B], reward + bonus [B, 1], (stride, offset)); the bonus is float32(beta) * log1p(dist) in
        float32"""
        stride, offset = self.lattice()
        dist = knn_dist(self.table, self.live, slots, self.k, stride, offset)
        with np.errstate(all="ignore"):
            bonus = (F(self.beta) * np.log1p(dist)).astype(F)
        return dist, bonus, (np.asarray(reward, F).reshape(-1, 1) + bonus.reshape(-1, 1)).astype(F), (stride, offset)


# ------------------------------------------------------------------------------------------------ the raw entry's cases
DIMS, KS, BS = (1, 3, 50, 64), (1, 3, 8), (1, 3, 65)
LATTICES = ((1, 0), (3, 0), (3, 2))
PAD_ROWS = 7                    # rows of the table above `live`


def lives(k):
    return (0, 1, k, k + 1, 65, 257, CHUNK + 1, 2 * CHUNK + 63)


def entry_inputs(d, B, live, seed=0, scale=1.0):
    """(table float32 [live + PAD_ROWS, d] whose rows >= live are NaN, slots int64 [B] inside the live rows; with B = 65
    three of them are -1, live and S - 1, and two pairs are duplicates)"""
    rs = np.random.RandomState(1000 * d + 10 * B + live + seed)
    S = live + PAD_ROWS
    table = (rs.standard_normal((S, d)) * scale).astype(F)
    table[live:] = np.nan
    slots = rs.randint(0, max(live, 1), B).astype(np.int64)
    if live == 0:
        slots[:] = rs.randint(-1, S, B)
    if B == 65:
        slots[60:63] = (-1, live, S - 1)
        slots[63], slots[64] = slots[0], slots[1]
    return table, slots


def entry_cases(d, k):
    """every (B, live, stride, offset) of the matrix for one (d, k)"""
    return [(B, live, stride, offset) for B in BS for live in lives(k) for stride, offset in LATTICES]
