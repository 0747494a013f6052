"""numpy restatement of the exploration bonus (a helper module: not collected).  The contract is the comment of
include/drqv2_hip.h ("exploration bonus"), stated here once more in int64 and uint32 arithmetic:

  cells       frame uint8 [N, 3, 84, 84] -> s int64 [N, 441]: the sum over the 3 channels and the 4 x 4 pixels of block
              (gy, gx) of the 21 x 21 grid, i = gy * 21 + gx
  centring    v_i = 441 * s_i - sum_j s_j
  projection  p_j = sum_i a(j, i) * v_i in int64, a(j, i) = +1 if fmix32(seed ^ (j * 441 + i) * 0x9E3779B9) & 1 else -1
  code        sum_j (p_j > 0) << j,  1 <= bits <= 24
  step        update: count[code_n] += 1 for every n, THEN c_n = count[code_n]; otherwise c_n = count[code_n] alone
  bonus       np.float32(beta) / np.sqrt(np.float32(c)); beta for c = 0; reward + bonus is one float32 add

It reads nothing but its arguments; the reference has no counterpart.
"""
import functools

import numpy as np

F = np.float32
M32 = 0xFFFFFFFF
GRID, CELLS, MAX_BITS = 21, 441, 24
FRAME_SHAPE = (3, 84, 84)


def fmix32(h):
    """the murmur3 finaliser on Python integers or uint64 arrays of 32-bit values"""
    h = h & M32
    h = h ^ (h >> 16)
    h = h * 0x85EBCA6B & M32
    h = h ^ (h >> 13)
    h = h * 0xC2B2AE35 & M32
    h = h ^ (h >> 16)
    return h


@functools.lru_cache(None)
def signs(bits, seed):
    """a(j, i) as int64 [bits, 441] of +1 / -1 (shared: never modified)"""
    k = np.arange(bits * CELLS, dtype=np.uint64)
    h = fmix32(np.uint64(seed & M32) ^ (k * np.uint64(0x9E3779B9) & np.uint64(M32)))
    a = np.where(h & np.uint64(1), 1, -1).astype(np.int64).reshape(bits, CELLS)
    a.setflags(write=False)
    return a


def sign(j, i, seed):
    """a(j, i) by the words of the contract, on Python integers"""
    return 1 if fmix32((seed & M32) ^ ((j * CELLS + i) * 0x9E3779B9 & M32)) & 1 else -1


def cells(frame):
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.shape[1:] == FRAME_SHAPE, (frame.dtype, frame.shape)
    n = frame.shape[0]
    return frame.astype(np.int64).reshape(n, 3, GRID, 4, GRID, 4).sum(axis=(1, 3, 5)).reshape(n, CELLS)


def centred(s):
    return CELLS * s - s.sum(axis=1, keepdims=True)


def projections(frame, bits, seed):
    """p int64 [N, bits]"""
    return centred(cells(frame)) @ signs(bits, seed).T


def codes(frame, bits, seed):
    assert 1 <= bits <= MAX_BITS
    p = projections(frame, bits, seed)
    return ((p > 0).astype(np.int64) << np.arange(bits, dtype=np.int64)).sum(axis=1).astype(np.int32)


def bonus_of(count, beta):
    """float32 [N]: beta / sqrt(c), beta where c = 0"""
    c = np.asarray(count, dtype=np.int32)
    root = np.sqrt(np.where(c == 0, 1, c).astype(F))          # the conversion and the root round once each
    return np.where(c == 0, F(beta), F(beta) / root).astype(F)


class SimHashOracle:
    def __init__(self, bits, beta, seed):
        assert 1 <= bits <= MAX_BITS
        self.bits, self.beta, self.seed = bits, F(beta), seed & M32
        self.table = np.zeros(1 << bits, np.int32)

    def count(self, code, update=True):
        """one step over the codes of the N environments: (counts int32 [N], bonus float32 [N])"""
        code = np.asarray(code, dtype=np.int64)
        if update:
            np.add.at(self.table, code, 1)            # every increment first, duplicates included
        c = self.table[code].copy()
        return c, bonus_of(c, self.beta)

    def step(self, frame, reward=None, update=True):
        """(codes int32 [N], counts int32 [N], bonus float32 [N], reward + bonus float32 [N] or None)"""
        code = codes(frame, self.bits, self.seed)
        c, b = self.count(code, update)
        total = None if reward is None else (np.asarray(reward, dtype=F) + b).astype(F)
        return code, c, b, total

    def distinct(self):
        return int(np.count_nonzero(self.table))


# ------------------------------------------------------------------------------------------------ inputs the tests share
def random_frames(n, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n,) + FRAME_SHAPE).astype(np.uint8)


def sequence(n, seed, steps=6):
    """`steps` frame batches uint8 [n, 3, 84, 84] and rewards float32 [n], rows copied explicitly:
       step 0  random frames
       step 1  random frames; row 0 all 0 and (n > 1) row 1 all 255: both have every projection zero
       step 2  step 0 again, whole (frames that repeat across steps)
       step 3  random frames; (n > 1) the last row is a copy of row 0, (n > 2) row 2 too: duplicates inside a step
       step 4  row i = row (i // 2) of step 3 (n > 1: every frame twice inside the step, and again across steps)
       step 5  random frames; row 0 is step 1's all-0 frame again
    further steps are random."""
    rs = np.random.RandomState(seed)
    draw = lambda: rs.randint(0, 256, size=(n,) + FRAME_SHAPE).astype(np.uint8)
    frames = [draw() for _ in range(steps)]
    frames[1][0] = 0
    if n > 1:
        frames[1][1] = 255
    frames[2] = frames[0].copy()
    if n > 1:
        frames[3][n - 1] = frames[3][0]
    if n > 2:
        frames[3][2] = frames[3][0]
    frames[4] = frames[3][np.arange(n) // 2].copy()
    frames[5][0] = frames[1][0]
    rewards = [rs.uniform(-1, 2, size=n).astype(F) for _ in range(steps)]
    return frames, rewards


def run(n, bits, beta, seed, frames, rewards):
    """the oracle over a sequence of counting steps: per step (codes, counts, bonus, total, the table after it, distinct)"""
    o = SimHashOracle(bits, beta, seed)
    out = []
    for f, r in zip(frames, rewards):
        out.append(o.step(f, r) + (o.table.copy(), o.distinct()))
    return out


def covers(out, n):
    """a run holds what it is there for: a duplicate code inside a step (n > 1) and at least two distinct codes"""
    dup = any(len(np.unique(step[0])) < n for step in out)
    return (dup or n == 1) and out[-1][5] >= 2


def refused_calls(FR, TAB, OUT, REW):
    """the argument lists drq_explore_simhash_step must refuse, around one well-formed list over four base addresses
    (the three outputs 0x100 apart from OUT, reward and reward_out 0x100 apart from REW)"""
    #     frame N bits seed beta update count code_out count_out    bonus_out    reward reward_out
    ok = [FR, 5, 16, 7, 0.1, 1, TAB, OUT, OUT + 0x100, OUT + 0x200, REW, REW + 0x100]
    sub = lambda k, v, base=ok: base[:k] + [v] + base[k + 1:]
    plain = sub(11, None, sub(10, None))                                   # no reward: well formed as well
    bad = [sub(k, None) for k in (0, 6, 7, 8, 9)]                          # every required pointer
    bad += [sub(k, None, plain) for k in (0, 6, 7, 8, 9)]
    bad += [sub(11, None), sub(10, None)]                                  # reward without reward_out, and the reverse
    bad += [sub(1, v) for v in (0, -1, 2 ** 31)]                           # N
    bad += [sub(2, v) for v in (0, -1, 25, 32, 2 ** 31 - 1)]               # bits
    bad += [sub(5, v) for v in (2, -1)]                                    # update
    bad += [sub(k, ok[k] + m) for k in (0, 6, 7, 8, 9, 10, 11) for m in (1, 2)]      # a pointer not 4-byte aligned
    assert len(bad) == 5 + 5 + 2 + 3 + 5 + 2 + 14
    return bad
