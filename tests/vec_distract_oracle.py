"""The distractions of include/drqv2_hip.h ("distractions") restated in numpy, from the header's text and not from the
kernel (a helper module: not collected).  Everything is integer arithmetic: Python integers for the draws and the scalars
of an episode (uint32 by `& MASK`), int64 arrays for the pixels -- every intermediate of the contract fits int32, so the
wider type changes nothing.

DistractOracle keeps the two state words per environment and records which branches of the contract its inputs took
(BRANCHES); require_branches() is what a test calls before it draws anything, to see it fail, and again afterwards, so that
no test passes on inputs that skip a branch.  refused_calls() lists the DRQ_EARG cases of drq_vec_distract for the CPU and
the GPU test alike.
"""
import numpy as np

MASK = 0xFFFFFFFF
K1, K2, K3 = 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35
SIDE, FRAME = 84, (3, 84, 84)
MAX_CAMERA, MAX_COLOR, MAX_BANK = 8, 128, 65536

BRANCHES = ("tri_rising", "tri_falling",                                    # both sides of the fold (camera or bank)
            "clamp_left", "clamp_right", "clamp_top", "clamp_bottom",      # the camera's edge replication
            "background", "foreground",                                     # keyed pixels of either kind
            "colour_clamp_0", "colour_clamp_255",                           # the foreground colour leaves 0 .. 255
            "negative_X", "negative_Y",                                     # the floor division of the noise below zero
            "bank_reversal",                                                # the clip played backward
            "reset_row", "step_row")                                        # the state step's two sides


def fmix32(h):
    h &= MASK
    h ^= h >> 16
    h = h * 0x85EBCA6B & MASK
    h ^= h >> 13
    h = h * 0xC2B2AE35 & MASK
    h ^= h >> 16
    return h


def fmix32_array(h):
    """fmix32 of a uint64 array that holds uint32 values"""
    h = h & MASK
    h = h ^ (h >> 16)
    h = h * 0x85EBCA6B & MASK
    h = h ^ (h >> 13)
    h = h * 0xC2B2AE35 & MASK
    return h ^ (h >> 16)


def ramp():
    """the background of the built-in tasks, u8 [3][84][84]: 32 + ((i + j) >> 2) in all three channels"""
    i, j = np.mgrid[0:SIDE, 0:SIDE]
    return np.broadcast_to((32 + ((i + j) >> 2)).astype(np.uint8), FRAME).copy()


class DistractOracle:
    def __init__(self, N, seed=0, camera=0, camera_period=4, color=0, bg_mode=0, bg_alpha=256, dynamic=True, key=None,
                 bank=None):
        assert 0 <= camera <= MAX_CAMERA and camera_period >= 1 and 0 <= color <= MAX_COLOR and 0 <= bg_alpha <= 256
        assert bg_mode in (0, 1, 2) and (bg_mode == 0 or key is not None) and (bg_mode != 2 or bank is not None)
        self.N, self.seed = int(N), int(seed) & MASK
        self.P, self.period, self.C, self.mode, self.a, self.dynamic = camera, camera_period, color, bg_mode, bg_alpha, bool(dynamic)
        self.key = None if key is None else np.asarray(key, np.uint8).reshape(FRAME)
        self.bank = None if bank is None else np.asarray(bank, np.uint8)
        assert self.bank is None or self.bank.shape[2:] == FRAME
        self.episode = np.zeros(self.N, np.uint32)
        self.t = np.zeros(self.N, np.uint32)
        self.seen = dict.fromkeys(BRANCHES, 0)

    # ---- bookkeeping
    def _see(self, name, yes=True):
        self.seen[name] += int(bool(yes))

    def require_branches(self, *names):
        """AssertionError naming every branch of `names` (default: all of BRANCHES) that no input has taken yet"""
        missing = [n for n in (names or BRANCHES) if not self.seen[n]]
        assert not missing, f"the inputs never took: {', '.join(missing)}"

    def tri(self, v, m):
        assert v >= 0
        if m == 0:
            return 0
        r = v % (2 * m)
        self._see("tri_rising" if r <= m else "tri_falling")
        return r if r <= m else 2 * m - r

    # ---- the contract
    def state_step(self, first=None, reset_all=False):
        for e in range(self.N):
            if reset_all or (first is not None and first[e]):
                self.episode[e] = (int(self.episode[e]) + 1) & MASK
                self.t[e] = 0
                self._see("reset_row")
            else:
                self.t[e] = (int(self.t[e]) + 1) & MASK
                self._see("step_row")

    def frame_of(self, e, frame):
        """the distracted frame of environment e, u8 [3][84][84], from its frame and the state as it is"""
        episode, t = int(self.episode[e]), int(self.t[e])
        tau = (t & 0xFFFFF) if self.dynamic else 0
        base = self.seed ^ (e * K1 & MASK) ^ (episode * K2 & MASK)
        draw = lambda k: fmix32(base ^ ((256 + k) * K3 & MASK))
        P, C = self.P, self.C
        travel = tau // self.period
        ox = self.tri(draw(0) % (2 * P + 1) + (draw(2) % 3) * travel, 2 * P) - P
        oy = self.tri(draw(1) % (2 * P + 1) + (draw(3) % 3) * travel, 2 * P) - P
        rows, cols = np.arange(SIDE) + oy, np.arange(SIDE) + ox
        self._see("clamp_top", rows.min() < 0), self._see("clamp_bottom", rows.max() > SIDE - 1)
        self._see("clamp_left", cols.min() < 0), self._see("clamp_right", cols.max() > SIDE - 1)
        si, sj = np.clip(rows, 0, SIDE - 1), np.clip(cols, 0, SIDE - 1)
        s = frame[:, si[:, None], sj[None, :]].astype(np.int64)                       # [3][84][84], at the source pixel
        if self.key is None:
            background = np.zeros((SIDE, SIDE), bool)
        else:
            background = (s == self.key[:, si[:, None], sj[None, :]]).all(0)
        self._see("background", background.any()), self._see("foreground", (~background).any())
        out = np.empty(FRAME, np.int64)
        i, j = np.mgrid[0:SIDE, 0:SIDE]
        if self.mode == 1:
            vx, vy = draw(11) % 5 - 2, draw(12) % 5 - 2
            X, Y = j + tau * vx, i + tau * vy
            self._see("negative_X", X.min() < 0), self._see("negative_Y", Y.min() < 0)
            gx, gy = X // 12, Y // 12                                                 # numpy's // rounds toward minus infinity
            fx, fy = X - 12 * gx, Y - 12 * gy
            assert fx.min() >= 0 and fx.max() <= 11 and fy.min() >= 0 and fy.max() <= 11
            d10 = draw(10)
        for c in range(3):
            gain = 256 - C + draw(4 + c) % (2 * C + 1)
            off = draw(7 + c) % (C + 1) - (C >> 1)
            raw = ((s[c] * gain + 128) >> 8) + off
            self._see("colour_clamp_0", (raw[~background] < 0).any())
            self._see("colour_clamp_255", (raw[~background] > 255).any())
            f = np.clip(raw, 0, 255)
            if self.mode == 0:
                n = s[c]
            elif self.mode == 1:
                def L(gy_, gx_):
                    h = np.uint64(d10 ^ (c * K1 & MASK)) ^ ((gy_ & MASK).astype(np.uint64) * K2 & MASK) \
                        ^ ((gx_ & MASK).astype(np.uint64) * K3 & MASK)
                    return (fmix32_array(h) >> 24).astype(np.int64)
                top = L(gy, gx) * (12 - fx) + L(gy, gx + 1) * fx
                bot = L(gy + 1, gx) * (12 - fx) + L(gy + 1, gx + 1) * fx
                n = (top * (12 - fy) + bot * fy + 72) // 144
            else:
                M, F = self.bank.shape[:2]
                m = draw(10) % M
                v = draw(11) % F + tau
                if F > 1:
                    self._see("bank_reversal", v % (2 * (F - 1)) > F - 1)
                n = self.bank[m, self.tri(v, F - 1), c].astype(np.int64)
            b = (self.a * n + (256 - self.a) * s[c] + 128) >> 8
            out[c] = np.where(background, b, f)
        assert out.min() >= 0 and out.max() <= 255
        return out.astype(np.uint8)

    def frames(self, frame):
        """the distracted frames of the state as it is (the entry with hold = 1)"""
        frame = np.asarray(frame, np.uint8).reshape((self.N,) + FRAME)
        return np.stack([self.frame_of(e, frame[e]) for e in range(self.N)])

    def apply(self, frame, first=None, reset_all=False):
        """one call of the entry: the state step, then the frames"""
        self.state_step(first, reset_all)
        return self.frames(frame)


# ---- the refused calls -------------------------------------------------------------------------------------------
ARGS = ("frame_in", "first", "key", "bank", "episode", "t", "N", "seed", "reset_all", "hold", "camera", "camera_period",
        "color", "bg_mode", "bg_alpha", "dynamic", "M", "F", "frame_out")


def good_call(frame_in, first, key, bank, state, frame_out, N=3):
    """a dict of arguments the entry accepts (mode 2, every pointer given); the addresses are the caller's: frame_in and
    frame_out of N frames that do not overlap, key of one frame, bank of 2 x 3 frames, all 16-byte aligned; state of
    2 N words, 4-byte aligned"""
    return dict(frame_in=frame_in, first=first, key=key, bank=bank, episode=state, t=state + 4 * N, N=N, seed=5, reset_all=0,
                hold=0, camera=8, camera_period=1, color=128, bg_mode=2, bg_alpha=256, dynamic=1, M=2, F=3, frame_out=frame_out)


def refused_calls(frame_in, first, key, bank, state, frame_out, N=3):
    """[(why, argument tuple)]: every DRQ_EARG case of the header, each one change away from good_call()"""
    good = good_call(frame_in, first, key, bank, state, frame_out, N)
    bad = [("null " + k, {k: None}) for k in ("frame_in", "frame_out", "episode", "t")]
    bad += [("N = 0", dict(N=0)), ("N < 0", dict(N=-1)), ("N > INT32_MAX", dict(N=2 ** 31))]
    bad += [(f"{k} = {v}", {k: v}) for k in ("reset_all", "hold", "dynamic") for v in (-1, 2)]
    bad += [("hold with reset_all", dict(hold=1, reset_all=1))]
    bad += [(f"{k} = {v}", {k: v}) for k, vs in (("camera", (-1, 9)), ("camera_period", (0, -3)), ("color", (-1, 129)),
                                                 ("bg_alpha", (-1, 257)), ("bg_mode", (-1, 3))) for v in vs]
    bad += [("noise without a key", dict(bg_mode=1, key=None)), ("bank without a key", dict(key=None)),
            ("mode 2 without a bank", dict(bank=None))]
    bad += [(f"mode 2 with {k} = {v}", {k: v}) for k in ("M", "F") for v in (0, -1, MAX_BANK + 1)]
    bad += [("frame_out == frame_in", dict(frame_out=frame_in)),
            ("frame_out inside frame_in", dict(frame_out=frame_in + 16)),
            ("frame_in inside frame_out", dict(frame_in=frame_out + (N - 1) * 3 * 84 * 84))]
    bad += [(f"{k} not 16-byte aligned", {k: good[k] + 8}) for k in ("frame_in", "frame_out", "key", "bank")]
    bad += [(f"{k} not 4-byte aligned", {k: good[k] + 2}) for k in ("episode", "t")]
    return [(why, tuple(dict(good, **change)[k] for k in ARGS)) for why, change in bad]


def accepted_calls(frame_in, first, key, bank, state, frame_out, N=3):
    """argument tuples at the edges of what the entry accepts (the GPU test launches them): what mode 0 and 1 do not read
    may be anything"""
    good = good_call(frame_in, first, key, bank, state, frame_out, N)
    ok = [{}, dict(first=None), dict(bg_mode=0, key=None, bank=None, M=0, F=0), dict(bg_mode=1, bank=None, M=-1, F=0),
          dict(bg_mode=0, bank=bank + 8), dict(hold=1), dict(reset_all=1), dict(camera=0, color=0, bg_alpha=0, camera_period=2 ** 31 - 1)]
    return [tuple(dict(good, **change)[k] for k in ARGS) for change in ok]


# ---- the runs the GPU tests compare -----------------------------------------------------------------------------------
STEPS, SEED = 40, 14          # under this seed the noise drifts toward negative X and negative Y in some episodes
# name -> (N, the oracle's keyword arguments but key and bank, keyed, banked).  Strengths at both ends of their ranges
# (camera 8 at period 1, colour 128 on frames that hold 0 and 255), alpha 0, 77 and 256, dynamic on and off, no key
SCENARIOS = {
    "camera8-colour128-unkeyed": (3, dict(camera=8, camera_period=1, color=128), False, False),
    "noise-alpha77": (3, dict(camera=2, camera_period=3, color=16, bg_mode=1, bg_alpha=77), True, False),
    "noise-static": (1, dict(camera=8, camera_period=1, bg_mode=1, dynamic=False), True, False),
    "bank": (3, dict(bg_mode=2), True, True),
    "bank-camera-colour-static": (1, dict(camera=3, camera_period=2, color=40, bg_mode=2, bg_alpha=200, dynamic=False), True, True),
    "identity-bank-alpha0": (1, dict(bg_mode=2, bg_alpha=0), True, True),
    "identity-keyed": (3, dict(), True, False),
    "identity-unkeyed": (1, dict(bg_alpha=0), False, False),
}
IDENTITY = tuple(k for k in SCENARIOS if k.startswith("identity"))
_RUNS = {}


def scene(r, key):
    """a frame u8 [3][84][84]: the key (or noise, without one) with a few rectangles over it -- one black, one white, the
    others random -- so that the frame holds 0 and 255 and, against the key, background and foreground"""
    frame = key.copy() if key is not None else r.randint(0, 256, FRAME).astype(np.uint8)
    for k in range(4):
        i, j, h, w = r.randint(0, 70), r.randint(0, 70), r.randint(3, 14), r.randint(3, 14)
        value = (0, 255)[k] if k < 2 else r.randint(0, 256, (3, 1, 1))
        frame[:, i:i + h, j:j + w] = value
    frame[:, 0, 0], frame[:, 83, 83] = 255, 0          # the corners the camera replicates
    return frame


def first_flags(s, N):
    """the flags of step s >= 1: environment e starts an episode when s + 3 e is a multiple of 13 -- three episodes per
    lane in 40 steps, staggered"""
    return np.array([(s + 3 * e) % 13 == 0 for e in range(N)], np.uint8)


def run_of(name):
    """the oracle's run of a scenario, computed once, shared, never modified: {"N", "kwargs", "key", "bank", "frames":
    [STEPS] u8 [N][3][84][84], "firsts": [STEPS] u8 [N] (None for step 0, the reset of all), "outs", "states": [STEPS]
    (episode, t), "oracle"}"""
    if name not in _RUNS:
        N, kw, keyed, banked = SCENARIOS[name]
        r = np.random.RandomState(sorted(SCENARIOS).index(name) + 100)
        key = r.randint(0, 256, FRAME).astype(np.uint8) if keyed else None
        bank = r.randint(0, 256, (2, 3) + FRAME).astype(np.uint8) if banked else None
        o = DistractOracle(N, seed=SEED, key=key, bank=bank, **kw)
        run = dict(N=N, kwargs=kw, key=key, bank=bank, frames=[], firsts=[], outs=[], states=[], oracle=o)
        for s in range(STEPS):
            frame = np.stack([scene(r, key) for _ in range(N)])
            first = None if s == 0 else first_flags(s, N)
            run["frames"].append(frame)
            run["firsts"].append(first)
            run["outs"].append(o.apply(frame, first, reset_all=s == 0))
            run["states"].append((o.episode.copy(), o.t.copy()))
        _RUNS[name] = run
    return _RUNS[name]
