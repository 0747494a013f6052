"""Episode statistics on the GPU: drq_vec_stats_step / _reset on poisoned, guarded memory against the numpy restatement of
the contract (tests/vec_stats_oracle.py) after EVERY step, the publish protocol of VecEpisodeStats, and the statistics
next to a VecFrameReplay that must not notice them.

Bounds.  ret, len, done, the log, episodes, length_sum, min_return and max_return are compared bit for bit: a running
return is one float32 add per step in step order, on the device as in numpy, and the others are integers or a min / max of
the same float32 values.  return_sum adds `episodes` float32 returns in float64 in an order of the kernel's own: whatever
the order, that is episodes - 1 roundings of partial sums none of which exceeds sum |return_j| in magnitude, each at most
2^-53 of it, so |return_sum - math.fsum| <= episodes * 2^-53 * sum |return_j| (fsum is the exact sum rounded once more,
which the spare one of the `episodes` covers).  A derived bound, not a measured one.

The reward of a reset row is NaN in every stream here: the contract says it is not read, and a NaN that was would stay in
the running return."""
import math

import numpy as np
import pytest
import torch

from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p, rs_
from tests.vec_stats_oracle import StatsOracle

pytestmark = pytest.mark.gpu
EARG = -1
NAMES = ("ret", "len", "done", "header", "log_return", "log_length", "log_env", "log_row")


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_stats_step" in _lib.PROTOTYPES, "the episode statistics entries are missing"
    return _lib.load()


def alloc_state(N, W, kind="out"):
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    shapes = ((N, f32), (N, i32), (N, i32), (8, i64), (W, f32), (W, i32), (W, i32), (W, i64))
    return [poison.alloc((n,), dt, "cuda", name=name, kind=kind) for name, (n, dt) in zip(NAMES, shapes)]


def stream(N, T, p_reset, seed, forced=()):
    """[(reward float32 [N], first bool [N] or None)]; forced: {row: "all" | "none" | "null" | [environments]}"""
    r = rs_(seed)
    forced = dict(forced)
    out = []
    for t in range(T):
        reward = r.standard_normal(N).astype(np.float32)
        first = r.uniform(size=N) < p_reset
        how = forced.get(t)
        if how == "all":
            first[:] = True
        elif how in ("none", "null"):
            first[:] = False
        elif how is not None:
            first[list(how)] = True
        out.append((reward, None if how == "null" else first))
    return out


def device_inputs(reward, first, t):
    """the inputs between guard bands; NaN where the row is a reset row: that reward is a dummy"""
    reward = reward.copy()
    reward[slice(None) if t == 0 else (first if first is not None else slice(0, 0))] = np.nan
    return dev(torch.from_numpy(reward), "reward"), None if first is None else dev(torch.from_numpy(first.astype(np.uint8)), "first")


def compare(state, o, where):
    """the device state against the oracle, every bit but return_sum's"""
    torch.cuda.synchronize()
    ret, ln, done, header, lr, ll, le, lrow = (s.cpu().numpy() for s in state)
    assert np.array_equal(ret.view(np.int32), o.ret.view(np.int32)), where
    assert np.array_equal(ln, o.len) and np.array_equal(done, o.done), where
    log, _ = o.log()
    assert np.array_equal(lr.view(np.int32), np.ascontiguousarray(log["return"]).view(np.int32)), where
    assert np.array_equal(ll, log["length"]) and np.array_equal(le, log["env"]) and np.array_equal(lrow, log["row"]), where
    rets = [float(c[0]) for c in o.counted]
    raw = header.view(np.uint8)
    assert header[0] == o.rows and header[1] == len(rets) and header[2] == sum(int(c[1]) for c in o.counted), where
    mn, mx = raw[32:40].view(np.float32)
    assert mn == (min(rets) if rets else np.inf) and mx == (max(rets) if rets else -np.inf), where
    assert not raw[40:].any(), where
    got, want, mass = float(raw[24:32].view(np.float64)[0]), math.fsum(rets), math.fsum(abs(x) for x in rets)
    print(f"{where}: episodes {len(rets)}, return_sum off by {abs(got - want):.3e}, bound {len(rets) * 2.0 ** -53 * mass:.3e}")
    assert abs(got - want) <= len(rets) * 2.0 ** -53 * mass, where


def run(lib, N, W, limit, rows, every=1):
    state = alloc_state(N, W)
    assert lib.drq_vec_stats_reset(*map(p, state), N, W, None) == 0
    o = StatsOracle(N, W, limit)
    compare(state, o, "reset")
    for t, (reward, first) in enumerate(rows):
        d_reward, d_first = device_inputs(reward, first, t)
        assert lib.drq_vec_stats_step(*map(p, state), N, W, limit, t, p(d_reward), p(d_first), None) == 0
        o.step(reward, first)
        if t % every == 0 or t == len(rows) - 1:
            compare(state, o, f"N={N} W={W} row {t}")
    return state, o


# ------------------------------------------------------------------------------------------------ the entry
# one chunk is 1,024 environments: below, at and above one, and more than two.  W = 100 and 1000 are smaller than what
# the all-reset row counts, in one chunk (1,024 > 100) and across three (2,500 > 1,000): the newest records must stay
FORCED = {10: "all", 11: "none", 12: "all", 20: [0], 21: [0], 30: "null", 31: "all", 32: "all"}


@pytest.mark.parametrize("N,W", [(1, 8), (3, 7), (64, 32), (1023, 4096), (1024, 100), (1025, 4096), (2500, 1000)])
def test_step_matches_the_oracle_after_every_step(lib, N, W):
    rows = stream(N, 48, 0.2, seed=N, forced=FORCED)
    state, o = run(lib, N, W, 0, rows)
    assert len(o.counted) >= 2 * N and o.done.min() >= 2           # rows 12 and 31 close an episode of every environment
    if W < N:
        assert len(o.counted) > W                                  # the log did wrap, within single calls too


def test_limit_counts_the_first_two_of_every_environment(lib):
    N, k = 70, 2
    state, o = run(lib, N, 256, k, stream(N, 60, 0.2, seed=5, forced={20: "none", 21: "all", 30: "none", 31: "all", 40: "none", 41: "all"}))
    assert len(o.counted) == k * N and (o.done > k).all() and o.snapshot().complete


def test_log_wraps_at_w_8(lib):
    state, o = run(lib, 3, 8, 0, stream(3, 60, 0.3, seed=1))
    assert len(o.counted) > 30


def test_reset_puts_everything_back(lib):
    N, W = 37, 16
    rows = stream(N, 20, 0.3, seed=2)
    state, o = run(lib, N, W, 0, rows, every=100)
    assert len(o.counted) > W
    assert lib.drq_vec_stats_reset(*map(p, state), N, W, None) == 0
    o = StatsOracle(N, W)
    compare(state, o, "after reset")
    for t, (reward, first) in enumerate(rows[:6]):                 # row 0 is a reset row again, whatever the flags say
        d_reward, d_first = device_inputs(reward, first, t)
        assert lib.drq_vec_stats_step(*map(p, state), N, W, 0, t, None if t == 0 else p(d_reward), p(d_first), None) == 0
        o.step(reward, first)
        compare(state, o, f"row {t} after reset")
    assert o.len.max() == 5


def test_refusals_write_nothing(lib):
    N, W = 5, 8
    state = [p(s) for s in alloc_state(N, W, kind="refused")]
    reward, first = dev(torch.zeros(N), "reward"), dev(torch.ones(N, dtype=torch.uint8), "first")
    mirror = poison.alloc((64 + 20 * W + 8,), torch.uint8, "cuda", name="mirror", kind="refused")
    step = lambda st=state, n=N, w=W, lim=0, row=1, rew=p(reward): lib.drq_vec_stats_step(*st, n, w, lim, row, rew, p(first), None)
    for k in range(8):
        st = state[:k] + [None] + state[k + 1:]
        assert step(st) == EARG and lib.drq_vec_stats_reset(*st, N, W, None) == EARG, k
        if k >= 3:
            assert lib.drq_vec_stats_publish(*st[3:], W, p(mirror), 1, None) == EARG, k
    for kw in (dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(w=0), dict(w=-8), dict(lim=-1), dict(row=-1), dict(rew=None)):
        assert step(**kw) == EARG, kw
    assert step(state[:3] + [state[3] + 4] + state[4:]) == EARG and step(state[:7] + [state[7] + 4]) == EARG
    assert lib.drq_vec_stats_reset(*state, 0, W, None) == EARG and lib.drq_vec_stats_reset(*state, N, 0, None) == EARG
    assert lib.drq_vec_stats_publish(*state[3:], 0, p(mirror), 1, None) == EARG
    assert lib.drq_vec_stats_publish(*state[3:], W, None, 1, None) == EARG
    assert lib.drq_vec_stats_publish(*state[3:], W, p(mirror) + 4, 1, None) == EARG
    poison.check()                                                 # nothing was written by a refused call


# ------------------------------------------------------------------------------------------------ the class
def same_snapshot(got, want):
    assert (got.rows, got.episodes, got.length_sum) == (want.rows, want.episodes, want.length_sum)
    assert got.min_return == want.min_return and got.max_return == want.max_return
    assert got.lost == want.lost and got.complete == want.complete
    assert got.records.dtype == want.records.dtype and got.records.tobytes() == want.records.tobytes()
    assert abs(got.return_sum - want.return_sum) <= want.episodes * 2.0 ** -53 * want.abs_return_sum
    if want.episodes:
        assert got.mean_return == got.return_sum / got.episodes and got.mean_length == want.mean_length
    else:
        assert math.isnan(got.mean_return) and math.isnan(got.mean_length)


def test_publish_protocol():
    """W = 7: odd (the int64 rows of the mirror need their padding) and small enough to wrap"""
    from drqv2_amd.replay import VecEpisodeStats
    N, W = 5, 7
    rows = stream(N, 60, 0.25, seed=3)
    st, o = VecEpisodeStats(N, "cuda", log_size=W), StatsOracle(N, W)
    assert st.poll() is None
    same_snapshot(st.read(), o.snapshot())                         # before any step: the initial state
    cu = lambda a: None if a is None else torch.from_numpy(a).cuda()

    def steps(lo, hi):
        for t in range(lo, hi):
            st.step(cu(rows[t][0]), cu(rows[t][1]))
            o.step(*rows[t])

    steps(0, 10)
    early, early_want = st.read(), o.snapshot()
    same_snapshot(early, early_want)
    assert early.seq == 2 and st.poll().seq == 2
    mirror = st._mirrors[1][1]
    kept = mirror.copy()
    for k in range(2):                                             # two further publishes: the mirror of `early` stays
        steps(10 + 5 * k, 15 + 5 * k)
        st.publish()
    torch.cuda.synchronize()
    assert np.array_equal(mirror, kept) and st.poll().seq == 4
    same_snapshot(early, early_want)
    same_snapshot(st.poll(), o.snapshot())
    prev = st.poll().episodes
    for k in range(4):                                             # four publishes with steps in between, one synchronise
        steps(20 + 10 * k, 30 + 10 * k)
        assert st.publish() == 5 + k
    torch.cuda.synchronize()
    snap, want = st.poll(), o.snapshot()
    assert snap.seq == 8 and not np.array_equal(mirror, kept)      # ... and the second reused the mirror of `early`
    same_snapshot(snap, want)
    assert want.episodes > prev + W and want.lost > 0              # the log wrapped since `prev`
    for since in (prev, want.episodes - 3, want.episodes, 0):
        (g_rec, g_missed), (w_rec, w_missed) = snap.since(since), want.since(since)
        assert g_missed == w_missed and g_rec.tobytes() == w_rec.tobytes(), since
    assert snap.since(prev)[1] == want.episodes - W - prev
    assert torch.equal(st.episode_return.cpu(), torch.from_numpy(o.ret))
    assert torch.equal(st.episode_length.cpu(), torch.from_numpy(o.len))
    st.reset()                                                     # one object, many evaluations
    o.reset()
    steps(0, 8)
    same_snapshot(st.read(), o.snapshot())


def test_host_inputs_and_the_limit():
    """numpy rows go through the pinned staging; max_episodes_per_env = 2 completes"""
    from drqv2_amd.replay import VecEpisodeStats
    N, k = 9, 2
    st, o = VecEpisodeStats(N, "cuda", log_size=64, max_episodes_per_env=k), StatsOracle(N, 64, k)
    snap = None
    for t, (reward, first) in enumerate(stream(N, 80, 0.2, seed=4)):
        args = (reward.astype(np.float64).reshape(N, 1), first) if t % 2 else (torch.from_numpy(reward), torch.from_numpy(first))
        st.step(*args)
        o.step(reward, first)
        if t % 20 == 19:
            snap = st.read()
            same_snapshot(snap, o.snapshot())
    assert snap.complete and snap.episodes == k * N


def test_next_to_the_ring():
    """a VecFrameReplay fed 40 steps with stats.step() after every add() on the same device tensors, and a twin fed
    without: the stores hold and draw the same bits, the statistics are the oracle's, act_batch() still runs"""
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    from tests.test_hip_vec_frames import store_stream
    from tests.test_hip_vec_replay import make_agent
    R, N, A = 16, 6, 3
    _, rows = store_stream(R, N, 40, seed=7)
    a, b = (VecFrameReplay(R, N, A, 3, 0.99, "cuda", seed=9, guard_rows=2) for _ in range(2))
    st, o = VecEpisodeStats(N, "cuda", log_size=32), StatsOracle(N, 32)
    cu = lambda x: torch.from_numpy(x).cuda()
    for frame, action, reward, discount, first in rows:
        d = [cu(x) for x in (frame, action, reward, discount, first)]
        a.add(*d)
        st.step(d[2], d[4])
        b.add(*(cu(x) for x in (frame, action, reward, discount, first)))
        o.step(reward, first)
    for name in ("first", "reward", "discount", "action", "frames"):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), name
    ba, bb = a.sample(24), b.sample(24)
    for k in range(5):
        assert torch.equal(ba[k].view(torch.uint8), bb[k].view(torch.uint8)), k
    assert torch.equal(a.last_steps, b.last_steps)
    snap = st.read()
    same_snapshot(snap, o.snapshot())
    assert snap.episodes >= 2 * (N - 1) and snap.rows == 40
    act = make_agent(A).act_batch(a.observation(), 0, True)
    assert act.shape == (N, A) and bool(torch.isfinite(act).all())
