"""Episode statistics for vectorised collection (VecEpisodeStats, drq_vec_stats_step / _publish / _reset): everything
that needs no GPU.  The numpy restatement of the contract (tests/vec_stats_oracle.py) against the reference's literal
book-keeping loop (train.py:133,186,189), its edge cases, the class's validation on the CPU, and the argument errors the
library reports before any launch."""
import math
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests.vec_stats_oracle import StatsOracle

NEW = ("drq_vec_stats_step", "drq_vec_stats_publish", "drq_vec_stats_reset")
EARG = -1


def test_header_prototypes_and_build_list():
    for name in NEW:
        abi.assert_prototype(name)
    from drqv2_amd import build
    assert "vecstats.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecstats.hip"))
    assert "episode statistics" in abi.text()


# ------------------------------------------------------------------------------------------------ oracle against train.py
def reference_loop(rewards, firsts):
    """one environment, the reference's own loop: `episode_step, episode_reward = 0, 0` (train.py:133), per step
    `episode_reward += time_step.reward; episode_step += 1` (:186,189), logged and set back when the episode ends
    (:147-155, :161-168).  rewards are np.float32, as the reference's environments hand them out (dmc.py:185-189); a
    reset row carries no reward.  Returns [(episode_reward, episode_step, row of the reset that ended it)]"""
    out = []
    episode_step, episode_reward = 0, np.float32(0)
    for t, (r, f) in enumerate(zip(rewards, firsts)):
        if f or t == 0:
            if episode_step >= 1:
                out.append((episode_reward, episode_step, t))
            episode_step, episode_reward = 0, np.float32(0)
            continue
        episode_reward += r
        episode_step += 1
    return out


def test_oracle_equals_the_reference_loop_per_environment():
    N, T = 5, 200
    r = np.random.RandomState(0)
    rewards = r.standard_normal((T, N)).astype(np.float32)
    firsts = r.uniform(size=(T, N)) < 0.1
    o = StatsOracle(N, W=4096)
    for t in range(T):
        o.step(rewards[t], firsts[t])
    rec = o.snapshot().records
    assert len(rec) > 5 * N
    for e in range(N):
        want = reference_loop(rewards[:, e], firsts[:, e])
        got = rec[rec["env"] == e]
        assert len(got) == len(want) >= 5
        for g, (ret, steps, row) in zip(got, want):
            assert type(ret) is np.float32 and g["return"].tobytes() == ret.tobytes()
            assert (int(g["length"]), int(g["row"])) == (steps, row)
    # the records are in the order (row, env), the totals are those of the records
    keys = [(int(x["row"]), int(x["env"])) for x in rec]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    s = o.snapshot()
    assert s.episodes == len(rec) and s.length_sum == int(rec["length"].sum()) and s.rows == T
    assert s.return_sum == math.fsum(float(x) for x in rec["return"])
    assert s.min_return == float(rec["return"].min()) and s.max_return == float(rec["return"].max())
    assert s.mean_return == s.return_sum / s.episodes and s.mean_length == s.length_sum / s.episodes


# ------------------------------------------------------------------------------------------------ edge cases of the oracle
def test_no_flags_no_episodes():
    o = StatsOracle(3)
    for t in range(20):
        o.step(np.ones(3, np.float32), None)
    s = o.snapshot()
    assert s.episodes == 0 and len(s.records) == 0 and math.isnan(s.mean_return) and math.isnan(s.mean_length)
    assert s.min_return == float("inf") and s.max_return == float("-inf") and s.rows == 20
    assert np.array_equal(o.len, [19, 19, 19]) and np.array_equal(o.ret, np.full(3, 19, np.float32))   # row 0 is a reset row


def test_two_resets_in_a_row_leave_no_empty_record():
    o = StatsOracle(2)
    one = np.ones(2, np.float32)
    for first in ([0, 0], [0, 0], [0, 0], [1, 0], [1, 0], [0, 0], [1, 0]):
        o.step(one, np.array(first, bool))
    rec = o.snapshot().records
    assert [(float(x["return"]), int(x["length"]), int(x["env"]), int(x["row"])) for x in rec] == [(2.0, 2, 0, 3), (1.0, 1, 0, 6)]
    assert o.done[0] == 2 and o.done[1] == 0 and o.len[1] == 6


def test_all_environments_reset_in_one_step_rank_in_env_order():
    N = 7
    o = StatsOracle(N)
    o.step(np.zeros(N, np.float32))
    o.step(np.arange(N, dtype=np.float32))
    o.step(np.zeros(N, np.float32), np.ones(N, bool))
    rec = o.snapshot().records
    assert rec["env"].tolist() == list(range(N)) and rec["return"].tolist() == list(range(N))
    log, written = o.log()
    assert written[:N].all() and not written[N:].any() and log["env"][:N].tolist() == list(range(N))


def test_log_wraps_at_w_8():
    N, W = 3, 8
    o = StatsOracle(N, W=W)
    r = np.random.RandomState(1)
    for t in range(60):
        o.step(r.standard_normal(N).astype(np.float32), r.uniform(size=N) < 0.3)
    s = o.snapshot()
    assert s.episodes > 30 and len(s.records) == W and s.lost == s.episodes - W
    assert s.records.tolist() == np.array(o.counted[-W:], dtype=s.records.dtype).tolist()
    log, written = o.log()
    assert written.all()
    for j in range(s.episodes - W, s.episodes):
        assert log[j % W] == np.array(o.counted[j], dtype=log.dtype)
    part, missed = s.since(s.episodes - 3)
    assert len(part) == 3 and missed == 0 and part[-1] == s.records[-1]
    part, missed = s.since(s.episodes - W - 5)
    assert len(part) == W and missed == 5
    part, missed = s.since(s.episodes)
    assert len(part) == 0 and missed == 0


def test_limit_counts_the_first_two_episodes_of_every_environment():
    N, k = 4, 2
    o, free = StatsOracle(N, limit=k), StatsOracle(N)
    r = np.random.RandomState(2)
    complete_at = None
    for t in range(120):
        rew, first = r.standard_normal(N).astype(np.float32), r.uniform(size=N) < 0.15
        o.step(rew, first)
        free.step(rew, first)
        if o.snapshot().complete and complete_at is None:
            complete_at = t
    s = o.snapshot()
    assert complete_at is not None and complete_at < 119 and s.complete and s.episodes == k * N
    assert (o.done > k).all()                                      # later episodes went by uncounted
    all_rec = free.snapshot().records
    for e in range(N):
        assert np.array_equal(s.records[s.records["env"] == e], all_rec[all_rec["env"] == e][:k])
    assert np.array_equal(o.ret, free.ret) and np.array_equal(o.len, free.len)     # ... but still reset ret / len
    assert not free.snapshot().complete


# ------------------------------------------------------------------------------------------------ the class on the CPU
def test_constructor_validation():
    from drqv2_amd.replay import VecEpisodeStats
    for kw in (dict(num_envs=0), dict(num_envs=-1), dict(num_envs=4, log_size=0), dict(num_envs=4, max_episodes_per_env=-1)):
        with pytest.raises(ValueError):
            VecEpisodeStats(device="cpu", **kw)
    st = VecEpisodeStats(4, "cpu", log_size=16, max_episodes_per_env=3)
    assert (st.N, st.W, st.limit, st.rows) == (4, 16, 3, 0) and st.poll() is None
    assert st.episode_return.shape == (4,) and st.episode_return.dtype == torch.float32
    assert st.episode_length.shape == (4,) and st.episode_length.dtype == torch.int32


def test_step_takes_what_add_takes_and_fails_loudly_without_a_gpu():
    """the same shape / dtype rules and messages as VecDeviceReplay.add for reward and first; then DrqError on the CPU"""
    from drqv2_amd.replay import VecDeviceReplay, VecEpisodeStats
    N = 3
    st = VecEpisodeStats(N, "cpu")
    store = VecDeviceReplay(8, N, (1, 4, 4), 2, 1, 0.99, "cpu", guard_rows=0)
    obs, act, ones = np.zeros((N, 1, 4, 4), np.uint8), np.zeros((N, 2), np.float32), np.ones(N, np.float32)
    bad = [(np.ones(N + 1, np.float32), None), (np.ones((N, 2), np.float32), None), (np.ones(N, np.int32), None),
           ([1.0] * N, None), (ones, np.zeros(N + 1, bool)), (ones, np.zeros(N, np.float32)), (ones, np.zeros((N, 1), bool))]
    for reward, first in bad:
        with pytest.raises(ValueError) as mine:
            st.step(reward, first)
        with pytest.raises(ValueError) as theirs:
            store.add(obs, act, reward, ones, first)
        assert str(mine.value) == str(theirs.value)
    for reward in (ones, np.ones((N, 1), np.float64), torch.ones(N)):
        with pytest.raises(_lib.DrqError, match="no CPU fallback"):
            st.step(reward, torch.zeros(N, dtype=torch.bool))
    for call in (st.publish, st.read, st.reset):
        with pytest.raises(_lib.DrqError, match="no CPU fallback"):
            call()
    assert st.rows == 0 and st.published == 0 and st.poll() is None


# ------------------------------------------------------------------------------------------------ refusals without a GPU
def test_entries_refuse_bad_arguments_before_any_launch():
    """host memory stands in for the device's: a refused call launches nothing, so nothing is ever dereferenced"""
    lib = _lib.load()
    N, W = 4, 8
    bufs = [torch.zeros(N, dtype=torch.float32), torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32),
            torch.zeros(8, dtype=torch.int64), torch.zeros(W, dtype=torch.float32), torch.zeros(W, dtype=torch.int32),
            torch.zeros(W, dtype=torch.int32), torch.zeros(W, dtype=torch.int64)]
    state = [b.data_ptr() for b in bufs]
    reward, first = torch.zeros(N).data_ptr(), torch.zeros(N, dtype=torch.uint8).data_ptr()
    mirror = torch.zeros(64 + 20 * W + 8, dtype=torch.uint8).data_ptr()
    step = lambda st=state, n=N, w=W, lim=0, row=1, rew=reward: lib.drq_vec_stats_step(*st, n, w, lim, row, rew, first, None)
    for k in range(8):
        st = state[:k] + [None] + state[k + 1:]
        assert step(st) == EARG, k
        assert lib.drq_vec_stats_reset(*st, N, W, None) == EARG, k
        if k >= 3:
            assert lib.drq_vec_stats_publish(*st[3:], W, mirror, 1, None) == EARG, k
    assert step(n=0) == EARG and step(n=-3) == EARG and step(n=2 ** 31) == EARG
    assert step(w=0) == EARG and step(w=-1) == EARG and step(lim=-1) == EARG and step(row=-1) == EARG
    assert step(rew=None) == EARG                                  # a null reward is for row 0 only
    assert step(state[:3] + [state[3] + 4] + state[4:]) == EARG    # a header that is not 8-byte aligned
    assert lib.drq_vec_stats_reset(*state, 0, W, None) == EARG and lib.drq_vec_stats_reset(*state, N, 0, None) == EARG
    assert lib.drq_vec_stats_publish(*state[3:], 0, mirror, 1, None) == EARG
    assert lib.drq_vec_stats_publish(*state[3:], W, None, 1, None) == EARG
    assert lib.drq_vec_stats_publish(*state[3:], W, mirror + 4, 1, None) == EARG
    assert all(not bool(b.any()) for b in bufs)
