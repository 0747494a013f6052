"""Episode files for the step-major ring (drqv2_amd/episodes.py, VecDeviceReplay.export_episodes / add_episodes,
drq_vec_export_rows, drq_vec_fill): everything that needs no GPU.  The two host plans on hand-built rings, to the entry;
the checks add_episodes() makes before any launch; the new entries in the header, the prototype table and the build list."""
import os

import numpy as np
import pytest

from drqv2_amd import _lib
from tests import abi

NEW = ("drq_vec_export_rows", "drq_vec_fill")
R, N = 12, 3


@pytest.fixture(scope="module")
def E():
    from drqv2_amd import episodes
    return episodes


def ring_flags(resets, T, row0=1):
    """the flags of a ring of R rows x N after T adds; resets[e] = the reset rows of environment e; row0: what the flag
    of row 0 holds (the rule does not read it).  Slots never written hold 1, as in a fresh store"""
    first = np.ones(R * N, np.uint8)
    for t in range(T):
        for e in range(N):
            first[(t % R) * N + e] = row0 if t == 0 else int(t in resets[e])
    return first


def closed_episodes(resets, T):
    """every (e, t0, length) with both reset rows added, zero-length ones left out: the enumeration from the schedule"""
    out = []
    for e in range(N):
        rs = sorted(t for t in set(resets[e]) | {0} if t < T)
        out += [(e, a, b - a - 1) for a, b in zip(rs, rs[1:]) if b - a - 1 >= 1]
    return out


# ------------------------------------------------------------------------------------------------ plan_export
WRAPPED = {0: {3, 10, 15}, 1: {8, 9, 14}, 2: {2}}     # T = 20: rows 8 .. 19 are live


def test_export_closed_open_headless_in_a_wrapped_ring(E):
    """T = 20 in a ring of 12: environment 0 holds the tail of an episode whose reset row 3 is gone, a closed episode
    10 .. 14 and an open one from 15; environment 1 two consecutive reset rows 8, 9, a closed episode 9 .. 13 and an
    open one; environment 2 nothing but the tail of the episode that began on row 2"""
    first = ring_flags(WRAPPED, 20)
    p = E.plan_export(first, 20, R, N)
    assert p.episodes == [(1, 9, 4), (0, 10, 4)]                   # ordered by (t1, e): t1 = 13, 14
    assert (p.zero_length, p.headless, p.open, p.short, p.next_row) == (1, 2, 2, 0, 20)
    q = E.plan_export(first, 20, R, N, include_open=True)
    assert q.episodes == [(1, 9, 4), (0, 10, 4), (0, 15, 4), (1, 14, 5)] and q.open == 0
    assert (q.zero_length, q.headless, q.short) == (1, 2, 0)
    for e, t0, n in q.episodes:                                    # every listed row is live and flagged as the rule says
        assert t0 >= 20 - R and t0 + n <= 19
        assert first[(t0 % R) * N + e] == 1 and not any(first[(t % R) * N + e] for t in range(t0 + 1, t0 + n + 1))


def test_export_row_0_and_consecutive_resets(E):
    """before the ring wraps: row 0 is a reset row whatever its flag holds; rows 4, 5, 6 of environment 1 are reset rows
    (two zero-length runs), row 9 = T - 1 of environment 2 is one too: an open episode of length 0"""
    resets = {0: {5}, 1: {4, 5, 6}, 2: {9}}
    for row0 in (0, 1):
        first = ring_flags(resets, 10, row0)
        assert first[0] == row0
        p = E.plan_export(first, 10, R, N)
        assert p.episodes == [(1, 0, 3), (0, 0, 4), (2, 0, 8)]
        assert (p.zero_length, p.headless, p.open, p.short) == (2, 0, 3, 0)
        q = E.plan_export(first, 10, R, N, include_open=True)
        assert q.episodes == [(1, 0, 3), (0, 0, 4), (2, 0, 8), (0, 5, 4), (1, 6, 3)]
        assert (q.zero_length, q.open) == (3, 0)                   # the open run of length 0 has nothing to write
    assert E.plan_export(np.ones(R * N, np.uint8), 0, R, N) == E.ExportPlan([], 0, 0, 0, 0, 0)
    p1 = E.plan_export(np.ones(R * N, np.uint8), 1, R, N)
    assert p1.episodes == [] and (p1.open, p1.zero_length) == (3, 0)


def test_export_min_length(E):
    first = ring_flags(WRAPPED, 20)
    p = E.plan_export(first, 20, R, N, include_open=True, min_length=5)
    assert p.episodes == [(1, 14, 5)] and p.short == 3 and (p.zero_length, p.headless, p.open) == (1, 2, 0)
    with pytest.raises(ValueError, match="min_length"):
        E.plan_export(first, 20, R, N, min_length=0)
    with pytest.raises(ValueError, match="flags"):
        E.plan_export(first[:-1], 20, R, N)


def test_export_periodic_calls_list_every_episode_once(E):
    """environment e resets every 4 + e rows; exports after 8, 14 and 20 rows, each from the previous next_row: together
    they list every closed episode of the schedule exactly once, although the ring has wrapped in between"""
    resets = {e: set(range(0, 40, 4 + e)) for e in range(N)}
    seen, start = [], None
    for T in (8, 14, 20):
        p = E.plan_export(ring_flags(resets, T), T, R, N, start_row=start)
        assert p.next_row == T and p.zero_length == 0 and p.short == 0 and p.open == N
        assert all(t0 + n + 1 >= (start or 0) for _, t0, n in p.episodes)
        seen += p.episodes
        start = p.next_row
    assert len(seen) == len(set(seen)) and sorted(seen) == sorted(closed_episodes(resets, 20))
    assert len(seen) == 4 + 3 + 3
    assert E.plan_export(ring_flags(resets, 20), 20, R, N, start_row=20).episodes == []      # nothing new, nothing listed
    # without start_row the last call lists what is still in the ring whole, the earlier ones again included
    again = E.plan_export(ring_flags(resets, 20), 20, R, N)
    assert set(again.episodes) == {ep for ep in closed_episodes(resets, 20) if ep[1] >= 8} and again.headless == 2


def test_export_table(E):
    tab = E.export_table([(1, 9, 2), (0, 10, 1)])
    assert tab.dtype == np.int32 and tab.tolist() == [[9, 1, 9], [10, 1, 9], [11, 1, 9], [10, 0, 10], [11, 0, 10]]
    assert E.export_table([]).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ plan_fill
def check_fill(E, plan, lengths, n_lanes):
    """the plan holds every episode exactly once, whole and in order, in one lane; the rest are pad rows at lane ends"""
    assert plan.episode.shape == plan.index.shape == (n_lanes, plan.L) and plan.episode.dtype == np.int64
    for i, n in enumerate(lengths):
        lanes, rows = np.nonzero(plan.episode == i)
        assert len(set(lanes.tolist())) == 1 and rows.tolist() == list(range(rows[0], rows[0] + n + 1))
        assert plan.index[lanes[0], rows].tolist() == list(range(n + 1))
    pad = plan.episode == E.PAD
    assert np.array_equal(pad, plan.index == E.PAD) and int(pad.sum()) == plan.pad_rows
    assert plan.pad_rows == n_lanes * plan.L - sum(n + 1 for n in lengths)
    for e in range(n_lanes):
        used = int((~pad[e]).sum())
        assert not pad[e, :used].any() and pad[e, used:].all()
    if lengths:
        assert not pad.all(axis=1).all() and (~pad).any(axis=0).all()     # L is the longest lane, no row is all pads


def test_fill_three_lanes_and_one(E):
    lengths = [5, 2, 2, 7, 1]
    p = E.plan_fill(lengths, 3)
    check_fill(E, p, lengths, 3)
    assert p.L == 11 and p.pad_rows == 11
    assert p.episode.tolist() == [[0] * 6 + [-1] * 5, [1] * 3 + [3] * 8, [2] * 3 + [4] * 2 + [-1] * 6]
    assert p.index[1].tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 7]
    q = E.plan_fill(lengths, 1)
    check_fill(E, q, lengths, 1)
    assert q.L == 22 and q.pad_rows == 0 and q.episode[0].tolist() == [0] * 6 + [1] * 3 + [2] * 3 + [3] * 8 + [4] * 2


def test_fill_ties_zero_episodes_and_refusals(E):
    p = E.plan_fill([1, 1, 1, 1], 3)                               # ties go to the lowest lane: 0, 1, 2, then 0 again
    check_fill(E, p, [1, 1, 1, 1], 3)
    assert p.episode.tolist() == [[0, 0, 3, 3], [1, 1, -1, -1], [2, 2, -1, -1]]
    p = E.plan_fill([3, 1], 2)                                     # [4, 2]: the next one would go to lane 1
    assert E.plan_fill([3, 1, 1], 2).episode.tolist() == [[0, 0, 0, 0], [1, 1, 2, 2]]
    z = E.plan_fill([], 3)
    assert z.L == 0 and z.episode.shape == (3, 0) and z.pad_rows == 0
    lone = E.plan_fill([2], 3)                                     # lanes that receive nothing are pads throughout
    assert lone.L == 3 and lone.pad_rows == 6 and (lone.episode[1:] == E.PAD).all()
    with pytest.raises(ValueError, match="transition"):
        E.plan_fill([2, 0], 3)
    with pytest.raises(ValueError, match="N"):
        E.plan_fill([2], 0)


def small_episodes(lengths, A=2, slot=(3, 2, 2), seed=0):
    r = np.random.RandomState(seed)
    return [{"frame": r.randint(0, 256, (n + 1,) + slot).astype(np.uint8),
             "action": r.uniform(-1, 1, (n + 1, A)).astype(np.float32),
             "reward": r.standard_normal((n + 1, 1)).astype(np.float32),
             "discount": r.uniform(size=n + 1).astype(np.float32)} for n in lengths]


def test_planned_rows_pads_and_chunks(E):
    """the rows of a plan: episode steps where the plan says so, first on index 0 only; a pad row is a reset row with
    action 0, reward 0, discount 1 and the lane's last written frame (zeros in a lane that got nothing); any split into
    chunks gives the same rows"""
    lengths = [5, 2, 2, 7, 1]
    eps = small_episodes(lengths)
    plan = E.plan_fill(lengths, 3)
    frame, action, reward, discount, first = E.planned_rows(plan, eps, 0, plan.L)
    assert frame.shape == (11, 3, 3, 2, 2) and action.shape == (11, 3, 2) and first.dtype == np.uint8
    for e in range(3):
        last = None
        for r in range(plan.L):
            i, k = int(plan.episode[e, r]), int(plan.index[e, r])
            if i == E.PAD:
                assert first[r, e] == 1 and reward[r, e] == 0 and discount[r, e] == 1 and not action[r, e].any()
                assert np.array_equal(frame[r, e], last)
            else:
                last = eps[i]["frame"][k]
                assert np.array_equal(frame[r, e], last) and np.array_equal(action[r, e], eps[i]["action"][k])
                assert reward[r, e] == eps[i]["reward"].reshape(-1)[k] and discount[r, e] == eps[i]["discount"][k]
                assert first[r, e] == (k == 0)
    whole = (frame, action, reward, discount, first)
    for cuts in ([0, 1, 11], [0, 4, 7, 11], list(range(12))):
        parts = [E.planned_rows(plan, eps, a, b) for a, b in zip(cuts, cuts[1:])]
        for j in range(5):
            assert np.array_equal(np.concatenate([p[j] for p in parts]), whole[j])
    lone = E.plan_fill([2], 3)
    f = E.planned_rows(lone, eps[1:2], 0, 3)
    assert not f[0][:, 1:].any() and f[4][:, 1:].all() and (f[3][:, 1:] == 1).all()
    out = [np.full_like(a, 7) for a in whole]                      # into given buffers: only the first n rows
    E.planned_rows(plan, eps, 2, 5, out=out)
    assert np.array_equal(out[0][:3], frame[2:5]) and (out[0][3:] == 7).all()


# ------------------------------------------------------------------------------------------------ add_episodes' checks
def stack_episode(n, A=2, seed=0):
    """an episode of n transitions as a FrameStackWrapper builds it: uint8 [n + 1, 9, 84, 84]"""
    r = np.random.RandomState(seed)
    f = r.randint(0, 256, (n + 1, 3, 84, 84)).astype(np.uint8)
    obs = np.stack([np.concatenate([f[max(t - 2, 0)], f[max(t - 1, 0)], f[t]]) for t in range(n + 1)])
    return {"observation": obs, "action": r.uniform(-1, 1, (n + 1, A)).astype(np.float32),
            "reward": r.standard_normal((n + 1, 1)).astype(np.float32), "discount": np.ones((n + 1, 1), np.float32)}


def test_add_episodes_validates_on_the_cpu_before_any_launch():
    from drqv2_amd.replay import VecDeviceReplay, VecFrameReplay
    vf = VecFrameReplay(16, 2, 2, 3, 0.99, "cpu")
    good = stack_episode(3)
    before = vf.T

    def broken(**kw):
        ep = dict(good)
        ep.update(kw)
        return ep
    with pytest.raises(ValueError, match=r"episode 1: action: .*action_dim = 2"):              # wrong A
        vf.add_episodes([good, broken(action=np.zeros((4, 3), np.float32))])
    with pytest.raises(ValueError, match=r"episode 0: action: float32 required, got float64"):
        vf.add_episodes([broken(action=good["action"].astype(np.float64))])
    with pytest.raises(ValueError, match=r"episode 0: reward: float32"):
        vf.add_episodes([broken(reward=good["reward"].astype(np.float16))])
    with pytest.raises(ValueError, match=r"episode 0: discount: shape"):
        vf.add_episodes([broken(discount=np.ones((3, 1), np.float32))])
    with pytest.raises(ValueError, match=r"episode 0: observation: .*uint8"):
        vf.add_episodes([broken(observation=good["observation"].astype(np.float32))])
    with pytest.raises(ValueError, match=r"episode 2: observation: .*at least one transition"):
        vf.add_episodes([good, good, {k: v[:1] for k, v in good.items()}])
    with pytest.raises(ValueError, match=r"episode 0: reward: the episode has no such field"):
        vf.add_episodes([{k: v for k, v in good.items() if k != "reward"}])
    noise = broken(observation=np.random.RandomState(1).randint(0, 256, (4, 9, 84, 84)).astype(np.uint8))
    with pytest.raises(ValueError, match=r"episode 1: observation: .*no (reset|frame) stack"):
        vf.add_episodes([good, noise])
    with pytest.raises(ValueError, match=r"L = 20 .*R = 16"):      # 3 episodes of 9 rows in 2 lanes: 18 + ... > 16
        vf.add_episodes([stack_episode(9, seed=s) for s in range(3)])
    # past its checks a store on the CPU refuses like add(): noise passes with check=False, single frames pass as they are
    singles = broken(observation=np.ascontiguousarray(good["observation"][:, 6:9]))
    for eps, kw in (([good], {}), ([noise], {"check": False}), ([singles], {}), ([], {})):
        with pytest.raises(_lib.DrqError, match="no CPU fallback"):
            vf.add_episodes(eps, **kw)
    vd = VecDeviceReplay(16, 2, (4, 4), 2, 3, 0.99, "cpu")
    with pytest.raises(ValueError, match=r"episode 0: observation: uint8 \[len \+ 1, 4, 4\]"):
        vd.add_episodes([good])
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        vd.add_episodes([broken(observation=np.zeros((4, 4, 4), np.uint8))])
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        vf.export_episodes("/nonexistent-and-never-made")
    assert vf.T == before and vd.T == 0


def test_add_episodes_reads_a_directory_oldest_first(tmp_path):
    """a directory goes through replay_buffer's own listing: reference-named files only, by name; the checks name the file"""
    import replay_buffer as RB
    from drqv2_amd.replay import VecFrameReplay
    good = stack_episode(2)
    RB.save_episode(good, tmp_path / "20200101T000000_0_2.npz")
    RB.save_episode({**good, "action": np.zeros((3, 5), np.float32)}, tmp_path / "20200101T000001_1_2.npz")
    RB.save_episode(good, tmp_path / "notes.npz")                  # no episode name: not listed
    vf = VecFrameReplay(16, 2, 2, 3, 0.99, "cpu")
    with pytest.raises(ValueError, match=r"20200101T000001_1_2\.npz: action"):
        vf.add_episodes(tmp_path)
    (tmp_path / "20200101T000001_1_2.npz").unlink()
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        vf.add_episodes(str(tmp_path))


# ------------------------------------------------------------------------------------------------ the ABI lists
def test_header_prototypes_and_build_list():
    for name in NEW:
        abi.assert_prototype(name)
    from drqv2_amd import build
    assert "vecepisodes.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecepisodes.hip"))
    assert "episode files for the step-major ring" in abi.text()


def test_refusals_need_no_gpu():
    """argument errors are reported before any launch"""
    lib = _lib.load()
    assert lib.drq_vec_export_rows(None, None, None, None, 4, 2, 1, 16, 1, None, 1, None, None, None, None, None) == -1
    assert lib.drq_vec_fill(None, None, None, None, None, 4, 2, 1, 16, 0, 1, None, None, None, None, None, None) == -1
