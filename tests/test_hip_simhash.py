"""The exploration bonus on the GPU: drq_explore_simhash_step and drqv2_amd.explore.SimHashBonus against the numpy
restatement (tests/simhash_oracle.py), which is the only thing they are compared with.

Bounds.  Everything is compared bit for bit.  Cell sums, centring, projections, codes and counts are integers.  The
bonus is (float)c, sqrt and one division, each correctly rounded in the kernel (build.py gives explore.hip
-fhip-fp32-correctly-rounded-divide-sqrt) as in numpy's float32 loops; reward + bonus is one float32 add of those values.
The counts of a step do not depend on the order of the workgroups: all increments precede all reads.

Shapes.  N = 1, 3, 65 (one environment, an odd few, more than a wave of them with a ragged end in the bonus launch),
bits = 1, 8, 24 (one bit on one wave, two rounds over the four waves, the most: six rounds), two seeds.  Frames: random
bytes, all 0 and all 255 (every projection zero: code 0), rows copied inside a step and across steps
(simhash_oracle.sequence), and frames of VecReach.  The oracle's runs are made once per configuration and shared."""
import gc

import numpy as np
import pytest
import torch

from tests import poison
from tests import simhash_oracle as S
from tests import vec_stats_oracle as VS
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p
from tests.test_hip_vec_replay import raw

pytestmark = pytest.mark.gpu
NS, BITS, SEEDS = (1, 3, 65), (1, 8, 24), (0, 0x9E3779B9)
BETA, DATA_SEED = 0.1, 11
F = np.float32
NAME = "drq_explore_simhash_step"


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert NAME in _lib.PROTOTYPES, "the exploration entry is missing"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def leave_no_cached_blocks():
    """the random frames uploaded here go back to the driver with the module, so that what a later test module gets from
    torch.empty does not depend on this one having run"""
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def runs():
    """the shared sequences and the oracle's runs over them: each computed once, on first use, never modified"""
    seqs, cache = {}, {}

    def get(N, bits, seed):
        if N not in seqs:
            seqs[N] = S.sequence(N, DATA_SEED)
        if (N, bits, seed) not in cache:
            cache[N, bits, seed] = S.run(N, bits, BETA, seed, *seqs[N])
        return seqs[N] + (cache[N, bits, seed],)
    return get


def make(N, bits=16, beta=BETA, seed=0):
    from drqv2_amd.explore import SimHashBonus
    return SimHashBonus(N, "cuda", bits=bits, beta=beta, seed=seed)


def same_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def same_step(b, ret, want, what, with_reward=True):
    """the newest step of SimHashBonus b and its return against one step of the oracle's run"""
    code, count, bonus, total = want[:4]
    same_bits(b.codes, code, (what, "codes"))
    same_bits(b.counts, count, (what, "counts"))
    same_bits(b.last_bonus, bonus, (what, "bonus"))
    same_bits(ret, total if with_reward else bonus, (what, "return"))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("N", NS)
def test_six_steps_with_repeats_and_duplicates_match_the_oracle(runs, N, bits, seed):
    """codes, counts, bonus, reward + bonus, the whole table and distinct() after every one of six counting steps whose
    frames repeat across steps and (N > 1) inside a step"""
    frames, rewards, want = runs(N, bits, seed)
    if bits > 1:
        assert S.covers(want, N), "the inputs no longer hold a duplicate inside a step and two distinct codes"
    b = make(N, bits, BETA, seed)
    for s, (f, r, w) in enumerate(zip(frames, rewards, want)):
        ret = b.step(torch.from_numpy(f).cuda(), torch.from_numpy(r).cuda())
        assert ret.is_cuda and ret.dtype == torch.float32 and tuple(ret.shape) == (N,)
        same_step(b, ret, w, s)
        same_bits(b.table, w[4], (s, "table"))
        d = b.distinct()
        assert d.is_cuda and d.dim() == 0 and int(d) == w[5], s
    assert int(b.table.sum()) == 6 * N


def test_frames_of_the_device_environment(runs):
    """N = 65 VecReach environments, 16 bits: the reset frames and those of 8 steps, without a reward"""
    from drqv2_amd.envs import VecReach
    N = 65
    env, b, o = VecReach(N, "cuda", episode_length=5, seed=3), make(N, 16, 0.5, 4), S.SimHashOracle(16, 0.5, 4)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    frame = env.reset()
    for s in range(9):
        ret = b.step(frame)
        w = o.step(frame.cpu().numpy())
        same_step(b, ret, w, s, with_reward=False)
        frame = env.step(torch.rand(N, 2, device="cuda", generator=g) * 2 - 1)[0]
    same_bits(b.table, o.table, "table")
    assert 2 <= int(b.distinct()) == o.distinct()


def test_a_step_that_only_reads(runs):
    N, bits, seed = 65, 8, SEEDS[1]
    frames, rewards, want = runs(N, bits, seed)
    b, o = make(N, bits, BETA, seed), S.SimHashOracle(bits, BETA, seed)
    ret = b.step(torch.from_numpy(frames[0]).cuda(), update=False)           # an empty table: every code is unseen
    assert not b.table.any() and int(b.distinct()) == 0
    same_bits(b.counts, np.zeros(N, np.int32), "counts of an empty table")
    same_bits(ret, np.full(N, BETA, F), "the bonus of an unseen code is beta")
    for s in range(2):
        b.step(torch.from_numpy(frames[s]).cuda())
        o.step(frames[s])
    table = b.table.clone()
    ret = b.step(torch.from_numpy(frames[3]).cuda(), torch.from_numpy(rewards[3]).cuda(), update=False)
    w = o.step(frames[3], rewards[3], update=False)
    assert (w[1] == 0).any() and (w[1] > 0).any(), "seen and unseen codes, on the oracle"
    same_step(b, ret, w, "read-only")
    assert torch.equal(b.table, table) and np.array_equal(o.table, table.cpu().numpy())


def test_bonus_of_large_counts_rounds_as_numpy_does():
    """a table written by hand: counts up to 2^31 - 1, among them integers that are no float32 (2^24 + 1, ...) and
    squares and their neighbours; 65 environments read them back through codes of their own frames"""
    N, bits, seed, beta = 65, 8, 5, 0.3
    frame = S.random_frames(N, 9)
    rs = np.random.RandomState(4)
    table = rs.randint(1, 2 ** 31 - 1, size=256).astype(np.int32)
    table[:24] = [1, 2, 3, 4, 15, 16, 17, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 1, 2 ** 31 - 129, 999999,
                  1000000, 1000001, 46340 ** 2, 46340 ** 2 - 1, 46340 ** 2 + 1, 7, 11, 13, 2 ** 30, 2 ** 30 + 65]
    table[100:180] = np.arange(5, 85)
    b = make(N, bits, beta, seed)
    b.table.copy_(torch.from_numpy(table))
    reward = rs.standard_normal(N).astype(F)
    ret = b.step(torch.from_numpy(frame).cuda(), torch.from_numpy(reward).cuda(), update=False)
    o = S.SimHashOracle(bits, beta, seed)
    o.table[:] = table
    same_step(b, ret, o.step(frame, reward, update=False), "large counts")
    # every one of the 256 values is read by some environment: the frames reach K distinct codes, so the values are
    # laid under those codes K at a time
    code = S.codes(frame, bits, seed)
    reached = np.unique(code)
    assert len(reached) >= 32
    for start in range(0, 256, len(reached)):
        t2 = np.ones(256, np.int32)
        t2[reached] = table[(start + np.arange(len(reached))) % 256]
        b.table.copy_(torch.from_numpy(t2))
        ret = b.step(torch.from_numpy(frame).cuda(), update=False)
        same_bits(b.counts, t2[code], start)
        same_bits(ret, S.bonus_of(t2[code], beta), start)


# ------------------------------------------------------------------------------------------------ the entry on poisoned memory
@pytest.mark.parametrize("with_reward", [False, True])
@pytest.mark.parametrize("N,bits", [(3, 8), (65, 24), (1, 1)])
def test_entry_writes_every_output_element_and_nothing_else(lib, runs, N, bits, with_reward):
    """drq_explore_simhash_step on guarded allocations: frames, table and reward between guard bands, the outputs full of
    the sentinel, fresh ones every step.  The outputs equal the oracle's (no count and no code is the 4-byte sentinel,
    and no bonus a NaN), so every element was written; check() finds every guard band intact, the table's included"""
    seed = SEEDS[1]
    frames, rewards, want = runs(N, bits, seed)
    table = dev(torch.zeros(1 << bits, dtype=torch.int32), "table")
    for s in range(4):
        frame, reward = dev(torch.from_numpy(frames[s]), "frame"), dev(torch.from_numpy(rewards[s]), "reward")
        code, count = (poison.alloc(N, torch.int32, "cuda", name=n) for n in ("code_out", "count_out"))
        bonus = poison.alloc(N, torch.float32, "cuda", name="bonus_out")
        total = poison.alloc(N, torch.float32, "cuda", name="reward_out", kind="out" if with_reward else "refused")
        assert lib.drq_explore_simhash_step(p(frame), N, bits, seed, BETA, 1, p(table), p(code), p(count), p(bonus),
                                            p(reward) if with_reward else None, p(total) if with_reward else None,
                                            None) == 0
        poison.check()
        w = want[s]
        same_bits(code, w[0], (s, "code"))
        same_bits(count, w[1], (s, "count"))
        same_bits(bonus, w[2], (s, "bonus"))
        if with_reward:
            same_bits(total, w[3], (s, "reward + bonus"))
        same_bits(table, w[4], (s, "table"))
        assert raw(frame).tobytes() == frames[s].tobytes() and raw(reward).tobytes() == rewards[s].tobytes()


def test_reward_out_may_be_the_reward_itself(lib, runs):
    N, bits, seed = 65, 8, SEEDS[0]
    frames, rewards, want = runs(N, bits, seed)
    table = dev(torch.zeros(1 << bits, dtype=torch.int32), "table")
    frame, reward = dev(torch.from_numpy(frames[0]), "frame"), dev(torch.from_numpy(rewards[0]), "reward")
    code, count = (poison.alloc(N, torch.int32, "cuda", name=n) for n in ("code_out", "count_out"))
    bonus = poison.alloc(N, torch.float32, "cuda", name="bonus_out")
    assert lib.drq_explore_simhash_step(p(frame), N, bits, seed, BETA, 1, p(table), p(code), p(count), p(bonus), p(reward),
                                        p(reward), None) == 0
    same_bits(reward, want[0][3], "in place")
    same_bits(bonus, want[0][2], "bonus")


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/simhash_oracle.refused_calls, held to return the error without a GPU by
    tests/test_cpu_simhash.py) on real allocations full of the sentinel: the error, and every byte is still poison"""
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    frame, table, out, rew = al(5 * 3 * 84 * 84, "frame"), al(4 << 16, "table"), al(0x300, "outputs"), al(0x200, "rewards")
    calls = S.refused_calls(p(frame), p(table), p(out), p(rew))
    for a in calls:
        assert lib.drq_explore_simhash_step(*a, None) == -1, a
    assert len(calls) == 36
    poison.check()


# ------------------------------------------------------------------------------------------------ the class: outputs, state
def test_outputs_rotate_over_two_sets(runs):
    """the tensors of step t are intact after step t + 1 and overwritten by step t + 2"""
    N, bits, seed = 3, 8, SEEDS[0]
    frames, rewards, want = runs(N, bits, seed)
    b = make(N, bits, BETA, seed)
    kept = []
    for s in range(5):
        ret = b.step(torch.from_numpy(frames[s]).cuda(), torch.from_numpy(rewards[s]).cuda())
        kept.append((ret, b.codes, b.counts, b.last_bonus))
        if s >= 1:
            for t, w, name in zip(kept[s - 1], (want[s - 1][3], want[s - 1][0], want[s - 1][1], want[s - 1][2]),
                                  ("return", "codes", "counts", "bonus")):
                same_bits(t, w, (s, "the step before", name))
        if s >= 2:
            for old, mid, new in zip(kept[s - 2], kept[s - 1], kept[s]):
                assert old.data_ptr() == new.data_ptr() != mid.data_ptr()
            same_bits(kept[s - 2][0], want[s][3], (s, "overwritten"))
    plain = b.step(torch.from_numpy(frames[5]).cuda())                  # without a reward the bonus itself is returned
    assert plain.data_ptr() == b.last_bonus.data_ptr()


def test_wrong_arguments_raise_before_any_launch():
    N = 3
    b = make(N, 8)
    frame, reward = torch.zeros((N, 3, 84, 84), dtype=torch.uint8, device="cuda"), torch.zeros(N, device="cuda")
    for bad in (frame.cpu(), frame[:2], frame.float(), frame.cpu().numpy()):
        with pytest.raises(ValueError):
            b.step(bad, reward)
    for bad in (reward.cpu(), reward[:2], reward.double(), [0.0] * N):
        with pytest.raises(ValueError):
            b.step(frame, bad)
    assert b._out is None and b.codes is None and not b.table.any()
    wide = torch.zeros((N, 3, 84, 168), dtype=torch.uint8, device="cuda")
    wide[:, :, :, ::2] = torch.from_numpy(S.random_frames(N, 1)).cuda()
    ret = b.step(wide[:, :, :, ::2], torch.ones(2 * N, device="cuda")[::2])          # views: copied, then as any other
    w = S.SimHashOracle(8, BETA, 0).step(S.random_frames(N, 1), np.ones(N, F))
    same_step(b, ret, w, "strided views")


def test_state_dict_into_a_fresh_object_gives_the_same_next_steps(runs):
    N, bits, seed = 65, 24, SEEDS[1]
    frames, rewards, want = runs(N, bits, seed)
    b = make(N, bits, BETA, seed)
    for s in range(3):
        b.step(torch.from_numpy(frames[s]).cuda(), torch.from_numpy(rewards[s]).cuda())
    sd = b.state_dict()
    assert all(not t.is_cuda for t in sd.values() if torch.is_tensor(t))
    assert sd["index"].numel() == want[2][5] and sd["index"].numel() == sd["count"].numel() < 3 * N + 1
    same_bits(sd["count"].numpy(), want[2][4][sd["index"].numpy()], "the saved counts")
    fresh = make(N, bits, BETA, seed)
    fresh.step(torch.from_numpy(frames[5]).cuda())                      # a used object: its table is replaced whole
    fresh.load_state_dict(sd)
    assert fresh.codes is None and torch.equal(fresh.table, b.table)
    for s in range(3, 6):
        f, r = torch.from_numpy(frames[s]).cuda(), torch.from_numpy(rewards[s]).cuda()
        ra, rb = b.step(f, r), fresh.step(f, r)
        assert raw(ra).tobytes() == raw(rb).tobytes(), s
        same_step(fresh, rb, want[s], s)
    same_bits(fresh.table, want[5][4], "table")
    with pytest.raises(ValueError, match=r"\bseed: saved"):
        make(N, bits, BETA, seed + 1).load_state_dict(sd)
    b.reset()
    assert not b.table.any() and int(b.distinct()) == 0 and b.codes is None


def test_checkpoint_round_trip_with_the_bonus(runs, tmp_path):
    """save(bonus=) after three steps, the object deleted, load(bonus=) into a fresh one: the next three steps are those
    of the uninterrupted run; a file saved without a bonus still loads, and says so when one is asked of it"""
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecReach
    N, bits, seed = 3, 16, SEEDS[0]
    frames, rewards, _ = runs(N, 8, seed)
    want = S.run(N, bits, BETA, seed, frames, rewards)
    env = VecReach(N, "cuda", seed=2)
    env.reset()
    b = make(N, bits, BETA, seed)
    for s in range(3):
        b.step(torch.from_numpy(frames[s]).cuda(), torch.from_numpy(rewards[s]).cuda())
    path, plain = str(tmp_path / "ck.pt"), str(tmp_path / "plain.pt")
    checkpoint.save(path, env=env, bonus=b, extra={"step": 3})
    checkpoint.save(plain, env=env, extra={"step": 3})
    del b
    gc.collect()
    fresh, env2 = make(N, bits, BETA, seed), VecReach(N, "cuda", seed=2)
    assert checkpoint.load(path, env=env2, bonus=fresh) == {"step": 3}
    for s in range(3, 6):
        ret = fresh.step(torch.from_numpy(frames[s]).cuda(), torch.from_numpy(rewards[s]).cuda())
        same_step(fresh, ret, want[s], s)
    same_bits(fresh.table, want[5][4], "table")
    assert checkpoint.load(plain, env=env2) == {"step": 3}
    with pytest.raises(ValueError, match="bonus"):
        checkpoint.load(plain, env=env2, bonus=fresh)


# ------------------------------------------------------------------------------------------------ the loop as written
def test_collection_loop_with_the_bonus_end_to_end():
    """VecReach -> bonus.step(frame, reward) -> VecFrameReplay.add() -> update(), 20 steps at N = 3, batch 8, hidden_dim
    64, the loop of INTEGRATION.md ("Exploration bonus").  It runs, the metrics are finite, and the ring's reward column
    is the environment's reward plus the oracle's bonus on the frames the ring holds"""
    import drqv2
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    N, A, ROWS, STEPS, B, bits, beta, seed = 3, 2, 32, 20, 8, 16, 0.1, 7
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 20, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = VecReach(N, "cuda", action_dim=A, episode_length=6, seed=3)
    store = VecFrameReplay(ROWS, N, A, 3, 0.99, "cuda", seed=2)
    store.batch_size = B
    stats = VecEpisodeStats(N, "cuda")
    bonus = make(N, bits, beta, seed)
    it = iter(store)
    zeros = torch.zeros(N, device="cuda")
    store.add(env.reset(), torch.zeros(N, A, device="cuda"), zeros, torch.ones(N, device="cuda"))
    stats.step(zeros)
    env_rewards, metrics = [], []
    for step in range(STEPS):
        action = agent.act_batch(store.observation(), step, False)
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, bonus.step(frame, reward), discount, first)
        stats.step(reward, first)                       # the statistics keep the environment's own reward
        env_rewards.append(reward.cpu().numpy().copy())
        if step >= STEPS - 4:
            metrics.append(agent.update(it, step))
    assert len(metrics) == 4 and all(np.isfinite(v) for m in metrics for v in m.values())
    held = (STEPS + 1) * N
    assert store.T == STEPS + 1 <= ROWS
    ring_frames = store.frames[:held].cpu().numpy().reshape(STEPS + 1, N, 3, 84, 84)
    ring_reward = store.reward[:held].cpu().numpy().reshape(STEPS + 1, N)
    o = S.SimHashOracle(bits, beta, seed)
    same_bits(ring_reward[0], np.zeros(N, F), "the reset row")
    for s in range(STEPS):
        w = o.step(ring_frames[s + 1], env_rewards[s])
        same_bits(ring_reward[s + 1], w[3], (s, "reward + bonus"))
        assert (w[2] > 0).all() and (ring_reward[s + 1] > env_rewards[s]).all()
    same_bits(bonus.table, o.table, "table")
    assert int(bonus.distinct()) == o.distinct() >= 2
    # the statistics are those of the environment's rewards alone (tests/vec_stats_oracle.py): the bonus is not in them
    first = store.first[:held].cpu().numpy().reshape(STEPS + 1, N)
    assert first[1:].any(), "the run holds reset rows"
    so = VS.StatsOracle(N)
    so.step(np.zeros(N, F))
    for s in range(STEPS):
        so.step(env_rewards[s], first[s + 1])
    snap, ws = stats.read(), so.snapshot()
    assert snap.rows == STEPS + 1 and snap.episodes == ws.episodes >= 1
    assert snap.records.tobytes() == ws.records.tobytes()
