"""Checkpoint and resume on the GPU: drq_vec_reach_render / VecReach.render() against the numpy restatement of the frame
rule (tests/vec_env_oracle.py), and the contract of drqv2_amd/checkpoint.py -- a run that is saved, torn down and restored
continues exactly as the uninterrupted run would have.

Bounds.  There are none: everything is compared bit for bit (the bytes of the tensors).  Every piece of the loop is
deterministic for a seed -- the environment and the rings are held to their oracles to the bit elsewhere, the update has
no atomics and is tested for run-to-run stability -- and every resume test carries its own control: the uninterrupted run
is made twice (A and A') and must equal itself before the resumed run B is compared with it, so a loop that is not
deterministic is reported as such and not as a checkpoint fault.

Shapes.  Render: N = 1, 3, 17 (one workgroup, odd, more than a few), A = 2, 5 (the state does not depend on A; the
environment's checks do), episode_length 4 over 12 steps so that reset rows occur.  The loop: N = 3, A = 2,
episode_length 5, a ring of 12 rows, nstep 3, guard_rows 2, batch 8, 40 steps with updates from step 6 on, saved after
step 22: the smallest at which the ring has wrapped at the save (24 rows > 12), resets are staggered, n-step windows are
cut, rows have left the tree and a look-ahead batch is pending.  The stacked store: N = 2, 10 rows, saved at T = 14."""
import gc

import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_env_oracle as E
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p, rs_
from tests.test_hip_vec_replay import raw

pytestmark = pytest.mark.gpu
U8 = poison.sentinel_of(torch.uint8)
SEED = 11
N, A, EL, ROWS, NSTEP, GUARD, B = 3, 2, 5, 12, 3, 2, 8
STEPS, CUT, FIRST_UPDATE = 40, 23, 6
RING = ("frames", "action", "reward", "discount", "first")


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_reach_render" in _lib.PROTOTYPES, "the render entry is missing"
    return _lib.load()


def test_the_entry_and_the_methods_exist(lib):
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import BatchIterator, VecDeviceReplay, VecEpisodeStats, VecFrameReplay
    assert hasattr(lib, "drq_vec_reach_render")
    assert callable(VecReach.render)
    for cls in (VecReach, BatchIterator, VecDeviceReplay, VecFrameReplay, VecEpisodeStats):
        assert callable(getattr(cls, "state_dict")) and callable(getattr(cls, "load_state_dict")), cls
    assert callable(checkpoint.save) and callable(checkpoint.load)


def same(got, want, what):
    """bit for bit, whatever it is: tensors and arrays by their bytes, containers element by element"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), what
        for k in want:
            same(got[k], want[k], (what, k))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, (what, i))
    elif torch.is_tensor(want):
        assert torch.is_tensor(got) and got.dtype == want.dtype and got.shape == want.shape, what
        assert raw(got).tobytes() == raw(want).tobytes(), what
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what
    elif isinstance(want, float):
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), what
    else:
        assert got == want, what


def oracle_frames(state):
    return np.stack([E.render(state["pos"][e], state["target"][e]) for e in range(len(state["t"]))])


# ------------------------------------------------------------------------------------------------ 1. render
@pytest.mark.parametrize("A_", [2, 5])
@pytest.mark.parametrize("N_", [1, 3, 17])
def test_render_is_the_frame_of_the_state(lib, N_, A_):
    """after reset() and after each of 12 steps: render() equals the frame the call returned and the oracle's frame rule
    on state(); it is another buffer, and it changes no state"""
    from drqv2_amd.envs import VecReach
    env = VecReach(N_, "cuda", action_dim=A_, episode_length=4, seed=SEED)
    r = rs_(100 + 10 * N_ + A_)
    resets = 0
    for s in range(-1, 12):
        if s < 0:
            frame = env.reset()
        else:
            frame, _, _, first = env.step(torch.from_numpy(r.uniform(-2, 2, (N_, A_)).astype(np.float32)).cuda())
            resets += int(first.sum())
        state = env.state()
        got = env.render()
        assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (N_, 3, 84, 84)
        assert got.data_ptr() != frame.data_ptr()
        same(got, frame, (s, "the frame the call returned"))
        same(got.cpu().numpy(), oracle_frames(state), (s, "the frame rule"))
        same(env.state(), state, (s, "state"))
        same(env.image(84, 3).permute(0, 3, 1, 2).contiguous(), got, (s, "image() reads the rendered frame"))
    assert resets >= N_, "episode_length 4 over 12 steps: every environment is reset at least once"


def test_render_entry_writes_every_byte_and_nothing_else(lib):
    """drq_vec_reach_render at N = 3 on guarded allocations: the output full of the sentinel, pos / target between guard
    bands.  The result equals the oracle's frames, which never hold the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or
    255), so every byte was written; check() finds every guard band intact; the five state tensors keep their bits"""
    o = E.ReachOracle(3, episode_length=4, seed=SEED)
    o.reset()
    r = rs_(5)
    for _ in range(3):
        o.step(r.uniform(-2, 2, (3, 2)).astype(np.float32))
    st = o.state()
    state = [dev(torch.from_numpy(st["pos"]), "pos"), dev(torch.from_numpy(st["target"]), "target"),
             dev(torch.from_numpy(st["t"]), "t"), dev(torch.from_numpy(st["episode"].view(np.int32)), "episode"),
             dev(torch.from_numpy(st["over"]), "over")]
    before = [raw(t) for t in state]
    out = poison.alloc((3, 3, 84, 84), torch.uint8, "cuda", name="frame")
    assert lib.drq_vec_reach_render(p(state[0]), p(state[1]), 3, p(out), None) == 0
    got = out.cpu().numpy()
    same(got, oracle_frames(st), "frame")
    assert not (got == U8).any()
    poison.check()
    for t, b, name in zip(state, before, ("pos", "target", "t", "episode", "over")):
        assert raw(t).tobytes() == b.tobytes(), name
    refused = poison.alloc((3, 3, 84, 84), torch.uint8, "cuda", name="frame", kind="refused")
    assert lib.drq_vec_reach_render(p(state[0]), None, 3, p(refused), None) == -1
    assert lib.drq_vec_reach_render(p(state[0]), p(state[1]), 0, p(refused), None) == -1
    poison.check()


# ------------------------------------------------------------------------------------------------ 2. the whole loop
def build_loop(prioritized, torch_seed, store_seed):
    """the objects of the documented loop; the agent is that of test_collection_loop_end_to_end (tests/test_hip_vec_env.py)"""
    import drqv2
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    torch.manual_seed(torch_seed)
    torch.cuda.manual_seed_all(torch_seed)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 20, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = VecReach(N, "cuda", action_dim=A, episode_length=EL, seed=3)
    store = VecFrameReplay(ROWS, N, A, NSTEP, 0.99, "cuda", seed=store_seed, guard_rows=GUARD,
                           priority_alpha=0.6 if prioritized else None)
    store.batch_size = B
    stats = VecEpisodeStats(N, "cuda")
    return {"agent": agent, "env": env, "store": store, "stats": stats, "iterator": iter(store)}


def staggered_reset(env):
    """reset(), then environment e is given t = e through the state dict: the time limits, and so the reset rows, fall on
    different steps whatever the actions are.  The frame is that of the reset (pos and target are untouched)"""
    frame = env.reset().clone()
    sd = env.state_dict()
    sd["t"] = torch.arange(env.N, dtype=torch.int32) % env.episode_length
    env.load_state_dict(sd)
    same(env.render(), frame, "the frame after a load is the frame of the state")
    return frame


def first_row(o):
    zeros = torch.zeros(N, device="cuda")
    o["store"].add(staggered_reset(o["env"]), torch.zeros(N, A, device="cuda"), zeros, torch.ones(N, device="cuda"))
    o["stats"].step(zeros)


def run_steps(o, lo, hi, rec):
    """steps lo .. hi-1 of the documented loop; rec[step] = what the step produced"""
    agent, env, store, stats, it = o["agent"], o["env"], o["store"], o["stats"], o["iterator"]
    for step in range(lo, hi):
        action = agent.act_batch(store.observation(), step, False)
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, reward, discount, first)
        stats.step(reward, first)
        row = {"action": action.clone(), "reward": reward.clone(), "first": first.clone()}
        if step >= FIRST_UPDATE:
            row["metrics"] = agent.update(it, step)
            row["index"], row["steps"] = store.last_index.clone(), store.last_steps.clone()      # of the look-ahead batch
            if store.tree is not None:
                row["weights"] = it._ahead.weights.clone()
        rec[step] = row


def final_state(o):
    agent, env, store, stats = o["agent"], o["env"], o["store"], o["stats"]
    eng = agent._engine
    snap = stats.read()
    out = {"params": eng.params.clone(), "adam_m": eng.adam_m.clone(), "adam_v": eng.adam_v.clone(),      # target included
           "opt_t": [agent.encoder_opt.t, agent.actor_opt.t, agent.critic_opt.t], "T": store.T,
           "tree": None if store.tree is None else store.tree.clone(), "env": env.state(),
           "stats": {"header": [snap.rows, snap.episodes, snap.length_sum, snap.return_sum, snap.min_return, snap.max_return],
                     "records": snap.records.copy()}}
    out.update((n, getattr(store, n).clone()) for n in RING)
    return out


def uninterrupted(prioritized):
    o = build_loop(prioritized, 5, 2)
    first_row(o)
    rec = {}
    run_steps(o, 0, STEPS, rec)
    return rec, final_state(o)


@pytest.fixture(scope="module")
def runs_a():
    """run A of either sampling mode: made once, shared, never modified"""
    cache = {}

    def get(prioritized):
        if prioritized not in cache:
            cache[prioritized] = uninterrupted(prioritized)
        return cache[prioritized]
    return get


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_resume_equals_no_interruption(lib, runs_a, tmp_path, prioritized):
    """A: 40 steps.  A': the same again -- the control.  B: 23 steps, save, every object deleted, the generators moved, new
    objects with other seeds, load, steps 23 .. 39.  Everything B records from step 23 on and its final state equal A's"""
    from drqv2_amd import checkpoint
    rec_a, end_a = runs_a(prioritized)
    assert rec_a[CUT - 1]["index"].shape == (3, B) and end_a["T"] == STEPS + 1 > 2 * ROWS
    firsts = torch.stack([rec_a[s]["first"] for s in range(STEPS)]).cpu().numpy()
    when = [set(np.flatnonzero(firsts[:, e])) for e in range(N)]
    assert all(when) and any(a != b for a in when for b in when), "resets must occur and be staggered"
    assert any(int(rec_a[s]["steps"].min()) < NSTEP for s in range(FIRST_UPDATE, STEPS)), "no cut n-step window"

    rec_c, end_c = uninterrupted(prioritized)
    same(rec_c, rec_a, "A' against A: the loop itself is not deterministic")
    same(end_c, end_a, "A' against A (final state): the loop itself is not deterministic")

    path = str(tmp_path / "loop.pt")
    o = build_loop(prioritized, 5, 2)
    first_row(o)
    rec_b = {}
    run_steps(o, 0, CUT, rec_b)
    assert o["iterator"]._ahead is not None, "a look-ahead batch must be pending at the save"
    checkpoint.save(path, extra={"step": CUT}, **o)
    same({s: rec_b[s] for s in range(CUT)}, {s: rec_a[s] for s in range(CUT)}, "B before the save")
    o.clear()
    del o
    gc.collect()
    torch.manual_seed(12345)
    torch.rand(5)
    torch.rand(5, device="cuda")
    torch.randn(7, device="cuda")
    o = build_loop(prioritized, 77, 99)                                    # other weights, another RandomState
    assert checkpoint.load(path, **o) == {"step": CUT}
    assert o["store"].T == CUT + 1 and o["iterator"]._ahead is not None
    same(o["store"].last_index, rec_a[CUT - 1]["index"], "the restored look-ahead batch")
    same(o["env"].render(), o["store"].frames[(CUT % ROWS) * N:(CUT % ROWS + 1) * N].view(N, 3, 84, 84), "the restored frame")
    run_steps(o, CUT, STEPS, rec_b)
    same({s: rec_b[s] for s in range(CUT, STEPS)}, {s: rec_a[s] for s in range(CUT, STEPS)}, "B after the resume")
    same(final_state(o), end_a, "B's final state")


# ------------------------------------------------------------------------------------------------ 3 - 5. stores without an agent
class EnvFeed:
    """rows from a VecReach driven by a seeded pool of actions: what add() takes"""

    def __init__(self, n, a, seed):
        from drqv2_amd.envs import VecReach
        self.env, self.n, self.a, self.seed = VecReach(n, "cuda", action_dim=a, episode_length=EL, seed=3), n, a, seed

    def row(self, t):
        if t == 0:
            z = torch.zeros(self.n, device="cuda")
            return staggered_reset(self.env), torch.zeros(self.n, self.a, device="cuda"), z, z + 1, None
        action = torch.from_numpy(rs_(self.seed + t).uniform(-2, 2, (self.n, self.a)).astype(np.float32)).cuda()
        frame, reward, discount, first = self.env.step(action)
        return frame, action, reward, discount, first

    def parts(self):
        return {"env": self.env}


class PoolFeed:
    """rows of stacked observations from a seeded pool: row t is a function of (seed, t) alone, so it needs no state"""

    def __init__(self, n, a, seed):
        self.n, self.a, self.seed = n, a, seed

    def row(self, t):
        r = rs_(self.seed + t)
        obs = torch.from_numpy(r.randint(0, 256, (self.n, 9, 84, 84)).astype(np.uint8)).cuda()
        action = torch.from_numpy(r.uniform(-1, 1, (self.n, self.a)).astype(np.float32)).cuda()
        reward = torch.from_numpy(r.uniform(0, 1, self.n).astype(np.float32)).cuda()
        discount = torch.from_numpy((r.uniform(0, 1, self.n) > 0.1).astype(np.float32)).cuda()
        first = torch.from_numpy((r.uniform(0, 1, self.n) < 0.2).astype(np.uint8)).cuda()
        return obs, action, reward, discount, first

    def parts(self):
        return {}


def td_errors(t, n):
    return torch.from_numpy(rs_(9000 + t).uniform(0, 2, n).astype(np.float32)).cuda()


def drive(store, feed, lo, hi, rec, it=None):
    """rows lo .. hi-1 added, a batch of 8 drawn after every add once a row is drawable.  it = None: sample(8) itself,
    and a prioritized batch writes its priorities at once.  With the store's iterator the order is update()'s: the batch
    drawn BEFORE this row was added is consumed, writes its priorities, and the next one is drawn ahead"""
    for t in range(lo, hi):
        store.add(*feed.row(t))
        blo, bhi = store.bounds()
        if bhi < blo:
            continue
        batch = next(it) if it is not None else store.sample(B)
        row = {"reward": batch[2].clone(), "discount": batch[3].clone(), "obs": batch[0].clone(), "next": batch[4].clone()}
        if store.tree is not None:
            row["weights"], row["tree_before"] = batch.weights.clone(), store.tree.clone()
            batch.update_priorities(td_errors(t, B))
            row["tree"] = store.tree.clone()
        if it is not None:
            it.prefetch()
        row["index"], row["steps"] = store.last_index.clone(), store.last_steps.clone()
        rec[store.T] = row


def ring_of(store):
    out = {n: getattr(store, n).clone() for n in RING}
    out["T"], out["tree"] = store.T, None if store.tree is None else store.tree.clone()
    return out


def frame_store(prioritized, seed):
    from drqv2_amd.replay import VecFrameReplay
    s = VecFrameReplay(ROWS, N, A, NSTEP, 0.99, "cuda", seed=seed, guard_rows=GUARD, priority_alpha=0.6 if prioritized else None)
    s.batch_size = B
    return s


def stack_store(prioritized, seed):
    from drqv2_amd.replay import VecDeviceReplay
    s = VecDeviceReplay(10, 2, (9, 84, 84), A, NSTEP, 0.99, "cuda", seed=seed, guard_rows=GUARD,
                        priority_alpha=0.6 if prioritized else None)
    s.batch_size = B
    return s


def interrupted_against_uninterrupted(make_store, make_feed, prioritized, cut, end, path, with_iterator=False):
    """the uninterrupted run twice (the control), then: `cut` rows, save, fresh objects with another seed, load, on to
    `end` rows.  Every draw after the save and the final ring equal the uninterrupted run's.  Returns that run"""
    from drqv2_amd import checkpoint
    whole = []
    for _ in range(2):
        store, feed, rec = make_store(prioritized, 1), make_feed(), {}
        drive(store, feed, 0, end, rec, iter(store) if with_iterator else None)
        whole.append((rec, ring_of(store)))
    same(whole[1], whole[0], "the uninterrupted run against itself: the loop is not deterministic")
    rec_a, ring_a = whole[0]
    assert len(rec_a) >= end - cut and ring_a["T"] == end

    store, feed, rec_b = make_store(prioritized, 1), make_feed(), {}
    it = iter(store) if with_iterator else None
    drive(store, feed, 0, cut, rec_b, it)
    parts = dict(feed.parts(), store=store, **({"iterator": it} if with_iterator else {}))
    checkpoint.save(path, **parts)
    live = min(cut, store.R) * store.N
    del store, feed, it, parts
    gc.collect()
    store, feed = make_store(prioritized, 4242), make_feed()
    it = iter(store) if with_iterator else None
    checkpoint.load(path, **dict(feed.parts(), store=store, **({"iterator": it} if with_iterator else {})))
    assert store.T == cut and (it is None or it._ahead is not None or cut <= NSTEP)
    fresh = make_store(prioritized, 0)
    for n in RING[1:]:                                                     # above the live slots: the constructor's values
        same(getattr(store, n)[live:], getattr(fresh, n)[live:], ("above the live slots", n))
    drive(store, feed, cut, end, rec_b, it)
    same({t: rec_b[t] for t in rec_a if t > cut}, {t: rec_a[t] for t in rec_a if t > cut}, "the draws after the resume")
    same(ring_of(store), ring_a, "the final ring")
    return rec_a


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_resume_before_the_wrap(lib, tmp_path, prioritized):
    """the ring and the environment without an agent, sample(8) after every add: saved at T = 5 < 12 rows (15 live slots
    of 36), loaded into a fresh store, on to T = 30"""
    from drqv2_amd import checkpoint
    interrupted_against_uninterrupted(frame_store, lambda: EnvFeed(N, A, 700), prioritized, 5, 30, str(tmp_path / "early.pt"))
    sd = torch.load(str(tmp_path / "early.pt"), weights_only=True)["store"]
    assert sd["T"] == 5 and all(sd[n].shape[0] == 5 * N for n in RING) and checkpoint.FORMAT == sd["format"]


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_resume_of_the_stacked_store_across_the_wrap(lib, tmp_path, prioritized):
    """VecDeviceReplay with obs_shape (9, 84, 84), N = 2, 10 rows: saved at T = 14, on to T = 30"""
    interrupted_against_uninterrupted(stack_store, lambda: PoolFeed(2, A, 300), prioritized, 14, 30, str(tmp_path / "stack.pt"))


def test_priorities_of_a_restored_pending_batch(lib, tmp_path):
    """through the iterator, in update()'s order: the batch that is pending at the save is consumed after the load, one
    row later, and writes the leaves it writes in the uninterrupted run (the tree after every update is compared) -- and
    it does write: that tree differs from the one before.  A restored batch whose stamp is guard_rows rows old writes
    nothing"""
    from drqv2_amd import checkpoint
    path = str(tmp_path / "per.pt")
    rec_a = interrupted_against_uninterrupted(frame_store, lambda: EnvFeed(N, A, 500), True, 20, 30, path, with_iterator=True)
    assert not torch.equal(rec_a[21]["tree"], rec_a[21]["tree_before"])

    store, feed = frame_store(True, 7), EnvFeed(N, A, 500)
    it = iter(store)
    checkpoint.load(path, store=store, iterator=it, env=feed.env)
    pending = it._ahead
    assert pending._stamp == 20 and store.T == 20
    for t in range(20, 20 + GUARD):                                        # guard_rows rows pass: the slots may be others'
        store.add(*feed.row(t))
    before = store.tree.clone()
    batch = next(it)
    assert batch is pending
    batch.update_priorities(td_errors(0, B))
    same(store.tree, before, "a batch overtaken by guard_rows rows must write nothing")


# ------------------------------------------------------------------------------------------------ 6. statistics
def test_stats_resume_mid_evaluation(lib):
    """max_episodes_per_env = 2, N = 3, saved after 8 steps (mid-evaluation), on to 30: complete, the totals and the
    records at the end equal the uninterrupted run's; a read() after the load equals the read() before the save"""
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import VecEpisodeStats
    header = lambda s: [s.rows, s.episodes, s.length_sum, s.return_sum, s.min_return, s.max_return, s.complete, s.lost]

    def steps(env, stats, lo, hi):
        for t in range(lo, hi):
            if t == 0:
                env.reset()
                stats.step(torch.zeros(N, device="cuda"))
                continue
            _, reward, _, first = env.step(torch.from_numpy(rs_(40 + t).uniform(-2, 2, (N, A)).astype(np.float32)).cuda())
            stats.step(reward, first)

    mk = lambda: (VecReach(N, "cuda", action_dim=A, episode_length=EL, seed=3),
                  VecEpisodeStats(N, "cuda", log_size=16, max_episodes_per_env=2))
    env, stats = mk()
    steps(env, stats, 0, 31)
    want, want_running = stats.read(), (stats.episode_return.clone(), stats.episode_length.clone(), stats.episodes_done.clone())
    assert want.complete and want.episodes == 2 * N
    final_env = env.state()

    env, stats = mk()
    steps(env, stats, 0, 9)
    mid = stats.read()
    assert 0 < mid.episodes < 2 * N and not mid.complete, "the save must fall into the evaluation"
    saved = stats.state_dict(), env.state_dict()
    del env, stats
    env, stats = mk()
    steps(env, stats, 0, 4)                                                # a used object, not a fresh one
    stats.load_state_dict(saved[0])
    env.load_state_dict(saved[1])
    again = stats.read()
    assert header(again) == header(mid) and again.records.tobytes() == mid.records.tobytes()
    steps(env, stats, 9, 31)
    got = stats.read()
    assert header(got) == header(want) and got.records.tobytes() == want.records.tobytes()
    same((stats.episode_return, stats.episode_length, stats.episodes_done), want_running, "the running tensors")
    same(env.state(), final_env, "the environment")
