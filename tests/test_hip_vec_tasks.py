"""Tasks and action repeat of the device environment on the GPU: drq_vec_task_step, VecReach(action_repeat=) and
VecPointMass against the numpy restatement (tests/vec_tasks_oracle.py), the new entry against drq_vec_reach_step, and the
loop around a point mass at action_repeat 2 -- ring, statistics, act_batch(), update(), checkpoint, evaluate().

Bounds.  Everything is compared bit for bit.  A macro step is single float32 operations in a fixed order (the file is
built with -ffp-contract=off) -- the sub-steps, and reward = reward + r * discount, discount = discount * d between them
-- and integer arithmetic after the two pixel centres; the oracle performs the same operations on numpy float32 scalars.
The rings and the statistics are copies and float32 adds of those values, held to their own oracles elsewhere.
return_sum: a point-mass row at repeat 2 is the float32 sum of two rewards, each a multiple of 2^-24 in [0, 1], hence
itself one; so is every float32 running return, which stays below 2^8; at most 32 of them sum to less than 2^13: 37
significant bits, exact in float64 in any order -- equal to the oracle's math.fsum.

Shapes.  N = 1, 3, 65 (one workgroup, odd, one more than a wave of environments), A = 2 and 6 (the row stride of the
action differs from the two columns read), repeat 1 .. 4 with episode_length 7, so the time limit falls inside a repeat
for 2, 3 and 4; 40 macro steps.  Actions: tests/vec_tasks_oracle.wild_actions -- uniform in [-2, 2], NaN, +-inf, and every
third environment homing on its target, so reach ends inside a repeat.  The oracle runs are made once per configuration,
shared and never modified; that each holds a row cut short by the target (reach), one cut short by the time limit and a
full-length row is asserted on the oracle's run (and, without a GPU, by tests/test_cpu_vec_tasks.py)."""
import gc

import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_stats_oracle as VS
from tests import vec_tasks_oracle as T
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p
from tests.test_hip_vec_replay import raw
from tests.vec_env_checks import (OUT, alloc_outs, entry_on_poisoned_memory, lib_fixture, refused_on_poisoned_memory, run_of,
                                  same_bits, same_state)

pytestmark = pytest.mark.gpu
L, STEPS, SEED = 7, 40, 5
CONFIGS = ((1, 2), (1, 6), (3, 2), (3, 6), (65, 2), (65, 6))
REPEATS = (1, 2, 3, 4)
STATE = ("pos", "target", "vel", "t", "episode", "over")
lib = lib_fixture("drq_vec_task_step", "the task entry is missing")


@pytest.fixture(scope="module")
def runs():
    """the oracle's runs: each computed once, on first use, shared and never modified"""
    return lambda task, N, A, k: run_of(T, (task, N, A, k, SEED, STEPS, L))


def cls_of(task):
    from drqv2_amd import envs
    return {"reach": envs.VecReach, "pointmass": envs.VecPointMass}[task]


# ------------------------------------------------------------------------------------------------ the classes against the oracle
@pytest.mark.parametrize("k", REPEATS)
@pytest.mark.parametrize("N,A", CONFIGS)
@pytest.mark.parametrize("task", T.TASKS)
def test_env_matches_the_oracle_bit_for_bit(runs, task, N, A, k):
    """reset(), then 40 macro steps: frame, reward, discount, first, last_substeps and state() after every step"""
    run = runs(task, N, A, k)
    assert T.covers(run, task, k), "the inputs no longer cover a row cut by the target, one cut by the time limit, a full one"
    env = cls_of(task)(N, "cuda", action_dim=A, episode_length=L, seed=SEED, action_repeat=k)
    frame = env.reset()
    same_bits(frame.cpu().numpy(), run["frame0"], "first frame")
    same_bits(env.last_substeps.cpu().numpy(), np.zeros(N, np.int32), "substeps of the reset")
    same_state(env.state(), run["state0"], "reset")
    kept = []
    for s in range(STEPS):
        out = env.step(torch.from_numpy(run["actions"][s]).cuda())
        assert len(out) == 4 and [t.dtype for t in out] == [torch.uint8, torch.float32, torch.float32, torch.uint8]
        sub = env.last_substeps
        assert sub.is_cuda and sub.dtype == torch.int32 and tuple(sub.shape) == (N,)
        for name, t, want in zip(OUT, out + (sub,), run["out"][s]):
            same_bits(t.cpu().numpy(), want, (s, name))
        same_state(env.state(), run["states"][s], s)
        kept.append(sub)
        if s >= 1:      # two output sets in turn: the set of the step before is intact, the one before that is reused
            same_bits(kept[s - 1].cpu().numpy(), run["out"][s - 1][4], (s, "the substeps of the step before"))
        if s >= 2:
            assert kept[s - 2].data_ptr() == sub.data_ptr() != kept[s - 1].data_ptr()


# ------------------------------------------------------------------------------------------------ the new entry against the old one
def test_task_reach_at_repeat_1_writes_the_bytes_of_the_old_entry(lib, runs):
    """N = 65, A = 6: both entries from the same state -- the oracle's after the reset, then each its own after every one
    of 16 steps, which hold reset rows, reached targets and time limits -- into poisoned outputs: the same bytes in
    frame, reward, discount, first and the five state arrays; substeps is 1 - first"""
    N, A = 65, 6
    run = runs("reach", N, A, 1)
    assert run["reached"] >= 1 and run["timed_out"] >= 1
    s0 = run["state0"]
    mk = lambda: [dev(torch.from_numpy(s0["pos"]), "pos"), dev(torch.from_numpy(s0["target"]), "target"),
                  dev(torch.from_numpy(s0["t"]), "t"), dev(torch.from_numpy(s0["episode"].view(np.int32)), "episode"),
                  dev(torch.from_numpy(s0["over"]), "over")]
    old, new = mk(), mk()
    for s in range(16):
        action = dev(torch.from_numpy(run["actions"][s]), "action")
        oo, on = alloc_outs(N, substeps=False), alloc_outs(N, substeps=False)
        sub = poison.alloc(N, torch.int32, "cuda", name="substeps")
        assert lib.drq_vec_reach_step(*(p(t) for t in old), N, A, p(action), SEED, L, 0, *(p(t) for t in oo), None) == 0
        assert lib.drq_vec_task_step(0, p(new[0]), p(new[1]), None, *(p(t) for t in new[2:]), N, A, p(action), SEED, L, 1, 0,
                                     *(p(t) for t in on), p(sub), None) == 0
        for name, a, b, want in zip(OUT, oo, on, run["out"][s]):
            assert raw(a).tobytes() == raw(b).tobytes(), (s, name)
            same_bits(b.cpu().numpy(), want, (s, name))
        for name, a, b in zip(("pos", "target", "t", "episode", "over"), old, new):
            assert raw(a).tobytes() == raw(b).tobytes(), (s, name)
        assert torch.equal(sub, 1 - on[3].to(torch.int32)), s
        poison.check()


# ------------------------------------------------------------------------------------------------ the entry on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 2), (65, 6)])
@pytest.mark.parametrize("task", T.TASKS)
def test_task_step_writes_every_output_byte_and_nothing_else(lib, runs, task, N, A):
    """drq_vec_task_step at repeat 3 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each.  The outputs equal the oracle's, which never holds the byte sentinel
    0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one, so every byte was written; check() finds the
    guard bands of outputs, state and action untouched.  Reach is given a vel array it must neither read nor write"""
    k = 3
    run = runs(task, N, A, k)
    z = lambda shape, dt, name: dev(torch.zeros(shape, dtype=dt), name)
    state = {"pos": z((N, 2), torch.float32, "pos"), "target": z((N, 2), torch.float32, "target"),
             "vel": z((N, 2), torch.float32, "vel") if task == "pointmass"
             else poison.alloc((N, 2), torch.float32, "cuda", name="vel", kind="refused"),
             "t": z(N, torch.int32, "t"), "episode": z(N, torch.int32, "episode"), "over": z(N, torch.uint8, "over")}
    entry_on_poisoned_memory(lambda action, reset_all, outs: lib.drq_vec_task_step(
        T.TASKS.index(task), *(p(state[n]) for n in STATE), N, A, action, SEED, L, k, reset_all, *outs, None), run, N,
        state=state, compared=[n for n in STATE if n != "vel" or task == "pointmass"])


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_tasks_oracle.refused_calls, all held to return the error without a GPU by
    tests/test_cpu_vec_tasks.py) on real allocations full of the sentinel: the error, and check() finds every byte of
    the state, the action, the frame and the four scalar outputs still poison"""
    refused_on_poisoned_memory(0x600, lambda S0, ACT, FR, SC: ((lib.drq_vec_task_step, T.refused_calls(S0, ACT, FR, SC), 54),))


# ------------------------------------------------------------------------------------------------ checkpoints
def test_point_mass_state_dict_resumes_bit_for_bit(runs):
    """N = 3, repeat 2: 6 steps, state_dict() with velocities that are not zero, 10 more steps; a fresh VecPointMass given
    the dict renders the saved frame and takes the same 10 steps to the bit"""
    from drqv2_amd.envs import VecPointMass
    N, A, k = 3, 2, 2
    run = runs("pointmass", N, A, k)
    mk = lambda: VecPointMass(N, "cuda", action_dim=A, episode_length=L, seed=SEED, action_repeat=k)
    env = mk()
    env.reset()
    for s in range(6):
        frame = env.step(torch.from_numpy(run["actions"][s]).cuda())[0]
    saved_frame = frame.clone()
    sd = env.state_dict()
    assert sd["vel"].abs().max() > 0 and 0 < int(sd["t"].max()) < L, "the save must fall inside an episode, in motion"
    same_bits(sd["vel"].numpy(), run["states"][5]["vel"], "the saved velocity")
    fresh = mk()
    fresh.load_state_dict(sd)
    assert raw(fresh.render()).tobytes() == raw(saved_frame).tobytes()
    same_state(fresh.state(), run["states"][5], "restored")
    for s in range(6, 16):
        action = torch.from_numpy(run["actions"][s]).cuda()
        a, b = env.step(action), fresh.step(action)
        for name, x, y, want in zip(OUT, a + (env.last_substeps,), b + (fresh.last_substeps,), run["out"][s]):
            assert raw(x).tobytes() == raw(y).tobytes(), (s, name)
            same_bits(y.cpu().numpy(), want, (s, name))
    same_state(fresh.state(), env.state(), "after 10 steps")
    with pytest.raises(ValueError, match="action_repeat"):
        VecPointMass(N, "cuda", action_dim=A, episode_length=L, seed=SEED, action_repeat=3).load_state_dict(sd)


def test_whole_loop_around_a_point_mass_resumes_bit_for_bit(lib, tmp_path):
    """the loop of tests/test_hip_checkpoint.py at its shapes (N = 3, a ring of 12 rows, 40 steps, saved after step 22,
    uniform sampling) around VecPointMass(action_repeat=2): A uninterrupted; B saved, every object deleted, the generators
    moved, new objects with other seeds, loaded, resumed.  What B records from the save on and its final state equal A's"""
    import drqv2
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecPointMass
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    from tests import test_hip_checkpoint as C

    def build_loop(torch_seed, store_seed):
        torch.manual_seed(torch_seed)
        torch.cuda.manual_seed_all(torch_seed)
        agent = drqv2.DrQV2Agent((9, 84, 84), (C.A,), "cuda", 1e-3, 20, 64, 0.01, 8, 1, "0.5", 0.3, True)
        env = VecPointMass(C.N, "cuda", action_dim=C.A, episode_length=C.EL, seed=3, action_repeat=2)
        store = VecFrameReplay(C.ROWS, C.N, C.A, C.NSTEP, 0.99, "cuda", seed=store_seed, guard_rows=C.GUARD)
        store.batch_size = C.B
        return {"agent": agent, "env": env, "store": store, "stats": VecEpisodeStats(C.N, "cuda"), "iterator": iter(store)}

    o = build_loop(5, 2)
    C.first_row(o)
    rec_a = {}
    C.run_steps(o, 0, C.STEPS, rec_a)
    end_a = C.final_state(o)
    assert "vel" in end_a["env"] and np.abs(end_a["env"]["vel"]).max() > 0
    firsts = torch.stack([rec_a[s]["first"] for s in range(C.STEPS)]).cpu().numpy()
    assert firsts[:C.CUT].any() and firsts[C.CUT:].any(), "resets on both sides of the save"

    path = str(tmp_path / "loop.pt")
    o = build_loop(5, 2)
    C.first_row(o)
    rec_b = {}
    C.run_steps(o, 0, C.CUT, rec_b)
    assert o["env"].state()["vel"].any(), "the save must catch the point masses in motion"
    checkpoint.save(path, extra={"step": C.CUT}, **o)
    o.clear()
    del o
    gc.collect()
    torch.manual_seed(12345)
    torch.rand(5)
    torch.randn(7, device="cuda")
    o = build_loop(77, 99)
    assert checkpoint.load(path, **o) == {"step": C.CUT}
    C.run_steps(o, C.CUT, C.STEPS, rec_b)
    C.same(rec_b, rec_a, "B against A")
    C.same(C.final_state(o), end_a, "B's final state")


# ------------------------------------------------------------------------------------------------ the whole loop
def test_collection_loop_around_a_point_mass_end_to_end():
    """VecPointMass(4, action_repeat 2, episode_length 7) -> add() -> stats.step() -> act_batch(observation()) -> two
    update() calls, 24 steps.  The task oracle is driven by the recorded actions afterwards: the ring holds its outputs,
    the episode statistics are the ones they imply (tests/vec_stats_oracle.py), the metrics are finite"""
    import drqv2
    from drqv2_amd.envs import VecPointMass
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    N, A, k, ROWS, STEPS_, B = 4, 2, 2, 32, 24, 16
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 20, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = VecPointMass(N, "cuda", action_dim=A, episode_length=L, seed=3, action_repeat=k)
    store = VecFrameReplay(ROWS, N, A, 3, 0.99, "cuda", seed=2)
    store.batch_size = B
    stats = VecEpisodeStats(N, "cuda")
    it = iter(store)
    zeros = torch.zeros(N, device="cuda")
    store.add(env.reset(), torch.zeros(N, A, device="cuda"), zeros, torch.ones(N, device="cuda"))
    stats.step(zeros)
    actions, metrics = [], []
    for step in range(STEPS_):
        action = agent.act_batch(store.observation(), step, False)
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, reward, discount, first)
        stats.step(reward, first)
        actions.append(action.cpu().numpy().copy())
        if step >= STEPS_ - 2:
            metrics.append(agent.update(it, step))
    snap = stats.read()
    assert len(metrics) == 2 and all(np.isfinite(v) for m in metrics for v in m.values())

    o, so = T.TaskOracle("pointmass", N, episode_length=L, seed=3, repeat=k), VS.StatsOracle(N)
    want = [(o.reset(), np.zeros(N, np.float32), np.ones(N, np.float32), np.ones(N, np.uint8))]
    so.step(np.zeros(N, np.float32))
    for a in actions:
        want.append(o.step(a)[:4])
        so.step(want[-1][1], want[-1][3])
    held = (STEPS_ + 1) * N
    assert store.T == STEPS_ + 1 <= ROWS
    same_bits(store.frames[:held].cpu().numpy().reshape(STEPS_ + 1, N, 3, 84, 84), np.stack([w[0] for w in want]), "frames")
    same_bits(store.reward[:held].cpu().numpy().reshape(STEPS_ + 1, N), np.stack([w[1] for w in want]), "reward")
    same_bits(store.discount[:held].cpu().numpy().reshape(STEPS_ + 1, N), np.stack([w[2] for w in want]), "discount")
    same_bits(store.first[:held].cpu().numpy().reshape(STEPS_ + 1, N), np.stack([w[3] for w in want]), "first")
    same_bits(store.action[N:held].cpu().numpy().reshape(STEPS_, N, A), np.stack(actions), "action")
    same_state(env.state(), o.state(), "final")
    ws = so.snapshot()
    rows_per_episode = -(-L // k)                                           # 2 + 2 + 2 + 1 simulator steps
    assert ws.episodes == N * (STEPS_ // (rows_per_episode + 1)) and o.timed_out >= ws.episodes
    assert (ws.records["length"] == rows_per_episode).all()                 # lengths count rows, not simulator steps
    assert snap.rows == STEPS_ + 1 and snap.episodes == ws.episodes and snap.length_sum == ws.length_sum
    assert snap.return_sum == ws.return_sum and snap.mean_return == ws.mean_return   # exact: see the module docstring
    assert snap.records.tobytes() == ws.records.tobytes()
    assert snap.min_return == ws.min_return and snap.max_return == ws.max_return


def test_evaluate_runs_a_point_mass():
    """evaluate() takes the class as it takes VecReach: one episode of each of N = 3 environments, every one ceil(7 / 2)
    rows long"""
    import drqv2
    from drqv2_amd.envs import VecPointMass
    from drqv2_amd.evaluate import evaluate
    N, A, k = 3, 2, 2
    torch.manual_seed(3)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    res = evaluate(agent, VecPointMass(N, "cuda", action_dim=A, episode_length=L, seed=7, action_repeat=k), 1, poll_every=4)
    snap = res.snapshot
    assert snap.complete and snap.episodes == N and len(snap.records) == N
    assert sorted(snap.records["env"].tolist()) == list(range(N))
    assert (snap.records["length"] == -(-L // k)).all()
    assert res.steps == 8           # an episode is counted on the row that carries `first`, the fifth step; polled every 4
    assert np.isfinite(snap.mean_return) and 0 <= snap.min_return <= snap.max_return <= L
