"""The device environment on the GPU: drq_vec_reach_step / drq_vec_reach_image and VecReach against the numpy restatement
of the task (tests/vec_env_oracle.py), and the whole collection loop -- observation() -> act_batch() -> step() -> add() ->
stats.step() -> update() -- driven by it.

Bounds.  Everything is compared bit for bit.  The task is single float32 operations in a fixed order (the file is built
with -ffp-contract=off) and integer arithmetic after the two pixel centres, the oracle performs the same operations on
numpy float32 scalars, and the hash is uint32 arithmetic.  The rings and the statistics are copies and float32 adds of
those values, already held to their own oracles elsewhere.  return_sum: every reward 1 - d2 is a multiple of 2^-24 (d2 in
[0.5, 1) has that ulp, d2 < 0.5 rounds the difference to it), so is every float32 running return, and at most 32 returns
below 6 sum to less than 2^8: 32 significant bits, exact in float64 in any order -- equal to the oracle's math.fsum.

Shapes.  N = 3 (odd, several workgroups) and N = 65 (one more than a wave of environments), episode_length 5, A = 2 and
A = 6 (the row stride of the action differs from the two columns read), 40 steps: about seven episodes per environment.
Actions are uniform in [-2, 2], so the clamp is hit; one in sixteen components is NaN; every third environment is aimed
straight at its target, so some reach it.  The oracle run is made once per configuration, shared and never modified;
that it holds a reached target, a time limit and two environments resetting on different steps is asserted on it."""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_env_oracle as E
from tests import vec_stats_oracle as VS
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p, rs_
from tests.test_hip_vec_replay import raw
from tests.vec_env_checks import U8, entry_on_poisoned_memory, lib_fixture, same_bits, same_state, state_words

pytestmark = pytest.mark.gpu
L, STEPS = 5, 40
CONFIGS = ((3, 2), (3, 6), (65, 2), (65, 6))
SEED = 11
STATE = ("pos", "target", "t", "episode", "over")
lib = lib_fixture("drq_vec_reach_step", "the device-environment entries are missing")


def reference_run(N, A, seed=SEED, steps=STEPS, episode_length=L):
    """the oracle driven for `steps` steps: the actions it was given and everything it returned.  Actions: uniform in
    [-2, 2]; environments 0, 3, 6, ... aim at their target (the exact difference over 0.1, unclamped: the environment
    clamps); one component in sixteen is NaN"""
    r = rs_(seed * 1000 + N * 10 + A)
    o = E.ReachOracle(N, episode_length=episode_length, seed=seed)
    run = {"frame0": o.reset(), "state0": o.state(), "actions": [], "out": [], "reset_steps": [set() for _ in range(N)]}
    for s in range(steps):
        a = r.uniform(-2, 2, (N, A)).astype(np.float32)
        a[::3, :2] = (o.target[::3] - o.pos[::3]) / np.float32(0.1)
        a[r.randint(0, 16, (N, A)) == 0] = np.nan
        out = o.step(a)
        for e in np.flatnonzero(out[3]):
            run["reset_steps"][e].add(s)
        run["actions"].append(a)
        run["out"].append(out)
    run["state"], run["reached"], run["timed_out"] = o.state(), o.reached, o.timed_out
    return run


@pytest.fixture(scope="module")
def runs():
    """computed once, shared, never modified"""
    return {cfg: reference_run(*cfg) for cfg in CONFIGS}


def covers(run):
    """a reached target, a time limit, a NaN and a clamped action, and two environments resetting on different steps"""
    acts = np.stack(run["actions"])[:, :, :2]
    staggered = any(a and b and a != b for a in run["reset_steps"] for b in run["reset_steps"])
    return (run["reached"] >= 1 and run["timed_out"] >= 1 and staggered and bool(np.isnan(acts).any())
            and bool((np.abs(np.nan_to_num(acts)) > 1).any()))


# ------------------------------------------------------------------------------------------------ VecReach against the oracle
@pytest.mark.parametrize("N,A", CONFIGS)
def test_vec_reach_matches_the_oracle_bit_for_bit(runs, N, A):
    """reset(), then 40 steps: frame, reward, discount and first after every step, the state at both ends"""
    from drqv2_amd.envs import VecReach
    run = runs[N, A]
    assert covers(run), "the inputs no longer cover a reached target, a time limit and staggered resets"
    env = VecReach(N, "cuda", action_dim=A, episode_length=L, seed=SEED)
    frame = env.reset()
    assert frame.is_cuda and frame.dtype == torch.uint8 and tuple(frame.shape) == (N, 3, 84, 84)
    same_bits(frame.cpu().numpy(), run["frame0"], "first frame")
    same_state(env.state(), run["state0"], keys=STATE)
    kept = []
    for s in range(STEPS):
        out = env.step(torch.from_numpy(run["actions"][s]).cuda())
        assert all(t.is_cuda for t in out) and [t.dtype for t in out] == [torch.uint8, torch.float32, torch.float32, torch.uint8]
        for name, t, want in zip(("frame", "reward", "discount", "first"), out, run["out"][s]):
            same_bits(t.cpu().numpy(), want, (s, name))
        kept.append(out)
        if s >= 1:      # two output sets in turn: the set of the step before is intact, the one before that is reused
            same_bits(kept[s - 1][0].cpu().numpy(), run["out"][s - 1][0], (s, "the frame of the step before"))
        if s >= 2:
            assert kept[s - 2][0].data_ptr() == out[0].data_ptr() and kept[s - 1][0].data_ptr() != out[0].data_ptr()
    same_state(env.state(), run["state"], keys=STATE)


# ------------------------------------------------------------------------------------------------ the entry on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 2), (65, 6)])
def test_reach_step_writes_every_output_byte_and_nothing_else(lib, runs, N, A):
    """drq_vec_reach_step on guarded allocations full of the sentinel: the reset of all, then 12 steps into fresh poisoned
    outputs each.  The outputs equal the oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255,
    a flag 0 or 1), so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    run = runs[N, A]
    z = lambda shape, dt: dev(torch.zeros(shape, dtype=dt))
    state = [z((N, 2), torch.float32), z((N, 2), torch.float32), z(N, torch.int32), z(N, torch.int32), z(N, torch.uint8)]
    entry_on_poisoned_memory(lambda action, reset_all, outs: lib.drq_vec_reach_step(
        *(p(t) for t in state), N, A, action, SEED, L, reset_all, *outs, None), run, N, substeps=False)
    o = E.ReachOracle(N, episode_length=L, seed=SEED)
    o.reset()
    for s in range(12):
        o.step(run["actions"][s])
    same_state(state_words(dict(zip(STATE, state)), STATE), o.state(), keys=STATE)


# ------------------------------------------------------------------------------------------------ the renderer-shaped image
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("S", [84, 168, 252, 336])
def test_image_is_the_replicated_frame_and_add_render_stores_the_frame(lib, runs, S, C):
    """image(S, C) against the oracle's k x k replication (the entry itself once more into poisoned memory), and two
    rings over 6 steps: one fed add_render(env.image(S, C), ...), one fed add(frame, ...) -- the same bytes"""
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import VecFrameReplay
    N, A = 3, 2
    run = runs[N, A]
    env = VecReach(N, "cuda", action_dim=A, episode_length=L, seed=SEED)
    a, b = (VecFrameReplay(16, N, A, 3, 0.99, "cuda", seed=1) for _ in range(2))
    for s in range(7):                                                             # the reset row, then 6 steps
        if s == 0:
            frame, action = env.reset(), torch.zeros(N, A, device="cuda")
            reward, discount, first = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"), None
        else:
            action = torch.from_numpy(run["actions"][s - 1]).cuda()
            frame, reward, discount, first = env.step(action)
        want = run["frame0"] if s == 0 else run["out"][s - 1][0]
        img = env.image(S, C)
        assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == (N, S, S, C)
        same_bits(img.cpu().numpy(), E.replicate(want, S, C), (s, "image"))
        a.add_render(img, action, reward, discount, first)
        b.add(frame, action, reward, discount, first)
        for n in ("frames", "action", "reward", "discount", "first"):
            assert np.array_equal(raw(getattr(a, n)[:(s + 1) * N]), raw(getattr(b, n)[:(s + 1) * N])), (s, n)
        same_bits(a.frames[s * N:(s + 1) * N].view(N, 3, 84, 84).cpu().numpy(), want, (s, "ring frames"))
    assert torch.equal(a.observation(), b.observation())
    out = poison.alloc((N, S, S, C), torch.uint8, "cuda", name="image")
    src = dev(torch.from_numpy(want), "frame")
    assert lib.drq_vec_reach_image(p(src), p(out), N, S, C, None) == 0
    same_bits(out.cpu().numpy(), E.replicate(want, S, C), "the entry")          # no 0xA5 in it: every byte was written
    assert not (out.cpu().numpy() == U8).any()


# ------------------------------------------------------------------------------------------------ the whole loop
def test_collection_loop_end_to_end():
    """observation() -> act_batch() -> step() -> add() -> stats.step(), update() once rows suffice: N = 8 environments of 6
    steps, a ring of 32 rows, 24 steps, batch 16.  The oracle is driven by the recorded actions afterwards: the ring's
    first / reward / discount / frames are its outputs, the episode statistics the ones it implies, the metrics finite"""
    import drqv2
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    N, A, EL, ROWS, T, B = 8, 2, 6, 32, 24, 16
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 20, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = VecReach(N, "cuda", action_dim=A, episode_length=EL, seed=3)
    store = VecFrameReplay(ROWS, N, A, 3, 0.99, "cuda", seed=2)
    store.batch_size = B
    stats = VecEpisodeStats(N, "cuda")
    it = iter(store)
    zeros = torch.zeros(N, device="cuda")
    store.add(env.reset(), torch.zeros(N, A, device="cuda"), zeros, torch.ones(N, device="cuda"))
    stats.step(zeros)
    actions, metrics = [], []
    for step in range(T):
        action = agent.act_batch(store.observation(), step, False)
        assert action.is_cuda and tuple(action.shape) == (N, A)
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, reward, discount, first)
        stats.step(reward, first)
        actions.append(action.cpu().numpy().copy())
        lo, hi = store.bounds()
        if hi >= lo:
            metrics.append(agent.update(it, step))
    snap = stats.read()
    assert len(metrics) == T - 3 + 1 and all(len(m) == 8 for m in metrics)
    assert all(np.isfinite(v) for m in metrics for v in m.values())

    o, so = E.ReachOracle(N, episode_length=EL, seed=3), VS.StatsOracle(N)
    want = [(o.reset(), np.zeros(N, np.float32), np.ones(N, np.float32), np.ones(N, np.uint8))]
    so.step(np.zeros(N, np.float32))
    for a in actions:
        want.append(o.step(a))
        so.step(want[-1][1], want[-1][3])
    assert store.T == T + 1 <= ROWS
    held = (T + 1) * N
    same_bits(store.frames[:held].cpu().numpy().reshape(T + 1, N, 3, 84, 84), np.stack([w[0] for w in want]), "frames")
    same_bits(store.reward[:held].cpu().numpy().reshape(T + 1, N), np.stack([w[1] for w in want]), "reward")
    same_bits(store.discount[:held].cpu().numpy().reshape(T + 1, N), np.stack([w[2] for w in want]), "discount")
    same_bits(store.first[:held].cpu().numpy().reshape(T + 1, N), np.stack([w[3] for w in want]), "first")
    same_bits(store.action[N:held].cpu().numpy().reshape(T, N, A), np.stack(actions), "action")
    same_state(env.state(), o.state(), keys=STATE)
    ws = so.snapshot()
    assert ws.episodes >= N and o.reached + o.timed_out >= ws.episodes           # every environment finished at least one
    assert snap.rows == T + 1 and snap.episodes == ws.episodes and snap.length_sum == ws.length_sum
    assert snap.return_sum == ws.return_sum and snap.mean_return == ws.mean_return   # exact: see the module docstring
    assert snap.records.tobytes() == ws.records.tobytes()
    assert snap.min_return == ws.min_return and snap.max_return == ws.max_return


# ------------------------------------------------------------------------------------------------ determinism
def test_same_seed_same_bytes_other_seed_other_frame(runs):
    from drqv2_amd.envs import VecReach
    N, A = 65, 6
    run = runs[N, A]
    envs = [VecReach(N, "cuda", action_dim=A, episode_length=L, seed=s) for s in (SEED, SEED, SEED + 1)]
    f = [e.reset().clone() for e in envs]
    assert torch.equal(f[0], f[1]) and not torch.equal(f[0], f[2])
    assert all(not torch.equal(f[0][e], f[2][e]) for e in range(N))               # the seed moves every environment
    for s in range(12):
        action = torch.from_numpy(run["actions"][s]).cuda()
        o0, o1 = envs[0].step(action), envs[1].step(action.clone())
        for x, y in zip(o0, o1):
            assert raw(x).tobytes() == raw(y).tobytes(), s
    s0, s1 = envs[0].state(), envs[1].state()
    same_state(s0, s1, keys=STATE)
    from drqv2_amd import _lib
    fresh = VecReach(N, "cuda", action_dim=A)
    with pytest.raises(_lib.DrqError, match="reset"):
        fresh.step(torch.zeros(N, A, device="cuda"))
