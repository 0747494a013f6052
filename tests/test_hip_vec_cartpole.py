"""The cartpole of the device environment on the GPU: drq_vec_cartpole_step / _render raw on poisoned memory, and
drqv2_amd.envs.VecCartpole against the numpy restatement (tests/vec_cartpole_oracle.py), through render(), image(),
state dicts and a checkpoint file.

Bounds.  Everything is compared bit for bit.  A sub-step is single correctly rounded float32 operations (+, -, *, /, sqrt)
in a fixed order -- the file is built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -- and the frame is
integer arithmetic after three floorf; the oracle performs the same operations on numpy float32 scalars and Python
integers.

Shapes.  N = 3, A = 1 and N = 5, A = 3 (odd, more than one workgroup, the action's row stride differs from the one column
read), repeat 1, 2 and 16, both variants, episode_length 7 and 40 macro steps (vec_cartpole_oracle.DRIVEN): the time limit
falls inside a repeat for 2 and 16, and t of environment e starts at e mod 7, so the resets stagger.  In seven steps no
cart reaches a rail end and no pole passes the vertical: two long episodes at repeat 16 (vec_cartpole_oracle.PHYSICS, 960
simulator steps each) do both.  The oracle's runs are made once, shared and never modified; what they cover is asserted
without a GPU by tests/test_cpu_vec_cartpole.py."""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_cartpole_oracle as O
from tests import vec_env_oracle as E
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p
from tests.test_hip_vec_replay import raw
from tests.vec_env_checks import OUT, entry_on_poisoned_memory, lib_fixture, same_bits, same_state

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
STATE = ("phys", "t", "episode", "over")
lib = lib_fixture("drq_vec_cartpole_step", "the cartpole entries are missing")
_RUNS = {}


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN or O.PHYSICS: computed once, on first use, shared, never modified"""
    if cfg not in _RUNS:
        _RUNS[cfg] = O.driven_run(*cfg) if len(cfg) == 4 else O.physics_run(*cfg)
    return _RUNS[cfg]


def make(cfg, episode_length=L):
    from drqv2_amd.envs import VecCartpole
    N, A, k, swing = cfg[:4]
    return VecCartpole(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, swing_up=swing)


def stagger(env, run):
    """the staggered t of the oracle's run into an environment that has just been reset, through load_state_dict()"""
    sd = env.state_dict()
    sd["t"] = torch.from_numpy(run["state0"]["t"])
    env.load_state_dict(sd)


def start(env, run):
    env.reset()
    stagger(env, run)


def follow(env, run, first, last):
    for s in range(first, last):
        out = env.step(torch.from_numpy(run["actions"][s]).cuda())
        assert len(out) == 4 and [t.dtype for t in out] == [torch.uint8, torch.float32, torch.float32, torch.uint8]
        for name, t, want in zip(OUT, out + (env.last_substeps,), run["out"][s]):
            same_bits(t.cpu().numpy(), want, (s, name))
        same_state(env.state(), run["states"][s], s)


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=lambda c: f"N{c[0]}-A{c[1]}-x{c[2]}-{'swingup' if c[3] else 'balance'}")
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn"""
    run = run_of(cfg)
    N = cfg[0]
    env = make(cfg)
    frame = env.reset()
    same_bits(frame.cpu().numpy(), run["frame0"], "first frame")
    same_bits(env.last_substeps.cpu().numpy(), np.zeros(N, np.int32), "substeps of the reset")
    stagger(env, run)
    same_state(env.state(), run["state0"], "reset")
    same_bits(env.render().cpu().numpy(), run["frame0"], "the frame does not depend on t")
    kept = []
    for s in range(O.STEPS):
        follow(env, run, s, s + 1)
        kept.append(env.last_substeps)
        if s >= 1:      # two output sets in turn: the set of the step before is intact, the one before that is reused
            same_bits(kept[s - 1].cpu().numpy(), run["out"][s - 1][4], (s, "the substeps of the step before"))
        if s >= 2:
            assert kept[s - 2].data_ptr() == kept[s].data_ptr() != kept[s - 1].data_ptr()


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: "swingup" if c[3] else "balance")
def test_long_episode_matches_the_oracle_through_rail_ends_and_the_vertical(cfg):
    """60 macro steps of 16 simulator steps in one episode: the carts hit both rail ends and stay there, the poles swing
    through hanging and over the top"""
    run = run_of(cfg)
    assert run["hit_left"] and run["hit_right"] and run["through_hanging"] and run["through_upright"]
    env = make(cfg, episode_length=cfg[5])
    same_bits(env.reset().cpu().numpy(), run["frame0"], "first frame")
    follow(env, run, 0, cfg[4])


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 1), (5, 3)])
@pytest.mark.parametrize("swing", [True, False])
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, swing):
    """drq_vec_cartpole_step at repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each; drq_vec_cartpole_render beside every one.  The outputs equal the
    oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one,
    so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    cfg = (N, A, 2, swing)
    run = run_of(cfg)
    z = lambda shape, dt, name: dev(torch.zeros(shape, dtype=dt), name)
    state = {"phys": z((N, 5), torch.float32, "phys"), "t": z(N, torch.int32, "t"), "episode": z(N, torch.int32, "episode"),
             "over": z(N, torch.uint8, "over")}

    def render_beside(s, want):
        again = poison.alloc((N, 3, 84, 84), torch.uint8, "cuda", name="rendered")
        assert lib.drq_vec_cartpole_render(p(state["phys"]), N, p(again), None) == 0
        same_bits(again.cpu().numpy(), want[0], (s, "render"))

    entry_on_poisoned_memory(lambda action, reset_all, outs: lib.drq_vec_cartpole_step(
        *(p(state[n]) for n in STATE), N, A, action, SEED, L, 2, reset_all, int(swing), *outs, None), run, N,
        state=state, compared=STATE, beside=render_beside,
        after_reset=lambda: state["t"].copy_(torch.from_numpy(run["state0"]["t"])))      # the stagger of the oracle's run


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_cartpole_oracle.refused_calls / refused_renders, all held to return the error without
    a GPU by tests/test_cpu_vec_cartpole.py) on real allocations full of the sentinel: the error, and check() finds every
    byte of the state, the action, the frame and the scalar outputs still poison"""
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    state, action, frame, scalars = al(0x400, "state"), al(0x100, "action"), al(5 * 3 * 84 * 84, "frame"), al(0x400, "scalars")
    calls = O.refused_calls(p(state), p(action), p(frame), p(scalars))
    for a in calls:
        assert lib.drq_vec_cartpole_step(*a, None) == -1, a
    renders = O.refused_renders(p(state), p(frame))
    for a in renders:
        assert lib.drq_vec_cartpole_render(*a, None) == -1, a
    assert len(calls) == 35 and len(renders) == 8
    poison.check()


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_render_after_load_state_dict_and_image_into_the_ring():
    """N = 5, A = 3, repeat 2, balance: 9 steps, state_dict(); a fresh environment given the dict renders the saved frame.
    image() of it at 168 x 168 x 4 is the frame with every pixel twice in both directions, and
    VecFrameReplay.add_render() of that image stores exactly the frame"""
    from drqv2_amd.replay import VecFrameReplay
    cfg = (5, 3, 2, False)
    run = run_of(cfg)
    N, A = cfg[:2]
    env = make(cfg)
    start(env, run)
    follow(env, run, 0, 9)
    want = run["out"][8][0]
    sd = env.state_dict()
    assert sd["kind"] == "VecCartpole" and sd["config"]["swing_up"] is False and tuple(sd["phys"].shape) == (N, 5)
    fresh = make(cfg)
    fresh.load_state_dict(sd)
    same_bits(fresh.render().cpu().numpy(), want, "the frame of the restored state")
    same_state(fresh.state(), run["states"][8], "restored")
    image = fresh.image(168, 4)
    same_bits(image.cpu().numpy(), E.replicate(want, 168, 4), "image()")
    ring = VecFrameReplay(16, N, A, 3, 0.99, "cuda", seed=1)
    ring.add_render(image, torch.zeros(N, A, device="cuda"), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"))
    same_bits(ring.frames[:N].cpu().numpy().reshape(N, 3, 84, 84), want, "the ring's row")
    with pytest.raises(ValueError, match="swing_up"):
        make((N, A, 2, True)).load_state_dict(sd)


def test_checkpoint_round_trip_continues_bit_for_bit(tmp_path):
    """N = 3, repeat 2, swing-up: 6 steps, checkpoint.save() inside an episode and in motion, 10 more steps; a fresh
    environment loaded from the file takes the same 10 steps to the bit, outputs and state"""
    from drqv2_amd import checkpoint
    cfg = (3, 1, 2, True)
    run = run_of(cfg)
    env = make(cfg)
    start(env, run)
    follow(env, run, 0, 6)
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=env, extra={"step": 6})
    saved = env.state()
    assert np.abs(saved["phys"][:, 4]).max() > 0 and 0 < int(saved["t"].max()) < L, "the save must fall inside an episode, in motion"
    fresh = make(cfg)
    assert checkpoint.load(path, env=fresh) == {"step": 6}
    same_state(fresh.state(), run["states"][5], "restored")
    assert raw(fresh.render()).tobytes() == run["out"][5][0].tobytes()
    follow(fresh, run, 6, 16)
    follow(env, run, 6, 16)
    same_state(fresh.state(), env.state(), "after 10 steps")


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks"""
    import drqv2
    from drqv2_amd.evaluate import VecVideo, evaluate
    cfg = (3, 1, 2, True)
    torch.manual_seed(3)
    agent = drqv2.DrQV2Agent((9, 84, 84), (1,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    video = VecVideo(3, "cuda", max_frames=64)
    res = evaluate(agent, make(cfg), 1, poll_every=4, video=video)
    snap = res.snapshot
    assert snap.complete and snap.episodes == 3 and sorted(snap.records["env"].tolist()) == [0, 1, 2]
    assert (snap.records["length"] == -(-L // 2)).all() and len(video) >= 5
    assert np.isfinite(snap.mean_return) and 0 <= snap.min_return <= snap.max_return <= L
