"""The catch of the device environment on the GPU: drq_vec_catch_step / _render raw on poisoned memory, and
drqv2_amd.envs.VecCatch against the numpy restatement (tests/vec_catch_oracle.py), through render(), image(), state dicts, a
checkpoint file, VecDistract, SimHashBonus and the frame ring.

Bounds.  Everything is compared bit for bit.  A sub-step is single correctly rounded float32 operations (+, -, *, /, sqrt)
in a fixed order -- the file is built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -- and the frame is
integer arithmetic after eight floorf; the oracle performs the same operations on numpy float32 scalars and Python
integers.

Shapes.  N = 3, A = 2 and N = 5, A = 4 (odd, more than one workgroup, the action's row stride differs from the two
columns read), repeat 1, 2 and 16, sparse and dense, episode_length 7 and 40 macro steps (vec_catch_oracle.DRIVEN): the
time limit falls inside a repeat for 2 and 16, and t of environment e starts at e mod 7, so the resets stagger.  Seven
steps from a hanging ball meet a slack or a taut tether and little else: two long episodes at repeat 16
(vec_catch_oracle.PHYSICS, 960 simulator steps of five hand-set environments each) meet every contact from every side,
the degenerate normal, every stop, every clamp and a ball at rest in the cup.  The poses (vec_catch_oracle.POSES) are where
the pixel rule can go wrong, at both ends of cup_width's range.  The oracle's runs are made once, shared and never
modified; what they cover is asserted without a GPU by tests/test_cpu_vec_catch.py."""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_catch_oracle as O
from tests import vec_env_oracle as E
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p
from tests.test_hip_vec_replay import raw
from tests.vec_env_checks import OUT, entry_on_poisoned_memory, lib_fixture, same_bits, same_state

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
STATE = ("phys", "t", "episode", "over")
lib = lib_fixture("drq_vec_catch_step", "the catch entries are missing")
_RUNS = {}


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN or O.PHYSICS: computed once, on first use, shared, never modified"""
    if cfg not in _RUNS:
        _RUNS[cfg] = O.driven_run(*cfg) if len(cfg) == 4 else O.physics_run(*cfg)
    return _RUNS[cfg]


def make(cfg, episode_length=L, width=O.WIDTH):
    from drqv2_amd.envs import VecCatch
    N, A, k, sparse = cfg[:4]
    return VecCatch(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, cup_width=width,
                    sparse=sparse)


def stagger(env, run):
    """the state the oracle's run starts from (its staggered t, the hand-set states of the physics runs) into an environment
    that has just been reset, through load_state_dict(), as a user of the class would write it"""
    sd = env.state_dict()
    for k in ("phys", "t"):
        sd[k] = torch.from_numpy(run["state0"][k])
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
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=lambda c: f"N{c[0]}-A{c[1]}-x{c[2]}-{'sparse' if c[3] else 'dense'}")
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


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: "sparse" if c[3] else "dense")
def test_long_episode_matches_the_oracle_through_every_contact_stop_and_clamp(cfg):
    """60 macro steps of 16 simulator steps in one episode of five hand-set environments: the tether taut and slack, both
    walls from inside and outside, the floor, the degenerate normal, all four stops, all three clamps, rest in the cup"""
    run = run_of(cfg)
    assert all(run["events"][name] >= 1 for name in O.EVENTS) and run["longest_rest"] >= 50
    env = make(cfg, episode_length=cfg[5])
    start(env, run)
    same_bits(env.render().cpu().numpy(), run["frame0"], "first frame")
    follow(env, run, 0, cfg[4])


def test_poses_render_as_the_oracle_draws_them():
    """every pose of O.POSES written through load_state_dict(), at its own cup_width (both ends of the range among them):
    the ball on the floor, against each wall, over the rim, the tether horizontal, vertical and of zero length, the cup in
    all four corners of its range with the ball at its farthest reach -- the end caps, the draw order and the roundings"""
    from drqv2_amd.envs import VecCatch
    for width in sorted({pose[1] for pose in O.POSES}):
        poses = [pose for pose in O.POSES if pose[1] == width]
        env = VecCatch(len(poses), "cuda", cup_width=width)
        sd = env.state_dict()
        sd["phys"] = torch.from_numpy(np.stack([pose[0] for pose in poses]))
        sd["reset"] = True
        env.load_state_dict(sd)
        want = np.stack([O.render(*pose) for pose in poses])
        same_bits(env.render().cpu().numpy(), want, ("poses of width", width))


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 2), (5, 4)])
@pytest.mark.parametrize("sparse", [True, False])
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, sparse):
    """drq_vec_catch_step at repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each; drq_vec_catch_render beside every one.  The outputs equal the
    oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one,
    so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    cfg = (N, A, 2, sparse)
    run = run_of(cfg)
    z = lambda shape, dt, name: dev(torch.zeros(shape, dtype=dt), name)
    state = {"phys": z((N, 8), torch.float32, "phys"), "t": z(N, torch.int32, "t"), "episode": z(N, torch.int32, "episode"),
             "over": z(N, torch.uint8, "over")}

    def render_beside(s, want):
        again = poison.alloc((N, 3, 84, 84), torch.uint8, "cuda", name="rendered")
        assert lib.drq_vec_catch_render(p(state["phys"]), N, O.WIDTH, p(again), None) == 0
        same_bits(again.cpu().numpy(), want[0], (s, "render"))

    entry_on_poisoned_memory(lambda action, reset_all, outs: lib.drq_vec_catch_step(
        *(p(state[n]) for n in STATE), N, A, action, SEED, L, 2, reset_all, O.WIDTH, int(sparse), *outs, None), run, N,
        state=state, compared=STATE, beside=render_beside,
        after_reset=lambda: state["t"].copy_(torch.from_numpy(run["state0"]["t"])))      # the stagger of the oracle's run


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_catch_oracle.refused_calls / refused_renders, all held to return the error without a
    GPU by tests/test_cpu_vec_catch.py) on real allocations full of the sentinel: the error, and check() finds every byte
    of the state, the action, the frame and the scalar outputs still poison"""
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    state, action, frame, scalars = al(0x400, "state"), al(0x100, "action"), al(5 * 3 * 84 * 84, "frame"), al(0x400, "scalars")
    calls = O.refused_calls(p(state), p(action), p(frame), p(scalars))
    for a in calls:
        assert lib.drq_vec_catch_step(*a, None) == -1, a
    renders = O.refused_renders(p(state), p(frame))
    for a in renders:
        assert lib.drq_vec_catch_render(*a, None) == -1, a
    assert len(calls) == 42 and len(renders) == 12
    poison.check()


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 4, repeat 2, dense: 9 steps, state_dict(); a fresh environment given the dict renders the saved frame and
    takes the next 5 steps to the bit.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel twice in
    both directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack a frame
    stacker would hold.  A dict of another width or reward form is refused, with the field named"""
    from drqv2_amd.replay import VecFrameReplay
    cfg = (5, 4, 2, False)
    run = run_of(cfg)
    N, A = cfg[:2]
    env = make(cfg)
    start(env, run)
    follow(env, run, 0, 9)
    want = run["out"][8][0]
    sd = env.state_dict()
    assert sd["kind"] == "VecCatch" and sd["config"]["sparse"] is False and sd["config"]["cup_width"] == O.WIDTH
    assert tuple(sd["phys"].shape) == (N, 8)
    fresh = make(cfg)
    fresh.load_state_dict(sd)
    same_bits(fresh.render().cpu().numpy(), want, "the frame of the restored state")
    same_state(fresh.state(), run["states"][8], "restored")
    same_bits(fresh.image(168, 4).cpu().numpy(), E.replicate(want, 168, 4), "image()")
    ring = VecFrameReplay(16, N, A, 3, 0.99, "cuda", seed=1)
    zeros, ones = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    ring.add(fresh.render(), torch.zeros(N, A, device="cuda"), zeros, ones, torch.ones(N, dtype=torch.uint8, device="cuda"))
    action = torch.from_numpy(run["actions"][9]).cuda()
    frame, reward, discount, first = fresh.step(action)
    ring.add(frame, torch.nan_to_num(action).clamp(-1, 1), reward, discount, first)
    newest, reset_row = run["out"][9][0], run["out"][9][3].astype(bool)[:, None, None, None]
    stack = np.concatenate([np.where(reset_row, newest, want)] * 2 + [newest], axis=1)      # a reset row fills the stack
    same_bits(ring.observation().cpu().numpy(), stack, "observation()")
    same_state(fresh.state(), run["states"][9], "after the step")
    follow(fresh, run, 10, 14)
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        make((N, A, 2, True)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bcup_width: saved 0.3, here 0.18"):
        make(cfg, width=O.HARD_WIDTH).load_state_dict(sd)


def test_checkpoint_round_trip_with_the_ball_in_flight_continues_bit_for_bit(tmp_path):
    """the sparse physics run (one episode, repeat 16): 3 macro steps, checkpoint.save() with the ball that the cup of
    environment 0 has flung upwards in flight -- the tether slack, no contact, both velocity components non-zero -- then
    8 more steps, through the moment the tether catches it again; a fresh environment loaded from the file takes the same 8 steps to the bit, outputs and state; the file carries
    cup_width and sparse, and an environment of another width refuses it"""
    from drqv2_amd import checkpoint
    cfg = O.PHYSICS[0]
    run = run_of(cfg)
    env = make(cfg, episode_length=cfg[5])
    start(env, run)
    follow(env, run, 0, 3)
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=env, extra={"step": 3})
    saved = env.state()
    hw = O.half_width(O.WIDTH)
    flying = [e for e in range(cfg[0]) if all(v == 0 for k, v in O.substep(tuple(saved["phys"][e]), np.float32(0), np.float32(0),
              hw)[1].items() if k != "slack") and saved["phys"][e, 6] != 0 and saved["phys"][e, 7] != 0]
    assert flying and 0 < int(saved["t"].max()) < cfg[5], "the save must fall inside an episode, with a ball in flight"
    config = torch.load(path, weights_only=True)["env"]["config"]
    assert config["cup_width"] == O.WIDTH and config["sparse"] is True
    with pytest.raises(ValueError, match="cup_width"):
        checkpoint.load(path, env=make(cfg, episode_length=cfg[5], width=O.HARD_WIDTH))
    fresh = make(cfg, episode_length=cfg[5])
    assert checkpoint.load(path, env=fresh) == {"step": 3}
    same_state(fresh.state(), run["states"][2], "restored")
    assert raw(fresh.render()).tobytes() == run["out"][2][0].tobytes()
    follow(fresh, run, 3, 11)
    follow(env, run, 3, 11)
    same_state(fresh.state(), env.state(), "after 8 steps")


def test_distractions_and_the_exploration_bonus_take_the_class():
    """N = 3: reset() and one step of VecDistract(env, distractor) against the distraction oracle applied to the catch
    oracle's frames -- no shape pixel is the background key -- and SimHashBonus of the plain frames and the sparse reward
    against its own oracle"""
    from drqv2_amd.distract import FrameDistractor, VecDistract
    from drqv2_amd.explore import SimHashBonus
    from tests import simhash_oracle as S
    from tests import vec_distract_oracle as D
    cfg = (3, 2, 2, True)
    run = run_of(cfg)
    N = cfg[0]
    kw = dict(seed=5, camera=8, camera_period=1, color=48)
    wrapped = VecDistract(make(cfg), FrameDistractor(N, "cuda", background="noise", background_alpha=200, key="env", **kw))
    o = D.DistractOracle(N, bg_mode=1, bg_alpha=200, key=D.ramp(), **kw)
    same_bits(wrapped.reset().cpu().numpy(), o.apply(run["frame0"], reset_all=True), "reset")
    stagger(wrapped.env, run)
    frame, reward, discount, first = wrapped.step(torch.from_numpy(run["actions"][0]).cuda())
    want = run["out"][0]
    same_bits(frame.cpu().numpy(), o.apply(want[0], want[3]), "the distracted frame")
    for got, w, what in ((reward, want[1], "reward"), (discount, want[2], "discount"), (first, want[3], "first"),
                         (wrapped.last_substeps, want[4], "substeps")):
        same_bits(got.cpu().numpy(), w, what)
    o.require_branches("background", "foreground")
    bonus, so = SimHashBonus(N, "cuda", bits=16, beta=0.5, seed=4), S.SimHashOracle(16, 0.5, 4)
    plain = make(cfg)
    start(plain, run)
    for s in range(2):
        frame, reward = plain.step(torch.from_numpy(run["actions"][s]).cuda())[:2]
        ret = bonus.step(frame, reward)
        code, count, extra, total = so.step(run["out"][s][0], run["out"][s][1])[:4]
        for got, w, what in ((bonus.codes, code, "codes"), (bonus.counts, count, "counts"), (bonus.last_bonus, extra, "bonus"),
                             (ret, total, "reward + bonus")):
            same_bits(got.cpu().numpy(), w, (s, what))


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks; a sparse return is a whole number of at most 7"""
    import drqv2
    from drqv2_amd.evaluate import VecVideo, evaluate
    cfg = (3, 2, 2, True)
    torch.manual_seed(3)
    agent = drqv2.DrQV2Agent((9, 84, 84), (2,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    video = VecVideo(3, "cuda", max_frames=64)
    res = evaluate(agent, make(cfg), 1, poll_every=4, video=video)
    snap = res.snapshot
    assert snap.complete and snap.episodes == 3 and sorted(snap.records["env"].tolist()) == [0, 1, 2]
    assert (snap.records["length"] == -(-L // 2)).all() and len(video) >= 5
    assert (snap.records["return"] == np.round(snap.records["return"])).all() and 0 <= snap.min_return <= snap.max_return <= L
