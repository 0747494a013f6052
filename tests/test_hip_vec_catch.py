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
import types

import numpy as np
import pytest
import torch

from tests import vec_catch_oracle as O
from tests import vec_env_checks as C
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.vec_env_checks import run_of, same_bits

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
lib = C.lib_fixture("drq_vec_catch_step", "the catch entries are missing")


def make(cfg, episode_length=L, width=O.WIDTH):
    from drqv2_amd.envs import VecCatch
    N, A, k, sparse = cfg[:4]
    return VecCatch(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, cup_width=width,
                    sparse=sparse)


T = types.SimpleNamespace(
    O=O, kind="VecCatch", make=make, words=(("phys", (8,), torch.float32),), staggered=("phys", "t"), also=None,
    step=lambda lib, cfg, state, action, reset_all, outs: lib.drq_vec_catch_step(
        *state.values(), cfg[0], cfg[1], action, SEED, L, cfg[2], reset_all, O.WIDTH, int(cfg[3]), *outs, None),
    render=lambda lib, cfg, state, frame: lib.drq_vec_catch_render(state["phys"], cfg[0], O.WIDTH, frame, None))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=lambda c: f"N{c[0]}-A{c[1]}-x{c[2]}-{'sparse' if c[3] else 'dense'}")
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn"""
    C.env_matches_the_oracle(T, cfg)


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: "sparse" if c[3] else "dense")
def test_long_episode_matches_the_oracle_through_every_contact_stop_and_clamp(cfg):
    """60 macro steps of 16 simulator steps in one episode of five hand-set environments: the tether taut and slack, both
    walls from inside and outside, the floor, the degenerate normal, all four stops, all three clamps, rest in the cup"""
    run = run_of(O, cfg)
    assert all(run["events"][name] >= 1 for name in O.EVENTS) and run["longest_rest"] >= 50
    env = make(cfg, episode_length=cfg[5])
    C.start(T, env, run)
    same_bits(env.render().cpu().numpy(), run["frame0"], "first frame")
    C.follow(T, env, run, 0, cfg[4])


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
    C.step_entry_on_poisoned_memory(T, lib, (N, A, 2, sparse))


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_catch_oracle.refused_calls / refused_renders, all held to return the error without a
    GPU by tests/test_cpu_vec_catch.py) on real allocations full of the sentinel: the error, and check() finds every byte
    of the state, the action, the frame and the scalar outputs still poison"""
    C.refused_on_poisoned_memory(0x400, lambda S0, ACT, FR, SC: ((lib.drq_vec_catch_step, O.refused_calls(S0, ACT, FR, SC), 42),
                                                                  (lib.drq_vec_catch_render, O.refused_renders(S0, FR), 12)))


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 4, repeat 2, dense: 9 steps, state_dict(); a fresh environment given the dict renders the saved frame and
    takes the next 5 steps to the bit.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel twice in
    both directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack a frame
    stacker would hold.  A dict of another width or reward form is refused, with the field named"""
    cfg = (5, 4, 2, False)
    sd = C.state_dict_image_and_ring(T, cfg)
    assert sd["config"]["sparse"] is False and sd["config"]["cup_width"] == O.WIDTH
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        make((5, 4, 2, True)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bcup_width: saved 0.3, here 0.18"):
        make(cfg, width=O.HARD_WIDTH).load_state_dict(sd)


def test_checkpoint_round_trip_with_the_ball_in_flight_continues_bit_for_bit(tmp_path):
    """the sparse physics run (one episode, repeat 16): 3 macro steps, checkpoint.save() with the ball that the cup of
    environment 0 has flung upwards in flight -- the tether slack, no contact, both velocity components non-zero -- then
    8 more steps, through the moment the tether catches it again; a fresh environment loaded from the file takes the same 8 steps to the bit, outputs and state; the file carries
    cup_width and sparse, and an environment of another width refuses it"""
    from drqv2_amd import checkpoint
    cfg = O.PHYSICS[0]

    def between(path, saved):
        hw = O.half_width(O.WIDTH)
        flying = [e for e in range(cfg[0]) if all(v == 0 for k, v in O.substep(tuple(saved["phys"][e]), np.float32(0), np.float32(0),
                  hw)[1].items() if k != "slack") and saved["phys"][e, 6] != 0 and saved["phys"][e, 7] != 0]
        assert flying and 0 < int(saved["t"].max()) < cfg[5], "the save must fall inside an episode, with a ball in flight"
        config = torch.load(path, weights_only=True)["env"]["config"]
        assert config["cup_width"] == O.WIDTH and config["sparse"] is True
        with pytest.raises(ValueError, match="cup_width"):
            checkpoint.load(path, env=make(cfg, episode_length=cfg[5], width=O.HARD_WIDTH))

    C.checkpoint_round_trip(T, cfg, tmp_path, 3, 8, between, episode_length=cfg[5])


def test_distractions_and_the_exploration_bonus_take_the_class():
    """N = 3: reset() and one step of VecDistract(env, distractor) against the distraction oracle applied to the catch
    oracle's frames -- no shape pixel is the background key -- and SimHashBonus of the plain frames and the sparse reward
    against its own oracle"""
    C.distractions_and_the_exploration_bonus(T, (3, 2, 2, True))


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks; a sparse return is a whole number of at most 7"""
    snap = C.evaluate_and_video(T, (3, 2, 2, True))
    assert (snap.records["return"] == np.round(snap.records["return"])).all() and 0 <= snap.min_return <= snap.max_return <= L
