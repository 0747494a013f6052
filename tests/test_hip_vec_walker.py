"""The walker of the device environment on the GPU: drq_vec_walker_step / _render raw on poisoned memory, and
drqv2_amd.envs.VecWalker against the numpy restatement (tests/vec_walker_oracle.py), through render(), image(), state dicts,
a checkpoint file, VecDistract, SimHashBonus and the frame ring.

Bounds.  Everything is compared bit for bit.  A sub-step is single correctly rounded float32 operations (+, -, *, /, sqrt)
in a fixed order -- the file is built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -- and the frame is
integer arithmetic after thirteen floorf; the oracle performs the same operations on numpy float32 scalars and Python
integers.

Shapes.  N = 3, A = 4 and N = 5, A = 6 (odd, more than one workgroup, the action's row stride differs from the four
columns read), repeat 1, 2 and 16, speed 0 and the walk speed, episode_length 7 and 40 macro steps
(vec_walker_oracle.DRIVEN): the time limit falls inside a repeat for 2 and 16, and t of environment e starts at e mod 7, so
the resets stagger.  Seven steps from a standing pose meet the ground under the feet and the force clamp and little else:
two long episodes at repeat 16 (vec_walker_oracle.PHYSICS, 960 simulator steps of five hand-set environments each) meet
every particle on the ground, every muscle at either limit, both clamps, the degenerate normal, the wrap both ways, a
fallen body and every regime of the reward.  The poses (vec_walker_oracle.POSES) are where the pixel rule can go wrong.
The oracle's runs are made once, shared and never modified; what they cover is asserted without a GPU by
tests/test_cpu_vec_walker.py."""
import types

import numpy as np
import pytest
import torch

from tests import vec_env_checks as C
from tests import vec_walker_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.vec_env_checks import run_of, same_bits

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
lib = C.lib_fixture("drq_vec_walker_step", "the walker entries are missing")


def make(cfg, episode_length=L, speed=None):
    from drqv2_amd.envs import VecWalker
    N, A, k = cfg[:3]
    return VecWalker(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k,
                     speed=cfg[3] if speed is None else speed)


T = types.SimpleNamespace(
    O=O, kind="VecWalker", make=make, words=(("phys", (24,), torch.float32),), staggered=("phys", "t"), also=None,
    step=lambda lib, cfg, state, action, reset_all, outs: lib.drq_vec_walker_step(
        *state.values(), cfg[0], cfg[1], action, SEED, L, cfg[2], reset_all, cfg[3], *outs, None),
    render=lambda lib, cfg, state, frame: lib.drq_vec_walker_render(state["phys"], cfg[0], frame, None))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=lambda c: f"N{c[0]}-A{c[1]}-x{c[2]}-{'walk' if c[3] else 'stand'}")
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn"""
    C.env_matches_the_oracle(T, cfg)


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: "walk" if c[3] else "stand")
def test_long_episode_matches_the_oracle_through_every_contact_limit_clamp_and_wrap(cfg):
    """60 macro steps of 16 simulator steps in one episode of five hand-set environments: every particle on the ground,
    every muscle at its lower and its upper limit, the force clamp, the speed clamp, the degenerate normal, the wrap in
    both directions, a fallen body, stand strictly inside (0, 1) and, at the walk speed, move at 0, inside and at 1"""
    run = run_of(O, cfg)
    assert all(run["events"][name] >= 1 for name in O.EVENTS if cfg[3] > 0 or not name.startswith("move_"))
    env = make(cfg, episode_length=cfg[5])
    C.start(T, env, run)
    same_bits(env.render().cpu().numpy(), run["frame0"], "first frame")
    C.follow(T, env, run, 0, cfg[4])


def test_poses_render_as_the_oracle_draws_them():
    """every pose of O.POSES written through load_state_dict(): upright, lying flat, the torso exactly horizontal with
    exactly vertical thighs and a knee and a foot at one point, a body at either side of the wrap's seam, a negative camera
    offset and offsets of exactly one stripe period either way (the floor and the modulo of negative integers), particles
    exactly at y = 0, a foot above the torso -- the end caps, the draw order and the roundings"""
    from drqv2_amd.envs import VecWalker
    env = VecWalker(len(O.POSES), "cuda")
    sd = env.state_dict()
    sd["phys"] = torch.from_numpy(np.stack(O.POSES))
    sd["reset"] = True
    env.load_state_dict(sd)
    same_bits(env.render().cpu().numpy(), np.stack([O.render(pose) for pose in O.POSES]), "poses")


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 4), (5, 6)])
@pytest.mark.parametrize("speed", [0.0, O.WALK_SPEED], ids=["stand", "walk"])
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, speed):
    """drq_vec_walker_step at repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each; drq_vec_walker_render beside every one.  The outputs equal the
    oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one,
    so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    C.step_entry_on_poisoned_memory(T, lib, (N, A, 2, speed))


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_walker_oracle.refused_calls / refused_renders, all held to return the error without a
    GPU by tests/test_cpu_vec_walker.py) on real allocations full of the sentinel: the error, and check() finds every byte
    of the state, the action, the frame and the scalar outputs still poison"""
    C.refused_on_poisoned_memory(0x400, lambda S0, ACT, FR, SC: ((lib.drq_vec_walker_step, O.refused_calls(S0, ACT, FR, SC), 41),
                                                                  (lib.drq_vec_walker_render, O.refused_renders(S0, FR), 8)))


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 6, repeat 2, the walk speed: 9 steps, state_dict(); a fresh environment given the dict renders the saved
    frame and takes the next 5 steps to the bit.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel
    twice in both directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack
    a frame stacker would hold.  A dict of another speed is refused, with the field named"""
    cfg = (5, 6, 2, O.WALK_SPEED)
    sd = C.state_dict_image_and_ring(T, cfg)
    assert sd["config"]["speed"] == O.WALK_SPEED
    with pytest.raises(ValueError, match=r"\bspeed: saved 0.3, here 0.6"):
        make(cfg, speed=O.RUN_SPEED).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bspeed: saved 0.3, here 0.0"):
        make(cfg, speed=0.0).load_state_dict(sd)


CUT = 5      # macro steps of the physics run before the save


def test_checkpoint_round_trip_mid_stride_continues_bit_for_bit(tmp_path):
    """the physics run at the walk speed (one episode, repeat 16): 5 macro steps, checkpoint.save() with the body that
    gait() drives mid-stride -- one foot on the ground, the other off it, every particle moving -- then 8 more steps; a
    fresh environment loaded from the file takes the same 8 steps to the bit, outputs and state; the file carries speed,
    and an environment of another speed refuses it"""
    from drqv2_amd import checkpoint
    cfg = O.PHYSICS[1]

    def between(path, saved):
        feet, v = saved["phys"][0, [13, 21]], saved["phys"][0].reshape(6, 4)[:, 2:]
        assert (feet == 0).sum() == 1 and (feet > 0).sum() == 1 and (v != 0).all(), "the save must fall mid-stride"
        assert 0 < int(saved["t"].max()) < cfg[5]
        assert torch.load(path, weights_only=True)["env"]["config"]["speed"] == O.WALK_SPEED
        with pytest.raises(ValueError, match="speed"):
            checkpoint.load(path, env=make(cfg, episode_length=cfg[5], speed=O.RUN_SPEED))

    C.checkpoint_round_trip(T, cfg, tmp_path, CUT, 8, between, episode_length=cfg[5])


def test_distractions_and_the_exploration_bonus_take_the_class():
    """N = 3: reset() and one step of VecDistract(env, distractor) against the distraction oracle applied to the walker
    oracle's frames -- no shape pixel, the ground's stripes among them, is the background key -- and SimHashBonus of the
    plain frames and the reward against its own oracle"""
    C.distractions_and_the_exploration_bonus(T, (3, 4, 2, O.WALK_SPEED))


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks; a step pays at most 1, so a return is in 0 .. 7"""
    snap = C.evaluate_and_video(T, (3, 4, 2, O.WALK_SPEED))
    assert 0 <= snap.min_return <= snap.max_return <= L
