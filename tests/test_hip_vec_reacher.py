"""The reacher of the device environment on the GPU: drq_vec_reacher_step / _render raw on poisoned memory, and
drqv2_amd.envs.VecReacher against the numpy restatement (tests/vec_reacher_oracle.py), through render(), image(), state
dicts, a checkpoint file, VecDistract, SimHashBonus and the frame ring.

Bounds.  Everything is compared bit for bit.  A sub-step is single correctly rounded float32 operations (+, -, *, /, sqrt)
in a fixed order -- the file is built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -- and the frame is
integer arithmetic after seven floorf; the oracle performs the same operations on numpy float32 scalars and Python
integers.

Shapes.  N = 3, A = 2 and N = 5, A = 4 (odd, more than one workgroup, the action's row stride differs from the two
columns read), repeat 1, 2 and 16, sparse and dense, episode_length 7 and 40 macro steps (vec_reacher_oracle.DRIVEN): the
time limit falls inside a repeat for 2 and 16, and t of environment e starts at e mod 7, so the resets stagger.  In seven
steps no joint leaves its quadrant: two long episodes at repeat 16 (vec_reacher_oracle.PHYSICS, 960 simulator steps each)
turn both joints through all four and run into the clamp of w.  The poses (vec_reacher_oracle.POSES) are where the pixel
rule can go wrong.  The oracle's runs are made once, shared and never modified; what they cover is asserted without a GPU
by tests/test_cpu_vec_reacher.py."""
import types

import numpy as np
import pytest
import torch

from tests import vec_env_checks as C
from tests import vec_reacher_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.vec_env_checks import run_of, same_bits

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
lib = C.lib_fixture("drq_vec_reacher_step", "the reacher entries are missing")


def make(cfg, episode_length=L, radius=O.DRIVEN_RADIUS):
    from drqv2_amd.envs import VecReacher
    N, A, k, sparse = cfg[:4]
    return VecReacher(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k,
                      target_radius=radius, sparse=sparse)


T = types.SimpleNamespace(
    O=O, kind="VecReacher", make=make, words=(("phys", (6,), torch.float32), ("target", (2,), torch.float32)),
    staggered=("phys", "target", "t"), also=None,
    step=lambda lib, cfg, state, action, reset_all, outs: lib.drq_vec_reacher_step(
        *state.values(), cfg[0], cfg[1], action, SEED, L, cfg[2], reset_all, O.DRIVEN_RADIUS, int(cfg[3]), *outs, None),
    render=lambda lib, cfg, state, frame: lib.drq_vec_reacher_render(state["phys"], state["target"], cfg[0], O.DRIVEN_RADIUS,
                                                                     frame, None))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=lambda c: f"N{c[0]}-A{c[1]}-x{c[2]}-{'sparse' if c[3] else 'dense'}")
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn"""
    C.env_matches_the_oracle(T, cfg)


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: "sparse" if c[3] else "dense")
def test_long_episode_matches_the_oracle_through_all_quadrants_and_the_clamp(cfg):
    """60 macro steps of 16 simulator steps in one episode: two arms driven round, two thrown into the clamp of w"""
    run = run_of(O, cfg)
    assert run["quadrants"][0] == run["quadrants"][1] == {0, 1, 2, 3} and run["clamped"] >= 1
    env = make(cfg, episode_length=cfg[5], radius=O.PHYSICS_RADIUS)
    C.start(T, env, run)
    same_bits(env.render().cpu().numpy(), run["frame0"], "first frame")
    C.follow(T, env, run, 0, cfg[4])


def test_poses_render_as_the_oracle_draws_them():
    """every pose of O.POSES written through load_state_dict(), at its own target_radius: the arm along each axis,
    folded, stretched, the fingertip over the target, the target under the upper arm -- the capsules' end caps, the draw
    order and the roundings"""
    from drqv2_amd.envs import VecReacher
    for radius in sorted({pose[2] for pose in O.POSES}):
        poses = [pose for pose in O.POSES if pose[2] == radius]
        env = VecReacher(len(poses), "cuda", target_radius=radius)
        sd = env.state_dict()
        sd["phys"], sd["target"] = (torch.from_numpy(np.stack([pose[k] for pose in poses])) for k in (0, 1))
        sd["reset"] = True
        env.load_state_dict(sd)
        want = np.stack([O.render(*pose) for pose in poses])
        same_bits(env.render().cpu().numpy(), want, ("poses of radius", radius))


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 2), (5, 4)])
@pytest.mark.parametrize("sparse", [True, False])
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, sparse):
    """drq_vec_reacher_step at repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each; drq_vec_reacher_render beside every one.  The outputs equal the
    oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one,
    so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    C.step_entry_on_poisoned_memory(T, lib, (N, A, 2, sparse))


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_reacher_oracle.refused_calls / refused_renders, all held to return the error without
    a GPU by tests/test_cpu_vec_reacher.py) on real allocations full of the sentinel: the error, and check() finds every
    byte of the state, the action, the frame and the scalar outputs still poison"""
    C.refused_on_poisoned_memory(0x500, lambda S0, ACT, FR, SC: ((lib.drq_vec_reacher_step, O.refused_calls(S0, ACT, FR, SC), 44),
                                                                  (lib.drq_vec_reacher_render, O.refused_renders(S0, FR), 13)))


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 4, repeat 2, dense: 9 steps, state_dict(); a fresh environment given the dict renders the saved frame and
    takes the next 5 steps to the bit.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel twice in
    both directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack a frame
    stacker would hold.  A dict of another radius or reward form is refused, with the field named"""
    cfg = (5, 4, 2, False)
    sd = C.state_dict_image_and_ring(T, cfg)
    assert sd["config"]["sparse"] is False and sd["config"]["target_radius"] == O.DRIVEN_RADIUS
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        make((5, 4, 2, True)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\btarget_radius: saved 0.3, here 0.15"):
        make(cfg, radius=0.15).load_state_dict(sd)


def test_checkpoint_round_trip_continues_bit_for_bit(tmp_path):
    """N = 3, repeat 2, sparse: 6 steps, checkpoint.save() inside an episode and in motion, 10 more steps; a fresh
    environment loaded from the file takes the same 10 steps to the bit, outputs and state; the file carries
    target_radius and sparse, and an environment of another radius refuses it"""
    from drqv2_amd import checkpoint
    cfg = (3, 2, 2, True)

    def between(path, saved):
        assert np.abs(saved["phys"][:, 2]).max() > 0 and 0 < int(saved["t"].max()) < L, "the save must fall inside an episode, in motion"
        config = torch.load(path, weights_only=True)["env"]["config"]
        assert config["target_radius"] == O.DRIVEN_RADIUS and config["sparse"] is True
        with pytest.raises(ValueError, match="target_radius"):
            checkpoint.load(path, env=make(cfg, radius=0.05))

    C.checkpoint_round_trip(T, cfg, tmp_path, 6, 10, between)


def test_distractions_and_the_exploration_bonus_take_the_class():
    """N = 3: reset() and one step of VecDistract(env, distractor) against the distraction oracle applied to the reacher
    oracle's frames -- no shape pixel is the background key -- and SimHashBonus of the plain frames and the sparse reward
    against its own oracle"""
    C.distractions_and_the_exploration_bonus(T, (3, 2, 2, True))


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks; a sparse return is a whole number of at most 7"""
    snap = C.evaluate_and_video(T, (3, 2, 2, True))
    assert (snap.records["return"] == np.round(snap.records["return"])).all() and 0 <= snap.min_return <= snap.max_return <= L
