"""The finger of the device environment on the GPU: drq_vec_finger_step / _render raw on poisoned memory, and
drqv2_amd.envs.VecFinger against the numpy restatement (tests/vec_finger_oracle.py), through render(), image(), state dicts,
a checkpoint file, VecDistract, SimHashBonus and the frame ring.

Bounds.  Everything is compared bit for bit.  A sub-step is single correctly rounded float32 operations (+, -, *, /, sqrt)
in a fixed order -- the file is built with -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -- and the frame is
integer arithmetic after nine floorf; the oracle performs the same operations in numpy float32 and Python integers.

Shapes.  N = 3, A = 2 and N = 5, A = 4 (odd, more than one workgroup, the action's row stride differs from the two
columns read), repeat 1, 2 and 16, both modes, sparse and dense, episode_length 7 and 40 macro steps
(vec_finger_oracle.DRIVEN): the time limit falls inside a repeat for 2 and 16, and t of environment e starts at e mod 7, so
the resets stagger.  Seven steps from rest meet no contact: one long episode per mode at repeat 16
(vec_finger_oracle.PHYSICS, 960 simulator steps of five hand-set environments) meets contacts on the rod's side, its cap
and its hinge end, the degenerate normal, a skipped separation, all three speed clamps, a rod left alone and every regime
of both rewards.  The poses (vec_finger_oracle.POSES) are where the pixel rule can go wrong.  The oracle's runs are made
once, shared and never modified; what they cover is asserted without a GPU by tests/test_cpu_vec_finger.py."""
import types

import numpy as np
import pytest
import torch

from tests import vec_env_checks as C
from tests import vec_finger_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.vec_env_checks import run_of, same_bits

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
MODES = ("spin", "turn")
lib = C.lib_fixture("drq_vec_finger_step", "the finger entries are missing")


def make(cfg, episode_length=L, **other):
    from drqv2_amd.envs import VecFinger
    N, A, k, mode, radius, sparse = cfg[:6]
    kw = dict(task=MODES[mode], target_radius=radius, sparse=sparse)
    kw.update(other)
    return VecFinger(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, **kw)


T = types.SimpleNamespace(
    O=O, kind="VecFinger", make=make, words=(("phys", (9,), torch.float32), ("target", (2,), torch.float32)),
    staggered=("phys", "target", "t"), also=None,
    step=lambda lib, cfg, state, action, reset_all, outs: lib.drq_vec_finger_step(
        *state.values(), cfg[0], cfg[1], action, SEED, L, cfg[2], reset_all, cfg[3], cfg[4], int(cfg[5]), *outs, None),
    render=lambda lib, cfg, state, frame: lib.drq_vec_finger_render(state["phys"], state["target"], cfg[0], cfg[3], cfg[4],
                                                                    frame, None))


def name(c):
    return f"N{c[0]}-A{c[1]}-x{c[2]}-{MODES[c[3]]}-{'sparse' if c[5] else 'dense'}"


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=name)
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn"""
    C.env_matches_the_oracle(T, cfg)


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: MODES[c[3]])
def test_long_episode_matches_the_oracle_through_every_contact_and_clamp(cfg):
    """60 macro steps of 16 simulator steps in one episode of five hand-set environments: contacts on the rod's side, cap
    and hinge end, the degenerate normal, a separation without a lever, the three speed clamps, a rod at rest that keeps
    its bits, and every regime of the mode's reward"""
    run = run_of(O, cfg)
    other = "turn_" if cfg[3] == 0 else "spin_"
    assert all(run["events"][name] >= 1 for name in O.EVENTS if not name.startswith(other)), run["events"]
    env = make(cfg, episode_length=cfg[7])
    C.start(T, env, run)
    same_bits(env.render().cpu().numpy(), run["frame0"], "first frame")
    C.follow(T, env, run, 0, cfg[6])


def test_poses_render_as_the_oracle_draws_them():
    """every pose of O.POSES written through load_state_dict(), in its own mode and at its own target_radius: links exactly
    horizontal and vertical, the fingertip over the hinge and over the rod's tip, the rod along each axis, the smallest and
    the largest target, segments of length zero -- the end caps, the draw order and the roundings"""
    from drqv2_amd.envs import VecFinger
    for mode, radius in sorted({pose[2:] for pose in O.POSES}):
        poses = [pose for pose in O.POSES if pose[2:] == (mode, radius)]
        env = VecFinger(len(poses), "cuda", task=MODES[mode], target_radius=radius)
        sd = env.state_dict()
        sd["phys"], sd["target"] = (torch.from_numpy(np.stack([pose[k] for pose in poses])) for k in (0, 1))
        sd["reset"] = True
        env.load_state_dict(sd)
        same_bits(env.render().cpu().numpy(), np.stack([O.render(pose) for pose in poses]), ("poses of", mode, radius))


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 2), (5, 4)])
@pytest.mark.parametrize("mode", [0, 1], ids=MODES)
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, mode):
    """drq_vec_finger_step at repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each; drq_vec_finger_render beside every one.  The outputs equal the
    oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one,
    so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    C.step_entry_on_poisoned_memory(T, lib, (N, A, 2, mode, O.TURN_EASY_RADIUS, True))


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_finger_oracle.refused_calls / refused_renders, all held to return the error without a
    GPU by tests/test_cpu_vec_finger.py) on real allocations full of the sentinel: the error, and check() finds every byte
    of the state, the action, the frame and the scalar outputs still poison"""
    C.refused_on_poisoned_memory(0x500, lambda S0, ACT, FR, SC: ((lib.drq_vec_finger_step, O.refused_calls(S0, ACT, FR, SC), 46),
                                                                  (lib.drq_vec_finger_render, O.refused_renders(S0, FR), 15)))


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 4, repeat 2, turn, dense: 9 steps, state_dict(); a fresh environment given the dict renders the saved
    frame and takes the next 5 steps to the bit.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel
    twice in both directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack
    a frame stacker would hold.  A dict of another mode, radius or reward form is refused, with the field named"""
    cfg = (5, 4, 2, 1, O.TURN_EASY_RADIUS, False)
    sd = C.state_dict_image_and_ring(T, cfg)
    assert sd["config"]["mode"] == "turn" and sd["config"]["sparse"] is False and sd["config"]["target_radius"] == O.TURN_EASY_RADIUS
    with pytest.raises(ValueError, match=r"\bmode: saved 'turn', here 'spin'"):
        make(cfg, task="spin").load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        make(cfg, sparse=True).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\btarget_radius: saved 0.1, here 0.04"):
        make(cfg, target_radius=O.TURN_HARD_RADIUS).load_state_dict(sd)


def test_checkpoint_round_trip_in_contact_continues_bit_for_bit(tmp_path):
    """the physics run of spin (one episode, repeat 16): O.CUT macro steps, checkpoint.save() while the fingertip of
    environment 0 touches the rod and all three of its velocities are non-zero, then 8 more steps; a fresh environment
    loaded from the file takes the same 8 steps to the bit, outputs and state; the file carries mode, target_radius and
    sparse, and an environment of another mode refuses it"""
    from drqv2_amd import checkpoint
    cfg = O.PHYSICS[0]

    def between(path, saved):
        gap = O.gap_many(saved["phys"][:1])[0][0]
        assert gap <= float(O.TOUCH) + 1e-4 and (saved["phys"][0, [2, 5, 8]] != 0).all(), "the save must fall in contact, in motion"
        assert 0 < int(saved["t"].max()) < cfg[7]
        config = torch.load(path, weights_only=True)["env"]["config"]
        assert (config["mode"], config["target_radius"], config["sparse"]) == ("spin", O.PHYSICS_RADIUS, True)
        with pytest.raises(ValueError, match="mode"):
            checkpoint.load(path, env=make(cfg, episode_length=cfg[7], task="turn"))

    C.checkpoint_round_trip(T, cfg, tmp_path, O.CUT, 8, between, episode_length=cfg[7])


def test_distractions_and_the_exploration_bonus_take_the_class():
    """N = 3: reset() and one step of VecDistract(env, distractor) against the distraction oracle applied to the finger
    oracle's frames -- no shape pixel is the background key -- and SimHashBonus of the plain frames and the sparse reward
    against its own oracle"""
    C.distractions_and_the_exploration_bonus(T, (3, 2, 2, 1, O.TURN_EASY_RADIUS, True))


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks; a step pays at most 1, so a return is in 0 .. 7"""
    snap = C.evaluate_and_video(T, (3, 2, 2, 0, O.TURN_EASY_RADIUS, True))
    assert 0 <= snap.min_return <= snap.max_return <= L
