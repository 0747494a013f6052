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
import types

import numpy as np
import pytest
import torch

from tests import vec_cartpole_oracle as O
from tests import vec_env_checks as C
from tests import vec_env_oracle as E
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.vec_env_checks import run_of, same_bits, same_state

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
lib = C.lib_fixture("drq_vec_cartpole_step", "the cartpole entries are missing")


def make(cfg, episode_length=L):
    from drqv2_amd.envs import VecCartpole
    N, A, k, swing = cfg[:4]
    return VecCartpole(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, swing_up=swing)


T = types.SimpleNamespace(
    O=O, kind="VecCartpole", make=make, words=(("phys", (5,), torch.float32),), staggered=("t",), also=None,
    step=lambda lib, cfg, state, action, reset_all, outs: lib.drq_vec_cartpole_step(
        *state.values(), cfg[0], cfg[1], action, SEED, L, cfg[2], reset_all, int(cfg[3]), *outs, None),
    render=lambda lib, cfg, state, frame: lib.drq_vec_cartpole_render(state["phys"], cfg[0], frame, None))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN, ids=lambda c: f"N{c[0]}-A{c[1]}-x{c[2]}-{'swingup' if c[3] else 'balance'}")
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn"""
    C.env_matches_the_oracle(T, cfg)


@pytest.mark.parametrize("cfg", O.PHYSICS, ids=lambda c: "swingup" if c[3] else "balance")
def test_long_episode_matches_the_oracle_through_rail_ends_and_the_vertical(cfg):
    """60 macro steps of 16 simulator steps in one episode: the carts hit both rail ends and stay there, the poles swing
    through hanging and over the top"""
    run = run_of(O, cfg)
    assert run["hit_left"] and run["hit_right"] and run["through_hanging"] and run["through_upright"]
    env = make(cfg, episode_length=cfg[5])
    same_bits(env.reset().cpu().numpy(), run["frame0"], "first frame")
    C.follow(T, env, run, 0, cfg[4])


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 1), (5, 3)])
@pytest.mark.parametrize("swing", [True, False])
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, swing):
    """drq_vec_cartpole_step at repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL action,
    then 12 steps into fresh poisoned outputs each; drq_vec_cartpole_render beside every one.  The outputs equal the
    oracle's, which never holds the byte sentinel 0xA5 (a frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one,
    so every byte was written; check() finds the guard bands of outputs, state and action untouched"""
    C.step_entry_on_poisoned_memory(T, lib, (N, A, 2, swing))


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_cartpole_oracle.refused_calls / refused_renders, all held to return the error without
    a GPU by tests/test_cpu_vec_cartpole.py) on real allocations full of the sentinel: the error, and check() finds every
    byte of the state, the action, the frame and the scalar outputs still poison"""
    C.refused_on_poisoned_memory(0x400, lambda S0, ACT, FR, SC: ((lib.drq_vec_cartpole_step, O.refused_calls(S0, ACT, FR, SC), 35),
                                                                  (lib.drq_vec_cartpole_render, O.refused_renders(S0, FR), 8)))


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_render_after_load_state_dict_and_image_into_the_ring():
    """N = 5, A = 3, repeat 2, balance: 9 steps, state_dict(); a fresh environment given the dict renders the saved frame.
    image() of it at 168 x 168 x 4 is the frame with every pixel twice in both directions, and
    VecFrameReplay.add_render() of that image stores exactly the frame"""
    from drqv2_amd.replay import VecFrameReplay
    cfg = (5, 3, 2, False)
    run = run_of(O, cfg)
    N, A = cfg[:2]
    env = make(cfg)
    C.start(T, env, run)
    C.follow(T, env, run, 0, 9)
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
    def between(path, saved):
        assert np.abs(saved["phys"][:, 4]).max() > 0 and 0 < int(saved["t"].max()) < L, "the save must fall inside an episode, in motion"

    C.checkpoint_round_trip(T, (3, 1, 2, True), tmp_path, 6, 10, between)


def test_evaluate_frame_stack_and_video_take_the_class():
    """evaluate() runs one episode of each of N = 3 environments of 7 simulator steps at repeat 2 (4 rows each) with a
    VecVideo beside it, as it does for the other tasks"""
    snap = C.evaluate_and_video(T, (3, 1, 2, True))
    assert np.isfinite(snap.mean_return) and 0 <= snap.min_return <= snap.max_return <= L
