"""The maze of the device environment on the GPU: drq_vec_maze_step / _render / _geodesic raw on poisoned memory, and
drqv2_amd.envs.VecMaze against the restatement (tests/vec_maze_oracle.py), through render(), geodesic(), image(), state
dicts, a checkpoint file, VecDistract, SimHashBonus, evaluate() and the frame ring.

Bounds.  Everything is compared bit for bit.  The generator, the flood fill, the sparse reward and the frame are integer
arithmetic (the frame after two floorf); a move is single float32 +, -, * and floorf in a fixed order and the dense
reward one correctly rounded division -- the file is built with -ffp-contract=off
-fhip-fp32-correctly-rounded-divide-sqrt; the oracle performs the same operations on numpy float32 scalars, and
generates the walls from sets of cell pairs with none of the device's bit tricks.

Shapes.  N = 3, A = 2 and N = 5, A = 4 (odd, more than one workgroup, the action's row stride differs from the two
columns read), repeat 1, 2 and 16, sparse and dense, size 3 (the smallest block) and size 8 (the boards filled to bit 63),
episode_length 7 and 40 macro steps (vec_maze_oracle.DRIVEN): the time limit falls inside a repeat for 2 and 16, and t of
environment e starts at e mod 7, so the resets stagger and the walls are generated again and again.  One configuration
draws from a pool of 2 layouts, one opens loops (VARIANTS).  Two long episodes at repeat 16 (PUSHED) hold a direction
beyond the clamp into walls and corners.  The poses (POSES) are where the move, the flood fill and the pixel rule can go
wrong.  The oracle's runs are made once, shared and never modified; what they cover is asserted without a GPU by
tests/test_cpu_vec_maze.py."""
import types

import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_env_checks as C
from tests import vec_maze_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import p
from tests.vec_env_checks import run_of, same_bits, same_state

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
lib = C.lib_fixture("drq_vec_maze_step", "the maze entries are missing")


def name_of(c):
    return f"N{c[0]}-A{c[1]}-x{c[2]}-{'sparse' if c[3] else 'dense'}-G{c[4]}" + ("" if len(c) == 5 else f"-loops{c[5]}-pool{c[6]}")


def make(cfg, episode_length=L, **kw):
    from drqv2_amd.envs import VecMaze
    N, A, k, sparse, size = cfg[:5]
    if len(cfg) == 8:
        kw = dict(dict(loops=cfg[5], layouts=cfg[6], layout_seed=cfg[7]), **kw)
    return VecMaze(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, size=size, sparse=sparse,
                   **kw)


T = types.SimpleNamespace(
    O=O, kind="VecMaze", make=make, staggered=("pos", "walls", "cells", "t"),
    words=(("pos", (2,), torch.float32), ("walls", (2,), torch.int64), ("cells", (2,), torch.int32)),
    also=lambda env, run, s: same_bits(env.geodesic().cpu().numpy(), run["geodesics"][s], (s, "geodesic()")),
    step=lambda lib, cfg, state, action, reset_all, outs: lib.drq_vec_maze_step(
        *state.values(), cfg[0], cfg[1], action, SEED, L, cfg[2], reset_all, cfg[4], 0, 0, 0, int(cfg[3]), *outs, None),
    render=lambda lib, cfg, state, frame: lib.drq_vec_maze_render(state["pos"], state["walls"], state["cells"], cfg[0], cfg[4],
                                                                  frame, None))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN + O.VARIANTS, ids=name_of)
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps, state() and
    geodesic() after every step; the two output sets are used in turn"""
    def first_geodesic(env, run):
        first = env.geodesic()
        same_bits(first.cpu().numpy(), run["geodesic0"], "the optimal path length of the first episodes")
        assert first.dtype == torch.int32 and first.is_cuda and first.data_ptr() != env.geodesic().data_ptr()

    C.env_matches_the_oracle(T, cfg, before_steps=first_geodesic)


@pytest.mark.parametrize("cfg", O.PUSHED, ids=lambda c: f"G{c[4]}-{'sparse' if c[3] else 'dense'}")
def test_long_episode_pushed_into_walls_and_corners_matches_the_oracle(cfg):
    """24 macro steps of 16 simulator steps in one episode, every direction held beyond the clamp: the limit cuts moves on
    all four sides, cells are entered through open sides, and no wall is crossed"""
    run = run_of(O, cfg)
    assert {m[2] for m in run["moves"]} == {"E", "W", "N", "S", None}
    env = make(cfg, episode_length=cfg[6], loops=64)
    same_bits(env.reset().cpu().numpy(), run["frame0"], "first frame")
    same_state(env.state(), run["state0"], "reset")
    C.follow(T, env, run, 0, cfg[5])


def test_poses_render_move_and_measure_as_the_oracle_does():
    """every pose of O.POSES written through load_state_dict(), per size: the agent at the margin in the four corners of a
    cell, on a cell boundary inside an open side, inside the goal cell, the goal in a corner cell, 8 x 8 with every wall
    closed (all 64 bits of both words set: read as unsigned, bits outside the block ignored) and every wall open -- the
    frame, geodesic(), and one step towards each diagonal from the pose"""
    from drqv2_amd.envs import VecMaze
    for size in sorted({pose[0] for pose in O.POSES}):
        poses = [pose for pose in O.POSES if pose[0] == size]
        n = len(poses)
        for push in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            env = VecMaze(n, "cuda", size=size, sparse=False, episode_length=50)
            sd = env.state_dict()
            sd["pos"], sd["walls"], sd["cells"] = (torch.from_numpy(np.stack([pose[k] for pose in poses])) for k in (1, 2, 3))
            sd["reset"] = True
            env.load_state_dict(sd)
            o = O.MazeOracle(n, episode_length=50, size=size, sparse=False)
            o.pos[:], o.walls[:], o.cells[:] = sd["pos"].numpy(), sd["walls"].numpy(), sd["cells"].numpy()
            same_bits(env.render().cpu().numpy(), o.frames(), ("poses of size", size))
            same_bits(env.geodesic().cpu().numpy(), o.geodesics(), ("geodesic() of the poses of size", size))
            action = np.tile(np.array(push, np.float32), (n, 1))
            out = env.step(torch.from_numpy(action).cuda())
            for name, t, want in zip(C.OUT, out + (env.last_substeps,), o.step(action)):
                same_bits(t.cpu().numpy(), want, (size, push, name))
            same_state(env.state(), o.state(), (size, push))


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("N,A", [(3, 2), (5, 4)])
@pytest.mark.parametrize("sparse", [True, False])
def test_step_entry_writes_every_output_byte_and_nothing_else(lib, N, A, sparse):
    """drq_vec_maze_step at size 8 and repeat 2 on guarded allocations full of the sentinel: the reset of all with a NULL
    action, then 12 steps into fresh poisoned outputs each; drq_vec_maze_render and drq_vec_maze_geodesic beside every
    one, into poisoned outputs of their own.  The outputs equal the oracle's, which never holds the byte sentinel 0xA5 (a
    frame is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one, so every byte was written; check() finds the guard
    bands of outputs, state and action untouched"""
    def geodesic_beside(state, s, run):
        dist = poison.alloc(N, torch.int32, "cuda", name="geodesic")
        assert lib.drq_vec_maze_geodesic(state["walls"], state["cells"], state["pos"], N, 8, p(dist), None) == 0
        same_bits(dist.cpu().numpy(), run["geodesic0"] if s < 0 else run["geodesics"][s], (s, "geodesic"))

    C.step_entry_on_poisoned_memory(T, lib, (N, A, 2, sparse, 8), beside=geodesic_beside)


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_maze_oracle.refused_calls / refused_renders / refused_geodesics, all held to return
    the error without a GPU by tests/test_cpu_vec_maze.py) on real allocations full of the sentinel: the error, and
    check() finds every byte of the state, the action, the frame and the scalar outputs still poison"""
    C.refused_on_poisoned_memory(0x600, lambda S0, ACT, FR, SC: ((lib.drq_vec_maze_step, O.refused_calls(S0, ACT, FR, SC), 52),
                                                                  (lib.drq_vec_maze_render, O.refused_renders(S0, FR), 15),
                                                                  (lib.drq_vec_maze_geodesic, O.refused_geodesics(S0, SC), 14)))


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 4, repeat 2, dense, size 8: 9 steps, state_dict(); a fresh environment given the dict renders the saved
    frame and takes the next 5 steps to the bit -- with another seed of its generator too, until the next reset, since
    the walls are state.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel twice in both
    directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack a frame
    stacker would hold.  A dict of another size or reward form is refused, with the field named"""
    cfg = (5, 4, 2, False, 8)
    sd = C.state_dict_image_and_ring(T, cfg)
    assert sd["config"]["sparse"] is False and sd["config"]["size"] == 8
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        make((5, 4, 2, True, 8)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bsize: saved 8, here 6"):
        make((5, 4, 2, False, 6)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bloops: saved 0, here 5"):
        make(cfg, loops=5).load_state_dict(sd)


def test_checkpoint_round_trip_continues_bit_for_bit(tmp_path):
    """N = 3, repeat 2, sparse, size 8, a pool of 2 layouts: 6 steps, checkpoint.save() inside an episode, 10 more steps; a
    fresh environment loaded from the file takes the same 10 steps to the bit, outputs and state; the file carries the
    five fields of the maze, and an environment of another pool refuses it"""
    from drqv2_amd import checkpoint
    cfg = O.VARIANTS[0]

    def between(path, saved):
        assert 0 < int(saved["t"].max()) < L, "the save must fall inside an episode"
        assert (saved["pos"] != run_of(O, cfg)["state0"]["pos"]).any() and saved["walls"].any()
        config = torch.load(path, weights_only=True)["env"]["config"]
        assert (config["size"], config["loops"], config["layouts"], config["layout_seed"], config["sparse"]) == (8, 0, 2, 77, True)
        with pytest.raises(ValueError, match="layout_seed"):
            checkpoint.load(path, env=make(cfg, layout_seed=78))

    C.checkpoint_round_trip(T, cfg, tmp_path, 6, 10, between)


def test_the_neighbours_take_the_class():
    """N = 3.  reset() and one step of VecDistract(env, distractor) with the "env" key against the distraction oracle
    applied to the maze oracle's frames -- no shape pixel is the background key; SimHashBonus of the plain frames and the
    sparse reward against its own oracle; evaluate() runs one episode of each environment of 7 simulator steps at repeat
    2 (4 rows each) with a VecVideo beside it, and a sparse return is a whole number of at most 7"""
    cfg = (3, 2, 2, True, 8)
    C.distractions_and_the_exploration_bonus(T, cfg)
    snap = C.evaluate_and_video(T, cfg)
    assert (snap.records["return"] == np.round(snap.records["return"])).all() and 0 <= snap.min_return <= snap.max_return <= L
