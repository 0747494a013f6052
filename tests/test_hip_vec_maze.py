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
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_env_oracle as E
from tests import vec_maze_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p
from tests.test_hip_vec_replay import raw
from tests.vec_env_checks import OUT, entry_on_poisoned_memory, lib_fixture, same_bits, same_state

pytestmark = pytest.mark.gpu
L, SEED = O.EPISODE_LENGTH, O.SEED
STATE = ("pos", "walls", "cells", "t", "episode", "over")
lib = lib_fixture("drq_vec_maze_step", "the maze entries are missing")
_RUNS = {}


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN, O.VARIANTS or O.PUSHED: computed once, on first use, shared,
    never modified"""
    if cfg not in _RUNS:
        _RUNS[cfg] = O.pushed_run(*cfg) if cfg in O.PUSHED else O.driven_run(*cfg)
    return _RUNS[cfg]


def name_of(c):
    return f"N{c[0]}-A{c[1]}-x{c[2]}-{'sparse' if c[3] else 'dense'}-G{c[4]}" + ("" if len(c) == 5 else f"-loops{c[5]}-pool{c[6]}")


def make(cfg, episode_length=L, **kw):
    from drqv2_amd.envs import VecMaze
    N, A, k, sparse, size = cfg[:5]
    if len(cfg) == 8:
        kw = dict(dict(loops=cfg[5], layouts=cfg[6], layout_seed=cfg[7]), **kw)
    return VecMaze(N, "cuda", action_dim=A, episode_length=episode_length, seed=SEED, action_repeat=k, size=size, sparse=sparse,
                   **kw)


def stagger(env, run):
    """the state the oracle's run starts from (its staggered t) into an environment that has just been reset, through
    load_state_dict(), as a user of the class would write it"""
    sd = env.state_dict()
    for k in ("pos", "walls", "cells", "t"):
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
        same_bits(env.geodesic().cpu().numpy(), run["geodesics"][s], (s, "geodesic()"))


# ------------------------------------------------------------------------------------------------ the class against the oracle
@pytest.mark.parametrize("cfg", O.DRIVEN + O.VARIANTS, ids=name_of)
def test_env_matches_the_oracle_bit_for_bit(cfg):
    """reset(), then 40 macro steps at episode_length 7: frame, reward, discount, first, last_substeps, state() and
    geodesic() after every step; the two output sets are used in turn"""
    run = run_of(cfg)
    N = cfg[0]
    env = make(cfg)
    frame = env.reset()
    same_bits(frame.cpu().numpy(), run["frame0"], "first frame")
    same_bits(env.last_substeps.cpu().numpy(), np.zeros(N, np.int32), "substeps of the reset")
    stagger(env, run)
    same_state(env.state(), run["state0"], "reset")
    same_bits(env.render().cpu().numpy(), run["frame0"], "the frame does not depend on t")
    first = env.geodesic()
    same_bits(first.cpu().numpy(), run["geodesic0"], "the optimal path length of the first episodes")
    assert first.dtype == torch.int32 and first.is_cuda and first.data_ptr() != env.geodesic().data_ptr()
    kept = []
    for s in range(O.STEPS):
        follow(env, run, s, s + 1)
        kept.append(env.last_substeps)
        if s >= 1:      # two output sets in turn: the set of the step before is intact, the one before that is reused
            same_bits(kept[s - 1].cpu().numpy(), run["out"][s - 1][4], (s, "the substeps of the step before"))
        if s >= 2:
            assert kept[s - 2].data_ptr() == kept[s].data_ptr() != kept[s - 1].data_ptr()


@pytest.mark.parametrize("cfg", O.PUSHED, ids=lambda c: f"G{c[4]}-{'sparse' if c[3] else 'dense'}")
def test_long_episode_pushed_into_walls_and_corners_matches_the_oracle(cfg):
    """24 macro steps of 16 simulator steps in one episode, every direction held beyond the clamp: the limit cuts moves on
    all four sides, cells are entered through open sides, and no wall is crossed"""
    run = run_of(cfg)
    assert {m[2] for m in run["moves"]} == {"E", "W", "N", "S", None}
    env = make(cfg, episode_length=cfg[6], loops=64)
    same_bits(env.reset().cpu().numpy(), run["frame0"], "first frame")
    same_state(env.state(), run["state0"], "reset")
    follow(env, run, 0, cfg[5])


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
            for name, t, want in zip(OUT, out + (env.last_substeps,), o.step(action)):
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
    cfg = (N, A, 2, sparse, 8)
    run = run_of(cfg)
    z = lambda shape, dt, name: dev(torch.zeros(shape, dtype=dt), name)
    state = {"pos": z((N, 2), torch.float32, "pos"), "walls": z((N, 2), torch.int64, "walls"),
             "cells": z((N, 2), torch.int32, "cells"), "t": z(N, torch.int32, "t"), "episode": z(N, torch.int32, "episode"),
             "over": z(N, torch.uint8, "over")}

    def beside(s, want):
        again = poison.alloc((N, 3, 84, 84), torch.uint8, "cuda", name="rendered")
        assert lib.drq_vec_maze_render(p(state["pos"]), p(state["walls"]), p(state["cells"]), N, 8, p(again), None) == 0
        same_bits(again.cpu().numpy(), want[0], (s, "render"))
        dist = poison.alloc(N, torch.int32, "cuda", name="geodesic")
        assert lib.drq_vec_maze_geodesic(p(state["walls"]), p(state["cells"]), p(state["pos"]), N, 8, p(dist), None) == 0
        same_bits(dist.cpu().numpy(), run["geodesic0"] if s < 0 else run["geodesics"][s], (s, "geodesic"))

    entry_on_poisoned_memory(lambda action, reset_all, outs: lib.drq_vec_maze_step(
        *(p(state[n]) for n in STATE), N, A, action, SEED, L, 2, reset_all, 8, 0, 0, 0, int(sparse), *outs, None), run, N,
        state=state, compared=STATE, beside=beside,
        after_reset=lambda: state["t"].copy_(torch.from_numpy(run["state0"]["t"])))      # the stagger of the oracle's run


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_maze_oracle.refused_calls / refused_renders / refused_geodesics, all held to return
    the error without a GPU by tests/test_cpu_vec_maze.py) on real allocations full of the sentinel: the error, and
    check() finds every byte of the state, the action, the frame and the scalar outputs still poison"""
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    state, action, frame, scalars = al(0x600, "state"), al(0x100, "action"), al(5 * 3 * 84 * 84, "frame"), al(0x400, "scalars")
    calls = O.refused_calls(p(state), p(action), p(frame), p(scalars))
    for a in calls:
        assert lib.drq_vec_maze_step(*a, None) == -1, a
    renders = O.refused_renders(p(state), p(frame))
    for a in renders:
        assert lib.drq_vec_maze_render(*a, None) == -1, a
    geodesics = O.refused_geodesics(p(state), p(scalars))
    for a in geodesics:
        assert lib.drq_vec_maze_geodesic(*a, None) == -1, a
    assert len(calls) == 52 and len(renders) == 15 and len(geodesics) == 14
    poison.check()


# ------------------------------------------------------------------------------------------------ frames, images, checkpoints
def test_state_dict_into_a_fresh_environment_image_and_the_ring():
    """N = 5, A = 4, repeat 2, dense, size 8: 9 steps, state_dict(); a fresh environment given the dict renders the saved
    frame and takes the next 5 steps to the bit -- with another seed of its generator too, until the next reset, since
    the walls are state.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel twice in both
    directions.  One VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack a frame
    stacker would hold.  A dict of another size or reward form is refused, with the field named"""
    from drqv2_amd.replay import VecFrameReplay
    cfg = (5, 4, 2, False, 8)
    run = run_of(cfg)
    N, A = cfg[:2]
    env = make(cfg)
    start(env, run)
    follow(env, run, 0, 9)
    want = run["out"][8][0]
    sd = env.state_dict()
    assert sd["kind"] == "VecMaze" and sd["config"]["sparse"] is False and sd["config"]["size"] == 8
    assert tuple(sd["walls"].shape) == (N, 2) and sd["walls"].dtype == torch.int64 and sd["cells"].dtype == torch.int32
    fresh = make(cfg)
    fresh.load_state_dict(sd)
    same_bits(fresh.render().cpu().numpy(), want, "the frame of the restored state")
    same_state(fresh.state(), run["states"][8], "restored")
    same_bits(fresh.geodesic().cpu().numpy(), run["geodesics"][8], "geodesic() of the restored state")
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
        make((N, A, 2, True, 8)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bsize: saved 8, here 6"):
        make((N, A, 2, False, 6)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bloops: saved 0, here 5"):
        make(cfg, loops=5).load_state_dict(sd)


def test_checkpoint_round_trip_continues_bit_for_bit(tmp_path):
    """N = 3, repeat 2, sparse, size 8, a pool of 2 layouts: 6 steps, checkpoint.save() inside an episode, 10 more steps; a
    fresh environment loaded from the file takes the same 10 steps to the bit, outputs and state; the file carries the
    five fields of the maze, and an environment of another pool refuses it"""
    from drqv2_amd import checkpoint
    cfg = O.VARIANTS[0]
    run = run_of(cfg)
    env = make(cfg)
    start(env, run)
    follow(env, run, 0, 6)
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=env, extra={"step": 6})
    saved = env.state()
    assert 0 < int(saved["t"].max()) < L, "the save must fall inside an episode"
    assert (saved["pos"] != run["state0"]["pos"]).any() and saved["walls"].any()
    config = torch.load(path, weights_only=True)["env"]["config"]
    assert (config["size"], config["loops"], config["layouts"], config["layout_seed"], config["sparse"]) == (8, 0, 2, 77, True)
    with pytest.raises(ValueError, match="layout_seed"):
        checkpoint.load(path, env=make(cfg, layout_seed=78))
    fresh = make(cfg)
    assert checkpoint.load(path, env=fresh) == {"step": 6}
    same_state(fresh.state(), run["states"][5], "restored")
    assert raw(fresh.render()).tobytes() == run["out"][5][0].tobytes()
    follow(fresh, run, 6, 16)
    follow(env, run, 6, 16)
    same_state(fresh.state(), env.state(), "after 10 steps")


def test_the_neighbours_take_the_class():
    """N = 3.  reset() and one step of VecDistract(env, distractor) with the "env" key against the distraction oracle
    applied to the maze oracle's frames -- no shape pixel is the background key; SimHashBonus of the plain frames and the
    sparse reward against its own oracle; evaluate() runs one episode of each environment of 7 simulator steps at repeat
    2 (4 rows each) with a VecVideo beside it, and a sparse return is a whole number of at most 7"""
    import drqv2
    from drqv2_amd.distract import FrameDistractor, VecDistract
    from drqv2_amd.evaluate import VecVideo, evaluate
    from drqv2_amd.explore import SimHashBonus
    from tests import simhash_oracle as S
    from tests import vec_distract_oracle as D
    cfg = (3, 2, 2, True, 8)
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
    torch.manual_seed(3)
    agent = drqv2.DrQV2Agent((9, 84, 84), (2,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    video = VecVideo(3, "cuda", max_frames=64)
    res = evaluate(agent, make(cfg), 1, poll_every=4, video=video)
    snap = res.snapshot
    assert snap.complete and snap.episodes == 3 and sorted(snap.records["env"].tolist()) == [0, 1, 2]
    assert (snap.records["length"] == -(-L // 2)).all() and len(video) >= 5
    assert (snap.records["return"] == np.round(snap.records["return"])).all() and 0 <= snap.min_return <= snap.max_return <= L
