"""The maze of the device environment (drq_vec_maze_step / _render / _geodesic, drqv2_amd.envs.VecMaze): everything that
needs no GPU.  The public surface and the DRQ_EARG cases (all are decided before any launch), the properties of the
restatement tests/vec_maze_oracle.py that make it a maze -- every generated maze is a connected spanning tree, loops only
open walls, pools are finite and disjoint, the flood fill is the breadth-first distance, no move crosses a wall, a
scripted controller finds every goal where doing nothing finds none -- and the condition on the inputs of the GPU tests
(tests/test_hip_vec_maze.py), which is a property of the oracle's runs alone.  No assertion here has a tolerance.

A simulator step is two axis moves, x then y, each inside one row or column; "no wall is crossed" is asserted for every
one of them.  (A whole step may enter a diagonal neighbour through two open sides, one per move.)"""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_maze_oracle as O
from tests import vec_skeleton_oracle as S

F = np.float32
STEP, RENDER, GEODESIC = "drq_vec_maze_step", "drq_vec_maze_render", "drq_vec_maze_geodesic"


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN, O.VARIANTS or O.PUSHED without its frames: computed once, never
    modified"""
    return S.run_of(O, cfg, frames=False)


def bfs(G, east, south, source):
    """breadth-first distances from cell `source` = (r, c) over sets of closed walls, with a queue: {(r, c): distance}.
    Nothing here knows of boards."""
    dist, queue = {source: 0}, collections.deque([source])
    while queue:
        r, c = queue.popleft()
        for nr, nc, closed in ((r, c + 1, (r, c) in east), (r, c - 1, (r, c - 1) in east), (r + 1, c, (r, c) in south),
                               (r - 1, c, (r - 1, c) in south)):
            if 0 <= nr < G and 0 <= nc < G and not closed and (nr, nc) not in dist:
                dist[nr, nc] = dist[r, c] + 1
                queue.append((nr, nc))
    return dist


def triples(n=200):
    return [(3 + 7919 * k, k % 11, 1 + k // 7) for k in range(n)]


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build_flags():
    header = abi.text()
    for name, nargs in ((STEP, 24), (RENDER, 7), (GEODESIC, 7)):
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs and name not in _lib.NO_STREAM and name in abi.stream_entries()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for text in ("Maze.", "is bit 8 r + c of a 64-bit board", "hg = G * 0.5f (exact);  cw = 2 / G rounded once",
                 "col(x) = clamp((int)floorf((x + 1) * hg), 0, G - 1);  row(y) = clamp((int)floorf((1 - y) * hg), 0, G - 1)",
                 "h_k = fmix32(s ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ k * 0xC2B2AE35)", "64-bit word (h_4 << 32 | h_3)",
                 "sym = h_5 & 7", "(h_k & 255) < loops, with k = 16 + 8 r + c", "k = 80 + 8 r + c",
                 "i1 == i0: i1 = (i1 + 1) mod G * G", "(east, south) = walls(layout_seed, 0, h_2 mod K)",
                 "x = ((float)c + 0.5f) * cw - 1;  y = 1 - ((float)r + 0.5f) * cw",
                 "d > 0 and wall_hi:  lim = edge_hi - 0.04f;  lim < p: lim = p;  n > lim: n = lim",
                 "d < 0 and wall_lo:  lim = edge_lo + 0.04f;  lim > p: lim = p;  n < lim: n = lim",
                 "x = move(x, ax * 0.05f, c == G - 1 or east bit (r, c), (float)(c + 1) * cw - 1,",
                 "y = move(y, ay * 0.05f, r == 0 or south bit (r - 1, c), 1 - (float)r * cw,",
                 "r_i = cell(pos) == goal ? 1 : 0", "r_i = (float)(G * G - d) / (float)(G * G)", "gives d = G * G",
                 "A.x = (int)floorf(x * 672 + 672.5f);  A.y = (int)floorf(672.5f - y * 672)", "|P - A|^2 <= 729"):
        assert text in header, text                                        # the rule is part of the contract
    from drqv2_amd import build, envs
    assert "vecmaze.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecmaze.hip"))
    assert "-ffp-contract=off" in build.FILE_FLAGS["vecmaze.hip"]
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    assert envs.VecMaze.TASK == "maze" and issubclass(envs.VecMaze, envs._VecTask) and envs.VecMaze._MIN_ACTION_DIM == 2
    assert envs.VecMaze._STATE == ("pos", "walls", "cells", "t", "episode", "over")
    with open(os.path.join(build.CSRC, "vecmaze.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("sinf", "cosf", "expf", "sqrtf", "__shared__", "atomic", "__shfl", "ballot"):   # no LDS, nothing crosses lanes
        assert banned not in src, banned
    assert "launch_env_step<Maze>" in src and "launch_env_render<Maze>" in src


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_maze.py repeats them on poisoned outputs.)"""
    lib = _lib.load()
    calls = O.refused_calls(0x10000, 0x20000, 0x30000, 0x40000)
    renders, geodesics = O.refused_renders(0x10000, 0x30000), O.refused_geodesics(0x10000, 0x40000)
    S.all_refused(((lib.drq_vec_maze_step, calls), (lib.drq_vec_maze_render, renders), (lib.drq_vec_maze_geodesic, geodesics)))
    ok = [0x10000, 0x10100, 0x10200, 0x10300, 0x10400, 0x10500, 5, 2, 0x20000, 7, 9, 2, 0, 6, 0, 0, 3, 1, 0x30000, 0x40000,
          0x40100, 0x40200, 0x40300]
    sub = lambda k, v: ok[:k] + [v] + ok[k + 1:]
    listed = [[None] + ok[1:], sub(1, None), sub(2, None), sub(1, 0x10104), sub(0, 0x10002), sub(2, 0x10202), sub(7, 1), sub(8, None)]
    listed += [sub(13, v) for v in (2, 5, 9)] + [sub(14, v) for v in (-1, 256)] + [sub(15, v) for v in (-1, 65536)]
    listed += [sub(17, v) for v in (2, -1)]
    for a in listed:                                                        # the cases the issue lists
        assert a in calls, a
    assert len(calls) == 52 and len(renders) == 15 and len(geodesics) == 14
    # the task entry still knows reach and the point mass only
    assert lib.drq_vec_task_step(4, *([0x10000] * 6), 5, 2, 0x20000, 7, 9, 2, 0, 0x30000, *([0x40000] * 4), None) == -1


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("G", O.SIZES)
def test_every_generated_maze_is_a_spanning_tree_that_loops_only_open(G):
    """200 (seed, e, episode) triples per size: a queue BFS from several cells reaches all G G cells; loops = 0 leaves
    exactly G G - 1 open sides, loops = 255 none closed, loops = 96 a subset of the tree's walls; no bit outside the
    block; start != goal; all 8 symmetries occur and are 8 different maps"""
    interior = 2 * G * (G - 1)
    syms, corner = set(), 0
    for seed, e, ep in triples():
        east, south = O.walls_of(G, seed, e, ep)
        assert len(east) + len(south) == interior - (G * G - 1)
        for source in ((0, 0), (G - 1, G - 1), (G // 2, 1), (seed % G, ep % G)):
            assert len(bfs(G, east, south, source)) == G * G, (seed, e, ep, source)
        be, bs = O.boards_of(G, seed, e, ep)
        assert be & ~O.block(G, G - 1) == 0 and bs & ~O.block(G - 1, G) == 0 and be < 2 ** 63 and bs < 2 ** 63
        assert O.unboard(be, G, 8, 8) == east and O.unboard(bs, G, 8, 8) == south
        assert O.boards_of(G, seed, e, ep, 255) == (0, 0)
        le, ls = O.walls_of(G, seed, e, ep, 96)
        assert le <= east and ls <= south and len(bfs(G, le, ls, (0, 0))) == G * G
        pos, walls, (start, goal) = O.reset_state(seed, e, ep, G)
        assert start != goal and walls == (be, bs) and O.cell_of(G, pos) == start
        assert all(r < G and c < G for r, c in (O.rc(start), O.rc(goal)))
        corner += O.code(G - 1, G - 1) in (start, goal)
        syms.add(O.symmetry_of(seed, e, ep))
    assert syms == set(range(8)) and corner >= 1               # at size 8 the corner cell is bit 63
    some = sum(len(O.walls_of(G, s, e, ep, 96)[0]) for s, e, ep in triples(20))
    assert 0 < some < sum(len(O.walls_of(G, s, e, ep)[0]) for s, e, ep in triples(20))      # 96 opens some walls, not all
    tree = O.tree(G, 3, 1, 4)
    images = {(frozenset(a), frozenset(b)) for a, b in (O.transform(G, *tree, sym) for sym in range(8))}
    assert len(images) == 8 and all(len(a) + len(b) == len(tree[0]) + len(tree[1]) for a, b in images)
    # the tree before the symmetry is the binary tree: the top row and the right column are corridors
    assert not any(r == 0 for r, c in tree[0]) and not any(c == G - 1 for r, c in tree[1])


def test_bit_63_is_in_use_at_size_8():
    """cell (7, 7) is bit 63: the flood fill's reach covers it, and a distance to it is the BFS's"""
    walls = O.boards_of(8, 3, 1, 4)
    east, south = O.walls_of(8, 3, 1, 4)
    assert O.code(7, 7) == 63
    assert O.geodesic(8, walls, 0, 63) == bfs(8, east, south, (0, 0))[7, 7]
    assert O.geodesic(8, walls, 63, 9) == bfs(8, east, south, (7, 7))[1, 1]
    assert O.as_u64(O.as_i64(2 ** 63 | 5)) == 2 ** 63 | 5 and O.as_i64(2 ** 64 - 1) == -1


def test_pools_are_finite_shared_and_disjoint():
    G = 6
    pairs = [(e, ep) for e in range(10) for ep in range(1, 21)]
    pooled = {O.reset_state(5, e, ep, G, layouts=4, layout_seed=9)[1] for e, ep in pairs}
    assert 2 <= len(pooled) <= 4
    assert pooled <= {O.boards_of(G, 9, 0, k) for k in range(4)}                # the pool is (layout_seed, 0, index)
    assert len({O.reset_state(5, e, ep, G)[1] for e, ep in pairs}) > 100          # fresh mazes
    other = {O.reset_state(5, e, ep, G, layouts=4, layout_seed=10)[1] for e, ep in pairs}
    assert not pooled & other
    a = {O.boards_of(G, 9, 0, k) for k in range(64)}
    assert not a & {O.boards_of(G, 10, 0, k) for k in range(64)}
    # start and goal are drawn per episode whatever the pool
    assert len({O.reset_state(5, e, ep, G, layouts=4, layout_seed=9)[2] for e, ep in pairs}) > 100
    # another seed of the environment draws from the same pool
    assert {O.reset_state(6, e, ep, G, layouts=4, layout_seed=9)[1] for e, ep in pairs} <= pooled | {O.boards_of(G, 9, 0, k) for k in range(4)}


@pytest.mark.parametrize("G", O.SIZES)
def test_flood_fill_is_the_breadth_first_distance(G):
    """every pair of cells of 20 mazes per size (trees and mazes with loops); a cell that is cut off is G G away"""
    for k, (seed, e, ep) in enumerate(triples(20)):
        loops = (0, 64)[k % 2]
        east, south = O.walls_of(G, seed, e, ep, loops)
        walls = (O.board(east), O.board(south))
        for r in range(G):
            for c in range(G):
                dist = bfs(G, east, south, (r, c))
                for (tr, tc), d in dist.items():
                    assert O.geodesic(G, walls, O.code(r, c), O.code(tr, tc)) == d
    closed = tuple(O.board(w) for w in O.all_walls(G))
    assert O.geodesic(G, closed, 0, O.code(1, 1)) == G * G and O.geodesic(G, closed, O.code(1, 1), O.code(1, 1)) == 0
    assert O.geodesic(G, (2 ** 64 - 1, 2 ** 64 - 1), 0, 1) == G * G and O.geodesic(G, (0, 0), 0, O.code(G - 1, G - 1)) == 2 * G - 2


# ------------------------------------------------------------------------------------------------ the move
def legal(G, move):
    before, after, cut, (east, south) = move
    if before == after:
        return True
    (r0, c0), (r1, c1) = sorted((O.rc(before), O.rc(after)))
    if (r1 - r0, c1 - c0) == (0, 1):
        return not O.bit(east, r0, c0)
    return (r1 - r0, c1 - c0) == (1, 0) and not O.bit(south, r0, c0)


def test_no_wall_is_crossed():
    """every axis move of every run: the cell is kept, or a 4-neighbour is entered through an open side; the pushed runs
    (repeat 16, directions held, beyond the clamp) are cut by the limit on all four sides and cross cells too"""
    for cfg in O.DRIVEN + O.VARIANTS + O.PUSHED:
        run, G = run_of(cfg), cfg[4]
        assert run["moves"] and all(legal(G, m) for m in run["moves"]), cfg
    for cfg in O.PUSHED:
        run = run_of(cfg)
        assert {m[2] for m in run["moves"]} == {"E", "W", "N", "S", None}, cfg
        assert sum(m[0] != m[1] for m in run["moves"]) >= 10, cfg
        k, G = O.cw(cfg[4]), cfg[4]
        for st in run["states"]:                                            # ... and stays the margin away from the boundary
            assert (np.abs(st["pos"]) <= F(F(F(G) * k) - F(1)) - O.MARGIN + F(1e-6)).all()


def test_a_move_at_the_limit_stays_and_a_point_behind_the_limit_is_not_pushed_back():
    G = 4
    closed = tuple(O.board(w) for w in O.all_walls(G))
    lim = F(F(F(F(2) * O.cw(G)) - F(1)) - O.MARGIN)                          # east limit of column 1
    pos, trace = O.substep(G, (lim, F(0.25)), closed, F(1), F(0))
    assert pos[0] == lim and trace[0][2] == "E"
    behind = F(lim + F(0.02))                                                 # written by a caller: inside the margin
    pos, _ = O.substep(G, (behind, F(0.25)), closed, F(1), F(0))
    assert pos[0] == behind
    pos, _ = O.substep(G, (behind, F(0.25)), closed, F(-1), F(0))
    assert pos[0] == F(behind + F(F(-1) * O.MOVE))


def test_a_scripted_controller_finds_every_goal_and_the_zero_action_none():
    """size 4, four environments, two episodes of 200 steps each: the controller that follows the geodesic field collects
    sparse reward in every episode; doing nothing collects none, since the start is never the goal"""
    got = O.controlled_returns(4)
    print(f"returns under the controller {got}")
    assert len(got) == 8 and all(v > 0 and v == round(v) for v in got)
    idle = O.controlled_returns(4, controlled=False)
    assert len(idle) == 8 and all(v == 0.0 for v in idle)


# ------------------------------------------------------------------------------------------------ the shared drive
def test_inputs_of_the_gpu_tests_cover_what_they_claim():
    """The runs and poses tests/test_hip_vec_maze.py compares on the GPU, on the oracle alone"""
    assert {c[4] for c in O.DRIVEN} == {3, 8} and {c[:2] for c in O.DRIVEN} == {(3, 2), (5, 4)}
    assert {c[2] for c in O.DRIVEN} == {1, 2, 16} and {c[3] for c in O.DRIVEN} == {True, False}
    assert any(c[6] == 2 for c in O.VARIANTS) and any(c[5] == 96 for c in O.VARIANTS)
    cuts, in_goal, crossed = set(), 0, 0
    for cfg in O.DRIVEN + O.VARIANTS:
        run = run_of(cfg)
        acts = np.stack(run["actions"])[:, :, :2]
        assert np.isnan(acts).any() and np.isinf(acts).any() and (np.abs(acts[np.isfinite(acts)]) > 1).any(), cfg
        firsts = np.stack([o[3] for o in run["out"]])
        # a repeat of 16 ends every episode of seven steps in its first row, whatever t was: only there all reset together
        assert firsts.any() and (cfg[2] > O.EPISODE_LENGTH or not (firsts.all(1) | ~firsts.any(1)).all()), "no stagger"
        assert run["reset_rows"] >= 1 and (cfg[2] == 1 or run["cut_by_limit"] >= 1), cfg     # a time limit inside a repeat
        assert all((o[2] == 1).all() for o in run["out"])                  # the discount is 1 on every row
        rewards = np.stack([o[1] for o in run["out"]])
        G = cfg[4]
        if cfg[3]:      # sparse: exact small integers
            assert (rewards == np.round(rewards)).all() and rewards.min() >= 0 and rewards.max() <= cfg[2]
            assert (rewards[firsts == 0] == 0).any(), cfg
        else:           # dense: multiples of 1 / (G G) summed, never more than the repeat
            assert (rewards[firsts == 0] > 0).all() and rewards.max() <= cfg[2]
        cuts |= {m[2] for m in run["moves"]}
        crossed += sum(m[0] != m[1] for m in run["moves"])
        in_goal += run["in_goal"]
        assert len({tuple(s["walls"].ravel()) for s in run["states"]}) > 1     # the walls change with the episodes
        assert all(0 <= d < G * G for g in run["geodesics"] for d in g)
    assert cuts == {"E", "W", "N", "S", None} and crossed >= 10 and in_goal >= 10, (cuts, crossed, in_goal)
    pooled = run_of(O.VARIANTS[0])
    assert len({tuple(w) for s in pooled["states"] for w in s["walls"]}) <= 2
    # the poses: the four corners of a cell at the margin, on a boundary inside an open side, inside the goal cell, the
    # goal in a corner cell, 8 x 8 with every wall closed (all 64 bits set) and open
    by = lambda G: [p for p in O.POSES if p[0] == G]
    corners = {(float(p[1][0]) > 0, float(p[1][1]) > 0) for p in by(3)}
    assert len(by(3)) == 4 and len(corners) == 4
    k = O.cw(3)
    for G, pos, walls, cells in by(3):
        assert O.cell_of(3, pos) == O.code(1, 1) and tuple(cells) == (O.code(1, 1), 0)
        for ax, ay in ((1, 1), (1, -1), (-1, 1), (-1, -1)):                    # wherever it is pushed, one coordinate holds
            new, _ = O.substep(3, tuple(pos), (O.as_u64(walls[0]), O.as_u64(walls[1])), F(ax), F(ay))
            assert O.cell_of(3, new) == O.code(1, 1)
        assert min(abs(abs(float(pos[0])) - float(k) / 2), abs(abs(float(pos[1])) - float(k) / 2)) < 0.041
    assert any(p[1][0] == 0 and O.col_of(4, p[1][0]) == 2 for p in by(4))      # x = 0 is the boundary of columns 1 and 2
    assert any(O.cell_of(p[0], p[1]) == p[3][1] for p in O.POSES)
    assert any(O.rc(int(p[3][1])) in ((0, 0), (p[0] - 1, 0), (0, p[0] - 1), (p[0] - 1, p[0] - 1)) for p in O.POSES)
    assert any(p[0] == 8 and tuple(p[2]) == (-1, -1) for p in O.POSES) and any(p[0] == 8 and tuple(p[2]) == (0, 0) for p in O.POSES)
    assert any(p[0] == 8 and p[3][1] == 63 for p in O.POSES)
    for G, pos, walls, cells in O.POSES:
        w = (O.as_u64(walls[0]), O.as_u64(walls[1]))
        frame = O.render(G, pos, w, cells)
        shape = (frame != O.BACKGROUND).any(0)
        assert set(np.unique(frame[:, shape])) == {64, 255} and not (frame == 0xA5).any()
        assert set(np.unique(frame)) <= set(range(32, 74)) | {255}
        colours = {tuple(v) for v in frame[:, shape].T}
        assert O.WALL_RGB in colours and O.AGENT_RGB in colours
        assert shape[0].all() and shape[-1].all() and shape[:, 0].all() and shape[:, -1].all()     # the boundary is wall
        assert not (frame == O.BACKGROUND).all(0)[shape].any()               # never VecDistract's background key


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_constructor_state_and_state_dict_without_a_device(tmp_path):
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecMaze, VecReacher
    env = VecMaze(3, "cpu")
    assert (env.A, env.episode_length, env.action_repeat) == (2, 200, 1)
    assert (env.size, env.loops, env.layouts, env.layout_seed, env.sparse) == (6, 0, 0, 0, True)
    with pytest.raises(ValueError, match="action_dim >= 2"):
        VecMaze(3, "cpu", action_dim=1)
    for name, bads in (("size", (2, 5, 9, 6.0, "6", None, True)), ("loops", (-1, 256, 0.5, None, True)),
                       ("layouts", (-1, 65536, 2.0, None, False)), ("layout_seed", (1.5, "a", None)),
                       ("sparse", (2, "yes", None, 0.5))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                VecMaze(3, "cpu", **{name: bad})
    kw = dict(action_dim=3, episode_length=7, seed=1, action_repeat=2, size=8, loops=96, layouts=4, layout_seed=-1, sparse=False)
    env = VecMaze(3, "cpu", **kw)
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        env.geodesic()
    with pytest.raises(ValueError, match=r"step\(\): action"):
        env.step(torch.zeros(3, 2))
    s = env.state()
    assert list(s) == ["pos", "walls", "cells", "t", "episode", "over"]
    assert s["pos"].shape == s["walls"].shape == s["cells"].shape == (3, 2)
    assert (s["pos"].dtype, s["walls"].dtype, s["cells"].dtype) == (np.float32, np.int64, np.int32)
    sd = env.state_dict()
    assert sd["kind"] == "VecMaze" and sd["config"] == {
        "N": 3, "A": 3, "episode_length": 7, "seed": 1, "task": "maze", "action_repeat": 2, "size": 8, "loops": 96,
        "layouts": 4, "layout_seed": 0xFFFFFFFF, "sparse": False}
    with pytest.raises(_lib.DrqError, match="GPU"):                        # the checks pass, then the device is refused
        VecMaze(3, "cpu", **kw).load_state_dict(sd)
    for field, other, message in (("size", 6, "size: saved 8, here 6"), ("loops", 0, "loops: saved 96, here 0"),
                                  ("layouts", 5, "layouts: saved 4, here 5"),
                                  ("layout_seed", 7, "layout_seed: saved 4294967295, here 7"),
                                  ("sparse", True, "sparse: saved False, here True")):
        with pytest.raises(ValueError, match=r"\b" + message):
            VecMaze(3, "cpu", **dict(kw, **{field: other})).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        VecReacher(3, "cpu", action_dim=3, episode_length=7, seed=1, action_repeat=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="walls: no tensor saved"):
        VecMaze(3, "cpu", **kw).load_state_dict({k: v for k, v in sd.items() if k != "walls"})
    with pytest.raises(ValueError, match="walls: saved torch.int32"):
        VecMaze(3, "cpu", **kw).load_state_dict(dict(sd, walls=sd["walls"].int()))
    # drqv2_amd.checkpoint takes the class with no special case: the file holds the dict as it is, bit 63 included
    # (with it, what no task decides: action_repeat, the methods, no CPU fallback, the skeleton's words)
    env.cells[2, 1] = 63
    ck = S.class_without_a_device(VecMaze, env, tmp_path, ("walls", (1, 0), -2 ** 63), methods=("background_key", "geodesic"))
    assert ck["env"]["config"] == sd["config"] and ck["env"]["walls"].dtype == torch.int64
    path = str(tmp_path / "env.pt")
    assert torch.equal(ck["env"]["cells"], env.cells) and int(ck["env"]["walls"][1, 0]) == -2 ** 63
    with pytest.raises(_lib.DrqError, match="GPU"):                        # load() reaches the environment with the dict intact
        checkpoint.load(path, env=VecMaze(3, "cpu", **kw))
