"""numpy / Python-int restatement of the device environment's maze (a helper module: not collected).  The contract is the
comment of include/drqv2_hip.h ("device environment", "Maze"), stated here once more: the draws, the generator, the
symmetries, the loops and the pools on sets of walls between cells (no bit tricks: the device's boards are compared with
these sets), the sub-step on np.float32 scalars, one rounding per operation in the written order, the flood fill on Python
integers and the pixel rule as rectangles around segments.  The hash is tests/vec_env_oracle.py's; the macro step is the
skeleton's (tests/vec_skeleton_oracle.py): d_i = 1, and the task never ends an episode.

  boards     cell (r, c) is bit 8 r + c; east bit (r, c): a wall between (r, c) and (r, c + 1); south bit: (r, c) | (r + 1, c)
  draws      h_k = fmix32(s ^ e 0x9E3779B9 ^ episode 0x85EBCA6B ^ k 0xC2B2AE35)
  walls      all closed; every cell but (0, G - 1) opens north or east (row 0 east, column G - 1 north, else bit 8 r + c of
             h_4 << 32 | h_3: set = north); symmetry h_5 & 7 (1: transpose, 2: columns mirrored, 4: rows mirrored, in this
             order); loops: a closed wall opens when (h_k & 255) < loops, k = 16 + 8 r + c (east) or 80 + 8 r + c (south);
             loops = 255 opens every wall
  reset      episode += 1, t = 0, over = 0; i0 = h_0 mod G G; i1 = h_1 mod G G, moved on by one when equal; cell i = (i / G, i mod G);
             layouts = 0: walls(seed, e, episode); K > 0: walls(layout_seed, 0, h_2 mod K); pos = the centre of the start cell
  sub-step   x, then y with the cell taken again: n = p + a 0.05; towards a wall: lim = edge -+ 0.04, never behind p
  reward     sparse: cell(pos) == goal; dense: (G G - d) / (G G), d the flood fill's distance
  frame      in 1/16 pixel, y downwards, W = 1344 / G (render below)
"""
import numpy as np

from tests import vec_skeleton_oracle as S
from tests.vec_env_oracle import BACKGROUND, F, M32, SIDE, fmix32
from tests.vec_skeleton_oracle import sanitise

SIZES = (3, 4, 6, 7, 8)
MOVE, MARGIN = F(0.05), F(0.04)
UNITS, WALL_T, AGENT_R2 = 1344, 12, 729
GOAL_RGB, WALL_RGB, AGENT_RGB = (64, 255, 64), (255, 255, 255), (255, 64, 255)
_P = 16 * np.arange(SIDE) + 8                      # a pixel's centre along either axis


def hdraw(seed, e, episode, k):
    return fmix32((seed & M32) ^ (e * 0x9E3779B9 & M32) ^ (episode * 0x85EBCA6B & M32) ^ (k * 0xC2B2AE35 & M32))


def hg(G):
    return F(F(G) * F(0.5))


def cw(G):
    return F(F(2) / F(G))


def code(r, c):
    return 8 * r + c


def rc(cell):
    return (cell >> 3) & 7, cell & 7


# ---- the generator, on sets of walls ----------------------------------------------------------------------------------
def all_walls(G):
    """every interior wall: (east, south), sets of the (r, c) whose east / south side they close"""
    return {(r, c) for r in range(G) for c in range(G - 1)}, {(r, c) for r in range(G - 1) for c in range(G)}


def tree(G, seed, e, episode):
    dirs = hdraw(seed, e, episode, 4) << 32 | hdraw(seed, e, episode, 3)
    east, south = all_walls(G)
    for r in range(G):
        for c in range(G):
            if (r, c) == (0, G - 1):
                continue
            north = False if r == 0 else True if c == G - 1 else bool(dirs >> (8 * r + c) & 1)
            if north:
                south.discard((r - 1, c))
            else:
                east.discard((r, c))
    return east, south


def symmetry_of(seed, e, episode):
    return hdraw(seed, e, episode, 5) & 7


def transform(G, east, south, sym):
    """the maze under the symmetry: every wall is a pair of cells, and the cells move"""
    def f(r, c):
        if sym & 1:
            r, c = c, r
        if sym & 2:
            c = G - 1 - c
        if sym & 4:
            r = G - 1 - r
        return r, c
    pairs = [((r, c), (r, c + 1)) for r, c in east] + [((r, c), (r + 1, c)) for r, c in south]
    new_east, new_south = set(), set()
    for a, b in pairs:
        (r0, c0), (r1, c1) = sorted((f(*a), f(*b)))
        assert (r1 - r0, c1 - c0) in ((0, 1), (1, 0))
        (new_east if r0 == r1 else new_south).add((r0, c0))
    return new_east, new_south


def walls_of(G, seed, e, episode, loops=0):
    """the generator: (east, south) as sets"""
    east, south = transform(G, *tree(G, seed, e, episode), symmetry_of(seed, e, episode))
    if loops == 255:
        return set(), set()
    if loops > 0:
        east = {(r, c) for r, c in east if (hdraw(seed, e, episode, 16 + 8 * r + c) & 255) >= loops}
        south = {(r, c) for r, c in south if (hdraw(seed, e, episode, 80 + 8 * r + c) & 255) >= loops}
    return east, south


def board(cells):
    b = 0
    for r, c in cells:
        b |= 1 << (8 * r + c)
    return b


def unboard(b, G, rows, cols):
    return {(r, c) for r in range(rows) for c in range(cols) if b >> (8 * r + c) & 1}


def boards_of(G, seed, e, episode, loops=0):
    east, south = walls_of(G, seed, e, episode, loops)
    return board(east), board(south)


def reset_state(seed, e, episode, G, loops=0, layouts=0, layout_seed=0):
    """(pos, walls, cells) of episode `episode` of environment e: float32 pair, two Python ints, two cell codes"""
    GG = G * G
    i0, i1 = hdraw(seed, e, episode, 0) % GG, hdraw(seed, e, episode, 1) % GG
    if i1 == i0:
        i1 = (i1 + 1) % GG
    r0, c0 = divmod(i0, G)
    if layouts > 0:
        walls = boards_of(G, layout_seed & M32, 0, hdraw(seed, e, episode, 2) % layouts, loops)
    else:
        walls = boards_of(G, seed, e, episode, loops)
    x = F(F(F(F(c0) + F(0.5)) * cw(G)) - F(1))
    y = F(F(1) - F(F(F(r0) + F(0.5)) * cw(G)))
    return (x, y), walls, (code(r0, c0), code(*divmod(i1, G)))


# ---- the sub-step ------------------------------------------------------------------------------------------------------
def _index(v, G):
    return min(max(int(np.floor(v)), 0), G - 1)


def col_of(G, x):
    return _index(F(F(x + F(1)) * hg(G)), G)


def row_of(G, y):
    return _index(F(F(F(1) - y) * hg(G)), G)


def cell_of(G, pos):
    return code(row_of(G, pos[1]), col_of(G, pos[0]))


def bit(b, r, c):
    return bool(b >> (8 * r + c) & 1)


def move(p, d, wall_hi, edge_hi, wall_lo, edge_lo):
    """one axis: (the new coordinate, "hi" / "lo" when the limit cut the move, else None)"""
    n = F(p + d)
    if d > 0 and wall_hi:
        lim = F(edge_hi - MARGIN)
        if lim < p:
            lim = p
        if n > lim:
            return lim, "hi"
    elif d < 0 and wall_lo:
        lim = F(edge_lo + MARGIN)
        if lim > p:
            lim = p
        if n < lim:
            return lim, "lo"
    return n, None


def substep(G, pos, walls, ax, ay):
    """one simulator step under the sanitised action -> (pos, trace): trace = [(cell before, cell after, side the limit
    cut: "E" / "W" / "N" / "S" / None)] for the x move and for the y move"""
    east, south = walls
    x, y = pos
    k = cw(G)
    c, r = col_of(G, x), row_of(G, y)
    nx, cut = move(x, F(ax * MOVE), c == G - 1 or bit(east, r, c), F(F(F(c + 1) * k) - F(1)),
                   c == 0 or bit(east, r, c - 1), F(F(F(c) * k) - F(1)))
    trace = [(code(r, c), code(r, col_of(G, nx)), {"hi": "E", "lo": "W", None: None}[cut])]
    x = nx
    c, r = col_of(G, x), row_of(G, y)
    ny, cut = move(y, F(ay * MOVE), r == 0 or bit(south, r - 1, c), F(F(1) - F(F(r) * k)),
                   r == G - 1 or bit(south, r, c), F(F(1) - F(F(r + 1) * k)))
    trace.append((code(r, c), code(row_of(G, ny), c), {"hi": "N", "lo": "S", None: None}[cut]))
    return (x, ny), trace


# ---- the flood fill ------------------------------------------------------------------------------------------------------
def block(rows, cols):
    return sum(((1 << cols) - 1) << (8 * r) for r in range(rows))


def geodesic(G, walls, frm, to):
    """the dilations of cell `frm` through open sides until cell `to` is covered; G G when the fill stops before that"""
    oe, os_ = block(G, G - 1) & ~walls[0], block(G - 1, G) & ~walls[1]
    reach, goal, d = 1 << (frm & 63), 1 << (to & 63), 0
    while not reach & goal:
        nxt = reach | (reach & oe) << 1 | (reach >> 1) & oe | (reach & os_) << 8 | (reach >> 8) & os_
        if nxt == reach:
            return G * G
        reach, d = nxt, d + 1
    return d


def reward_of(G, pos, walls, goal, sparse):
    at = cell_of(G, pos)
    if sparse:
        return F(1) if at == goal else F(0)
    return F(F(G * G - geodesic(G, walls, at, goal)) / F(G * G))


# ---- the frame -------------------------------------------------------------------------------------------------------------
def _near(lo, hi):
    """the pixel centres within WALL_T of the interval [lo, hi] along one axis"""
    return (_P >= lo - WALL_T) & (_P <= hi + WALL_T)


def wall_mask(G, walls):
    W = UNITS // G
    m = np.zeros((SIDE, SIDE), bool)
    segments = [(0, 0, 0, UNITS), (UNITS, UNITS, 0, UNITS), (0, UNITS, 0, 0), (0, UNITS, UNITS, UNITS)]      # x0, x1, y0, y1
    segments += [((c + 1) * W, (c + 1) * W, r * W, (r + 1) * W) for r, c in unboard(walls[0], G, G, G - 1)]
    segments += [(c * W, (c + 1) * W, (r + 1) * W, (r + 1) * W) for r, c in unboard(walls[1], G, G - 1, G)]
    for x0, x1, y0, y1 in segments:
        m |= _near(y0, y1)[:, None] & _near(x0, x1)[None, :]
    return m


def agent_centre(pos):
    return (int(np.floor(F(F(pos[0] * F(672)) + F(672.5)))), int(np.floor(F(F(672.5) - F(pos[1] * F(672))))))


def render(G, pos, walls, cells):
    """the frame of one state"""
    W = UNITS // G
    gr, gc = rc(int(cells[1]))
    inset = lambda k: (_P >= k * W + W // 4) & (_P < (k + 1) * W - W // 4)
    AX, AY = agent_centre(pos)
    agent = ((_P - AX) ** 2)[None, :] + ((_P - AY) ** 2)[:, None] <= AGENT_R2
    frame = np.stack([BACKGROUND] * 3)
    for m, rgb in ((inset(gr)[:, None] & inset(gc)[None, :], GOAL_RGB), (wall_mask(G, walls), WALL_RGB), (agent, AGENT_RGB)):
        for ch in range(3):
            frame[ch][m] = rgb[ch]
    return frame


def as_i64(b):
    """a board as the int64 a tensor holds"""
    return int(np.array(b & (2 ** 64 - 1), np.uint64).view(np.int64))


def as_u64(v):
    return int(np.array(v, np.int64).view(np.uint64))


def geodesics_of(G, state):
    """the flood fill's distance from every environment's cell to its goal, of the state words `state`: int32 [N]"""
    return np.array([geodesic(G, (as_u64(w[0]), as_u64(w[1])), cell_of(G, pos), int(cells[1]))
                     for pos, w, cells in zip(state["pos"], state["walls"], state["cells"])], np.int32)


class MazeOracle(S.SkeletonOracle):
    WORDS = (("pos", (2,), F), ("walls", (2,), np.int64), ("cells", (2,), np.int32))

    def __init__(self, num_envs, episode_length=200, seed=0, repeat=1, size=6, loops=0, layouts=0, layout_seed=0, sparse=True,
                 frames=True):
        assert size in SIZES and 0 <= loops <= 255 and 0 <= layouts <= 65535
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.G, self.loops, self.layouts = int(size), int(loops), int(layouts)
        self.layout_seed, self.sparse = int(layout_seed) & M32, bool(sparse)
        # what a run met: every axis move as (cell before, cell after, side cut, walls), sub-steps in the goal cell
        self.moves = []
        self.in_goal = 0

    def walls_of(self, e):
        return as_u64(self.walls[e, 0]), as_u64(self.walls[e, 1])

    def geodesics(self):
        return geodesics_of(self.G, self.state())

    def new_episode(self, e, ep):
        pos, walls, cells = reset_state(self.seed, e, ep, self.G, self.loops, self.layouts, self.layout_seed)
        self.pos[e], self.cells[e] = pos, cells
        self.walls[e] = [as_i64(w) for w in walls]

    def sanitise(self, row):
        return sanitise(row[0]), sanitise(row[1])

    def frame(self, e):
        return render(self.G, self.pos[e], self.walls_of(e), self.cells[e])

    def substep(self, e, a):
        walls, goal = self.walls_of(e), int(self.cells[e, 1])
        pos, trace = substep(self.G, tuple(self.pos[e]), walls, *a)
        self.moves += [m + (walls,) for m in trace]
        self.in_goal += cell_of(self.G, pos) == goal
        self.pos[e] = pos
        return reward_of(self.G, pos, walls, goal, self.sparse), F(1), False


_SEEN = ("moves", "in_goal", "cut_by_limit", "full", "reset_rows")


# ---- the scripted controller: what makes the task solvable (it lives here, not in the library) ------------------------------
def neighbours(G, walls, cell):
    """the cells behind the open sides of `cell`, with the unit step (dx, dy) in world coordinates towards each"""
    r, c = rc(cell)
    out = []
    if c < G - 1 and not bit(walls[0], r, c):
        out.append((code(r, c + 1), (1, 0)))
    if c > 0 and not bit(walls[0], r, c - 1):
        out.append((code(r, c - 1), (-1, 0)))
    if r < G - 1 and not bit(walls[1], r, c):
        out.append((code(r + 1, c), (0, -1)))
    if r > 0 and not bit(walls[1], r - 1, c):
        out.append((code(r - 1, c), (0, 1)))
    return out


def centre_of(G, cell):
    r, c = rc(cell)
    return (c + 0.5) * 2.0 / G - 1.0, 1.0 - (r + 0.5) * 2.0 / G


def controller_action(G, pos, walls, goal):
    """towards the centre of the neighbour that is nearer to the goal along the geodesic field (of the goal cell itself
    when the point is in it), at full speed until the last step: float32 [ax, ay] in [-1, 1]"""
    at = cell_of(G, pos)
    nxt = at if at == goal else min(neighbours(G, walls, at), key=lambda n: geodesic(G, walls, n[0], goal))[0]
    tx, ty = centre_of(G, nxt)
    return [F(np.clip((tx - float(pos[0])) / 0.05, -1, 1)), F(np.clip((ty - float(pos[1])) / 0.05, -1, 1))]


def controlled_returns(size, N=4, episodes=2, episode_length=200, seed=0, controlled=True):
    """the sparse return of every episode of a run under the controller (or under the zero action): [N x episodes]"""
    o = MazeOracle(N, episode_length=episode_length, seed=seed, size=size, frames=False)
    o.reset()
    returns, total = [], np.zeros(N)
    while len(returns) < N * episodes:
        a = np.zeros((N, 2), F)
        if controlled:
            for e in range(N):
                a[e] = controller_action(size, o.pos[e], o.walls_of(e), int(o.cells[e, 1]))
        _, reward, _, first, _ = o.step(a)
        total += reward
        if o.over.all():
            returns += total.tolist()
            total[:] = 0
    return returns


# ---- the driven runs the CPU and the GPU tests share ------------------------------------------------------------------
STEPS, EPISODE_LENGTH, SEED = 40, 7, 5
# (N, A, repeat, sparse, size): the smallest block, and the one that fills the boards
DRIVEN = tuple((N, A, k, sparse, size) for size in (3, 8) for (N, A) in ((3, 2), (5, 4)) for k in (1, 2, 16) for sparse in (True, False))
# (N, A, repeat, sparse, size, loops, layouts, layout_seed)
VARIANTS = ((3, 2, 2, True, 8, 0, 2, 77), (5, 4, 2, False, 8, 96, 0, 0))
# (N, A, repeat, sparse, size, steps, episode_length): long episodes pushed into walls and corners
PUSHED = ((5, 2, 16, True, 3, 24, 1000), (5, 2, 16, False, 8, 24, 1000))


def _run(o, steps, actions):
    """S.record, and the geodesic distances of the first state and of the state after every step"""
    run = S.record(o, steps, actions, _SEEN)
    run["geodesic0"], run["geodesics"] = geodesics_of(o.G, run["state0"]), [geodesics_of(o.G, st) for st in run["states"]]
    return run


def driven_run(N, A, repeat, sparse, size, loops=0, layouts=0, layout_seed=0, seed=SEED, steps=STEPS,
               episode_length=EPISODE_LENGTH, frames=True):
    """The oracle driven for `steps` macro steps: the actions it was given, everything it returned (the frames only if
    asked for: they are most of the time), the state and the geodesic distances after every step.  Half of the action
    rows of an environment are S.wild_actions, half the controller's times 1.5 (beyond the clamp), so that in episodes of
    seven steps walls are met and goals are entered.  The reset is staggered (S.stagger)"""
    r = np.random.RandomState(seed * 100003 + N * 101 + A * 17 + repeat * 3 + int(sparse) + size * 1009 + loops + layouts)
    o = MazeOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, size=size, loops=loops, layouts=layouts,
                   layout_seed=layout_seed, sparse=sparse, frames=frames)
    o.reset()
    S.stagger(o)

    def actions(s):
        a = S.wild_actions(r, N, A)
        for e in np.flatnonzero(r.randint(0, 2, N)):
            if not o.over[e]:
                a[e, :2] = np.array(controller_action(size, o.pos[e], o.walls_of(e), int(o.cells[e, 1])), F) * F(1.5)
        return a
    return _run(o, steps, actions)


_PUSHES = ((1, 1), (1, -1), (-1, -1), (-1, 1), (1, 0), (0, 1), (-1, 0), (0, -1))


def pushed_run(N, A, repeat, sparse, size, steps, episode_length, seed=SEED, frames=True):
    """one long episode under actions that hold a direction, diagonal or along an axis, for three macro steps of `repeat`
    simulator steps and lie beyond the clamp: every environment is pushed into walls and corners and slides along them"""
    o = MazeOracle(N, episode_length=episode_length, seed=seed, repeat=repeat, size=size, loops=64, sparse=sparse, frames=frames)
    o.reset()

    def actions(s):
        a = np.zeros((N, A), F)
        for e in range(N):
            a[e, :2] = np.array(_PUSHES[(e + s // 3) % 8], F) * F(1.5)
        return a
    return _run(o, steps, actions)


def run(cfg, frames=True):
    """the run of a configuration of DRIVEN, VARIANTS or PUSHED"""
    return pushed_run(*cfg, frames=frames) if cfg in PUSHED else driven_run(*cfg, frames=frames)


# ---- the poses the frame, the move and the flood fill are compared at: (size, pos, walls, cells) -------------------------------
def _edge(G, k):
    return F(F(F(k) * cw(G)) - F(1))


def _pose(G, pos, east, south, start, goal):
    return G, np.array(pos, F), np.array([as_i64(east), as_i64(south)], np.int64), np.array([code(*start), code(*goal)], np.int32)


def _poses():
    poses = []
    e3, s3 = (board(w) for w in all_walls(3))
    lo, hi = F(_edge(3, 1) + MARGIN), F(_edge(3, 2) - MARGIN)      # the margins of the middle cell of a closed 3 x 3 maze
    up, down = F(F(F(1) - F(F(1) * cw(3))) - MARGIN), F(F(F(1) - F(F(2) * cw(3))) + MARGIN)
    for x in (lo, hi):
        for y in (up, down):
            poses.append(_pose(3, (x, y), e3, s3, (1, 1), (0, 0)))          # the four corners of a cell; the goal in a corner cell
    poses.append(_pose(4, (0.0, 0.25), 0, 0, (1, 1), (3, 3)))               # exactly on a cell boundary inside an open side
    poses.append(_pose(4, (_edge(4, 1), F(F(1) - F(F(3) * cw(4)))), 0, 0, (1, 1), (0, 3)))    # on a crossing of two open lines
    ge, gs = boards_of(6, 3, 1, 1)
    poses.append(_pose(6, centre_of(6, code(2, 3)), ge, gs, (0, 0), (2, 3)))    # inside the goal cell
    poses.append(_pose(6, (0.31, -0.52), ge, gs, (0, 0), (5, 0)))               # a generated maze, the goal in a corner cell
    poses.append(_pose(8, centre_of(8, code(7, 7)), 2 ** 64 - 1, 2 ** 64 - 1, (7, 7), (0, 0)))    # every wall closed: all bits set
    poses.append(_pose(8, (-0.9, 0.9), 0, 0, (0, 0), (7, 7)))                   # every wall open; the goal is bit 63
    ge, gs = boards_of(8, 9, 2, 4, loops=40)
    poses.append(_pose(8, (0.124, -0.126), ge, gs, (3, 4), (7, 0)))             # a generated 8 x 8 maze with loops
    return tuple(poses)


POSES = _poses()


# ---- the argument lists the entries refuse: shared by the CPU and the GPU test -----------------------------------------
def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_maze_step must refuse, around one well-formed list over the four given base addresses
    (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     pos walls       cells       t           episode     over        N  A  action seed L repeat reset size loops layouts
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, S0 + 0x400, S0 + 0x500, 5, 2, ACT, 7, 9, 2, 0, 6, 0, 0,
          3, 1, FR, SC, SC + 0x100, SC + 0x200, SC + 0x300]         # layout_seed sparse frame reward discount first substeps
    bad = S.refused_steps(ok, "w w8 w w w b N A action - L repeat reset - - - - - frame w w b w",
                          {13: (0, 1, 2, 5, 9, 16, -3), 14: (-1, 256), 15: (-1, 65536), 17: (2, -1)})     # size, loops, layouts, sparse
    assert len(bad) == 12 + 27 + 3 + 1 + 9
    return bad


def refused_renders(S0, FR):
    """the argument lists drq_vec_maze_render must refuse: (pos, walls, cells, N, size, frame)"""
    return S.refused_reads([S0, S0 + 0x100, S0 + 0x200, 3, 6, FR], "w w8 w N - frame", {4: (5, 0, 9)})


def refused_geodesics(S0, OUT):
    """the argument lists drq_vec_maze_geodesic must refuse: (walls, cells, pos, N, size, out)"""
    return S.refused_reads([S0 + 0x100, S0 + 0x200, S0, 3, 6, OUT], "w8 w w N - w", {4: (5, 2, 10)})
