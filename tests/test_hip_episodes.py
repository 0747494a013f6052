"""Episode files for the step-major ring on the GPU: drq_vec_fill against drq_vec_add and drq_vec_export_rows against the
ring and drq_vec_stack_gather on poisoned, guarded memory; export_episodes() against the numpy restatement of the device
environment (tests/vec_env_oracle.py); add_episodes() against a twin store fed by add(); the prioritized tree; and
update() on a prefilled store.

Bounds.  Every comparison is of copied bytes -- frames, float32 words, flags, and a tree two stores build with the same
launches on the same operands -- so every one is exact.

Coverage, continuing the map of tests/test_hip_entries.py:
  here            vec_export_rows, vec_fill (each with its DRQ_EARG cases on refused, poisoned outputs)"""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_env_oracle as EO
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p, rs_
from tests.test_hip_vec_replay import make_agent, reseed

pytestmark = pytest.mark.gpu
EARG = -1
OBS, FRAME, FB = (9, 84, 84), (3, 84, 84), 3 * 84 * 84
R, N = 16, 3


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_fill" in _lib.PROTOTYPES, "the episode-file entries are missing"
    return _lib.load()


@pytest.fixture(scope="module")
def ops():
    from drqv2_amd import ops as o
    return o


@pytest.fixture(scope="module")
def E():
    from drqv2_amd import episodes
    return episodes


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ drq_vec_fill
def poisoned_ring(fb, A, seed):
    """the five arrays of a ring of R x N between guard bands, holding what an older lap left there"""
    r = rs_(seed)
    return [dev(torch.from_numpy(r.randint(0, 256, (R * N, fb)).astype(np.uint8)), "frames"),
            dev(torch.from_numpy(r.standard_normal((R * N, A)).astype(np.float32)), "action"),
            dev(torch.from_numpy(r.standard_normal(R * N).astype(np.float32)), "reward"),
            dev(torch.from_numpy(r.uniform(size=R * N).astype(np.float32)), "discount"),
            dev(torch.from_numpy(r.randint(0, 2, R * N).astype(np.uint8)), "first")]


@pytest.mark.parametrize("T,n", [(0, 1), (0, 5), (13, 7), (5, R)])
@pytest.mark.parametrize("A", [1, 2, 6])
@pytest.mark.parametrize("fb", [16, FB])
def test_fill_equals_row_by_row_adds(lib, ops, fb, A, T, n):
    """one drq_vec_fill of n rows from row T against n drq_vec_add calls on a twin ring with the same contents: n = 1;
    from the empty ring (row 0 is a reset row although its flags say otherwise); 13 + 7 > 16 wraps inside the launch;
    n = R rewrites every slot, starting in the middle.  frame_bytes = 16: one piece per frame, and 21,168: 1,323 pieces,
    a ragged last trip.  A = 1: action rows of 4 bytes.  Every array of both rings bit for bit, guard bands intact"""
    r = rs_(100 * n + T + A)
    src = [r.randint(0, 256, (n, N, fb)).astype(np.uint8), r.standard_normal((n, N, A)).astype(np.float32),
           r.standard_normal((n, N)).astype(np.float32), r.uniform(size=(n, N)).astype(np.float32),
           (r.uniform(size=(n, N)) < 0.4).astype(np.uint8)]
    src[4][0] = 0                                                  # with T = 0: flags the rule for row 0 overrides
    ring, twin = poisoned_ring(fb, A, 7), poisoned_ring(fb, A, 7)
    d_src = [dev(torch.from_numpy(a), f"src{k}") for k, a in enumerate(src)]
    ops.vec_fill(*ring, R, N, T, *d_src)
    for i in range(n):
        rows = [dev(torch.from_numpy(a[i]), f"row{k}") for k, a in enumerate(src)]
        assert lib.drq_vec_add(*(p(t) for t in twin), R, N, A, fb, T + i, *(p(t) for t in rows), None) == 0
    torch.cuda.synchronize()
    for a, b, name in zip(ring, twin, ("frames", "action", "reward", "discount", "first")):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    first = ring[4].cpu().numpy().reshape(R, N)
    old = poisoned_ring(fb, A, 7)[4].cpu().numpy().reshape(R, N)
    for i in range(n):                                             # ... and the twin is no accident
        want = np.ones(N, np.uint8) if T + i == 0 else src[4][i]
        assert np.array_equal(first[(T + i) % R], want), i
        assert np.array_equal(ring[0].cpu().numpy().reshape(R, N, fb)[(T + i) % R], src[0][i])
    untouched = [q for q in range(R) if q not in {(T + i) % R for i in range(n)}]
    assert np.array_equal(first[untouched], old[untouched])


def test_fill_refusals(lib):
    fb, A, n = 16, 2, 3
    ring = [poison.alloc(s, d, "cuda", name=nm, kind="refused") for s, d, nm in (
        ((R * N, fb), torch.uint8, "frames"), ((R * N, A), torch.float32, "action"), ((R * N,), torch.float32, "reward"),
        ((R * N,), torch.float32, "discount"), ((R * N,), torch.uint8, "first"))]
    src = [dev(torch.zeros(s, dtype=d), nm) for s, d, nm in (
        ((n, N, fb), torch.uint8, "src_frames"), ((n, N, A), torch.float32, "src_action"), ((n, N), torch.float32, "src_reward"),
        ((n, N), torch.float32, "src_discount"), ((n, N), torch.uint8, "src_first"))]
    ok = [p(t) for t in ring] + [R, N, A, fb, 2, n] + [p(t) for t in src]
    bad = [ok[:k] + [None] + ok[k + 1:] for k in (0, 1, 2, 3, 4, 11, 12, 13, 14, 15)]           # every pointer
    for k, v in ((5, 0), (6, 0), (6, -1), (7, 0), (8, 0), (8, 24), (8, -16), (9, -1), (10, 0), (10, -2), (10, R + 1)):
        bad.append(ok[:k] + [v] + ok[k + 1:])                      # R, N, A, frame_bytes, T, n
    bad.append([ok[0] + 8] + ok[1:])                               # frames / src_frames not 16-byte aligned
    bad.append(ok[:11] + [ok[11] + 4] + ok[12:])
    bad.append(ok[:1] + [ok[1] + 2] + ok[2:])                      # a float pointer inside a word
    for a in bad:
        assert lib.drq_vec_fill(*a, None) == EARG, a[5:11]
    poison.check()                                                 # nothing was written by a refused call
    for t in ring:
        poison.forget(t)
    assert lib.drq_vec_fill(*ok, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ drq_vec_export_rows
XT = 22                                                            # rows added: the ring of 16 has wrapped
# environment 0: one episode from row 8 on.  environment 1: resets on 9, 15, 16 (15 is ring row 15, 16 ring row 0) and
# 20.  environment 2: resets on 7, 18, 19
X_RESETS = {0: {8}, 1: {9, 15, 16, 20}, 2: {7, 18, 19}}
# (t, e, t0): t0 = t; t0 = t - 1; deep inside an episode; stacks that reach across the ring's wrap (rows 14 .. 17)
X_TABLE = [(8, 0, 8), (9, 0, 8), (10, 0, 8), (21, 0, 8), (16, 0, 8), (17, 0, 8), (15, 1, 15), (16, 1, 16), (17, 1, 16),
           (18, 1, 16), (14, 1, 9), (19, 2, 19), (20, 2, 19), (21, 2, 19), (17, 2, 7), (15, 2, 7), (10, 0, 8)]


def export_stores(A):
    """a VecFrameReplay and a VecDeviceReplay of small stacked observations fed XT rows with the resets above"""
    from drqv2_amd.replay import VecDeviceReplay, VecFrameReplay
    r = rs_(A)
    vf = VecFrameReplay(R, N, A, 3, 0.99, "cuda", guard_rows=2)
    vd = VecDeviceReplay(R, N, (2, 4, 4), A, 3, 0.99, "cuda", guard_rows=2)
    for t in range(XT):
        first = np.array([t in X_RESETS[e] for e in range(N)])
        row = (r.uniform(-1, 1, (N, A)).astype(np.float32), r.standard_normal(N).astype(np.float32),
               r.uniform(size=N).astype(np.float32), first)
        vf.add(cu(r.randint(0, 256, (N,) + FRAME).astype(np.uint8)), *(cu(a) for a in row))
        vd.add(cu(r.randint(0, 256, (N, 2, 4, 4)).astype(np.uint8)), *(cu(a) for a in row))
    return vf, vd


@pytest.mark.parametrize("A", [1, 6])
def test_export_rows_equal_the_ring_and_the_stack_gather(ops, A):
    """the table above, and a table of one entry: scalars = the ring's, the canonical 0, 0, 1 where t == t0 (the ring
    holds random values there); obs = FrameBatch.stacks() of the same slots on the single-frame ring, the slot itself on
    the stacked one"""
    vf, vd = export_stores(A)
    for store in (vf, vd):
        for entries in (X_TABLE, X_TABLE[7:8], X_TABLE[2:3]):
            table = torch.tensor(entries, dtype=torch.int32)
            obs, act, rew, disc = ops.vec_export_rows(store.frames, store.action, store.reward, store.discount, R, N,
                                                      dev(table, "table"), store._stack)
            slots = torch.tensor([(t % R) * N + e for t, e, _ in entries], dtype=torch.int64).cuda()
            reset = torch.tensor([t == t0 for t, _, t0 in entries]).cuda()
            assert obs.shape == (len(entries), store.stack_bytes)
            if store is vf:
                assert torch.equal(obs, store.sample(4).stacks(slots))
            else:
                assert torch.equal(obs, store.frames[slots])
            want = [torch.where(reset[:, None], torch.zeros_like(act), store.action[slots]),
                    torch.where(reset, torch.zeros_like(rew), store.reward[slots]),
                    torch.where(reset, torch.ones_like(disc), store.discount[slots])]
            for got, w in zip((act, rew, disc), want):
                assert torch.equal(got.view(torch.int32), w.view(torch.int32))
            assert bool(reset.any()) or len(entries) == 1
    assert float(vf.reward[(8 % R) * N].abs()) > 0                 # the ring does hold something else on a reset row


def test_export_rows_refusals_and_entries_outside_the_ring(lib):
    fb, A, M = 16, 2, 4
    r = rs_(3)
    frames = dev(torch.from_numpy(r.randint(0, 256, (R * N, fb)).astype(np.uint8)), "frames")
    action, reward, discount = (dev(torch.from_numpy(r.standard_normal(s).astype(np.float32)), nm) for s, nm in (
        ((R * N, A), "action"), ((R * N,), "reward"), ((R * N,), "discount")))
    table = dev(torch.tensor([(5, 1, 3), (5, N, 3), (5, -1, 3), (2, 0, 3)], dtype=torch.int32), "table")
    outs = [poison.alloc(s, d, "cuda", name=nm, kind="refused") for s, d, nm in (
        ((M, fb), torch.uint8, "obs"), ((M, A), torch.float32, "act"), ((M,), torch.float32, "rew"), ((M,), torch.float32, "disc"))]
    ok = [p(frames), p(action), p(reward), p(discount), R, N, A, fb, 1, p(table), M] + [p(t) for t in outs]
    bad = [ok[:k] + [None] + ok[k + 1:] for k in (0, 1, 2, 3, 9, 11, 12, 13, 14)]
    for k, v in ((4, 0), (5, 0), (5, -3), (6, 0), (7, 0), (7, 8), (8, 0), (8, 2), (8, 9), (10, 0), (10, -1)):
        bad.append(ok[:k] + [v] + ok[k + 1:])                      # R, N, A, frame_bytes, stack, M
    bad.append([ok[0] + 4] + ok[1:])
    bad.append(ok[:11] + [ok[11] + 8] + ok[12:])
    bad.append(ok[:9] + [ok[9] + 2] + ok[10:])
    for a in bad:
        assert lib.drq_vec_export_rows(*a, None) == EARG, a[4:11]
    poison.check()
    for t in outs:
        poison.partial(t)                                          # from here on: written in part, guards still checked
    assert lib.drq_vec_export_rows(*ok, None) == 0
    torch.cuda.synchronize()
    # entry 0 is a step of the ring; an environment outside [0, N) and t < t0 leave their rows as they were
    assert torch.equal(outs[0][0], frames[5 * N + 1]) and float(outs[2][0]) == float(reward[5 * N + 1])
    for t in outs:
        assert (t[1:].contiguous().view(torch.uint8).cpu().numpy().reshape(3, -1).view(
            {1: np.uint8, 4: np.int32}[t.element_size()]) == poison.sentinel_of(t.dtype)).all()


# ------------------------------------------------------------------------------------------------ round trips
TN, TR, TA, TT, TLEN, TSEED = 3, 24, 2, 20, 4, 21


def reach_run():
    """TT rows of the reach task in numpy: environments 0 and 2 walk to their targets (episodes end early, at different
    times), environment 1 moves at random (its episodes run into the limit of 4).  Returns the rows
    (frame, action, reward, discount, first) as the collection loop hands them to add()"""
    o = EO.ReachOracle(TN, episode_length=TLEN, seed=TSEED)
    r = rs_(100 + TSEED)
    rows = [(o.reset(), np.zeros((TN, TA), np.float32), np.zeros(TN, np.float32), np.ones(TN, np.float32),
             np.ones(TN, np.uint8))]
    for _ in range(1, TT):
        seek = np.clip((o.target - o.pos) * 10, -1, 1).astype(np.float32)
        noise = r.uniform(-1, 1, (TN, TA)).astype(np.float32)
        a = np.where(np.arange(TN)[:, None] == 1, noise, seek).astype(np.float32)
        frame, reward, discount, first = o.step(a)
        rows.append((frame, a, reward, discount, first))
    return rows


def oracle_episodes(rows):
    """the closed episodes of such a run as the files must hold them, in numpy: [(e, t0, dict)], ordered by (t1, e)"""
    out = []
    for e in range(TN):
        resets = [t for t in range(len(rows)) if rows[t][4][e]]
        for t0, t1 in zip(resets, resets[1:]):
            n = t1 - 1 - t0
            if n < 1:
                continue
            f = [rows[t][0][e] for t in range(t0, t1)]
            ep = {"observation": np.stack([np.concatenate([f[max(k - 2, 0)], f[max(k - 1, 0)], f[k]]) for k in range(n + 1)]),
                  "action": np.stack([rows[t][1][e] for t in range(t0, t1)]),
                  "reward": np.array([[rows[t][2][e]] for t in range(t0, t1)], np.float32),
                  "discount": np.array([[rows[t][3][e]] for t in range(t0, t1)], np.float32)}
            ep["action"][0], ep["reward"][0], ep["discount"][0] = 0, 0, 1     # the reset transition's dummies
            out.append((t1 - 1, e, t0, ep))
    out.sort(key=lambda x: x[:2])
    return [(e, t0, ep) for _, e, t0, ep in out]


def collected_store():
    """a VecFrameReplay fed the run by the device environment itself"""
    from drqv2_amd.envs import VecReach
    from drqv2_amd.replay import VecFrameReplay
    rows = reach_run()
    store = VecFrameReplay(TR, TN, TA, 3, 0.99, "cuda", seed=5)
    env = VecReach(TN, "cuda", action_dim=TA, episode_length=TLEN, seed=TSEED)
    junk = torch.full((TN, TA), 0.25, device="cuda")               # what a loop may hand to add() beside a reset frame
    store.add(env.reset(), junk, torch.zeros(TN, device="cuda"), torch.ones(TN, device="cuda"))
    for t in range(1, TT):
        action = cu(rows[t][1])
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, reward, discount, first)
    return store, rows


def same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        elif k == "rng":
            assert a[k][0] == b[k][0] and torch.equal(a[k][1], b[k][1]) and a[k][2:] == b[k][2:]
        else:
            assert a[k] == b[k], k


def episode_bytes(ep):
    return b"".join(np.ascontiguousarray(ep[k]).tobytes() for k in ("observation", "action", "reward", "discount"))


@pytest.fixture(scope="module")
def exported(tmp_path_factory, E):
    """round trip 1 runs once: the directory, the report and what went into it"""
    import replay_buffer as RB
    d = tmp_path_factory.mktemp("episodes")
    store, rows = collected_store()
    before = store.state_dict()
    # 5 steps per chunk: episodes of up to 5 steps straddle chunk boundaries, both pinned sets are reused
    report = store.export_episodes(d, chunk_bytes=5 * (3 * FB + 4 * TA + 20))
    after = store.state_dict()
    again = store.export_episodes(d, start_row=report.next_row)
    files = [fn for fn, _, _ in RB._episode_files(d)]
    return {"dir": d, "store": store, "rows": rows, "report": report, "again": again, "before": before, "after": after,
            "files": files, "final": store.state_dict()}


def test_export_equals_the_oracle_episodes(exported, E):
    """every file equals the episode recomputed in numpy -- stacks, actions, rewards, discounts -- under the
    reference's name; the counts are the plan's; a second call from next_row writes nothing; the store is unchanged"""
    import replay_buffer as RB
    rows, report = exported["rows"], exported["report"]
    want = oracle_episodes(rows)
    assert len({ep["action"].shape[0] for _, _, ep in want}) >= 3  # the resets are staggered: lengths 1 .. 4
    flags = np.ones((TR, TN), np.uint8)
    flags[:TT] = np.stack([r[4] for r in rows])
    plan = E.plan_export(flags.reshape(-1), TT, TR, TN)
    assert plan.episodes == [(e, t0, ep["action"].shape[0] - 1) for e, t0, ep in want]
    assert (report.episodes, report.transitions, report.next_row) == (len(want), sum(n for _, _, n in plan.episodes), TT)
    assert (report.zero_length, report.headless, report.open, report.short) == (plan.zero_length, plan.headless, plan.open,
                                                                             plan.short) == (0, 0, TN, 0)
    assert [str(f) for f in report.files] == [str(f) for f in sorted(report.files, key=lambda f: int(f.stem.split("_")[1]))]
    assert sorted(map(str, report.files)) == sorted(map(str, exported["files"])) and len(report.files) == len(want)
    for i, (fn, (e, t0, ep)) in enumerate(zip(report.files, want)):
        ts, idx, n = fn.stem.split("_")
        assert (int(idx), int(n)) == (i, ep["action"].shape[0] - 1) and len(ts) == 15 and ts[8] == "T"
        got = RB.load_episode(fn)
        assert sorted(got) == ["action", "discount", "observation", "reward"]
        for k in got:
            assert got[k].dtype == ep[k].dtype and got[k].shape == ep[k].shape, (fn.name, k)
            assert np.array_equal(got[k], ep[k]), (fn.name, k, e, t0)
        assert got["observation"].shape[1:] == OBS and got["reward"].shape == (int(n) + 1, 1)
    again = exported["again"]
    assert again.files == [] and (again.episodes, again.transitions, again.next_row, again.open) == (0, 0, TT, TN)
    same_state(exported["before"], exported["after"])
    same_state(exported["before"], exported["final"])


def feed_planned(E, twin, eps):
    """add() by add(), the rows add_episodes() plans for the episode dicts eps"""
    from drqv2_amd.replay import newest_frames
    prepared = [{"frame": newest_frames(ep["observation"]), "action": ep["action"], "reward": ep["reward"],
                 "discount": ep["discount"]} for ep in eps]
    plan = E.plan_fill([ep["action"].shape[0] - 1 for ep in eps], twin.N)
    for r in range(plan.L):
        frame, action, reward, discount, first = E.planned_rows(plan, prepared, r, r + 1)
        twin.add(cu(frame[0]), cu(action[0]), cu(reward[0]), cu(discount[0]), cu(first[0]))
    return plan


def planned_twin(E, eps, store):
    """a store like `store`, fed by add() with the planned rows"""
    kw = dict(priority_alpha=store.priority_alpha) if store.priority_alpha else {}
    twin = type(store)(store.R, store.N, store.A, store.nstep, store.gamma, "cuda", seed=5, guard_rows=store.guard_rows, **kw)
    return twin, feed_planned(E, twin, eps)


def same_ring(a, b):
    """T and every slot that has been written (the rest of `frames` is whatever the allocator handed out)"""
    torch.cuda.synchronize()
    assert a.T == b.T
    live = min(a.T, a.R) * a.N
    for name in a._RING:
        assert torch.equal(getattr(a, name)[:live], getattr(b, name)[:live]), name
        if name != "frames":
            assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_files_load_and_refill_a_ring_of_another_shape(exported, E, tmp_path):
    """the files load into the episode store (single frames: its own stack check passes) with as many transitions as
    the report counts; add_episodes(directory) into a ring of 2 x 40 equals a twin fed by add() with the planned rows;
    exporting that ring again gives the same episodes, byte for byte"""
    import replay_buffer as RB
    from drqv2_amd.replay import VecFrameReplay
    d, report = exported["dir"], exported["report"]
    loader = RB.make_replay_loader(d, 1000, 8, 0, False, 3, 0.99, device="cuda", obs_shape=OBS, action_dim=TA, seed=1,
                                   single_frames=True)
    assert len(loader._store) == report.transitions and len(loader._store.episodes) == report.episodes
    eps = [RB.load_episode(fn) for fn in exported["files"]]
    store = VecFrameReplay(40, 2, TA, 3, 0.99, "cuda", seed=5)
    # 7 rows per chunk: several launches, the pinned sets used in turn
    fill = store.add_episodes(d, chunk_bytes=7 * 2 * (FB + 4 * TA + 9))
    twin, plan = planned_twin(E, eps, store)
    assert fill == (report.episodes, report.transitions, plan.L, plan.pad_rows) and store.T == plan.L <= 40
    assert fill.rows * 2 == fill.transitions + fill.episodes + fill.pad_rows
    same_ring(store, twin)
    back = store.export_episodes(tmp_path, include_open=True)      # the longest environment's last episode is still open
    assert back.episodes == report.episodes and back.transitions == report.transitions and back.short == 0
    got = sorted(episode_bytes(RB.load_episode(fn)) for fn in back.files)
    assert got == sorted(episode_bytes(ep) for ep in eps) and len(set(got)) == len(got)


def test_prefill_of_a_prioritized_store_builds_the_same_tree(exported, E):
    """priority_alpha = 0.6, episode dicts as the source, on top of rows the store already holds: after add_episodes the
    tree equals the twin's, bit for bit, and one sample() draws the same batch with the same weights on both"""
    import replay_buffer as RB
    from drqv2_amd.replay import PrioritizedBatch, VecFrameReplay
    every = [RB.load_episode(fn) for fn in exported["files"]]

    def same_draw(store, twin):
        same_ring(store, twin)
        assert torch.equal(store.tree, twin.tree) and float(store.tree[1]) > 0
        a, b = store.sample(16), twin.sample(16)
        assert isinstance(a, PrioritizedBatch) and torch.equal(store.last_index, twin.last_index)
        assert torch.equal(store.last_steps, twin.last_steps) and int(store.last_steps.min()) >= 1
        assert torch.equal(a.weights.view(torch.int32), b.weights.view(torch.int32))
        for k in range(5):
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k

    # all episodes into 40 rows in one chunk; five of them (at most 18 rows per environment) into 18 rows, 4 rows a chunk
    for rows_, eps, chunk in ((40, every, 256 << 20), (18, every[:5], 4 * 2 * (FB + 4 * TA + 9))):
        store = VecFrameReplay(rows_, 2, TA, 3, 0.99, "cuda", seed=5, guard_rows=2, priority_alpha=0.6)
        twin, plan = planned_twin(E, eps, store)
        assert plan.L <= rows_
        store.add_episodes(eps, chunk_bytes=chunk)
        same_draw(store, twin)
    # a second prefill on top of the first, in one chunk as large as a prioritized store allows: the ring of 18 wraps
    # inside add_episodes and the tree follows row by row
    store.add_episodes(every[5:10])
    feed_planned(E, twin, every[5:10])
    assert store.T > 18
    same_draw(store, twin)


def frame_set(eps):
    """the newest frame of every step of the episodes, as byte strings"""
    return {np.ascontiguousarray(f).tobytes() for ep in eps for f in ep["observation"][:, -3:]}


def test_live_rows_after_a_prefill_stay_apart_from_it(exported, tmp_path):
    """what a collection loop does after add_episodes(): the reset row of every environment FLAGGED as one (only row 0
    of an empty ring is a reset row by itself), then live steps.  An export of everything returns the prefilled episodes
    unchanged, byte for byte, beside the live one; an export from the row behind that reset row returns the live one
    only.  Without the flag the live frames would continue the last prefilled episode of every environment"""
    import replay_buffer as RB
    from drqv2_amd.replay import VecFrameReplay
    eps = [RB.load_episode(fn) for fn in exported["files"]]
    store = VecFrameReplay(64, 2, TA, 3, 0.99, "cuda", seed=5)
    L = store.add_episodes(exported["dir"]).rows
    r = rs_(8)
    live = [r.randint(0, 256, (2,) + FRAME).astype(np.uint8) for _ in range(4)]
    zeros, ones = torch.zeros(2, device="cuda"), torch.ones(2, device="cuda")
    flag = lambda v: torch.full((2,), v, dtype=torch.uint8, device="cuda")
    store.add(cu(live[0]), torch.zeros(2, TA, device="cuda"), zeros, ones, flag(1))
    for f in live[1:3]:
        store.add(cu(f), torch.full((2, TA), 0.5, device="cuda"), ones, ones, flag(0))
    store.add(cu(live[3]), torch.zeros(2, TA, device="cuda"), zeros, ones, flag(1))      # closes the live episodes
    whole = store.export_episodes(tmp_path / "all")
    got = [RB.load_episode(fn) for fn in whole.files]
    old = [ep for ep in got if not frame_set([ep]) & {f.tobytes() for fr in live for f in fr}]
    assert sorted(map(episode_bytes, old)) == sorted(map(episode_bytes, eps))
    new = [ep for ep in got if not any(ep is o for o in old)]
    assert len(new) == 2 and all(ep["action"].shape[0] == 3 for ep in new) and not frame_set(new) & frame_set(eps)
    assert {int(np.array_equal(ep["observation"][0, 6:9], live[0][1])) for ep in new} == {0, 1}     # one per environment
    for ep in new:
        e = int(np.array_equal(ep["observation"][0, 6:9], live[0][1]))
        want = [live[k][e] for k in range(3)]
        assert np.array_equal(ep["observation"], np.stack([np.concatenate([want[max(k - 2, 0)], want[max(k - 1, 0)], want[k]])
                                                           for k in range(3)]))
    tail = store.export_episodes(tmp_path / "tail", start_row=L + 1)
    assert tail.episodes == 2 and sorted(episode_bytes(RB.load_episode(fn)) for fn in tail.files) == sorted(map(episode_bytes, new))


def test_demo_prefill_and_export(exported, tmp_path, monkeypatch, capsys):
    """tools/vec_train_demo.py --prefill-dir D --export-dir O, run in this process: 12 steps of 2 environments with
    episodes of 4 steps and no update.  O receives the episodes collected live and nothing of D: no file repeats a
    prefilled episode and no frame of D appears in one (the first live episode is not the continuation of a prefilled
    one), and every file is a frame-stacked episode of at most 4 transitions"""
    import os
    import runpy
    import sys
    import replay_buffer as RB
    from drqv2_amd.replay import newest_frames
    demo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "vec_train_demo.py")
    out = tmp_path / "live"
    monkeypatch.setattr(sys, "argv", [demo] + ("--steps 12 --envs 2 --rows 64 --report 6 --warmup 1000 --episode-length 4 "
                                               "--batch 8 --feature-dim 20 --hidden-dim 64 --seed 1").split()
                        + ["--prefill-dir", str(exported["dir"]), "--export-dir", str(out)])
    path = list(sys.path)
    try:
        runpy.run_path(demo, run_name="__main__")
    finally:
        sys.path[:] = path
    text = capsys.readouterr().out
    assert f"prefilled from {exported['dir']}: {exported['report'].episodes} episodes" in text and "exported" in text
    eps = [RB.load_episode(fn) for fn in exported["files"]]
    got = [RB.load_episode(fn) for fn, _, _ in RB._episode_files(out)]
    assert 2 <= len(got) <= 12 and len({episode_bytes(ep) for ep in got}) == len(got)
    assert not frame_set(got) & frame_set(eps)
    for ep in got:
        assert 1 <= ep["action"].shape[0] - 1 <= 4 and newest_frames(ep["observation"], check=True).shape[1:] == FRAME
        assert not ep["action"][0].any() and ep["reward"][0, 0] == 0 and ep["discount"][0, 0] == 1


def test_update_runs_on_a_prefilled_store(exported):
    """agent.update(iter(prefilled_store), step): finite metrics at B = 8"""
    import replay_buffer as RB
    from drqv2_amd.replay import VecFrameReplay
    store = VecFrameReplay(40, 2, TA, 3, 0.99, "cuda", seed=5)
    store.add_episodes([RB.load_episode(fn) for fn in exported["files"]])
    store.batch_size = 8
    ag = make_agent(TA)
    reseed()
    m = ag.update(iter(store), 0)
    assert len(m) == 8 and all(np.isfinite(v) for v in m.values())
    # the loop goes on: every environment restarts with a reset row
    store.add(torch.zeros((2,) + FRAME, dtype=torch.uint8, device="cuda"), torch.zeros(2, TA, device="cuda"),
              torch.zeros(2, device="cuda"), torch.ones(2, device="cuda"), torch.ones(2, dtype=torch.uint8, device="cuda"))
    m = ag.update(iter(store), 2)
    assert all(np.isfinite(v) for v in m.values())
