"""The k-NN bonus on the GPU: drq_explore_knn, drqv2_amd.explore.KnnBonus and RandomFeatures against the numpy restatement
(tests/knn_oracle.py), which is the only thing the kernel is compared with.

Bounds.  Everything the kernel writes is compared bit for bit: a squared distance is a chain of single float32 operations
in a fixed order (build.py gives knn.hip -ffp-contract=off), min and max are exact, the square root is correctly rounded
(-fhip-fp32-correctly-rounded-divide-sqrt), so neither the dealing of candidates to workgroups nor the order of the merge
can show.  tests/test_cpu_knn.py shows that these inputs tell a contracted build from a correct one.  The batch reward is
reward + beta * log1p(dist): torch's device log1p is not pinned to the bit, so that one operation is compared with numpy's
float32 log1p within 2 ulp of the bonus (and the sum within the same absolute amount plus its own rounding).  RandomFeatures is
held to the oracle's float64 encoder by the bound of the existing encoder-forward parity test
(tests/test_hip_step.py::test_module_forwards_and_soft_update: 2e-6 normwise); its projection runs in float64 on both sides.

Shapes.  The raw entry: d = 1, 3, 50, 64 (one element, a padded quad, the flagship, the most); k = 1, 3, 8; B = 1, 3, 65 (a
ragged wave); live = 0, 1, k, k + 1, 65, 257, C + 1 and 2C + 63 with C = 128 the candidate chunk (two and three workgroups
per query with a ragged last chunk: the merge across workgroups); stride 1, and 3 with offsets 0 and 2.  More chunks than
workgroups (a workgroup walks three chunks) and more than one tile of 256 queries have a case each."""
import gc

import numpy as np
import pytest
import torch

from tests import knn_oracle as K
from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p

pytestmark = pytest.mark.gpu
F = np.float32
NAME = "drq_explore_knn"


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert NAME in _lib.PROTOTYPES, "the k-NN entry is missing"
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def leave_no_cached_blocks():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def same_bits(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), (what, got, want)


def run_entry(lib, table, live, slots, k, stride=1, offset=0, d_table=None, d_slots=None):
    """one call on guarded inputs and poisoned outputs; the distances, checked to have been written in full"""
    S, d = table.shape
    B = len(slots)
    d_table = dev(torch.from_numpy(table), "table") if d_table is None else d_table
    d_slots = dev(torch.from_numpy(slots), "slots") if d_slots is None else d_slots
    dist = poison.alloc(B, torch.float32, "cuda", name="dist")
    need = lib.drq_explore_knn_ws_bytes(B, live, stride)
    ws = poison.alloc(max(1, need // 4), torch.float32, "cuda", name="ws", kind="ws")
    assert lib.drq_explore_knn(p(d_table), S, d, live, p(d_slots), B, k, stride, offset, p(dist), p(ws), need, None) == 0
    torch.cuda.synchronize()
    return dist


# ------------------------------------------------------------------------------------------------ the raw entry
@pytest.mark.parametrize("k", K.KS)
@pytest.mark.parametrize("d", K.DIMS)
def test_entry_matches_the_oracle_bit_for_bit(lib, d, k):
    """B x live x lattice for one (d, k); the rows >= live are NaN (nothing beyond live may be read: the results are the
    oracle's, which never sees them), the slots of B = 65 hold -1, live, S - 1 and two duplicates"""
    for B, live, stride, offset in K.entry_cases(d, k):
        table, slots = K.entry_inputs(d, B, live)
        got = run_entry(lib, table, live, slots, k, stride, offset)
        want = K.knn_dist(table, live, slots, k, stride, offset)
        same_bits(got, want, (B, live, stride, offset))
        if B == 65 and live >= 65 + k and stride == 1:
            assert (want[:60] > 0).all() and not want[60:63].any()
        poison.check()
        poison.reset()


def test_rows_beyond_live_are_not_read_even_where_they_would_win(lib):
    """the rows >= live hold copies of the queries' own rows: a kernel that read one would return 0"""
    d, k, live, B = 50, 1, 2 * K.CHUNK + 63, 65
    table, slots = K.entry_inputs(d, B, live, seed=5)
    slots[60:63] = slots[:3]
    table[live:] = table[slots[:K.PAD_ROWS]]
    want = K.knn_dist(table, live, slots, k)
    assert (want > 0).all()
    same_bits(run_entry(lib, table, live, slots, k), want, "copies beyond live")
    same_bits(run_entry(lib, table, live, slots, k, 3, 2), K.knn_dist(table, live, slots, k, 3, 2), "copies beyond live, stride 3")


def test_slots_outside_the_live_rows_give_zero(lib):
    d, live = 3, 65
    table, _ = K.entry_inputs(d, 3, live)
    slots = np.array([-1, live, live + K.PAD_ROWS - 1, -2 ** 40, 2 ** 40, 5], np.int64)
    got = run_entry(lib, table, live, slots, 3).cpu().numpy()
    assert not got[:5].any() and got[5] > 0
    same_bits(got, K.knn_dist(table, live, slots, 3), "outside")


def test_duplicated_rows_and_duplicated_queries(lib):
    d, live, B = 50, 257, 65
    table, slots = K.entry_inputs(d, B, live, seed=9)
    table[10:20] = table[5]                          # eleven equal rows: zero distances, equal k-th values
    table[200] = table[100]
    slots[:8] = (5, 10, 19, 100, 200, 5, 5, 19)
    for k in (1, 3, 8):
        want = K.knn_dist(table, live, slots, k)
        assert want[0] == 0 and want[1] == 0 and (k > 1 or want[3] == 0) and want[5] == want[0]
        same_bits(run_entry(lib, table, live, slots, k), want, k)


def test_distances_that_overflow(lib):
    d, live, B, k = 50, K.CHUNK + 1, 65, 3
    table, slots = K.entry_inputs(d, B, live, seed=2, scale=4e18)         # a squared difference is near 3e37, fifty of them overflow
    table[7] = table[3]                              # one finite (zero) distance among the infinite ones
    slots[0], slots[1] = 3, 7
    want = K.knn_dist(table, live, slots, k)
    assert np.isinf(want[:60]).all() and np.isinf(K.knn_dist(table, live, slots, 2)[0])
    same_bits(run_entry(lib, table, live, slots, k), want, "overflow")
    same_bits(run_entry(lib, table, live, slots, 1), K.knn_dist(table, live, slots, 1), "overflow, k = 1")
    assert K.knn_dist(table, live, slots, 1)[0] == 0


def test_a_nan_row_counts_as_infinitely_far(lib):
    d, live, B = 3, 65, 3
    table, slots = K.entry_inputs(d, B, live, seed=4)
    table[11] = np.nan
    slots[:] = (0, 11, 12)
    for k in (1, 8):
        want = K.knn_dist(table, live, slots, k)
        assert np.isinf(want[1]) and np.isfinite(want[0])         # a NaN query is infinitely far from everything
        same_bits(run_entry(lib, table, live, slots, k), want, k)
    # 12 live rows, row 11 NaN: slot 0 has ten finite distances and one infinite one among its eleven others
    few = np.array([0, 1], np.int64)
    want = K.knn_dist(table[:20], 12, few, 8)
    assert np.isfinite(want).all()
    same_bits(run_entry(lib, table[:20].copy(), 12, few, 8), want, "k = 8 of 11 others")
    table[3:11] = np.nan                                          # now three finite ones: the 8th smallest is +infinity
    want = K.knn_dist(table[:20], 12, few, 8)
    assert np.isinf(want).all()
    same_bits(run_entry(lib, table[:20].copy(), 12, few, 8), want, "the k-th is a NaN row")


@pytest.mark.parametrize("d", [3, 50])
def test_more_chunks_than_workgroups(lib, d):
    """1,025 chunks for one tile of queries: 512 workgroups, workgroup 0 walks chunks 0, 512 and 1,024 (the ragged one)"""
    live, B, k = 1024 * K.CHUNK + 63, 3, 3
    table, slots = K.entry_inputs(d, B, live, seed=1)
    slots[:] = (0, live - 1, 512 * K.CHUNK + 5)
    same_bits(run_entry(lib, table, live, slots, k), K.knn_dist(table, live, slots, k), "1,025 chunks")


def test_more_than_one_tile_of_queries(lib):
    d, live, B, k = 3, 257, 300, 3
    table, slots = K.entry_inputs(d, B, live, seed=6)
    same_bits(run_entry(lib, table, live, slots, k), K.knn_dist(table, live, slots, k), "B = 300")
    same_bits(run_entry(lib, table, live, slots, k, 3, 2), K.knn_dist(table, live, slots, k, 3, 2), "B = 300, stride 3")


def test_two_runs_of_one_call_give_the_same_bits(lib):
    d, live, B, k = 50, 2 * K.CHUNK + 63, 65, 3
    table, slots = K.entry_inputs(d, B, live)
    dt, ds = dev(torch.from_numpy(table), "table"), dev(torch.from_numpy(slots), "slots")
    a = run_entry(lib, table, live, slots, k, d_table=dt, d_slots=ds)
    b = run_entry(lib, table, live, slots, k, d_table=dt, d_slots=ds)
    assert a.data_ptr() != b.data_ptr()
    same_bits(a, b.cpu().numpy(), "two runs")
    assert dt.cpu().numpy().tobytes() == table.tobytes() and ds.cpu().numpy().tobytes() == slots.tobytes()


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    table, slots, dist, ws = al(100 * 50 * 4, "table"), al(64, "slots"), al(32, "dist"), al(4096, "ws")
    good = dict(table=p(table), S=100, d=50, live=100, slots=p(slots), B=8, k=3, stride=1, offset=0, dist=p(dist), ws=p(ws),
                ws_bytes=4096)
    call = lambda **kw: lib.drq_explore_knn(*{**good, **kw}.values(), None)
    for bad in (dict(table=None), dict(slots=None), dict(dist=None), dict(S=0), dict(d=0), dict(d=65), dict(live=-1),
                dict(live=101), dict(B=0), dict(k=0), dict(k=9), dict(stride=0), dict(offset=1), dict(stride=2, offset=2),
                dict(dist=p(dist) + 2), dict(slots=p(slots) + 4), dict(ws=p(ws) + 4)):
        assert call(**bad) == -1, bad
    for bad in (dict(ws=None), dict(ws_bytes=255)):
        assert call(**bad) == -2, bad
    poison.check()


# ------------------------------------------------------------------------------------------------ KnnBonus on a ring
N, R, A, DIM = 3, 16, 2, 6


def ring_run(steps, k=3, beta=0.05, candidates=None, seed=4, store_kw=None, objs=None, start=0, batch=8):
    """VecReach -> VecFrameReplay.add -> observe(features made from the frame) -> one batch per step handed out by
    bonus.batches() and the next one prefetched, as update() does: every batch's last_dist, bonus and reward against the
    oracle.  objs: the objects of an earlier call (or restored ones) to go on with.  Returns them and the list of (dist,
    reward) bytes, one per batch"""
    from drqv2_amd.envs import VecReach
    from drqv2_amd.explore import KnnBonus
    from drqv2_amd.replay import VecFrameReplay
    if objs is None:
        store = VecFrameReplay(R, N, A, 3, 0.99, "cuda", seed=2, guard_rows=2, **(store_kw or {}))
        store.batch_size = batch
        objs = dict(store=store, env=VecReach(N, "cuda", action_dim=A, episode_length=7, seed=3),
                    bonus=KnnBonus(store, dim=DIM, k=k, beta=beta, candidates=candidates, seed=seed),
                    oracle=K.KnnOracle(R, N, DIM, k, beta, candidates, seed), it=iter(store))
    store, env, bonus, oracle, it = (objs[n] for n in ("store", "env", "bonus", "oracle", "it"))
    batches = bonus.batches(it)
    out = []
    proj = torch.from_numpy(np.random.RandomState(8).standard_normal((3 * 84 * 84, DIM)).astype(F)).cuda()
    for step in range(start, start + steps):
        if step == 0:
            frame = env.reset()
            store.add(frame, torch.zeros(N, A, device="cuda"), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"))
        else:
            g = torch.Generator(device="cuda")
            g.manual_seed(step)
            action = torch.rand(N, A, device="cuda", generator=g) * 2 - 1
            frame, reward, discount, first = env.step(action)
            store.add(frame, action, reward, discount, first)
        y = (frame.reshape(N, -1).float() / 255.0) @ proj                  # any float32 [N, DIM] will do: the oracle gets its bits
        bonus.observe(y)
        oracle.observe(y.cpu().numpy(), store.T)
        if store.bounds()[1] < store.bounds()[0]:
            continue
        ahead = it.peek()                                                 # drawn by the step before (now, the first time)
        raw_reward = ahead[2].clone()                                     # the look-ahead batch is still unrelabelled
        b = next(batches)
        assert b is ahead and type(b).__name__ in ("FrameBatch", "_PrioritizedFrames")
        slots = b.slots.cpu().numpy()
        want_dist, want_bonus, want_reward, lattice = oracle.apply(slots, raw_reward.cpu().numpy())
        assert (bonus.last_stride, bonus.last_offset) == lattice
        same_bits(bonus.last_dist, want_dist, (step, "dist"))
        got_bonus, got_reward = bonus.last_bonus.cpu().numpy(), b[2].cpu().numpy()
        tol = 2 * np.spacing(np.abs(want_bonus))                          # 2 ulp of the one float32 log1p (times beta)
        assert (np.abs(got_bonus - want_bonus) <= tol).all(), step
        assert (np.abs(got_reward - want_reward) <= tol[:, None] + np.spacing(np.abs(want_reward))).all(), step
        same_bits(b[2], (raw_reward.cpu().numpy() + got_bonus[:, None]).astype(F), (step, "reward += bonus, one float32 add"))
        out.append((bonus.last_dist.cpu().numpy().tobytes(), got_reward.tobytes()))
        batches.prefetch()                                                # what update() does after its launches
    return objs, out


def test_bonus_on_a_wrapped_ring_matches_the_oracle():
    objs, out = ring_run(2 * R + 5)
    assert objs["store"].T > R and objs["bonus"].live == R * N and len(out) >= R
    assert objs["bonus"].last_dist.gt(0).any()


def test_candidates_bound_the_work_with_a_stride():
    objs, _ = ring_run(R + 6, candidates=10, k=2)
    assert objs["bonus"].last_stride == 5 and objs["bonus"].live == 48         # ceil(48 / 10)


def test_prioritized_batches_keep_their_class_weights_and_priorities():
    objs, _ = ring_run(R + 3, store_kw=dict(priority_alpha=0.6))
    store, bonus = objs["store"], objs["bonus"]
    b = bonus.apply(store.sample(8))
    from drqv2_amd.replay import PrioritizedBatch
    assert isinstance(b, PrioritizedBatch) and b.weights.shape == (8,) and float(b.weights.max()) == 1.0
    b.update_priorities(torch.full((8,), 0.5, device="cuda"))
    torch.cuda.synchronize()


def test_demonstration_rows_get_no_bonus():
    from drqv2_amd.explore import KnnBonus
    from drqv2_amd.replay import VecDeviceReplay
    from tests.test_hip_vec_demos import small_episode
    FB, nstep, D = 16, 3, 9
    store = VecDeviceReplay(R, N, (FB,), A, nstep, 0.99, "cuda", seed=5, guard_rows=2, demo_rows=D)
    store.add_demonstrations([small_episode(n, s, store.slot_shape, A) for n, s in ((4, 1), (5, 2), (4, 3))])
    store.demo_fraction = 0.5
    bonus = KnnBonus(store, dim=DIM, k=2, beta=0.5)
    oracle = K.KnnOracle(R, N, DIM, 2, 0.5)
    rs = np.random.RandomState(3)
    for t in range(R + 4):
        store.add(torch.from_numpy(rs.randint(0, 256, (N, FB)).astype(np.uint8)).cuda(),
                  torch.zeros(N, A, device="cuda"), torch.ones(N, device="cuda"), torch.ones(N, device="cuda"),
                  torch.full((N,), int(t % 6 == 0), dtype=torch.uint8, device="cuda"))
        y = rs.standard_normal((N, DIM)).astype(F)
        bonus.observe(torch.from_numpy(y).cuda())
        oracle.observe(y, store.T)
    batch = store.sample(8)
    before = batch[2].clone()
    bonus.apply(batch)
    Bd = store.last_demo_count
    slots = batch.slots.cpu().numpy()
    assert Bd == 4 and (slots[:Bd] >= R * N).all() and (slots[Bd:] < R * N).all()
    same_bits(bonus.last_dist, oracle.apply(slots, before.cpu().numpy())[0], "dist")
    assert not bonus.last_dist[:Bd].any() and bonus.last_dist[Bd:].gt(0).all()
    assert torch.equal(batch[2][:Bd], before[:Bd]) and (batch[2][Bd:] > before[Bd:]).all()


def test_save_load_into_fresh_objects_and_continue_bit_for_bit(tmp_path):
    """the run saved after R + 3 steps -- a look-ahead batch pending, unrelabelled -- and continued in fresh objects hands
    out the distances and rewards of the uninterrupted run, byte for byte"""
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecReach
    from drqv2_amd.explore import KnnBonus
    from drqv2_amd.replay import VecFrameReplay
    first, tail = R + 3, 6
    _, whole = ring_run(first + tail, candidates=10)
    objs, head = ring_run(first, candidates=10)
    assert head == whole[:len(head)] and len(whole) == len(head) + tail
    assert objs["it"]._ahead is not None
    path = str(tmp_path / "knn.pt")
    checkpoint.save(path, store=objs["store"], iterator=objs["it"], env=objs["env"], bonus=objs["bonus"], extra={"step": first})
    oracle = objs["oracle"]                                # host state: goes on as it is
    del objs
    gc.collect()
    store = VecFrameReplay(R, N, A, 3, 0.99, "cuda", seed=2, guard_rows=2)
    store.batch_size = 8
    fresh = dict(store=store, env=VecReach(N, "cuda", action_dim=A, episode_length=7, seed=3),
                 bonus=KnnBonus(store, dim=DIM, k=3, beta=0.05, candidates=10, seed=4), oracle=oracle, it=iter(store))
    assert checkpoint.load(path, store=store, iterator=fresh["it"], env=fresh["env"], bonus=fresh["bonus"]) == {"step": first}
    _, cont = ring_run(tail, objs=fresh, start=first)
    assert cont == whole[len(head):]


# ------------------------------------------------------------------------------------------------ RandomFeatures
def test_random_features_shape_seed_generators_and_the_oracle():
    from drqv2_amd.explore import RandomFeatures
    from oracle import drq_oracle as O
    from tests.test_hip_step import nerr
    torch.manual_seed(7)
    torch.cuda.manual_seed_all(7)
    cpu, gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    f, g = RandomFeatures((9, 84, 84), 50, "cuda", seed=11), RandomFeatures((9, 84, 84), 50, "cuda", seed=11)
    obs = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (3, 9, 84, 84)).astype(np.uint8)).cuda()
    y = f(obs)
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(), gpu)
    assert y.shape == (3, 50) and y.dtype == torch.float32 and y.is_cuda and y.is_contiguous() and not y.requires_grad
    same_bits(g(obs), y.cpu().numpy(), "the same seed")
    assert not torch.equal(RandomFeatures((9, 84, 84), 50, "cuda", seed=12)(obs), y)
    enc = {k: v.double().cpu() for k, v in f.encoder.state_dict().items()}
    feat = O.encoder_forward(enc, obs.double().cpu())
    lin, ln = f.head[0], f.head[1]
    ref = torch.nn.functional.layer_norm(feat @ lin.weight.double().cpu().t() + lin.bias.double().cpu(), (50,),
                                         ln.weight.double().cpu(), ln.bias.double().cpu(), ln.eps)
    # the bound of tests/test_hip_step.py::test_module_forwards_and_soft_update for the encoder forward against this oracle
    assert nerr(y, ref) <= 2e-6
