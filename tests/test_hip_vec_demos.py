"""Demonstrations in the step-major replay on the GPU: drq_vec_sample_mixed on poisoned, guarded memory against the numpy
restatement tests/vec_demo_oracle.py (two VecOracle geometries, so every window is oracle.nstep_sample's), and
VecDeviceReplay(demo_rows=D) -- filling, mixed draws across wraps, update() and checkpoints -- against the same oracle
and against a store without demonstrations.

Bounds.  Everything is compared bit for bit, for the reasons tests/test_hip_vec_replay.py gives: integers, one IEEE
double product truncated on both sides, copies, and the reference's float32 n-step operations in the reference's order.

Shapes.  R = 12, D = 9, B = 7, K = 4: the smallest that hold a wrapped ring, a partition with one unfilled row, every
branch of the choice among the partition rows (the oracle asserts that) and Bd = 1, 3 and B.

Coverage, continuing the map of tests/test_hip_entries.py:
  here            vec_sample_mixed (with every DRQ_EARG case on refused, poisoned outputs)"""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_demo_oracle as M
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, out, p, rs_
from tests.test_hip_replay import OBS, episode
from tests.test_hip_vec_replay import ARRAYS, compare, device_row, engine_state, make_agent, reseed

pytestmark = pytest.mark.gpu
EARG = -1
R, D, B, K = 12, 9, 7, 4
NAMES = [n for n, _ in ARRAYS]


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_sample_mixed" in _lib.PROTOTYPES, "the mixed draw's entry is missing"
    return _lib.load()


# ------------------------------------------------------------------------------------------------ drq_vec_sample_mixed
def scenario(N, A, FB, nstep, gamma=0.99, T=2 * R + 5, seed=0):
    """the oracle with the partition of vec_demo_oracle.fill_partition (Td = 8 of D = 9 rows) and a ring that has wrapped
    (T = 2R + 5, guard_rows 0: the entry takes lo and hi), random resets and a few terminal discounts"""
    mo = M.MixedOracle(R, D, N, A, FB, nstep, gamma, guard_rows=0)
    M.fill_partition(mo, seed + 1)
    r = rs_(seed + 2)
    for _ in range(T):
        mo.add(r.randint(0, 256, (N, FB)), r.uniform(-1, 1, (N, A)), r.standard_normal(N),
               np.where(r.uniform(size=N) < 0.15, 0.0, 1.0), r.uniform(size=N) < 0.2)
    assert mo.live.T > R and mo.Td < D
    return mo


def upload(mo):
    whole = mo.whole()
    return whole, {n: dev(torch.from_numpy(whole[n]), n) for n in NAMES}


def run_mixed(lib, mo, d, u, Bd, materialise):
    N, A, FB = mo.N, mo.A, mo.fb
    lo, hi = mo.live.bounds()
    n = u.shape[0]
    o = dict(idx=out(3, n, dtype=torch.int64, name="idx"), act=out(n, A, name="act"), rew=out(n, name="rew"),
             disc=out(n, name="disc"), steps=out(n, dtype=torch.int32, name="steps"))
    fr = (d["frames"], out(n, FB, dtype=torch.uint8, name="obs"), out(n, FB, dtype=torch.uint8, name="next_obs")) \
        if materialise else (None, None, None)
    rc = lib.drq_vec_sample_mixed(p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), R, D, N, A, FB, lo, hi,
                                  mo.Td, p(dev(torch.from_numpy(u), "u")), n, Bd, u.shape[1], mo.nstep, mo.live.gamma,
                                  p(o["idx"]), p(o["act"]), p(o["rew"]), p(o["disc"]), p(o["steps"]), p(fr[0]), p(fr[1]),
                                  p(fr[2]), None)
    assert rc == 0
    torch.cuda.synchronize()
    return o, fr


@pytest.mark.parametrize("Bd", [1, 3, 7])
@pytest.mark.parametrize("FB", [16, 48])
@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("nstep", [1, 3])
@pytest.mark.parametrize("N", [1, 3])
def test_mixed_draw_matches_the_oracle_bit_for_bit(lib, N, nstep, A, FB, Bd):
    """As many draws as there are crafted u rows, each rotated once more through the partition rows of the batch, so that
    with Bd = 1 too every branch of the choice is taken by a partition row: the oracle's require_branches() says so
    before the test ends.  Each draw without and with frame copies: idx [3][B], action, reward, discount, steps, and
    both frame outputs, bit for bit; partition rows index >= R N, ring rows < R N (asserted in the oracle's sample())"""
    mo = scenario(N, A, FB, nstep, seed=10 * N + nstep)
    whole, d = upload(mo)
    crafted = M.crafted_rows(mo, K)
    r = rs_(Bd)
    for j in range(len(crafted)):
        u = r.random_sample((B, K))
        for b in range(min(Bd, len(crafted))):
            u[b] = crafted[(j + b) % len(crafted)]
        if Bd < B:
            u[-1] = [0.0, np.nextafter(1.0, 0.0), 0.0, np.nextafter(1.0, 0.0)]      # the ends of the ring's table
        else:
            u[-1] = [np.nextafter(1.0, 0.0), 0.0, np.nextafter(1.0, 0.0), 0.0]      # ... and of the partition's
        want = mo.sample(u, Bd)
        o, _ = run_mixed(lib, mo, d, u, Bd, False)
        compare(o, want)
        om, (frames, obs, nxt) = run_mixed(lib, mo, d, u, Bd, True)
        compare(om, want)
        assert np.array_equal(obs.cpu().numpy(), want["obs"]) and np.array_equal(nxt.cpu().numpy(), want["next_obs"])
        assert np.array_equal(obs.cpu().numpy(), whole["frames"][want["idx"][0]])
        assert np.array_equal(nxt.cpu().numpy(), whole["frames"][want["idx"][1]])
    mo.require_branches(empty=N == 3)
    for n in NAMES:                                                # the draws wrote nothing into the store
        assert np.array_equal(d[n].cpu().numpy(), whole[n]), n


def test_mixed_draw_second_block_of_the_scalar_part(lib):
    """B = 300 without copies: the scalar part takes two workgroups, and the split Bd = 259 lies inside the second"""
    mo = scenario(3, 2, 16, 3, seed=5)
    _, d = upload(mo)
    u = rs_(6).random_sample((300, K))
    o, _ = run_mixed(lib, mo, d, u, 259, False)
    compare(o, mo.sample(u, 259))


def test_mixed_draw_refusals(lib):
    N, A, FB, nstep = 3, 2, 16, 3
    mo = scenario(N, A, FB, nstep, seed=1)
    _, d = upload(mo)
    lo, hi = mo.live.bounds()
    Td, n = mo.Td, 4
    u = dev(torch.from_numpy(rs_(3).random_sample((n, K))), "u")
    ref = lambda shape, dt, name: poison.alloc(shape, dt, "cuda", name=name, kind="refused")
    outs = [ref((3, n), torch.int64, "idx"), ref((n, A), torch.float32, "act"), ref((n,), torch.float32, "rew"),
            ref((n,), torch.float32, "disc"), ref((n,), torch.int32, "steps")]
    fo = [ref((n, FB), torch.uint8, "obs"), ref((n, FB), torch.uint8, "next_obs")]
    #      0              1               2               3                4  5  6  7  8   9   10  11  12    13 14 15 16     17
    ok = [p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), R, D, N, A, FB, lo, hi, Td, p(u), n, 2, K, nstep, 0.99] + \
        [p(t) for t in outs] + [None, None, None]
    bad = []
    for k in (0, 1, 2, 3, 12, 18, 19, 20, 21, 22):                 # every required pointer
        a = list(ok)
        a[k] = None
        bad.append(a)
    # what drq_vec_sample refuses: R, N, A, B, K, nstep <= 0; frame_bytes; the ring's lo < 1, hi < lo (no drawable ring
    # row), hi - lo + 1 + nstep > R
    assert hi - lo + 1 + nstep == R                                # so one more step or one more row is one too many
    for k, v in ((4, 0), (6, 0), (6, -3), (7, 0), (13, 0), (15, 0), (16, 0), (16, -1), (8, 24), (8, 0), (9, 0), (10, lo - 1),
                 (16, nstep + 1), (9, lo - 1)):
        a = list(ok)
        a[k] = v
        bad.append(a)
    # the partition: D <= 0, Td < 0, Td > D, Bd outside [0, B], Bd > 0 with Td - nstep < 1
    for k, v in ((5, 0), (5, -1), (11, -1), (11, D + 1), (14, -1), (14, n + 1), (11, nstep), (11, 0)):
        a = list(ok)
        a[k] = v
        bad.append(a)
    full = [p(d["frames"]), p(fo[0]), p(fo[1])]
    for miss in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):        # some but not all of frames / obs_out / next_obs_out
        a = list(ok)
        a[23:26] = [None if i in miss else q for i, q in enumerate(full)]
        bad.append(a)
    a = list(ok)
    a[23:26] = [full[0], full[1] + 4, full[2]]                     # obs_out not 16-byte aligned
    bad.append(a)
    for a in bad:
        assert lib.drq_vec_sample_mixed(*a, None) == EARG, a[4:17]
    poison.check()                                                 # nothing was written by a refused call
    for t in outs + fo:
        poison.forget(t)
    assert lib.drq_vec_sample_mixed(*ok, None) == 0 and lib.drq_vec_sample_mixed(*(ok[:23] + full), None) == 0
    # what is not read is not refused: the ring's rows when every batch row is a demonstration (no live row need
    # exist), the partition's when none is
    only_demos, only_ring = list(ok), list(ok)
    only_demos[9], only_demos[10], only_demos[14] = 1, 0, n
    only_ring[11], only_ring[14] = 0, 0
    assert lib.drq_vec_sample_mixed(*only_demos, None) == 0 and lib.drq_vec_sample_mixed(*only_ring, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the store
FBS, NS, AS, NSTEP, GAMMA, GUARD = 16, 3, 2, 3, 0.9, 4


def small_episode(n, seed, shape=(FBS,), A=AS):
    r = rs_(seed)
    d = np.ones((n + 1, 1), np.float32)
    d[-1] = 0.0 if seed % 2 else 1.0
    return {"observation": r.randint(0, 256, (n + 1,) + shape).astype(np.uint8),
            "action": r.uniform(-1, 1, (n + 1, A)).astype(np.float32),
            "reward": r.standard_normal((n + 1, 1)).astype(np.float32), "discount": d}


FIRST_CALL = [(2, 1), (1, 2), (3, 3), (1, 4)]       # (transitions, seed): L = 4 rows, one pad row on lane 0
SECOND_CALL = [(1, 5), (2, 6)]                      # L = 3 rows, lane 2 receives nothing: pad rows with zero frames


def planned(store, spec):
    """(episode dicts, the planned rows) of one add_demonstrations() call, by the host planning the store uses"""
    from drqv2_amd import episodes as E
    eps = [small_episode(n, s, store.slot_shape, store.A) for n, s in spec]
    plan = E.plan_fill([n for n, _ in spec], store.N)
    rows = E.planned_rows(plan, [dict(frame=e["observation"], action=e["action"], reward=e["reward"], discount=e["discount"])
                                 for e in eps], 0, plan.L)
    return eps, plan, rows


def new_store(demo_rows=D, seed=21, **kw):
    from drqv2_amd.replay import VecDeviceReplay
    return VecDeviceReplay(R, NS, (FBS,), AS, NSTEP, GAMMA, "cuda", seed=seed, guard_rows=GUARD, demo_rows=demo_rows, **kw)


def fill_demos(vs, mo=None):
    """both calls; returns the partition's five arrays as the planned rows say they must be (the filled slots)"""
    want = {n: [] for n in NAMES}
    for spec in (FIRST_CALL, SECOND_CALL):
        eps, plan, rows = planned(vs, spec)
        before = vs.demo_rows_filled
        rep = vs.add_demonstrations(eps)
        assert rep.rows == plan.L and rep.episodes == len(spec) and rep.pad_rows == plan.pad_rows
        assert vs.demo_rows_filled == before + plan.L
        for n, a in zip(NAMES, rows):
            want[n].append(a.reshape((plan.L * vs.N,) + a.shape[2:]))
        for i in range(plan.L):
            if mo is not None:
                mo.add_demo(*(a[i] for a in rows))
    return {n: np.concatenate(v) for n, v in want.items()}


def live_row(r, N=NS, A=AS, fb=FBS):
    return (r.randint(0, 256, (N, fb)).astype(np.uint8), r.uniform(-1, 1, (N, A)).astype(np.float32),
            r.standard_normal(N).astype(np.float32), np.where(r.uniform(size=N) < 0.1, 0.0, 1.0).astype(np.float32),
            r.uniform(size=N) < 0.2)


def partition_bytes(vs):
    torch.cuda.synchronize()
    return {n: vs._demo[n].cpu().numpy().copy() for n in NAMES}


def got_of(vs, b):
    return dict(idx=vs.last_index, act=b[1], rew=b[2], disc=b[3], steps=vs.last_steps)


def test_add_demonstrations_writes_the_planned_rows_appends_and_never_evicts():
    vs = new_store()
    empty = partition_bytes(vs)
    want = fill_demos(vs)
    Td = vs.demo_rows_filled
    assert Td == 7 and vs.demo_bounds() == (1, 7 - NSTEP) and vs.T == 0
    got = partition_bytes(vs)
    for n in NAMES:
        assert np.array_equal(got[n][:Td * NS], want[n]), n                      # the planned rows, bit for bit
        assert np.array_equal(got[n][Td * NS:], empty[n][Td * NS:]), n           # the rows behind them: untouched
    assert (want["first"].reshape(Td, NS)[[0, 4]] == 1).all()                    # each call starts on reset rows
    assert not want["frames"].reshape(Td, NS, FBS)[4:, 2].any()                  # the lane that received nothing
    assert torch.equal(vs.first, torch.ones_like(vs.first)) and not vs.frames.any()      # the ring has not been touched
    with pytest.raises(ValueError, match="need L = 4 rows per lane behind the 7 already filled"):
        vs.add_demonstrations([small_episode(3, 9)])
    after = partition_bytes(vs)
    assert vs.demo_rows_filled == Td and all(np.array_equal(after[n], got[n]) for n in NAMES)     # nothing written


def test_fraction_zero_draws_what_a_store_without_demonstrations_draws(monkeypatch):
    from drqv2_amd import replay
    calls = []
    real = replay.launch
    monkeypatch.setattr(replay, "launch", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    plain, vs = new_store(demo_rows=0), new_store()
    fill_demos(vs)
    assert vs.demo_fraction == 0.0
    r = rs_(2)
    draws = 0
    for _ in range(3 * R):
        row = live_row(r)
        plain.add(*(torch.from_numpy(x).cuda() for x in row))
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
        if plain.bounds()[1] < plain.bounds()[0]:
            continue
        a, b = plain.sample(B), vs.sample(B)
        for x, y in zip(list(a) + [plain.last_index, plain.last_steps], list(b) + [vs.last_index, vs.last_steps]):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        assert vs.last_demo_count == 0 and b.frames.shape[0] == (R + D) * NS and b.frames.data_ptr() == vs.frames.data_ptr()
        assert a.frames is plain.frames
        draws += 1
    assert draws > 2 * R and vs.T == 3 * R
    assert "drq_vec_sample_mixed" not in calls and calls.count("drq_vec_sample") == 2 * draws
    assert plain.rng.random_sample() == vs.rng.random_sample()


def test_fraction_half_draws_equal_the_oracle_across_wraps():
    """a draw after each of 3R live adds (and, before any live row, a batch of demonstrations alone), the fraction at
    0.5: Bd = 4 of B = 7.  Every batch is the oracle's for the same seed, bit for bit; afterwards the partition's five
    arrays are byte for byte what add_demonstrations left and the ring is the oracle's"""
    from drqv2_amd import _lib
    vs = new_store()
    mo = M.MixedOracle(R, D, NS, AS, FBS, NSTEP, GAMMA, guard_rows=GUARD)
    twin = np.random.RandomState(21)
    vs.demo_fraction = 0.5
    with pytest.raises(_lib.DrqError, match=r"add_demonstrations\(\) first"):
        vs.sample(B)
    fill_demos(vs, mo)
    left = partition_bytes(vs)
    with pytest.raises(_lib.DrqError, match="no drawable row"):
        vs.sample(B)                                                # Bd < B needs a live row
    vs.demo_fraction = 1.0                                          # ... a batch of demonstrations alone does not
    b = vs.sample(B)
    compare(got_of(vs, b), mo.sample(twin.random_sample((B, K)), B))
    assert vs.last_demo_count == B
    vs.demo_fraction = 0.5
    r = rs_(2)
    draws = 0
    for _ in range(3 * R):
        row = live_row(r)
        mo.add(*row)
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
        lo, hi = mo.live.bounds()
        assert vs.bounds() == (lo, hi)
        if hi < lo:
            with pytest.raises(_lib.DrqError, match="no drawable row"):
                vs.sample(B)
            continue
        b = vs.sample(B)
        want = mo.sample(twin.random_sample((B, K)), 4)
        compare(got_of(vs, b), want)
        assert vs.last_demo_count == 4 and torch.equal(b[0], vs.last_index[0]) and torch.equal(b[4], vs.last_index[1])
        assert b.frames.shape[0] == (R + D) * NS and b.frames.data_ptr() == vs.frames.data_ptr()
        fr = b.frames.cpu().numpy()
        assert np.array_equal(fr[want["idx"][0]], want["obs"]) and np.array_equal(fr[want["idx"][1]], want["next_obs"])
        draws += 1
    assert vs.T == 3 * R and draws >= 3 * R - NSTEP
    now = partition_bytes(vs)
    for n in NAMES:
        assert np.array_equal(now[n], left[n]), n                   # 3R live adds never reached the partition
        assert np.array_equal(getattr(vs, n).cpu().numpy(), mo.live.ring()[0][n]), n
    assert twin.random_sample() == vs.rng.random_sample()


def test_materialised_mixed_batch_is_the_oracles():
    """indexed=False: the reference's 5-tuple, its frames copied by the draw itself from the whole allocation"""
    vs = new_store(indexed=False)
    mo = M.MixedOracle(R, D, NS, AS, FBS, NSTEP, GAMMA, guard_rows=GUARD)
    fill_demos(vs, mo)
    r = rs_(4)
    for _ in range(R + 3):
        row = live_row(r)
        mo.add(*row)
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
    vs.demo_fraction = 0.4                                          # int(2.8 + 0.5) = 3
    obs, act, rew, disc, nxt = vs.sample(B)
    want = mo.sample(np.random.RandomState(21).random_sample((B, K)), 3)
    compare(dict(idx=vs.last_index, act=act, rew=rew, disc=disc, steps=vs.last_steps), want)
    assert obs.shape == (B, FBS) and rew.shape == (B, 1) and vs.last_demo_count == 3
    assert np.array_equal(obs.cpu().numpy(), want["obs"]) and np.array_equal(nxt.cpu().numpy(), want["next_obs"])


def test_update_from_a_mixed_indexed_batch_equals_update_from_it_materialised():
    """The observation shape and batch size of test_update_from_the_ring_equals_update_from_materialised_batches, the
    fraction at 0.5 (Bd = 8 of 16): parameters, Adam moments and metrics bit for bit over three updates, rows added in
    between.  The indexed batch's frames are the whole allocation, its first eight rows index the partition"""
    from drqv2_amd.replay import IndexedBatch, VecDeviceReplay
    N, A, Bu, Rr = 3, 3, 16, 16
    demos = [episode(n, A, seed=40 + n) for n in (3, 2, 4, 2)]
    outs = []
    for indexed in (False, True):
        vs = VecDeviceReplay(Rr, N, OBS, A, 3, 0.99, "cuda", seed=5, indexed=indexed, demo_rows=D)
        vs.batch_size = Bu
        assert vs.add_demonstrations(demos).rows == 6              # lanes of 4, 3 + 3 and 5 rows
        vs.demo_fraction = 0.5
        ag = make_agent(A)
        reseed()
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for t in range(12):
            vs.add(*device_row(g, N, A, ag, t))
        it = iter(vs)
        ms = []
        for u in range(3):
            ms.append(ag.update(it, 2 * u))
            assert vs.last_demo_count == 8
            for _ in range(2):
                vs.add(*device_row(g, N, A, ag, vs.T))
        b = next(it)
        assert isinstance(b, IndexedBatch) == indexed
        assert all(np.isfinite(v) for m in ms for v in m.values())
        idx = vs.last_index.cpu().numpy()
        assert (idx[:, :8] >= Rr * N).all() and (idx[:, 8:] < Rr * N).all() and int(vs.last_steps.min()) >= 1
        if indexed:
            assert b.frames.shape[0] == (Rr + D) * N and b.frames.data_ptr() == vs.frames.data_ptr()
        else:
            assert b[0].shape == (Bu,) + OBS and b[0].dtype == torch.uint8
        outs.append((ms, vs.last_steps.clone(), vs.last_index.clone()) + engine_state(ag))
    (m0, *a0), (m1, *a1) = outs
    assert m0 == m1
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)


def test_checkpoint_restores_partition_fraction_and_the_draws_that_follow(tmp_path):
    """save after some mixed draws with a look-ahead batch pending, restore into a fresh store and iterator: the pending
    batch and the next draws -- the fraction changed mid-run, rows added in between -- equal the uninterrupted store's"""
    from drqv2_amd import checkpoint
    a = new_store()
    a.batch_size = B
    fill_demos(a)
    a.demo_fraction = 0.5
    r = rs_(8)
    for _ in range(R + 2):
        a.add(*(torch.from_numpy(x).cuda() for x in live_row(r)))
    ia = iter(a)
    for _ in range(3):
        next(ia)
    ia.prefetch()                                                   # a mixed batch drawn ahead: indices into the partition
    assert a.last_demo_count == 4 and int(a.last_index.max()) >= R * NS
    path = tmp_path / "ck.pt"
    checkpoint.save(path, store=a, iterator=ia)
    b = new_store(seed=99)
    b.batch_size = B
    ib = iter(b)
    checkpoint.load(path, store=b, iterator=ib)
    assert b.demo_rows_filled == a.demo_rows_filled == 7 and b.demo_fraction == 0.5
    pa, pb = partition_bytes(a), partition_bytes(b)
    assert all(np.array_equal(pa[n], pb[n]) for n in NAMES)
    same = lambda x, y: all(torch.equal(s.view(torch.uint8), t.view(torch.uint8)) for s, t in zip(x, y))
    x, y = next(ia), next(ib)                                       # the pending batch, rebuilt over the restored store
    assert same(x, y) and y.frames.shape[0] == (R + D) * NS and torch.equal(x.frames, y.frames)
    r2 = rs_(9)
    for step, fraction in enumerate((0.5, 0.25, 0.25, 1.0, 0.0, 0.8)):
        a.demo_fraction = b.demo_fraction = fraction
        row = live_row(r2)
        a.add(*(torch.from_numpy(v).cuda() for v in row))
        b.add(*(torch.from_numpy(v).cuda() for v in row))
        x, y = next(ia), next(ib)
        assert same(x, y) and torch.equal(a.last_index, b.last_index) and torch.equal(a.last_steps, b.last_steps), step
        assert a.last_demo_count == b.last_demo_count == int(B * fraction + 0.5)
    assert a.last_demo_count == 6                                   # int(7 * 0.8 + 0.5)
