"""Step-major replay on the GPU: drq_vec_add and drq_vec_sample on poisoned, guarded memory against the numpy restatement
tests/vec_oracle.py (whose windows are oracle.nstep_sample's), and VecDeviceReplay against the episode store, through
DrQV2Agent.update() and across the guard rows.

Bounds.  Everything is compared bit for bit: slots and window lengths are integers; the candidate choice is one IEEE
double product, truncated, on both sides; action rows and frames are copies; the n-step reward / discount are the
reference's float32 operations in the reference's order, one rounding each (drq_nstep_gather's arithmetic, which
tests/test_hip_replay.py holds to the same function).  Updates fed by the same transitions through indices and through
materialised frames run the same launches on the same bytes.

Coverage, continuing the map of tests/test_hip_entries.py:
  here            vec_add, vec_sample (both with every DRQ_EARG case on refused, poisoned outputs)"""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_oracle as V
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, f32, out, p, rs_
from tests.test_hip_replay import OBS, episode

pytestmark = pytest.mark.gpu
EARG = -1
R, FB, B, K = 16, 16, 40, 4
ARRAYS = (("frames", torch.uint8), ("action", torch.float32), ("reward", torch.float32), ("discount", torch.float32),
          ("first", torch.uint8))


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_sample" in _lib.PROTOTYPES, "the step-major replay entries are missing"
    return _lib.load()


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))


def raw(t):
    """the bytes of a tensor, on the host"""
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().copy()


def store_shapes(N, A):
    return {"frames": (R * N, FB), "action": (R * N, A), "reward": (R * N,), "discount": (R * N,), "first": (R * N,)}


# ------------------------------------------------------------------------------------------------ drq_vec_add
@pytest.mark.parametrize("N,A", [(3, 2), (1, 21), (3, 21)])
def test_vec_add(lib, N, A):
    """rows t = 0 (first forced), 5 (src_first NULL: zeros), R + 2 (lands in row 2), 2R + 5 (row 5 again, overwritten):
    after every call each array is read back whole -- the row equals the sources, every other byte is what it was, for
    the slots never written the poison"""
    shapes = store_shapes(N, A)
    store = {n: poison.alloc(shapes[n], dt, "cuda", name=n, kind="ws") for n, dt in ARRAYS}
    want = {n: raw(store[n]) for n, _ in ARRAYS}
    per_slot = {"frames": FB, "action": 4 * A, "reward": 4, "discount": 4, "first": 1}
    r = rs_(N * 100 + A)
    for t, with_first in ((0, True), (5, False), (R + 2, True), (2 * R + 5, True)):
        src = {"frames": u8(r.randint(0, 256, (N, FB))), "action": f32(r.uniform(-1, 1, (N, A))),
               "reward": f32(r.standard_normal(N)), "discount": f32(r.uniform(0, 1, N)),
               "first": u8(r.randint(0, 2, N)) if t else u8(np.zeros(N))}
        d = {n: dev(src[n], "src_" + n) for n in src}
        assert lib.drq_vec_add(*(p(store[n]) for n, _ in ARRAYS), R, N, A, FB, t, p(d["frames"]), p(d["action"]),
                               p(d["reward"]), p(d["discount"]), p(d["first"]) if with_first else None, None) == 0
        if t == 0:
            src["first"] = u8(np.ones(N))
        elif not with_first:
            src["first"] = u8(np.zeros(N))
        row = t % R
        for n, _ in ARRAYS:
            w = per_slot[n] * N
            want[n][row * w:(row + 1) * w] = raw(src[n])
            assert np.array_equal(raw(store[n]), want[n]), (t, n)
    assert row == 5 and (raw(store["first"])[2 * N:3 * N] <= 1).all()
    untouched = np.ones(R, bool)
    untouched[[0, 2, 5]] = False
    assert (raw(store["first"]).reshape(R, N)[untouched] == poison.sentinel_of(torch.uint8)).all()
    assert (store["reward"].view(torch.int32).cpu().numpy().reshape(R, N)[untouched] == poison.SENTINEL).all()


def test_vec_add_refusals(lib):
    N, A = 3, 2
    shapes = store_shapes(N, A)
    store = [poison.alloc(shapes[n], dt, "cuda", name=n, kind="refused") for n, dt in ARRAYS]
    src = [dev(u8(np.zeros((N, FB))), "obs"), dev(f32(np.zeros((N, A)))), dev(f32(np.zeros(N))), dev(f32(np.ones(N))),
           dev(u8(np.zeros(N)), "first")]
    ok = [p(t) for t in store] + [R, N, A, FB, 3] + [p(t) for t in src]
    bad = []
    for k in list(range(5)) + list(range(10, 14)):                # every required pointer (src_first may be NULL)
        a = list(ok)
        a[k] = None
        bad.append(a)
    for k, v in ((5, 0), (5, -1), (6, 0), (7, 0), (8, 0), (8, 24), (8, -16), (9, -1)):   # R, N, A, frame_bytes, t
        a = list(ok)
        a[k] = v
        bad.append(a)
    a = list(ok)
    a[10] = ok[10] + 4                                            # src_obs not 16-byte aligned
    bad.append(a)
    for a in bad:
        assert lib.drq_vec_add(*a, None) == EARG, a[5:10]
    poison.check()                                                # nothing was written by a refused call
    for t in store:
        poison.forget(t)
    assert lib.drq_vec_add(*ok, None) == 0                        # the unbroken call is accepted


# ------------------------------------------------------------------------------------------------ drq_vec_sample
def scenario(N, A, nstep, gamma, T, seed, empty_only=False):
    """A ring with every case of the draw in its drawable rows lo .. hi (guard_rows 0: the kernel takes lo and hi).
    Environment m (the only one when N = 1, else 1): non-reset rows lo .. r0-1 (nstep - 1 of them: a window cut after
    every number of steps), then resets at r0, r0+1 and at hi-1, hi, so a walk from r0 goes forward over a second reset row
    to r0+2 and one from hi-1 wraps to lo; its terminal row r0-1 has discount 0.  N = 3: environment 0 is one long
    episode (reset at 7 only), environment 2 nothing but reset rows.  N = 1: single resets at r0 and hi, which leaves a
    full window among the eleven drawable rows of nstep 5.  Returns the oracle, the crafted u rows and the cases they
    must produce."""
    lo, hi = V.bounds(T, R, nstep, 0)
    m = 1 if N == 3 else 0
    r0 = lo + nstep - 1
    mid, tail = ({r0, r0 + 1}, {hi - 1, hi}) if N == 3 else ({r0}, {hi})
    v, w0 = max(mid) + 1, min(tail)                               # first valid row behind r0; where the wrapping walk starts
    assert v <= w0 - 1
    resets = {m: mid | tail}
    if N == 3:
        resets[0], resets[2] = {7}, set(range(T))
    if empty_only:
        resets = {e: set(range(T)) for e in range(N)}
    r = rs_(seed)
    vo = V.VecOracle(R, N, A, FB, nstep, gamma, guard_rows=0)
    for t in range(T):
        first = np.array([t in resets.get(e, ()) for e in range(N)], np.uint8)
        disc = np.where(r.uniform(size=N) < 0.15, 0.0, 1.0).astype(np.float32)
        if t == r0 - 1:
            disc[m] = 0.0
        vo.add(r.randint(0, 256, (N, FB)), r.uniform(-1, 1, (N, A)), r.standard_normal(N), disc, first)
    M = (hi - lo + 1) * N
    cell = lambda t, e: (((t - lo) * N + e) + 0.5) / M
    if empty_only:
        return vo, [[cell(lo + 1, 0)] * K], {"empty"}
    if N == 3:
        x, y, z = cell(lo, 2), cell(hi, 2), cell(lo + 3, 2)       # reset rows to reject
        ok = cell(lo + 1, 0)
    else:
        x, y, z = cell(r0, 0), cell(hi, 0), cell(r0, 0)
        ok = cell(v, 0)
    rows = [[ok, x, y, z], [x, ok, y, z], [x, y, ok, z], [x, y, z, ok],
            [cell(r0, m), x, y, z],                                # all reset rows: walk forward to v
            [cell(w0, m), y, x, z]]                                # ... the walk wraps to lo
    rows += [[cell(r0 - i, m)] * K for i in range(1, nstep)]                                     # cut after i steps
    need = {"accept0", "accept1", "accept2", "accept3", "walk", "walk_wrap", "full"} | {f"cut{i}" for i in range(1, nstep)}
    if N == 3:
        rows.append([cell(lo + 2, 2), x, y, z])
        need.add("empty")
    return vo, rows, need


def run_sample(lib, vo, u, materialise):
    N, A = vo.N, vo.A
    ring, _ = vo.ring()
    lo, hi = vo.bounds()
    d = {n: dev(torch.from_numpy(ring[n]), n) for n, _ in ARRAYS}
    n_rows = u.shape[0]
    o = dict(idx=out(3, n_rows, dtype=torch.int64, name="idx"), act=out(n_rows, A, name="act"), rew=out(n_rows, name="rew"),
             disc=out(n_rows, name="disc"), steps=out(n_rows, dtype=torch.int32, name="steps"))
    fr = (d["frames"], out(n_rows, FB, dtype=torch.uint8, name="obs"), out(n_rows, FB, dtype=torch.uint8, name="next_obs")) \
        if materialise else (None, None, None)
    rc = lib.drq_vec_sample(p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), R, N, A, FB, lo, hi,
                            p(dev(torch.from_numpy(u), "u")), n_rows, u.shape[1], vo.nstep, vo.gamma, p(o["idx"]), p(o["act"]),
                            p(o["rew"]), p(o["disc"]), p(o["steps"]), p(fr[0]), p(fr[1]), p(fr[2]), None)
    assert rc == 0
    torch.cuda.synchronize()
    for n, _ in ARRAYS:                                            # the draw writes nothing into the store
        assert np.array_equal(d[n].cpu().numpy(), ring[n]), n
    return o, fr, d


def compare(o, want):
    assert np.array_equal(o["idx"].cpu().numpy(), want["idx"])
    assert np.array_equal(o["steps"].cpu().numpy(), want["steps"])
    assert np.array_equal(raw(o["act"]), want["action"].view(np.uint8).reshape(-1))
    assert np.array_equal(raw(o["rew"]), want["reward"].view(np.uint8))
    assert np.array_equal(raw(o["disc"]), want["discount"].view(np.uint8))


@pytest.mark.parametrize("T", [14, 2 * R + 5])
@pytest.mark.parametrize("nstep,gamma,A", [(1, 0.99, 2), (3, 0.99, 21), (5, 0.9, 2)])
def test_vec_sample_matches_oracle_bit_for_bit(lib, nstep, gamma, A, T):
    """N = 3, before the ring wraps and after (T = 2R + 5).  The crafted rows first, random ones up to B = 40; the
    oracle's tally must name every case before anything is compared.  Then the same draw materialised: both frame
    outputs equal frames[idx], every byte, and the rest does not change"""
    vo, crafted, need = scenario(3, A, nstep, gamma, T, seed=T + nstep)
    u = np.concatenate([np.array(crafted), rs_(nstep).random_sample((B - len(crafted), K))])
    u[-1] = [0.0, 0.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 0.0)]
    want = vo.sample(u)
    assert need <= set(want["tally"]), sorted(need - set(want["tally"]))
    assert [c for c in want["tally"] if c.startswith("cut")] == [] or nstep > 1
    o, _, _ = run_sample(lib, vo, u, False)
    compare(o, want)
    om, (frames, obs, nxt), _ = run_sample(lib, vo, u, True)
    compare(om, want)
    fr = frames.cpu().numpy()
    assert np.array_equal(obs.cpu().numpy(), fr[want["idx"][0]]) and np.array_equal(nxt.cpu().numpy(), fr[want["idx"][1]])
    assert np.array_equal(obs.cpu().numpy(), want["obs"]) and np.array_equal(nxt.cpu().numpy(), want["next_obs"])


@pytest.mark.parametrize("nstep,gamma,A", [(1, 0.99, 21), (3, 0.9, 2), (5, 0.99, 2)])
def test_vec_sample_single_environment(lib, nstep, gamma, A):
    """N = 1 after the wrap: every case in the one environment; the steps = 0 row from a ring of nothing but reset rows;
    B = 300 covers a second block of the scalar part"""
    vo, crafted, need = scenario(1, A, nstep, gamma, 2 * R + 5, seed=nstep)
    u = np.concatenate([np.array(crafted), rs_(9).random_sample((300 - len(crafted), K))])
    want = vo.sample(u)
    assert need <= set(want["tally"]), sorted(need - set(want["tally"]))
    o, _, _ = run_sample(lib, vo, u, False)
    compare(o, want)
    vo, crafted, need = scenario(1, A, nstep, gamma, 2 * R + 5, seed=nstep, empty_only=True)
    u = np.array(crafted + [[0.3, 0.9, 0.1, 0.5]])
    want = vo.sample(u)
    assert set(want["tally"]) == {"empty"} and (want["steps"] == 0).all()
    om, (frames, obs, nxt), _ = run_sample(lib, vo, u, True)
    compare(om, want)
    assert (want["idx"][0] == want["idx"][2]).all() and (want["idx"][1] == want["idx"][2]).all()
    assert np.array_equal(obs.cpu().numpy(), want["obs"]) and np.array_equal(nxt.cpu().numpy(), want["next_obs"])
    assert float(om["rew"].abs().max()) == 0.0 and float(om["disc"].abs().max()) == 0.0


def test_vec_sample_refusals(lib):
    N, A, nstep = 3, 2, 3
    vo, crafted, _ = scenario(N, A, nstep, 0.99, 2 * R + 5, seed=1)
    ring, _ = vo.ring()
    lo, hi = vo.bounds()
    d = {n: dev(torch.from_numpy(ring[n]), n) for n, _ in ARRAYS}
    u = dev(torch.from_numpy(np.array(crafted[:4])), "u")
    n = 4
    ref = lambda shape, dt, name: poison.alloc(shape, dt, "cuda", name=name, kind="refused")
    outs = [ref((3, n), torch.int64, "idx"), ref((n, A), torch.float32, "act"), ref((n,), torch.float32, "rew"),
            ref((n,), torch.float32, "disc"), ref((n,), torch.int32, "steps")]
    fo = [ref((n, FB), torch.uint8, "obs"), ref((n, FB), torch.uint8, "next_obs")]
    ok = [p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), R, N, A, FB, lo, hi, p(u), n, K, nstep, 0.99] + \
        [p(t) for t in outs] + [None, None, None]
    bad = []
    for k in (0, 1, 2, 3, 10, 15, 16, 17, 18, 19):                 # every required pointer
        a = list(ok)
        a[k] = None
        bad.append(a)
    # R, N, A, B, K, nstep <= 0; frame_bytes; lo < 1; hi < lo; hi - lo + 1 + nstep > R
    for k, v in ((4, 0), (5, 0), (5, -3), (6, 0), (11, 0), (12, 0), (13, 0), (13, -1), (7, 24), (7, 0), (8, 0), (9, lo - 1),
                 (13, nstep + 1), (8, lo - 1)):
        a = list(ok)
        a[k] = v
        bad.append(a)
    assert hi - lo + 1 + nstep == R                                # so one more step or one more row is one too many
    full = [p(d["frames"]), p(fo[0]), p(fo[1])]
    for miss in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):        # some but not all of frames / obs_out / next_obs_out
        a = list(ok)
        a[20:23] = [None if i in miss else q for i, q in enumerate(full)]
        bad.append(a)
    for a in bad:
        assert lib.drq_vec_sample(*a, None) == EARG, a[4:15]
    poison.check()                                                 # nothing was written by a refused call
    for t in outs + fo:
        poison.forget(t)
    assert lib.drq_vec_sample(*ok, None) == 0 and lib.drq_vec_sample(*(ok[:20] + full), None) == 0


# ------------------------------------------------------------------------------------------------ the store
def make_agent(A):
    import drqv2
    torch.manual_seed(3)
    return drqv2.DrQV2Agent(OBS, (A,), "cuda", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, True)


def reseed():
    torch.manual_seed(11)
    torch.cuda.manual_seed_all(11)


def engine_state(ag):
    eng = ag._engine
    torch.cuda.synchronize()
    return eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()


def test_same_transitions_as_the_episode_store():
    """three environments in lockstep, episodes of 10 steps, fed whole into a DeviceReplay and row by row (numpy rows:
    the staged path) into a VecDeviceReplay.  Every transition either store draws is oracle.nstep_sample on its episode,
    bit for bit, frames included: nstep steps from the episode store and for full windows, k = last_steps where the
    episode's end cuts the window"""
    from drqv2_amd.replay import DeviceReplay, VecDeviceReplay
    from oracle import drq_oracle as O
    N, A, nstep, gamma, L, n_draw = 3, 2, 3, 0.99, 10, 24
    rp = DeviceReplay(200, OBS, A, nstep, gamma, "cuda", seed=3)
    vs = VecDeviceReplay(R, N, OBS, A, nstep, gamma, "cuda", seed=4, indexed=False)
    assert len(vs) == 0
    eps, starts, cut = {}, {}, 0
    for j in range(3):
        for e in range(N):
            eps[j, e] = episode(L, A, seed=10 * j + e)
            starts[rp.add_episode(eps[j, e])] = (j, e)
        for i in range(L + 1):
            col = lambda key: np.stack([eps[j, e][key][i] for e in range(N)])
            vs.add(col("observation"), col("action"), col("reward"), col("discount"),
                   np.full(N, i == 0) if j or i else None)
            if i % 4 != 3 or vs.T <= nstep:
                continue
            lo, hi = vs.bounds()
            assert len(vs) == (hi - lo + 1) * N
            obs, act, rew, disc, nxt = (t.cpu().numpy() for t in vs.sample(n_draw))
            steps = vs.last_steps.cpu().numpy()
            assert obs.shape == (n_draw,) + OBS and rew.shape == (n_draw, 1) and act.shape == (n_draw, A)
            for b, s in enumerate(vs.last_index[2].tolist()):
                e, k = s % N, int(steps[b])
                t = next(t for t in range(lo, hi + 1) if t % R == s // N)      # fewer than R drawable rows: one match
                assert 1 <= k <= nstep
                ep, idx = eps[t // (L + 1), e], t % (L + 1)
                assert idx >= 1 and k == min(nstep, L - idx + 1)
                cut += k < nstep
                o, a, r, d, n = O.nstep_sample(ep, idx, k, gamma)
                assert np.array_equal(obs[b], o) and np.array_equal(nxt[b], n) and np.array_equal(act[b], a)
                assert rew[b, 0].tobytes() == r[0].tobytes() and disc[b, 0].tobytes() == d[0].tobytes(), (b, t, e, k)
    assert cut > 0
    pos = rp.draw_positions(48)
    obs, act, rew, disc, nxt = (t.cpu().numpy() for t in rp.gather(pos))
    for b, q in enumerate(pos.tolist()):
        s = max(x for x in starts if x <= q)
        o, a, r, d, n = O.nstep_sample(eps[starts[s]], q - s, nstep, gamma)
        assert np.array_equal(obs[b], o) and np.array_equal(nxt[b], n) and np.array_equal(act[b], a)
        assert rew[b, 0].tobytes() == r[0].tobytes() and disc[b, 0].tobytes() == d[0].tobytes()


def device_row(g, N, A, ag, t, reset_every=6):
    """one row of device tensors; the action comes out of act_batch and never leaves the device"""
    obs = torch.randint(0, 256, (N,) + OBS, dtype=torch.uint8, device="cuda", generator=g)
    action = ag.act_batch(obs, t, False)
    assert action.is_cuda and action.shape == (N, A) and action.dtype == torch.float32
    reward = torch.randn(N, device="cuda", generator=g)
    discount = torch.ones(N, 1, device="cuda")
    first = (torch.arange(N, device="cuda") + t) % reset_every == 0
    return obs, action, reward, discount, first


def test_update_from_the_ring_equals_update_from_materialised_batches():
    """IndexedBatch from the ring through DrQV2Agent.update() against the same draws materialised (indexed=False, same
    seed): parameters, Adam moments and metrics bit for bit over three updates, rows added from device tensors in
    between (the iterator has drawn one batch ahead by then)"""
    from drqv2_amd.replay import IndexedBatch, VecDeviceReplay
    N, A, Bu = 3, 3, 16
    outs = []
    for indexed in (False, True):
        vs = VecDeviceReplay(R, N, OBS, A, 3, 0.99, "cuda", seed=5, indexed=indexed)
        vs.batch_size = Bu
        ag = make_agent(A)
        reseed()
        g = torch.Generator(device="cuda")
        g.manual_seed(7)
        for t in range(12):
            row = device_row(g, N, A, ag, t)
            vs.add(*row)
        torch.cuda.synchronize()
        s = (vs.T - 1) % R * N
        assert torch.equal(vs.action[s:s + N], row[1]) and torch.equal(vs.frames[s:s + N], row[0].view(N, -1))
        assert vs.first[s:s + N].tolist() == row[4].to(torch.uint8).tolist() and vs.first[:N].tolist() == [1] * N
        it = iter(vs)
        ms = []
        for u in range(3):
            ms.append(ag.update(it, 2 * u))
            for _ in range(2):
                vs.add(*device_row(g, N, A, ag, vs.T))
        b = next(it)
        assert isinstance(b, IndexedBatch) == indexed and vs.last_steps.shape == (Bu,)
        assert all(np.isfinite(v) for m in ms for v in m.values())
        if indexed:
            assert b.frames is vs.frames and b[0].dtype == torch.int64 and b[1].shape == (Bu, A) and b[2].shape == (Bu, 1)
        else:
            assert b[0].shape == (Bu,) + OBS and b[0].dtype == torch.uint8
        outs.append((ms, vs.last_steps.clone()) + engine_state(ag))
    (m0, *a0), (m1, *a1) = outs
    assert m0 == m1
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)


def test_guard_rows_keep_a_batch_drawn_ahead_valid():
    """a batch drawn through the iterator's prefetch(), then guard_rows - 1 rows of other data: the frames at its indices
    have not changed and the update it feeds is, bit for bit, the update taken before the adds"""
    from drqv2_amd.replay import VecDeviceReplay
    N, A = 3, 3
    vs = VecDeviceReplay(R, N, OBS, A, 3, 0.99, "cuda", seed=8)
    assert vs.guard_rows == 8
    vs.batch_size = 16
    feeder = make_agent(A)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for t in range(R + 5):                                         # wrapped: the next rows overwrite old ones
        vs.add(*device_row(g, N, A, feeder, t))
    it = iter(vs)
    it.prefetch()
    b = it._ahead
    before = vs.frames[b[0]].clone(), vs.frames[b[4]].clone()
    ring_before = vs.frames.clone()
    early = make_agent(A)
    reseed()
    m_early = early.update(iter([b]), 0)
    for _ in range(vs.guard_rows - 1):
        vs.add(*device_row(g, N, A, feeder, vs.T))
    torch.cuda.synchronize()
    assert int((vs.frames != ring_before).any(1).sum()) == (vs.guard_rows - 1) * N       # the adds did overwrite rows
    assert torch.equal(vs.frames[b[0]], before[0]) and torch.equal(vs.frames[b[4]], before[1])
    late = make_agent(A)
    reseed()
    m_late = late.update(it, 0)                                    # hands out b, the batch drawn ahead
    assert m_early == m_late and len(m_late) == 8
    for x, y in zip(engine_state(early), engine_state(late)):
        assert torch.equal(x, y)


def test_store_draws_equal_the_oracle_across_wraps():
    """50 draws while the ring wraps three times, rows from device tensors with random resets: the store's batches are
    the oracle's for the same seed (u = one random_sample((B, K)) per batch), bit for bit, and no drawn row lies outside
    [lo, hi]; before nstep + 1 rows exist sample() refuses"""
    from drqv2_amd import _lib
    from drqv2_amd.replay import VecDeviceReplay
    N, A, nstep, gamma = 3, 2, 3, 0.9
    vs = VecDeviceReplay(R, N, (FB,), A, nstep, gamma, "cuda", seed=21)
    vo = V.VecOracle(R, N, A, FB, nstep, gamma, guard_rows=8)
    twin = np.random.RandomState(21)
    r = rs_(2)
    draws = 0
    while draws < 50:
        row = (r.randint(0, 256, (N, FB)).astype(np.uint8), r.uniform(-1, 1, (N, A)).astype(np.float32),
               r.standard_normal(N).astype(np.float32), np.where(r.uniform(size=N) < 0.1, 0.0, 1.0).astype(np.float32),
               r.uniform(size=N) < 0.2)
        vo.add(*row)
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
        lo, hi = vo.bounds()
        assert vs.bounds() == (lo, hi) and vs.T == vo.T
        if hi < lo:
            assert vs.T <= nstep and len(vs) == 0
            with pytest.raises(_lib.DrqError, match="no drawable row"):
                vs.sample(B)
            continue
        assert len(vs) == (hi - lo + 1) * N
        b = vs.sample(B)
        want = vo.sample(twin.random_sample((B, K)))
        got = dict(idx=vs.last_index, act=b[1], rew=b[2], disc=b[3], steps=vs.last_steps)
        assert torch.equal(b[0], vs.last_index[0]) and torch.equal(b[4], vs.last_index[1]) and b.frames is vs.frames
        compare(got, want)
        for t, e in want["rows"]:
            assert lo <= t <= hi
        draws += 1
    assert vs.T >= 3 * R
    ring, _ = vo.ring()
    for n, _ in ARRAYS:
        assert np.array_equal(getattr(vs, n).cpu().numpy(), ring[n]), n
