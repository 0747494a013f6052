"""Single frames in the episode store on the GPU: drq_nstep_gather_frames on poisoned, guarded memory against the slot rule
and the frame-stack simulator of tests/episode_frames_oracle.py and against drq_nstep_gather, DeviceReplay(single_frames=
True) against the stacked DeviceReplay fed the same episodes -- draw by draw, through DrQV2Agent.update() and through
replay_buffer.make_replay_loader.

Bounds.  Everything is compared bit for bit.  The gather copies bytes.  Its scalars are drq_nstep_gather's operations on
the same operands in the same order (one shared device function).  The two stores place, evict and draw by the same host
code from the same RandomState, so they name the same positions; the fused aug+conv1 launch runs the same instructions
on the same bytes whichever way its source addresses were found, and so does every launch behind it.

Coverage, continuing the map of tests/test_hip_entries.py:
  here            nstep_gather_frames (with every DRQ_EARG case on refused, poisoned outputs)"""
import numpy as np
import pytest
import torch

from tests import episode_frames_oracle as EF
from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p, rs_
from tests.test_hip_vec_replay import engine_state, make_agent, reseed

pytestmark = pytest.mark.gpu
EARG = -1
OBS = (9, 84, 84)
R = 23


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_nstep_gather_frames" in _lib.PROTOTYPES, "the single-frame episode store's entry is missing"
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the kernel
_layouts = {}


def layout(fb, A):
    """a store of R = 23 slots after a wrap: episodes [start, steps] (0, 4), (6, 2), (8, 3), (11, 5), (16, 7) live --
    one at slot 0, one that ends on slot R - 1 -- and slots 4, 5 stale: frames and flags of the evicted episode (0, 6).
    Built once per shape and left unchanged"""
    if (fb, A) not in _layouts:
        r = rs_(fb + A)
        shape = {48: (3, 4, 4), 21168: (3, 84, 84)}[fb]
        lay = EF.Layout(R, A, shape, seed=5)
        for n in (6, 2, 3, 5, 7, 4):
            lay.add(EF.episode(r, n, A, shape))
        assert lay.episodes == [[6, 2], [8, 3], [11, 5], [16, 7], [0, 4]] and lay.first[0] == 1
        _layouts[fb, A] = lay
    return _layouts[fb, A]


def run_frames(lib, d, lay, pos, nstep, fb, A, frames=True):
    """one launch on poisoned outputs -> (obs, act, rew, disc, next_obs) as numpy, floats as their int32 bits"""
    B = len(pos)
    u8 = lambda: poison.alloc((B, 3 * fb), torch.uint8, "cuda", name="stacks") if frames else None
    f = lambda *sh: poison.partial(poison.alloc(sh, torch.float32, "cuda", name="scalars"))
    obs, act, rew, disc, nxt = u8(), f(B, A), f(B), f(B), u8()
    d_pos = dev(torch.tensor(pos, dtype=torch.int64), "pos")
    assert lib.drq_nstep_gather_frames(p(d["frames"]), p(d["first"]), R, p(d["action"]), p(d["reward"]), p(d["discount"]),
                                       p(d_pos), B, A, fb, nstep, 0.99, p(obs), p(act), p(rew), p(disc), p(nxt), None) == 0
    bits = lambda t: t.view(torch.int32).cpu().numpy()
    return (obs.cpu().numpy() if frames else None, bits(act), bits(rew), bits(disc), nxt.cpu().numpy() if frames else None)


def run_stacked(lib, d, pos, nstep, fb, A):
    """drq_nstep_gather's scalars for the same positions (all of them inside the store)"""
    B = len(pos)
    f = lambda *sh: poison.alloc(sh, torch.float32, "cuda", name="ref")
    act, rew, disc = f(B, A), f(B), f(B)
    d_pos = dev(torch.tensor(pos, dtype=torch.int64), "pos")
    assert lib.drq_nstep_gather(p(d["frames"]), p(d["action"]), p(d["reward"]), p(d["discount"]), p(d_pos), B, A, fb, nstep,
                                0.99, None, p(act), p(rew), p(disc), None, None) == 0
    return tuple(t.view(torch.int32).cpu().numpy() for t in (act, rew, disc))


@pytest.mark.parametrize("B", [1, 5, 7])
@pytest.mark.parametrize("nstep", [1, 3])
@pytest.mark.parametrize("A", [1, 6])
@pytest.mark.parametrize("fb", [48, 21168])
def test_kernel_matches_the_simulator_and_nstep_gather(lib, fb, A, nstep, B):
    """every drawable position of the layout and positions outside the store, B rows per launch: the stacks are the
    simulator's observations (and the rule's bytes), action / reward / discount the bits of drq_nstep_gather, rows of
    positions outside [1, R - nstep] stay poison; the store sits between guard bands and is unchanged"""
    lay = layout(fb, A)
    good = lay.drawable(nstep)
    # start+1 (the obs stack is the reset stack), start+2, start+3, the last drawable position of the episode that ends
    # on slot R-1, the episode at slot 0
    assert {17, 18, 19, R - nstep, 1} <= set(good) and (nstep == 3 or {7, 9, 10} <= set(good))
    bad = [0, -1, R - nstep + 1, R, R + 5, 2 ** 62, -2 ** 62]
    order = rs_(B).permutation(len(good) + len(bad)).tolist()
    pos = [(good + bad)[i] for i in order]
    pos += good[:(-len(pos)) % B]
    d = {k: dev(torch.from_numpy(getattr(lay, k)), k) for k in ("frames", "first", "action", "reward", "discount")}
    sent8, sent32 = poison.sentinel_of(torch.uint8), np.int32(poison.sentinel_of(torch.float32))
    seen_bad = 0
    for c in range(0, len(pos), B):
        chunk = pos[c:c + B]
        obs, act, rew, disc, nxt = run_frames(lib, d, lay, chunk, nstep, fb, A)
        ok = [i for i, q in enumerate(chunk) if 1 <= q <= R - nstep]
        if ok:
            ract, rrew, rdisc = run_stacked(lib, d, [chunk[i] for i in ok], nstep, fb, A)
        for j, i in enumerate(ok):
            q = chunk[i]
            assert np.array_equal(obs[i], lay.stacked[q - 1]) and np.array_equal(nxt[i], lay.stacked[q + nstep - 1]), q
            assert np.array_equal(obs[i], EF.stack_at(lay.frames, lay.first, q - 1)), q
            assert np.array_equal(act[i], ract[j]) and rew[i] == rrew[j] and disc[i] == rdisc[j], q
            assert np.array_equal(act[i].view(np.float32), lay.action[q])
        for i in set(range(len(chunk))) - set(ok):
            assert (obs[i] == sent8).all() and (nxt[i] == sent8).all(), chunk[i]
            assert (act[i] == sent32).all() and rew[i] == sent32 and disc[i] == sent32, chunk[i]
            seen_bad += 1
    assert seen_bad == len(bad)
    # the scalars alone: obs == next_obs == NULL
    chunk = pos[:B]
    _, act, rew, disc, _ = run_frames(lib, d, lay, chunk, nstep, fb, A, frames=False)
    ok = [i for i, q in enumerate(chunk) if 1 <= q <= R - nstep]
    if ok:
        ract, rrew, rdisc = run_stacked(lib, d, [chunk[i] for i in ok], nstep, fb, A)
        assert np.array_equal(act[ok], ract) and np.array_equal(rew[ok], rrew) and np.array_equal(disc[ok], rdisc)
    for i in set(range(len(chunk))) - set(ok):
        assert (act[i] == sent32).all() and rew[i] == sent32 and disc[i] == sent32
    torch.cuda.synchronize()
    for k, t in d.items():
        assert np.array_equal(t.cpu().numpy(), getattr(lay, k)), k


def test_kernel_reads_in_range_for_any_flags(lib):
    """no flag pattern takes a read outside the store: all flags 0 (every stack reaches two slots back, around slot 0) and
    all 1, between guard bands of NaN poison"""
    fb, A, nstep = 48, 2, 2
    lay = layout(fb, 1)
    arr = {"frames": lay.frames, "action": rs_(0).uniform(-1, 1, (R, A)).astype(np.float32), "reward": lay.reward,
           "discount": lay.discount}
    pos = list(range(1, R - nstep + 1))
    for flag in (0, 1):
        first = np.full(R, flag, np.uint8)
        d = {k: dev(torch.from_numpy(v), k) for k, v in dict(arr, first=first).items()}
        obs, act, rew, disc, nxt = run_frames(lib, d, lay, pos, nstep, fb, A)
        for i, q in enumerate(pos):
            assert np.array_equal(obs[i], EF.stack_at(lay.frames, first, q - 1)), (flag, q)
            assert np.array_equal(nxt[i], EF.stack_at(lay.frames, first, q + nstep - 1)), (flag, q)
    assert EF.stack_slots(np.zeros(R, np.uint8), 0) == (R - 2, R - 1, 0)


def test_kernel_refusals(lib):
    fb, A, B, nstep = 48, 2, 4, 3
    z = lambda *sh, dt=torch.float32: dev(torch.zeros(sh, dtype=dt))
    frames, first = z(R, fb, dt=torch.uint8), z(R, dt=torch.uint8)
    action, reward, discount = z(R, A), z(R), z(R)
    pos = dev(torch.arange(1, B + 1, dtype=torch.int64), "pos")
    ref = lambda sh, dt: poison.alloc(sh, dt, "cuda", name="out", kind="refused")
    obs, nxt = ref((B, 3 * fb), torch.uint8), ref((B, 3 * fb), torch.uint8)
    act, rew, disc = ref((B, A), torch.float32), ref((B,), torch.float32), ref((B,), torch.float32)
    ok = [p(frames), p(first), R, p(action), p(reward), p(discount), p(pos), B, A, fb, nstep, 0.99, p(obs), p(act), p(rew),
          p(disc), p(nxt)]
    bad = []
    for k in (0, 1, 3, 4, 5, 6, 12, 13, 14, 15, 16):              # every pointer; obs or next_obs alone is one too
        bad.append(ok[:k] + [None] + ok[k + 1:])
    for k, v in ((2, 0), (2, -1), (7, 0), (7, -1), (8, 0), (8, -1), (9, 0), (9, 24), (9, -16), (10, 0), (10, -1)):
        bad.append(ok[:k] + [v] + ok[k + 1:])                      # R, B, A, frame_bytes, nstep
    for k, off in ((0, 4), (12, 8), (16, 8), (6, 4), (3, 2), (4, 2), (5, 2), (13, 2), (14, 2), (15, 2)):
        bad.append(ok[:k] + [ok[k] + off] + ok[k + 1:])            # misaligned
    for a in bad:
        assert lib.drq_nstep_gather_frames(*a, None) == EARG, a[2:12]
    poison.check()                                                 # nothing was written by a refused call
    for t in (obs, nxt, act, rew, disc):
        poison.forget(t)
    assert lib.drq_nstep_gather_frames(*ok, None) == 0
    assert lib.drq_nstep_gather_frames(*(ok[:12] + [None] + ok[13:16] + [None]), None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ store against store
CAP, SA, NSTEP = 40, 3, 3
LENS = (9, 5, 12, NSTEP + 1, 2, 11, 8, 13, 6, 3, 14, 7, 10, 9)      # 40 slots: wraps after the fifth, three times in all

_episodes = {}


def episodes(seed=1):
    if seed not in _episodes:
        r = rs_(seed)
        _episodes[seed] = [EF.episode(r, n, SA) for n in LENS]
    return _episodes[seed]


def two_stores(mode, seed=9):
    from drqv2_amd.replay import DeviceReplay
    kw = dict(priority_alpha=0.6) if mode.startswith("per") else {}
    kw["indexed"] = not mode.endswith("materialised")
    mk = lambda **k: DeviceReplay(CAP, OBS, SA, NSTEP, 0.99, "cuda", seed=seed, **kw, **k)
    return mk(single_frames=True), mk()


def feed(sf, sd, ep, k):
    """the stacked store takes the stacked episode; the single-frame store stacked and single-frame input in turn"""
    e = EF.npz_fields(ep)
    assert sd.add_episode(e) == sf.add_episode(dict(e, observation=ep["frames"]) if k % 2 else e)


@pytest.mark.parametrize("mode", ["uniform", "per", "materialised", "per-materialised"])
def test_store_draws_equal_the_stacked_store(mode):
    """two DeviceReplays, same seed, same simulated episodes, 40 slots (episodes wrap and evict), two draws after every
    add: positions, action, reward, discount and the materialised obs / next_obs bit for bit; prioritized: positions and
    weights before and after a round of update_priorities, and the trees"""
    from drqv2_amd.replay import FrameBatch, IndexedBatch, PrioritizedBatch
    sf, sd = two_stores(mode)
    assert sf.frames.shape == (CAP, 21168) and sd.frames.shape == (CAP, 63504) and sf.first.is_cuda
    B, r, wrapped = 24, rs_(3), 0
    for k, ep in enumerate(episodes()):
        head = sf._head
        feed(sf, sd, ep, k)
        wrapped += sf._head <= head
        assert sf.episodes == sd.episodes and len(sf) == len(sd) and sf._head == sd._head
        if not any(n - 1 >= NSTEP for _, n in sf.episodes):
            continue
        for rnd in range(2):
            bf, bd = sf.sample(B), sd.sample(B)
            if mode.endswith("materialised"):
                mf, md = bf, bd
                assert isinstance(mf, tuple) and not hasattr(mf, "frames")
                assert mf[0].shape == (B,) + OBS and mf[0].dtype == torch.uint8 and mf[2].shape == (B, 1)
            else:
                assert isinstance(bf, FrameBatch) and bf.frames is sf.frames and bf.ring == (sf.first, CAP, 1)
                assert isinstance(bd, IndexedBatch) and not hasattr(bd, "ring")
                assert torch.equal(bf[0], bd[0]) and torch.equal(bf[4], bd[4])
                mf, md = bf.materialize(OBS), bd.materialize(OBS)
            for j in (1, 2, 3):
                assert torch.equal(mf[j].view(torch.int32), md[j].view(torch.int32)), (k, j)
            assert torch.equal(mf[0], md[0]) and torch.equal(mf[4], md[4]), k
            if mode.startswith("per"):
                assert isinstance(bf, PrioritizedBatch) and isinstance(bd, PrioritizedBatch)
                assert torch.equal(bf._pos, bd._pos)
                assert torch.equal(bf.weights.view(torch.int32), bd.weights.view(torch.int32))
                td = torch.from_numpy(r.exponential(size=B).astype(np.float32)).cuda()
                bf.update_priorities(td)
                bd.update_priorities(td)
                assert torch.equal(sf.tree, sd.tree)
    assert wrapped == 3 and sf._placements == len(LENS)
    lay = EF.Layout(CAP, SA)                                       # ... and the store holds what the restatement holds
    for ep in episodes():
        lay.add(ep)
    assert sf.episodes == lay.episodes
    live = lay.live_slots()
    assert np.array_equal(sf.first.cpu().numpy()[live], lay.first[live])
    assert np.array_equal(sf.frames.cpu().numpy()[live], lay.frames[live])
    if mode.startswith("per"):
        assert float(bf.weights.min()) < 1.0                       # the priorities did shape the draw


# ------------------------------------------------------------------------------------------------ the whole update
@pytest.mark.parametrize("mode,dtype", [("uniform", "fp32"), ("per", "fp32"), ("uniform", "bf16")])
def test_update_from_single_frames_equals_update_from_stacks(mode, dtype):
    """two agents, same seed, two update() calls fed by the two stores' iterators (one batch drawn ahead), on stores that
    have wrapped and evicted: every parameter, Adam moment and metric bit for bit, and the trees of the prioritized
    stores"""
    outs = []
    for which in (0, 1):
        sf, sd = two_stores(mode, seed=5)
        store = (sf, sd)[which]
        store.batch_size = 16
        ag = make_agent(SA)
        ag.set_compute_dtype(dtype)
        reseed()
        for k, ep in enumerate(episodes(2)[:8]):
            feed(sf, sd, ep, k)
        it = iter(store)
        ms = [ag.update(it, 2 * u) for u in range(2)]
        assert all(np.isfinite(v) for m in ms for v in m.values()) and len(ms[0]) == 8
        tree = store.tree.clone() if mode == "per" else torch.zeros(1)
        outs.append((ms, tree) + engine_state(ag))
    (m0, *a0), (m1, *a1) = outs
    assert m0 == m1
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)
    if mode == "per":
        leaves = a0[0][a0[0].numel() // 2:]
        assert int(((leaves > 0) & (leaves != 1.0)).sum()) > 0     # the updates' errors did reach the tree


# ------------------------------------------------------------------------------------------------ the loader
def test_loader_yields_the_default_loaders_batches(tmp_path):
    """make_replay_loader(single_frames=True) over a directory of stacked .npz episodes, as the reference's storage writes
    them, against the default loader with the same seed; an episode that is no frame stack is skipped like an unreadable
    file unless check_stacks is off"""
    import replay_buffer as rb
    eps = episodes()[:6]
    dirs = []
    for name in ("stacked", "single", "loose"):
        d = tmp_path / name
        d.mkdir()
        for i, ep in enumerate(eps):
            rb.save_episode(EF.npz_fields(ep), d / f"20240101T0000{i:02d}_{i}_{ep['frames'].shape[0] - 1}.npz")
        dirs.append(d)
    kw = dict(device="cuda", obs_shape=OBS, action_dim=SA, seed=4)
    l0 = rb.make_replay_loader(dirs[0], 60, 16, 0, False, NSTEP, 0.99, **kw)
    l1 = rb.make_replay_loader(dirs[1], 60, 16, 0, False, NSTEP, 0.99, single_frames=True, **kw)
    s0, s1 = l0._store, l1._store
    assert s1.single_frames and s1.check_stacks and not s0.single_frames and s1.frames.shape[1] * 3 == s0.frames.shape[1]
    assert s0.episodes == s1.episodes and len(s0.episodes) == 6
    i0, i1 = iter(l0), iter(l1)
    for _ in range(3):
        b0, b1 = next(i0), next(i1)
        assert len(b0) == len(b1) == 5 and b1[0].shape == (16,) + OBS
        for x, y in zip(b0, b1):
            assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    # indexed through the loader: a FrameBatch; its stacks are the default loader's frames
    from drqv2_amd.replay import FrameBatch
    broken = EF.npz_fields(eps[2])
    broken["observation"] = broken["observation"].copy()
    broken["observation"][3, 1, 5, 5] ^= 1
    rb.save_episode(broken, dirs[2] / "20240101T000002_2_11.npz")
    l2 = rb.make_replay_loader(dirs[2], 60, 16, 0, False, NSTEP, 0.99, single_frames=True, indexed=True, **kw)
    assert len(l2._store.episodes) == 5
    l3 = rb.make_replay_loader(dirs[2], 60, 16, 0, False, NSTEP, 0.99, single_frames=True, check_stacks=False, indexed=True,
                               **kw)
    assert len(l3._store.episodes) == 6 and not l3._store.check_stacks
    bi = next(iter(l3))
    assert isinstance(bi, FrameBatch) and bi.ring == (l3._store.first, l3._store.capacity, 1)
    rb._REGISTRY.clear()
