"""Single-frame step-major replay on the GPU: drq_vec_stack_gather on poisoned, guarded memory against the restatement of
the reference's FrameStackWrapper (tests/vec_frames_oracle.py), drq_conv1_aug_fwd_frames against drq_conv1_aug_fwd on the
gathered stacks, and VecFrameReplay against a VecDeviceReplay fed the oracle's stacks -- draw by draw and through
DrQV2Agent.update().

Bounds.  Everything is compared bit for bit.  The gather copies bytes.  The fused launch runs the same instructions on
the same bytes whichever way its source addresses were found, and so does every launch behind it.  The two stores
compute the same bounds (guard_rows against guard_rows + 2), consume the same random numbers and hold the same flags,
actions, rewards and discounts, so their draws, windows, n-step sums, trees and weights are the same operations on the
same operands.

Coverage, continuing the map of tests/test_hip_entries.py:
  here            vec_stack_gather (with every DRQ_EARG case on refused, poisoned outputs), conv1_aug_fwd_frames,
                  conv1_aug_fwd_frames_bf16, update_phase_frames (through update())"""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_frames_oracle as VF
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, f32, p, rnd, rs_
from tests.test_hip_vec_replay import engine_state, make_agent, reseed

pytestmark = pytest.mark.gpu
EARG = -1
OBS, FRAME, FB = (9, 84, 84), (3, 84, 84), 3 * 84 * 84


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_stack_gather" in _lib.PROTOTYPES, "the single-frame replay entries are missing"
    return _lib.load()


@pytest.fixture(scope="module")
def ops():
    from drqv2_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ the streams
GR, GN, GT = 12, 3, 30      # the gather's ring: wraps twice, N odd
# environment 0: never reset after row 0.  environment 1: resets on the consecutive rows 20 and 21 -- row 22 has a reset
# one row back, row 23 two rows back -- and on 3 and 4 for the ring before it wraps.  environment 2: a reset on row 24,
# ring row 0, the row just after the second wrap, and on 12, the one after the first; and on 5
GATHER_RESETS = {1: {3, 4, 20, 21}, 2: {5, 12, 24}}


def gather_stream(T, fb_shape=FRAME, seed=0):
    r = rs_(seed)
    fs = VF.FrameStream(GR, GN)
    for t in range(T):
        fs.add(r.randint(0, 256, (GN,) + fb_shape), [t in GATHER_RESETS.get(e, ()) for e in range(GN)])
    return fs


def store_stream(R, N, T, seed):
    """rows for the two stores: single frames, flags, actions, rewards, discounts.  Environment 0 is never reset,
    environment e > 0 every 5 + e rows and once on two consecutive rows: no environment goes without a non-reset row
    for more than two rows, and row 1 is none"""
    r = rs_(seed)
    fs = VF.FrameStream(R, N)
    rows = []
    for t in range(T):
        first = np.array([e > 0 and (t % (5 + e) == e + 2 or t == 17 + e or t == 18 + e) for e in range(N)])
        frame = r.randint(0, 256, (N,) + FRAME).astype(np.uint8)
        fs.add(frame, first)
        rows.append((frame, r.uniform(-1, 1, (N, 3)).astype(np.float32), r.standard_normal(N).astype(np.float32),
                     np.where(r.uniform(size=N) < 0.1, 0.0, 1.0).astype(np.float32), first))
    return fs, rows


# ------------------------------------------------------------------------------------------------ drq_vec_stack_gather
@pytest.mark.parametrize("T", [2, 7, 14, GT])
@pytest.mark.parametrize("shape", [FRAME, (3, 4, 4)])
def test_stack_gather_matches_the_frame_stack_wrapper(lib, ops, T, shape):
    """every row whose stack is still in the ring, through the slot list (shuffled, with repeats) and through the row
    form; T = 2 and 7: before the ring wraps (row 0 is a reset row: nothing below it is addressed), 14: wrapped once,
    30: twice.  The ring sits between guard bands, the output is poisoned"""
    fs = gather_stream(T, shape)
    fb = int(np.prod(shape))
    frames, first = fs.ring()
    if T == GT:                                                    # the schedule holds what it is meant to hold
        f = np.array(fs.first)
        assert not f[1:, 0].any() and f[20, 1] and f[21, 1] and not f[22, 1] and not f[23, 1] and f[24, 2] and 24 % GR == 0
    rows = [t for t in range(max(0, T - GR + 2), T)]              # rows t-2 .. t are distinct ring rows still held
    if T <= GR:
        rows = list(range(T))
    d_frames, d_first = dev(torch.from_numpy(frames), "frames"), dev(torch.from_numpy(first), "first")
    pairs = [(t, e) for t in rows for e in range(GN)]
    order = rs_(T).permutation(len(pairs)).tolist() + [0, len(pairs) - 1, 0]
    slots = torch.tensor([(pairs[i][0] % GR) * GN + pairs[i][1] for i in order], dtype=torch.int64)
    got = ops.vec_stack_gather(d_frames, d_first, GR, GN, dev(slots, "slots"))
    want = np.stack([fs.stacks[pairs[i][0]][pairs[i][1]].reshape(-1) for i in order])
    assert got.shape == (len(order), 3 * fb) and np.array_equal(got.cpu().numpy(), want)
    cases = {len(set(VF.stack_slots(first, GR, GN, int(s)))) for s in slots.tolist()}
    assert cases == ({1, 2, 3} if T > 2 else {1, 2})
    for t in {rows[0], rows[-1], T - 1} | ({24} if T == GT else set()):
        got = ops.vec_stack_gather(d_frames, d_first, GR, GN, None, t)
        assert np.array_equal(got.cpu().numpy(), fs.stacks[t].reshape(GN, -1)), t
    torch.cuda.synchronize()
    assert np.array_equal(d_frames.cpu().numpy(), frames) and np.array_equal(d_first.cpu().numpy(), first)


def test_stack_gather_reads_in_range_for_any_flags(lib, ops):
    """no flag pattern takes a read outside the ring: all flags 0 (every stack reaches two rows back, around the ring's
    start) and all 1, on a ring between guard bands of NaN poison; a slot outside the ring writes nothing"""
    r = rs_(5)
    frames = r.randint(0, 256, (GR * GN, 48)).astype(np.uint8)
    d_frames = dev(torch.from_numpy(frames), "frames")
    slots = torch.arange(GR * GN, dtype=torch.int64)
    for flag in (0, 1):
        first = np.full(GR * GN, flag, np.uint8)
        got = ops.vec_stack_gather(d_frames, dev(torch.from_numpy(first), "first"), GR, GN, dev(slots, "slots")).cpu().numpy()
        want = np.stack([np.concatenate([frames[q] for q in VF.stack_slots(first, GR, GN, s)]) for s in range(GR * GN)])
        assert np.array_equal(got, want)
    bad = torch.tensor([0, -1, GR * GN, 5], dtype=torch.int64)
    out = poison.alloc((4, 3 * 48), torch.uint8, "cuda", name="out")
    assert lib.drq_vec_stack_gather(p(d_frames), p(dev(torch.from_numpy(first), "first")), GR, GN, 48, p(dev(bad, "bad")), 0, 4,
                                    p(out), None) == 0
    got = out.cpu().numpy()
    assert (got[1:3] == poison.sentinel_of(torch.uint8)).all() and np.array_equal(got[3], np.tile(frames[5], 3))


def test_stack_gather_refusals(lib):
    fb, n = 48, 4
    frames = dev(torch.zeros((GR * GN, fb), dtype=torch.uint8), "frames")
    first = dev(torch.ones(GR * GN, dtype=torch.uint8), "first")
    slots = dev(torch.arange(n, dtype=torch.int64), "slots")
    out = poison.alloc((n, 3 * fb), torch.uint8, "cuda", name="out", kind="refused")
    ok = [p(frames), p(first), GR, GN, fb, p(slots), 0, n, p(out)]
    bad = []
    for k in (0, 1, 8):                                            # every required pointer
        bad.append(ok[:k] + [None] + ok[k + 1:])
    for k, v in ((2, 0), (2, -1), (3, 0), (3, -2), (4, 0), (4, 24), (4, -16), (7, 0), (7, -1)):   # R, N, frame_bytes, n
        bad.append(ok[:k] + [v] + ok[k + 1:])
    bad.append([ok[0] + 4] + ok[1:])                               # frames / out not 16-byte aligned
    bad.append(ok[:8] + [ok[8] + 8])
    bad.append(ok[:5] + [ok[5] + 4] + ok[6:])                      # slots not 8-byte aligned
    row = ok[:5] + [None, 3, GN, ok[8]]
    bad.append(row[:6] + [-1] + row[7:])                           # the row form: t < 0, n != N
    bad.append(row[:7] + [GN - 1] + row[8:])
    bad.append(row[:7] + [GN + 1] + row[8:])
    for a in bad:
        assert lib.drq_vec_stack_gather(*a, None) == EARG, a[2:8]
    poison.check()                                                 # nothing was written by a refused call
    poison.forget(out)
    assert lib.drq_vec_stack_gather(*ok, None) == 0 and lib.drq_vec_stack_gather(*row, None) == 0


# ------------------------------------------------------------------------------------------------ fused aug + conv1
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n", [3, 5])
def test_fused_aug_conv1_gathers_stacks_bit_for_bit(ops, n, bf16):
    """drq_conv1_aug_fwd_frames(_bf16) on the ring against drq_conv1_aug_fwd(_bf16) on the stacks drq_vec_stack_gather
    produces: y and the stored encoder input, every bit; n_store = n.  The indices of each view meet all three cases of
    the rule, among them the stacks that reach around the ring's start"""
    fs = gather_stream(GT)
    frames, first = fs.ring()
    slot = lambda t, e: (t % GR) * GN + e
    picks = [slot(21, 1), slot(22, 1), slot(25, 0), slot(24, 2), slot(26, 2)]       # 1, 2, 3 slots; 1; 3 across the wrap
    picks1 = [slot(29, 0), slot(21, 1), slot(25, 2), slot(23, 1), slot(20, 1)]      # 3 slots, 1, 2, 3, 1
    idx, idx1 = (torch.tensor(q[:n], dtype=torch.int64) for q in (picks, picks1))
    for ix in (idx, idx1):
        assert {len(set(VF.stack_slots(first, GR, GN, int(s)))) for s in ix.tolist()} == {1, 2, 3}
    r = rs_(n)
    sh, sh1 = (f32(r.randint(0, 9, (n, 2))) for _ in range(2))
    sh[0], sh1[0] = torch.tensor([0.0, 8.0]), torch.tensor([8.0, 0.0])
    w, b = rnd(32, 9, 3, 3, seed=5, scale=0.2), rnd(32, seed=6, scale=0.1)
    d_frames, d_first = dev(torch.from_numpy(frames), "frames"), dev(torch.from_numpy(first), "first")
    d = [dev(t) for t in (idx, sh, idx1, sh1, w, b)]
    y1, x1 = ops.conv1_aug_fwd_frames(d_frames, d_first, GR, GN, d[0], d[1], d[2], d[3], d[4], d[5], n_store=n, bf16=bf16)
    obs, obs1 = (ops.vec_stack_gather(d_frames, d_first, GR, GN, ix).view(n, *OBS) for ix in (d[0], d[2]))
    want = np.stack([fs.stacks[21][1], fs.stacks[22][1], fs.stacks[25][0], fs.stacks[24][2], fs.stacks[26][2]][:n])
    assert np.array_equal(obs.cpu().numpy(), want)
    y0, x0 = ops.conv1_aug_fwd(obs, d[1], obs1, d[3], d[4], d[5], n_store=n, bf16=bf16)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and torch.equal(x0.view(torch.int32), x1.view(torch.int32))
    assert float(y1.abs().sum()) > 0 and float(x1[:n].abs().sum()) > 0 and float(x1[n:].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ store against store
SR, SN, SA, NSTEP, G = 16, 3, 3, 3, 2


def two_stores(mode, seed=9):
    from drqv2_amd.replay import VecDeviceReplay, VecFrameReplay
    kw = dict(priority_alpha=0.6) if mode == "per" else {}
    kw["indexed"] = mode != "materialised"
    vf = VecFrameReplay(SR, SN, SA, NSTEP, 0.99, "cuda", seed=seed, guard_rows=G, **kw)
    vd = VecDeviceReplay(SR, SN, OBS, SA, NSTEP, 0.99, "cuda", seed=seed, guard_rows=G + 2, **kw)
    return vf, vd


def feed(vf, vd, fs, rows, t):
    frame, action, reward, discount, first = rows[t]
    cu = lambda a: torch.from_numpy(a).cuda()
    vf.add(cu(frame), cu(action), cu(reward), cu(discount), cu(first))
    vd.add(cu(fs.stacks[t]), cu(action), cu(reward), cu(discount), cu(first))


@pytest.mark.parametrize("mode", ["uniform", "per", "materialised"])
def test_store_draws_equal_the_stacked_store(mode):
    """a VecFrameReplay(guard_rows = g) fed single frames against a VecDeviceReplay(guard_rows = g + 2) fed the oracle's
    stacks, same seed, nstep 3, a draw after every add once rows exist, 40 rows (the ring wraps twice): action, reward,
    discount, last_steps, the slots and the materialised obs / next_obs bit for bit; prioritized: the weights too, with
    priorities renewed after every draw"""
    from drqv2_amd.replay import FrameBatch, PrioritizedBatch
    fs, rows = store_stream(SR, SN, 40, seed=1)
    vf, vd = two_stores(mode)
    B, draws = 24, 0
    r = rs_(3)
    for t in range(40):
        feed(vf, vd, fs, rows, t)
        lo, hi = vf.bounds()
        assert (lo, hi) == vd.bounds() == VF.bounds(t + 1, SR, NSTEP, G)
        if hi < lo:
            continue
        assert fs.has_drawable(lo, hi)                             # the stores' precondition: no steps = 0 row can occur
        bf, bd = vf.sample(B), vd.sample(B)
        draws += 1
        assert torch.equal(vf.last_index, vd.last_index) and torch.equal(vf.last_steps, vd.last_steps)
        assert int(vf.last_steps.min()) >= 1
        for k in (1, 2, 3):
            assert torch.equal(bf[k].view(torch.int32), bd[k].view(torch.int32)), (t, k)
        if mode == "materialised":
            mf, md = bf, bd
            assert mf[0].shape == (B,) + OBS and mf[0].dtype == torch.uint8
        else:
            assert isinstance(bf, FrameBatch) and bf.frames is vf.frames and bf.ring == (vf.first, SR, SN)
            assert torch.equal(bf[0], bd[0]) and torch.equal(bf[4], bd[4])
            mf, md = bf.materialize(OBS), bd.materialize(OBS)
        assert torch.equal(mf[0], md[0]) and torch.equal(mf[4], md[4]), t
        for b, s in enumerate(vf.last_index[0].tolist()[:4]):     # ... and they are the wrapper's observations
            tt = next(x for x in range(t, t - SR, -1) if x % SR == s // SN)
            assert np.array_equal(mf[0][b].cpu().numpy(), fs.stacks[tt][s % SN])
        if mode == "per":
            assert isinstance(bf, PrioritizedBatch) and torch.equal(bf.weights.view(torch.int32), bd.weights.view(torch.int32))
            td = torch.from_numpy(r.exponential(size=B).astype(np.float32)).cuda()
            bf.update_priorities(td)
            bd.update_priorities(td)
            assert torch.equal(vf.tree, vd.tree)
    assert draws >= 35 and vf.T > 2 * SR
    if mode == "per":
        assert float(bf.weights.min()) < 1.0                       # the priorities did shape the draw


# ------------------------------------------------------------------------------------------------ the whole update
@pytest.mark.parametrize("mode,dtype", [("uniform", "fp32"), ("per", "fp32"), ("uniform", "bf16")])
def test_update_from_single_frames_equals_update_from_stacks(mode, dtype):
    """two agents, same seed, three update() calls fed by the two stores' iterators (one batch drawn ahead), a row added
    between updates -- fewer than either store's guard_rows, so both renew their priorities -- on a ring that has
    wrapped: every parameter, Adam moment and metric bit for bit, and the trees of the prioritized stores"""
    fs, rows = store_stream(SR, SN, 26, seed=2)
    outs = []
    for which in (0, 1):
        vf, vd = two_stores(mode, seed=5)
        store = (vf, vd)[which]
        store.batch_size = 16
        ag = make_agent(SA)
        ag.set_compute_dtype(dtype)
        reseed()
        for t in range(20):
            feed(vf, vd, fs, rows, t)
        assert fs.has_drawable(*vf.bounds())
        it = iter(store)
        ms = []
        for u in range(3):
            ms.append(ag.update(it, 2 * u))
            feed(vf, vd, fs, rows, vf.T)
        assert all(np.isfinite(v) for m in ms for v in m.values()) and len(ms[0]) == 8
        tree = store.tree.clone() if mode == "per" else torch.zeros(1)
        outs.append((ms, store.last_steps.clone(), tree) + engine_state(ag))
    (m0, *a0), (m1, *a1) = outs
    assert m0 == m1
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)
    if mode == "per":
        leaves = a0[1][a0[1].numel() // 2:]
        assert int(((leaves > 0) & (leaves != 1.0)).sum()) > 0     # the updates' errors did reach the tree


def test_observation_is_the_wrappers_and_feeds_act_batch():
    """observation() after every add equals the oracle's current stacks; the two buffers alternate; act_batch on it
    equals act_batch on the oracle's stacks"""
    from drqv2_amd import _lib
    fs, rows = store_stream(SR, SN, 22, seed=4)
    vf, vd = two_stores("uniform")
    with pytest.raises(_lib.DrqError, match="no row"):
        vf.observation()
    ag = make_agent(SA)
    prev = None
    for t in range(22):
        feed(vf, vd, fs, rows, t)
        o = vf.observation()
        assert o.shape == (SN,) + OBS and o.dtype == torch.uint8 and o.is_cuda
        assert np.array_equal(o.cpu().numpy(), fs.stacks[t]), t
        if prev is not None:
            assert o.data_ptr() != prev.data_ptr() and np.array_equal(prev.cpu().numpy(), fs.stacks[t - 1])
        prev = o
    a0 = ag.act_batch(vf.observation(), 0, True)
    a1 = ag.act_batch(torch.from_numpy(fs.stacks[21]).cuda(), 0, True)
    assert a0.is_cuda and a0.shape == (SN, SA) and torch.equal(a0, a1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from drqv2_amd import _lib
    from drqv2_amd.replay import VecFrameReplay
    with pytest.raises(ValueError, match="frame_shape"):
        VecFrameReplay(SR, SN, SA, NSTEP, 0.99, "cuda", frame_shape=(9, 84, 84))
    fs, rows = store_stream(SR, SN, 12, seed=6)
    vf, vd = two_stores("uniform")
    for t in range(12):
        feed(vf, vd, fs, rows, t)
    vf.batch_size = 16
    ag = make_agent(SA)
    t0 = (ag.critic_opt.t, ag.encoder_opt.t, ag.actor_opt.t)
    ag._engine.pg = object()                                       # what enable_data_parallel leaves
    try:
        with pytest.raises(_lib.DrqError, match="data parallelism"):
            ag.update(iter(vf), 0)
    finally:
        ag._engine.pg = None
    ag.set_behavior_cloning(2.5)
    with pytest.raises(_lib.DrqError, match="behaviour cloning"):
        ag.update(iter(vf), 0)
    ag.set_behavior_cloning(None)
    assert (ag.critic_opt.t, ag.encoder_opt.t, ag.actor_opt.t) == t0      # a refused update moved nothing
    pf, pd = two_stores("per")
    for t in range(12):
        feed(pf, pd, fs, rows, t)
    pf.batch_size = 16
    ag.set_compute_dtype("bf16")
    with pytest.raises(_lib.DrqError, match="bf16"):
        ag.update(iter(pf), 0)
    ag.set_compute_dtype("fp32")
    assert len(ag.update(iter(pf), 0)) == 8 and len(ag.update(iter(vf), 2)) == 8
