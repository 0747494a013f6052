"""Renderer images on the GPU: drq_vec_add_render on poisoned, guarded memory against the numpy restatement of the resize
rule (tests/vec_render_oracle.py) and against drq_vec_add fed the restatement's frames, and VecFrameReplay.add_render()
against add(oracle(image)) -- ring, flags, scalars, observation(), draws, trees and a whole DrQV2Agent.update().

Bounds.  Everything is compared bit for bit.  The resize is integer arithmetic whose sums fit 32 bits (255.5 * 336^2 <
2^31), so the kernel's separable order and the oracle's single einsum give the same integers and the one division the
same bytes.  The scalars are copies made by the device code drq_vec_add runs.  Two stores that hold the same bytes and
share a seed run the same launches on the same operands from there on.

Shapes.  N = 3 environments (odd, more than one workgroup column), R = 8 rows, A = 2.  Image sizes 84 (one tap of weight
84), 85 (odd, rows of 255 bytes at Cin = 3: no row but the first starts on a dword), 128 and 168 (the renderers'), 255,
257 (the first size with five taps on an axis), 335 (the most staged rows and LDS per band) and 336 (four whole taps, the
largest sums); Cin 3 and 4.  The image's first byte lies 0, 4, 8 and 12 bytes past a 16-byte boundary in turn, so the
first and the last 16-byte piece of the array are partly outside it.

Coverage, continuing the map of tests/test_hip_entries.py:
  here            vec_add_render (with every DRQ_EARG case on refused, poisoned outputs)"""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_render_oracle as VR
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, f32, p, rs_
from tests.test_hip_vec_replay import ARRAYS, engine_state, make_agent, raw, reseed, u8

pytestmark = pytest.mark.gpu
EARG = -1
R, N, A, FB = 8, 3, 2, 3 * 84 * 84
SIZES = (84, 85, 128, 168, 255, 257, 335, 336)


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_add_render" in _lib.PROTOTYPES, "the renderer-image entry is missing"
    return _lib.load()


SHAPES = {"frames": (R * N, FB), "action": (R * N, A), "reward": (R * N,), "discount": (R * N,), "first": (R * N,)}


def ring(kind):
    return {n: poison.alloc(SHAPES[n], dt, "cuda", name=n, kind=kind) for n, dt in ARRAYS}


def image_at(img, off):
    """the image on the device with its first byte `off` bytes into a guarded allocation whose other bytes are poison;
    returns (the allocation, the address of the image)"""
    flat = np.full(img.size + 16, poison.sentinel_of(torch.uint8), np.uint8)
    flat[off:off + img.size] = img.reshape(-1)
    d = dev(torch.from_numpy(flat), "src_image")
    return d, p(d) + off


# ------------------------------------------------------------------------------------------------ drq_vec_add_render
@pytest.mark.parametrize("Cin", [3, 4])
@pytest.mark.parametrize("S", SIZES)
def test_vec_add_render_matches_the_oracle_and_vec_add(lib, S, Cin):
    """rows t = 0 (first forced), 5 (src_first NULL; environment 1 renders all 255: the largest sums), 8 = R (ring row 0
    again), 13 (row 5 again): after every call the ring equals, byte for byte, a second ring that drq_vec_add fills from
    the oracle's frames and the same scalar sources; the frames of the row are the oracle's, every other row is what it
    was, for the rows never written the poison"""
    got, ref = ring("ws"), ring("ws")
    r = rs_(S * 10 + Cin)
    rows_written = set()
    for k, (t, with_first) in enumerate(((0, True), (5, False), (R, True), (R + 5, True))):
        img = r.randint(0, 256, (N, S, S, Cin)).astype(np.uint8)
        if t == 5:
            img[1] = 255
        frames = VR.resize(img)
        src = {"action": f32(r.uniform(-1, 1, (N, A))), "reward": f32(r.standard_normal(N)),
               "discount": f32(r.uniform(0, 1, N)), "first": u8(r.randint(0, 2, N))}
        d = {n: dev(src[n], "src_" + n) for n in src}
        scal = [p(d["action"]), p(d["reward"]), p(d["discount"]), p(d["first"]) if with_first else None]
        keep, addr = image_at(img, 4 * k)
        assert lib.drq_vec_add_render(*(p(got[n]) for n, _ in ARRAYS), R, N, A, t, addr, S, Cin, *scal, None) == 0
        assert lib.drq_vec_add(*(p(ref[n]) for n, _ in ARRAYS), R, N, A, FB, t, p(dev(torch.from_numpy(frames), "frames")),
                               *scal, None) == 0
        rows_written.add(t % R)
        for n, _ in ARRAYS:
            assert np.array_equal(raw(got[n]), raw(ref[n])), (t, n)
        row = raw(got["frames"]).reshape(R, N, 3, 84, 84)[t % R]
        assert np.array_equal(row, frames), t
        if t == 5:
            assert (row[1] == 255).all()
        want_first = np.ones(N) if t == 0 else (src["first"].numpy() != 0 if with_first else np.zeros(N))
        assert np.array_equal(raw(got["first"]).reshape(R, N)[t % R], want_first.astype(np.uint8))
    untouched = np.array([i not in rows_written for i in range(R)])
    assert rows_written == {0, 5} and untouched.sum() == R - 2
    assert (raw(got["frames"]).reshape(R, -1)[untouched] == poison.sentinel_of(torch.uint8)).all()
    assert (raw(got["first"]).reshape(R, N)[untouched] == poison.sentinel_of(torch.uint8)).all()
    assert (got["reward"].view(torch.int32).cpu().numpy().reshape(R, N)[untouched] == poison.SENTINEL).all()
    assert (got["action"].view(torch.int32).cpu().numpy().reshape(R, N * A)[untouched] == poison.SENTINEL).all()


def test_vec_add_render_refusals(lib):
    S, Cin = 128, 4
    store = list(ring("refused").values())
    img = dev(u8(np.zeros((N, S, S, Cin))), "image")
    src = [dev(f32(np.zeros((N, A)))), dev(f32(np.zeros(N))), dev(f32(np.ones(N))), dev(u8(np.zeros(N)), "first")]
    ok = [p(t) for t in store] + [R, N, A, 3, p(img), S, Cin] + [p(t) for t in src]
    bad = []
    for k in (0, 1, 2, 3, 4, 9, 12, 13, 14):                      # every required pointer (src_first may be NULL)
        bad.append(ok[:k] + [None] + ok[k + 1:])
    for k, vals in ((5, (0, -1)), (6, (0, -1, 2 ** 31 // 21 + 1)), (7, (0, -1)), (8, (-1,)),      # R, N, A, t
                    (10, (83, 0, 337, 4096)), (11, (0, 1, 2, 5))):                                 # S, Cin
        for v in vals:
            bad.append(ok[:k] + [v] + ok[k + 1:])
    for mis in (4, 8):
        bad.append([ok[0] + mis] + ok[1:])                        # frames not 16-byte aligned
    for mis in (1, 2, 3):
        bad.append(ok[:9] + [ok[9] + mis] + ok[10:])              # src_image not 4-byte aligned
    for a in bad:
        assert lib.drq_vec_add_render(*a, None) == EARG, a[5:12]
    poison.check()                                                # nothing was written by a refused call
    for t in store:
        poison.forget(t)
    assert lib.drq_vec_add_render(*ok, None) == 0                 # the unbroken call is accepted
    assert lib.drq_vec_add_render(*(ok[:15] + [None]), None) == 0


# ------------------------------------------------------------------------------------------------ store against store
SR, SA, NSTEP, G = 16, 3, 3, 2
STEPS = 2 * SR + 3
STORE_SIZES = ((128, 4), (84, 3), (168, 4), (100, 3), (257, 4))      # a renderer may change its size between steps


def stream(T, seed):
    """rows for the two stores: images, their frames by the oracle, actions, rewards, discounts, flags.  Environment 0
    is never reset, environment e > 0 every 5 + e rows and once on two consecutive rows, so every environment holds a
    non-reset row among the drawable ones and row 1 is none"""
    r = rs_(seed)
    rows = []
    for t in range(T):
        S, Cin = STORE_SIZES[t % len(STORE_SIZES)]
        img = r.randint(0, 256, (N, S, S, Cin)).astype(np.uint8)
        first = np.array([e > 0 and (t % (5 + e) == e + 2 or t == 17 + e or t == 18 + e) for e in range(N)])
        rows.append((img, VR.resize(img), r.uniform(-1, 1, (N, SA)).astype(np.float32),
                     r.standard_normal(N).astype(np.float32), np.where(r.uniform(size=N) < 0.1, 0.0, 1.0).astype(np.float32),
                     first))
    return rows


@pytest.fixture(scope="module")
def rows():
    """computed once, shared, never modified"""
    return stream(STEPS, seed=1)


def two_stores(alpha, seed=9):
    from drqv2_amd.replay import VecFrameReplay
    kw = dict(priority_alpha=alpha) if alpha else {}
    return tuple(VecFrameReplay(SR, N, SA, NSTEP, 0.99, "cuda", seed=seed, guard_rows=G, **kw) for _ in range(2))


def cu(a):
    return torch.from_numpy(a).cuda()


def feed(rendered, plain, row, host=False, render=True):
    img, frame, action, reward, discount, first = row
    scal = (action, reward, discount, first) if host else tuple(cu(a) for a in (action, reward, discount, first))
    if render:
        rendered.add_render(img if host else cu(img), *scal)
    else:
        rendered.add(frame if host else cu(frame), *scal)
    plain.add(cu(frame), *(cu(a) for a in (action, reward, discount, first)))


def same_store(a, b):
    assert a.T == b.T and a.bounds() == b.bounds()
    held = min(a.T, a.R) * a.N                                     # the frames of a slot never written are not initialised
    for n in ("frames", "action", "reward", "discount", "first"):
        assert np.array_equal(raw(getattr(a, n)[:held]), raw(getattr(b, n)[:held])), n
    assert torch.equal(a.observation(), b.observation())
    if a.tree is not None:
        assert torch.equal(a.tree, b.tree)


def same_draws(a, b, n=3, B=24, seed=3):
    from drqv2_amd.replay import FrameBatch, PrioritizedBatch
    r = rs_(seed)
    for _ in range(n):
        ba, bb = a.sample(B), b.sample(B)
        assert isinstance(ba, FrameBatch) and ba.frames is a.frames
        assert torch.equal(a.last_index, b.last_index) and torch.equal(a.last_steps, b.last_steps)
        assert int(a.last_steps.min()) >= 1
        assert torch.equal(ba[0], bb[0]) and torch.equal(ba[4], bb[4])
        for k in (1, 2, 3):
            assert torch.equal(ba[k].view(torch.int32), bb[k].view(torch.int32)), k
        ma, mb = ba.materialize(), bb.materialize()
        assert torch.equal(ma[0], mb[0]) and torch.equal(ma[4], mb[4])
        if a.tree is not None:
            assert isinstance(ba, PrioritizedBatch) and torch.equal(ba.weights.view(torch.int32), bb.weights.view(torch.int32))
            td = cu(r.exponential(size=B).astype(np.float32))
            ba.update_priorities(td)
            bb.update_priorities(td)
            assert torch.equal(a.tree, b.tree)


@pytest.mark.parametrize("alpha", [None, 0.6])
def test_store_fed_images_equals_store_fed_the_oracles_frames(rows, alpha):
    """add_render(image) against add(oracle(image)) on two stores of one seed, 2 rows + 3 steps with resets (the ring wraps
    twice), image sizes and channel counts changing from step to step: the five arrays, observation() and, prioritized,
    the whole tree after every step; three draws at the end, with the priorities renewed in between"""
    a, b = two_stores(alpha)
    for t in range(STEPS):
        feed(a, b, rows[t])
        same_store(a, b)
        assert np.array_equal(a.observation()[:, 6:9].cpu().numpy(), rows[t][1])      # the newest frame is the oracle's
    assert a.T == STEPS > 2 * SR
    same_draws(a, b)
    if alpha:
        leaves = a.tree[a.tree.numel() // 2:]
        assert int((leaves > 0).sum()) > 0 and int(((leaves > 0) & (leaves != 1.0)).sum()) > 0


def test_host_images_and_alternating_adds(rows):
    """numpy images go through the pinned buffer (reallocated when the shape changes) and give the same bytes; a store
    on which add() and add_render() alternate, from the host and from the device, equals one fed add() alone"""
    a, b = two_stores(None)
    shapes = set()
    for t in range(STEPS):
        feed(a, b, rows[t], host=True)
        assert a._render_stage[0].is_pinned() and tuple(a._render_stage[0].shape) == rows[t][0].shape
        shapes.add(tuple(a._render_stage[0].shape))
        if t % 7 == 0 or t == STEPS - 1:
            same_store(a, b)
    assert len(shapes) == len(STORE_SIZES)
    same_draws(a, b, n=1)
    c, d = two_stores(0.6)
    for t in range(STEPS):
        feed(c, d, rows[t], host=t % 4 >= 2, render=t % 2 == 0)
    same_store(c, d)
    same_draws(c, d, n=1)
    img = cu(rows[0][0])
    with pytest.raises(ValueError, match=r"add_render\(\): image"):
        c.add_render(img.permute(0, 3, 1, 2), *(cu(x) for x in rows[0][2:]))
    assert c.T == STEPS


def test_update_from_rendered_store_equals_update_from_plain_store(rows):
    """one whole update() at B = 16 fed by each of the two stores: metrics, parameters and Adam moments bit for bit"""
    outs = []
    for which in (0, 1):
        a, b = two_stores(None, seed=5)
        for t in range(20):
            feed(a, b, rows[t])
        store = (a, b)[which]
        store.batch_size = 16
        ag = make_agent(SA)
        reseed()
        m = ag.update(iter(store), 0)
        assert len(m) == 8 and all(np.isfinite(v) for v in m.values())
        outs.append((m, store.last_steps.clone()) + engine_state(ag))
    (m0, *s0), (m1, *s1) = outs
    assert m0 == m1
    for x, y in zip(s0, s1):
        assert torch.equal(x, y)
