"""Prioritized sampling on the step-major ring, on the GPU: drq_vec_per_advance / _sample / _update on poisoned, guarded
memory against the numpy restatement tests/vec_per_oracle.py, and VecDeviceReplay(priority_alpha=...) against it through
the iterator, through DrQV2Agent.update() and across the guard rows.

Bounds.  Leaves set by the advance, every sum of the tree, slots, window lengths, action rows and the n-step reward /
discount are compared bit for bit: they are copies, integers, IEEE double additions in a fixed order, or the reference's
float32 operations in the reference's order (tests/test_hip_vec_replay.py).  The two places with a device pow keep the
bounds tests/test_hip_per.py holds the episode store's tree to: leaves written by a priority update 1e-12 relative (two
fp64 pow implementations), weights 1e-6 relative (the device pow plus one float32 rounding, 6e-8), the largest exactly 1."""
import numpy as np
import pytest
import torch

from tests import per_oracle as P
from tests import poison
from tests import vec_oracle as V
from tests import vec_per_oracle as VP
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, f32, out, p, rs_
from tests.test_hip_per import bits64, f64, i64, inner_ok
from tests.test_hip_replay import OBS
from tests.test_hip_vec_replay import ARRAYS, compare, device_row, engine_state, make_agent, raw, reseed

pytestmark = pytest.mark.gpu
EARG = -1
R, FB, A = 16, 16, 2


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_per_sample" in _lib.PROTOTYPES, "the prioritized step-major replay entries are missing"
    return _lib.load()


def random_row(r, N, A_=A, p_reset=0.2, force=()):
    first = r.uniform(size=N) < p_reset
    first[list(force)] = True
    return (r.randint(0, 256, (N, FB)).astype(np.uint8), r.uniform(-1, 1, (N, A_)).astype(np.float32),
            r.standard_normal(N).astype(np.float32), np.where(r.uniform(size=N) < 0.1, 0.0, 1.0).astype(np.float32), first)


def ring_on_device(vo):
    ring, _ = vo.ring()
    return ring, {n: dev(torch.from_numpy(ring[n]), n) for n, _ in ARRAYS}


def same_tree(got, want):
    return np.array_equal(bits64(got), bits64(want))


# ------------------------------------------------------------------------------------------------ drq_vec_per_advance
@pytest.mark.parametrize("guard", [0, 2])
@pytest.mark.parametrize("N", [1, 3, 1030])
def test_advance(lib, N, guard):
    """2R + 4 rows through drq_vec_add + drq_vec_per_advance: after every add the whole device tree -- leaves, inner
    nodes, tree[0] -- is the restatement's, bit for bit.  N = 1030: the loops stride past 1,024 threads and R N = 16,480 is
    no power of two (the 16,288 padding leaves stay 0).  At T = R the running maximum is raised by hand on both sides:
    the rows entering afterwards start there"""
    nstep = 3
    vp = VP.VecPEROracle(R, N, A, FB, nstep, 0.99, guard_rows=guard)
    L = vp.L
    assert L == {1: 16, 3: 64, 1030: 32768}[N] and L >= R * N
    shapes = {"frames": (R * N, FB), "action": (R * N, A), "reward": (R * N,), "discount": (R * N,), "first": (R * N,)}
    store = {n: poison.alloc(shapes[n], dt, "cuda", name=n, kind="ws") for n, dt in ARRAYS}
    tree = dev(f64(vp.tree), "tree")
    r = rs_(N + guard)
    entered = left = 0
    for t in range(2 * R + 4):
        row = random_row(r, N, force=(0,) if t in (6, 7, 20) else ())      # two adjacent reset rows in environment 0
        vp.add(*row)
        d = [dev(torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8 if i in (0, 4) else np.float32))) for i, x in enumerate(row)]
        assert lib.drq_vec_add(*(p(store[n]) for n, _ in ARRAYS), R, N, A, FB, t, *(p(x) for x in d), None) == 0
        T = t + 1
        enter, leave = VP.entering_leaving(T, R, nstep, guard)
        assert lib.drq_vec_per_advance(p(tree), L, p(store["first"]), R, N, T, enter, leave, None) == 0
        entered += enter >= 0
        left += leave >= 0
        got = tree.cpu().numpy()
        assert same_tree(got, vp.tree), (T, enter, leave)
        assert inner_ok(got) and not got[L + R * N:].any()
        if T == R:
            vp.tree[0] = 2.5
            tree[:1] = 2.5
    assert entered == 2 * R + 4 - nstep and left == 2 * R + 4 - (R - guard) > R
    assert (got[L:] == 2.5).sum() > 0 and set(np.unique(got[L:]).tolist()) == {0.0, 2.5}
    assert np.array_equal(got[L:] > 0, vp.expected_leaf_mask())


# ------------------------------------------------------------------------------------------------ drq_vec_per_sample
def scenario(nstep, T, N=3, guard=0, empty=False, alpha=1.0):
    """A ring of T rows.  Environment 1 holds, from row lo on, nstep - 1 non-reset rows and then two reset rows: windows
    cut after every number of steps; the other environments reset at random.  Then one priority update (alpha 1) that
    spreads the leaves over six orders of magnitude, the cut windows and one full one on top"""
    vp = VP.VecPEROracle(R, N, A, FB, nstep, 0.99, guard_rows=guard, alpha=alpha)
    lo, hi = V.bounds(T, R, nstep, guard)
    r0 = lo + nstep - 1
    r = rs_(T + nstep)
    for t in range(T):
        first = r.uniform(size=N) < 0.15
        first[1] = t in (r0, r0 + 1)
        if empty:
            first[:] = True
        vp.add(*random_row(r, N)[:4], first)
    if empty:
        return vp
    valid = np.nonzero(vp.expected_leaf_mask())[0]
    td = (10.0 ** r.uniform(-3, 3, valid.size)).astype(np.float32)
    top = [V.slot(r0 - i, 1, R, N) for i in range(1, nstep)] + [V.slot(r0 + 2, 1, R, N)]
    td[np.isin(valid, top)] = 1e3
    vp.update(valid, td)
    leaves = vp.tree[vp.L:][valid]
    assert leaves.max() / leaves.min() > 10.0 ** (5 * alpha)
    return vp


def run_per_sample(lib, vp, u, beta):
    vo = vp.vo
    ring, d = ring_on_device(vo)
    lo, hi = vo.bounds()
    B = u.shape[0]
    tree = dev(f64(vp.tree), "tree")
    o = dict(idx=out(3, B, dtype=torch.int64, name="idx"), act=out(B, vo.A, name="act"), rew=out(B, name="rew"),
             disc=out(B, name="disc"), steps=out(B, dtype=torch.int32, name="steps"), w=out(B, name="weights"))
    rc = lib.drq_vec_per_sample(p(tree), vp.L, p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), vo.R, vo.N,
                                vo.A, vo.T, lo, hi, p(dev(f64(u), "u")), B, vo.nstep, vo.gamma, beta, p(o["idx"]), p(o["act"]),
                                p(o["rew"]), p(o["disc"]), p(o["steps"]), p(o["w"]), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert same_tree(tree.cpu().numpy(), vp.tree)                 # the draw writes neither the tree ...
    for n, _ in ARRAYS:                                            # ... nor the store
        assert np.array_equal(d[n].cpu().numpy(), ring[n]), n
    return o


@pytest.mark.parametrize("T", [R + 1, 2 * R + 5])
@pytest.mark.parametrize("nstep", [1, 3])
@pytest.mark.parametrize("B", [1, 37, 256, 1100])
def test_sample(lib, B, nstep, T):
    """T = R + 1: the draw right after the wrap (ring row 0 has just been overwritten and is a head row)"""
    vp = scenario(nstep, T)
    vp.beta = 0.4
    r = rs_(B + T)
    u = r.random_sample(B)
    u[0], u[-1] = (0.0, np.nextafter(1.0, 0.0)) if B > 1 else (u[0], u[0])
    want = vp.sample(u)
    lo, hi = vp.bounds()
    assert all(lo <= t <= hi for t, _ in want["rows"])
    if B >= 256:
        assert set(want["steps"].tolist()) == set(range(1, nstep + 1))     # a window cut at every offset, and full ones
    o = run_per_sample(lib, vp, u, vp.beta)
    compare(o, want)
    wh = o["w"].cpu().numpy().astype(np.float64)
    rel = float(np.abs(wh / want["weights"] - 1).max())
    print(f"vec_per_sample B={B} nstep={nstep} T={T}: weights max rel err {rel:.3e}, min weight {wh.min():.4g}")
    assert rel <= 1e-6
    assert wh.max() == 1.0
    if B >= 256:
        assert wh.min() < 0.5                                      # the spread of the priorities reaches the weights


def test_sample_empty_tree(lib):
    """every drawable row is a reset row: the tree is all zeros and every batch row is the empty one, finite everywhere
    (the autouse check: every output written, no NaN, guards intact)"""
    vp = scenario(3, 2 * R + 5, empty=True)
    assert not vp.tree[1:].any() and vp.tree[0] == 1.0
    B = 1100
    u = rs_(1).random_sample(B)
    want = vp.sample(u)
    o = run_per_sample(lib, vp, u, 0.4)
    compare(o, want)
    lo, _ = vp.bounds()
    s = V.slot(lo, 0, R, 3)
    assert (o["idx"].cpu().numpy() == s).all() and not o["steps"].any() and not o["rew"].any() and not o["disc"].any()
    assert (o["w"].cpu().numpy() == 1.0).all()
    assert bool(torch.isfinite(o["act"]).all())


# ------------------------------------------------------------------------------------------------ drq_vec_per_update
@pytest.mark.parametrize("B", [8, 256, 1100])
def test_update(lib, B):
    """rows 0 and B-1 name the same position (the highest row wins); rows 1 .. 4 a reset row inside lo .. hi, a slot of
    row lo-1, one of row hi+1 and a padding leaf >= R N, all four with an error larger than any other: skipped, untouched,
    not in tree[0]; rows 5, 6 a NaN and a negative error.  A second call with an infinite error in row B-1"""
    N, nstep, alpha, eps = 3, 3, 0.6, 1e-6
    vp = scenario(nstep, 2 * R + 5, guard=2, alpha=alpha)
    vo, L = vp.vo, vp.L
    vp.tree[0] = 1.25e3
    lo, hi = vp.bounds()
    valid = np.nonzero(vp.expected_leaf_mask())[0]
    a, b, c = valid[[0, 7, 13]].tolist()
    reset = next(V.slot(t, e, R, N) for t in range(lo, hi + 1) for e in range(N) if vo.first[t][e])
    skipped = [reset, V.slot(lo - 1, 1, R, N), V.slot(hi + 1, 2, R, N), R * N + 1]
    r = rs_(B)
    rest = np.setdiff1d(valid, [a, b, c])
    pos = np.concatenate([[a], skipped, [b, c], r.choice(rest, B - 8), [a]]).astype(np.int64)
    td = r.uniform(0, 50, B).astype(np.float32)
    td[1:5], td[5], td[6] = 1e30, np.nan, -4.0
    assert pos.size == B and td[0] != td[B - 1]
    ring, d = ring_on_device(vo)
    tree = dev(f64(vp.tree), "tree")
    pd = dev(i64(pos), "pos")
    for call in range(2):
        if call == 1:
            td[B - 1] = np.inf
        before = vp.tree.copy()
        assert lib.drq_vec_per_update(p(tree), L, p(d["first"]), R, N, vo.T, lo, hi, p(pd), p(dev(f32(td), "td")), B, alpha,
                                      eps, None) == 0
        got = tree.cpu().numpy()
        written = vp.update(pos, td)
        named = np.array(sorted(written), np.int64)
        assert not set(skipped) & set(written) and {a, b, c} <= set(written)
        rel = float(np.abs(got[L + named] / vp.tree[L + named] - 1).max())
        print(f"vec_per_update B={B} call {call}: leaves max rel err {rel:.3e}")
        assert rel <= 1e-12
        last = (np.float64(min(td[B - 1], np.finfo(np.float32).max)) + eps) ** alpha
        assert abs(got[L + a] / last - 1) <= 1e-12
        assert abs(got[L + b] / eps ** alpha - 1) <= 1e-12 and abs(got[L + c] / eps ** alpha - 1) <= 1e-12
        others = np.setdiff1d(np.arange(L), named)
        assert np.array_equal(bits64(got[L + others]), bits64(before[L + others]))      # unnamed or skipped: untouched
        assert inner_ok(got) and same_tree(got[1:L], P.build(got[L:])[1:L])             # sums of the device's own leaves
        assert got[0] == max(before[0], got[L + named].max())
        assert np.isfinite(got[1]) and np.array_equal(got[L:] > 0, vp.expected_leaf_mask())
        if call == 0:
            assert got[0] == 1.25e3 < (1e30 + eps) ** alpha         # the skipped rows' errors did not get there
        else:
            assert got[0] == got[L + a] > 1e22
        vp.tree[:] = got                                           # the second call starts from the device's leaves
    for n, _ in ARRAYS:
        assert np.array_equal(d[n].cpu().numpy(), ring[n]), n


# ------------------------------------------------------------------------------------------------ ring == episode store
@pytest.fixture(scope="module")
def small_ring(lib):
    """A ring of R = 8 rows, N = 3, nstep 3, guard 0 after T = 2R + 5 adds with no reset flag but the one row 0 always
    carries (long overwritten): every drawable slot holds a transition, which is what the episode store's entries assume
    of a positive leaf.  The tree is the device's own: drq_vec_per_advance after every add, then one priority update of
    all drawable slots with random errors.  Host copies; the tests upload them and leave them as they are."""
    Rs, N, nstep, T = 8, 3, 3, 2 * 8 + 5
    vp = VP.VecPEROracle(Rs, N, A, FB, nstep, 0.99, guard_rows=0)
    L = vp.L
    shapes = {"frames": (Rs * N, FB), "action": (Rs * N, A), "reward": (Rs * N,), "discount": (Rs * N,), "first": (Rs * N,)}
    store = {n: torch.zeros(shapes[n], dtype=dt, device="cuda") for n, dt in ARRAYS}
    tree = f64(vp.tree).cuda()
    r = rs_(8)
    for t in range(T):
        row = random_row(r, N, p_reset=0.0)
        vp.add(*row)
        d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8 if i in (0, 4) else np.float32)).cuda() for i, x in enumerate(row)]
        assert lib.drq_vec_add(*(p(store[n]) for n, _ in ARRAYS), Rs, N, A, FB, t, *(p(x) for x in d), None) == 0
        enter, leave = VP.entering_leaving(t + 1, Rs, nstep, 0)
        assert lib.drq_vec_per_advance(p(tree), L, p(store["first"]), Rs, N, t + 1, enter, leave, None) == 0
    lo, hi = vp.bounds()
    assert (lo, hi) == (T - Rs + 1, T - nstep) and not store["first"].any()
    valid = np.nonzero(vp.expected_leaf_mask())[0]
    assert valid.size == (hi - lo + 1) * N and same_tree(tree.cpu().numpy(), vp.tree)
    td = (10.0 ** r.uniform(-3, 3, valid.size)).astype(np.float32)
    assert lib.drq_vec_per_update(p(tree), L, p(store["first"]), Rs, N, T, lo, hi, p(i64(valid).cuda()), p(f32(td).cuda()),
                                  valid.size, 0.6, 1e-6, None) == 0
    torch.cuda.synchronize()
    got = tree.cpu().numpy()
    assert inner_ok(got) and np.array_equal(got[L:] > 0, vp.expected_leaf_mask()) and np.unique(got[L + valid]).size > 10
    return dict(R=Rs, N=N, nstep=nstep, T=T, L=L, lo=lo, hi=hi, valid=valid, tree=got,
                ring={n: store[n].cpu() for n, _ in ARRAYS})


@pytest.mark.parametrize("B", [1, 37, 1100])
def test_ring_draw_equals_the_episode_stores(lib, small_ring, B):
    """The descent and the weights are one piece of device code for both stores: on a ring without reset rows
    drq_per_sample with n_valid = (hi - lo + 1) N and the same u names the same positions and gives the same weights as
    drq_vec_per_sample, bit for bit.  B = 1100 strides past the 1,024 threads"""
    s = small_ring
    Rs, N, L, lo, hi, beta = s["R"], s["N"], s["L"], s["lo"], s["hi"], 0.4
    u = rs_(B).random_sample(B)
    u[0], u[-1] = (0.0, np.nextafter(1.0, 0.0)) if B > 1 else (u[0], u[0])
    d = {n: dev(s["ring"][n], n) for n, _ in ARRAYS}
    tree, ud = dev(f64(s["tree"]), "tree"), dev(f64(u), "u")
    o = dict(idx=out(3, B, dtype=torch.int64, name="idx"), act=out(B, A, name="act"), rew=out(B, name="rew"),
             disc=out(B, name="disc"), steps=out(B, dtype=torch.int32, name="steps"), w=out(B, name="weights"))
    assert lib.drq_vec_per_sample(p(tree), L, p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), Rs, N, A,
                                  s["T"], lo, hi, p(ud), B, s["nstep"], 0.99, beta, p(o["idx"]), p(o["act"]), p(o["rew"]),
                                  p(o["disc"]), p(o["steps"]), p(o["w"]), None) == 0
    idx, w = out(3, B, dtype=torch.int64, name="flat idx"), out(B, name="flat weights")
    assert lib.drq_per_sample(p(tree), L, p(ud), B, s["nstep"], (hi - lo + 1) * N, beta, p(idx), p(w), None) == 0
    torch.cuda.synchronize()
    pos = o["idx"][2].cpu().numpy()
    assert np.isin(pos, s["valid"]).all() and (B == 1 or np.unique(pos).size > 1)
    assert np.array_equal(idx[2].cpu().numpy(), pos)
    assert np.array_equal(raw(w), raw(o["w"])) and float(o["w"].max()) == 1.0
    assert same_tree(tree.cpu().numpy(), s["tree"])


@pytest.mark.parametrize("B", [8, 1100])
def test_ring_update_equals_the_episode_stores(lib, small_ring, B):
    """The priority update is one piece of device code for both stores: for positions among the drawable slots, repeats
    included, drq_per_update and drq_vec_per_update leave identical trees, all 2L doubles, bit for bit"""
    s = small_ring
    Rs, N, L = s["R"], s["N"], s["L"]
    r = rs_(B)
    pos = r.choice(s["valid"], B).astype(np.int64)
    pos[-1] = pos[0]
    td = (10.0 ** r.uniform(-3, 3, B)).astype(np.float32)
    assert np.unique(pos).size < B and td[0] != td[-1]
    first = dev(s["ring"]["first"], "first")
    pd, tdd = dev(i64(pos), "pos"), dev(f32(td), "td")
    flat, ring = dev(f64(s["tree"]), "flat tree"), dev(f64(s["tree"]), "ring tree")
    assert lib.drq_per_update(p(flat), L, p(pd), p(tdd), B, 0.6, 1e-6, None) == 0
    assert lib.drq_vec_per_update(p(ring), L, p(first), Rs, N, s["T"], s["lo"], s["hi"], p(pd), p(tdd), B, 0.6, 1e-6,
                                  None) == 0
    torch.cuda.synchronize()
    got = ring.cpu().numpy()
    assert same_tree(flat.cpu().numpy(), got)
    assert inner_ok(got) and not same_tree(got, s["tree"]) and got[0] == max(s["tree"][0], got[L:].max())


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(lib):
    """every DRQ_EARG case of the three entries: the outputs stay poison, the tree stays what it was"""
    N, nstep = 3, 3
    vp = scenario(nstep, 2 * R + 5, guard=0)
    vo, L, T = vp.vo, vp.L, vp.T
    lo, hi = vp.bounds()
    assert hi - lo + 1 + nstep == R and hi + nstep == T and lo - 1 == T - R
    _, d = ring_on_device(vo)
    tree = dev(f64(vp.tree), "tree")
    n = 4
    ref = lambda shape, dt, name: poison.alloc(shape, dt, "cuda", name=name, kind="refused")
    outs = [ref((3, n), torch.int64, "idx"), ref((n, A), torch.float32, "act"), ref((n,), torch.float32, "rew"),
            ref((n,), torch.float32, "disc"), ref((n,), torch.int32, "steps"), ref((n,), torch.float32, "weights")]
    u = dev(f64(np.full(n, 0.5)), "u")

    def variants(ok, nulls, values):
        for k in nulls:
            yield [None if i == k else v for i, v in enumerate(ok)]
        for k, v in values:
            yield [v if i == k else x for i, x in enumerate(ok)]

    # advance: tree, L, first, R, N, T, enter_t, leave_t
    ok = [p(tree), L, p(d["first"]), R, N, T, hi, lo - 1]
    bad = list(variants(ok, (0, 2), ((1, L - 1), (1, 0), (1, L // 2), (3, 0), (4, 0), (4, -1), (5, 0), (6, -2), (6, T),
                                     (7, -2), (7, T), (6, T - R - 1), (7, T - R - 1), (7, hi))))
    for a in bad:
        assert lib.drq_vec_per_advance(*a, None) == EARG, a[1:]
    # sample: tree, L, first, action, reward, discount, R, N, A, T, lo, hi, u, B, nstep, gamma, beta, six outputs
    ok = [p(tree), L, p(d["first"]), p(d["action"]), p(d["reward"]), p(d["discount"]), R, N, A, T, lo, hi, p(u), n, nstep,
          0.99, 0.4] + [p(t) for t in outs]
    bad = list(variants(ok, (0, 2, 3, 4, 5, 12, 17, 18, 19, 20, 21, 22),
                        ((1, L + 1), (1, 0), (1, L // 2), (6, 0), (7, 0), (8, 0), (13, 0), (14, 0), (16, -0.1),
                         (16, float("nan")), (10, 0), (11, lo - 1), (14, nstep + 1), (10, lo - 1), (11, hi + 1), (9, T - 1),
                         (9, T + 1))))
    for a in bad:
        assert lib.drq_vec_per_sample(*a, None) == EARG, a[6:17]
    # update: tree, L, first, R, N, T, lo, hi, pos, td_abs, B, alpha, eps
    pos, td = dev(i64(np.arange(n)), "pos"), dev(f32(np.ones(n)), "td")
    ok_u = [p(tree), L, p(d["first"]), R, N, T, lo, hi, p(pos), p(td), n, 0.6, 1e-6]
    bad = list(variants(ok_u, (0, 2, 8, 9), ((1, L - 1), (1, L // 2), (3, 0), (4, 0), (10, 0), (11, 0.0), (11, -1.0),
                                             (11, float("nan")), (12, -1e-9), (6, 0), (7, lo - 1), (7, T), (6, lo - 1),
                                             (5, T + 1))))
    for a in bad:
        assert lib.drq_vec_per_update(*a, None) == EARG, a[3:8]
    poison.check()                                                 # nothing was written by a refused call
    torch.cuda.synchronize()
    assert same_tree(tree.cpu().numpy(), vp.tree)
    # no row enters or leaves: accepted, and nothing is launched
    assert lib.drq_vec_per_advance(p(tree), L, p(d["first"]), R, N, T, -1, -1, None) == 0
    assert same_tree(tree.cpu().numpy(), vp.tree)
    for t in outs:
        poison.forget(t)
    assert lib.drq_vec_per_sample(*ok, None) == 0 and lib.drq_vec_per_update(*ok_u, None) == 0      # the unbroken calls


# ------------------------------------------------------------------------------------------------ the store
def store_tree(vs):
    torch.cuda.synchronize()
    return vs.tree.cpu().numpy()


def check_batch(b, vs, want):
    from drqv2_amd.replay import IndexedBatch, PrioritizedBatch
    assert isinstance(b, PrioritizedBatch) and isinstance(b, IndexedBatch) and b.frames is vs.frames
    assert np.array_equal(b[0].cpu().numpy(), want["idx"][0]) and np.array_equal(b[4].cpu().numpy(), want["idx"][1])
    assert np.array_equal(b._pos.cpu().numpy(), want["pos"])
    assert np.array_equal(raw(b[1]), want["action"].view(np.uint8).reshape(-1))
    assert np.array_equal(raw(b[2]), want["reward"].view(np.uint8)) and np.array_equal(raw(b[3]), want["discount"].view(np.uint8))
    w = b.weights.cpu().numpy().astype(np.float64)
    assert b.weights.dtype == torch.float32 and float(np.abs(w / want["weights"] - 1).max()) <= 1e-6 and w.max() == 1.0


def renew(vs, vp, pos, td):
    """the restatement's priority update, then the device tree against it: leaves just written to 1e-12 (pow), all others
    bit for bit, the sums those of the device's own leaves, tree[0] the maximum of what it was and the device's new
    leaves.  The restatement continues from the device's leaves, so later comparisons are bit for bit again.  Returns the
    positions written"""
    L, top = vp.L, vp.tree[0]
    written = vp.update(pos, td)
    got = store_tree(vs)
    named = np.array(sorted(written), np.int64)
    if named.size:
        assert float(np.abs(got[L + named] / vp.tree[L + named] - 1).max()) <= 1e-12
    others = np.setdiff1d(np.arange(L), named)
    assert np.array_equal(bits64(got[L + others]), bits64(vp.tree[L + others]))
    assert inner_ok(got) and same_tree(got[1:L], P.build(got[L:])[1:L])
    assert got[0] == max([top] + got[L + named].tolist())
    vp.tree[:] = got
    return written


def test_store_loop_matches_oracle():
    """3R adds; from the first drawable row on, every step consumes the batch the iterator drew one add earlier (its
    prefetch()), renews its priorities with synthetic errors and lets the iterator draw ahead again.  Tree and batches
    are the restatement's at every step.  At the end a batch overtaken by guard_rows adds writes nothing"""
    from drqv2_amd.replay import VecDeviceReplay
    Rr, N, Bs, nstep, gamma, guard = 32, 4, 16, 3, 0.9, 8
    vs = VecDeviceReplay(Rr, N, (FB,), A, nstep, gamma, "cuda", seed=21, guard_rows=guard, priority_alpha=0.6)
    vs.batch_size = Bs
    vp = VP.VecPEROracle(Rr, N, A, FB, nstep, gamma, guard_rows=guard, alpha=0.6, beta=vs.priority_beta, eps=vs.priority_eps)
    assert vs.tree_leaves == vp.L == 128 and vs.tree.dtype == torch.float64 and same_tree(store_tree(vs), vp.tree)
    twin, r = np.random.RandomState(21), rs_(2)
    it = iter(vs)
    held, renewed, partly = None, 0, 0
    for step in range(3 * Rr):
        row = random_row(r, N, p_reset=0.15)
        vp.add(*row)
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
        assert vs.bounds() == vp.bounds() and same_tree(store_tree(vs), vp.tree), step
        lo, hi = vp.bounds()
        if hi < lo:
            continue
        b = next(it)                                               # the batch drawn ahead, one add ago; the first: now
        want = held if held is not None else vp.sample(twin.random_sample(Bs))
        check_batch(b, vs, want)
        td = (10.0 ** r.uniform(-3, 2, Bs)).astype(np.float32)
        b.update_priorities(torch.from_numpy(td).cuda())
        written = renew(vs, vp, want["pos"], td)
        renewed += len(written)
        partly += len(written) < len(set(want["pos"].tolist()))      # a position left the drawable rows with the add
        it.prefetch()
        held = vp.sample(twin.random_sample(Bs))
        check_batch(it._ahead, vs, held)
        assert torch.equal(vs.last_index[2], it._ahead._pos) and vs.last_steps.cpu().tolist() == held["steps"].tolist()
    assert vs.T == 3 * Rr and renewed > 10 * Bs and partly > 0 and vp.tree[0] > 1.0
    assert np.array_equal(store_tree(vs)[vp.L:] > 0, vp.expected_leaf_mask())
    # guard_rows - 1 adds: still written; one more: dropped as a whole
    b = next(it)
    for i in range(guard):
        if i == guard - 1:
            before = store_tree(vs).copy()
            b.update_priorities(torch.full((Bs,), 77.0, device="cuda"))
            assert not same_tree(store_tree(vs), before)
        row = random_row(r, N, p_reset=0.15)
        vp.add(*row)
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
    before = store_tree(vs).copy()
    b.update_priorities(torch.full((Bs,), 1e6, device="cuda"))
    assert same_tree(store_tree(vs), before) and before[0] < 1e3


class WIndexed(tuple):
    """a batch type of the caller's own: indices and frames like an IndexedBatch, a `weights` attribute, no priorities"""


def test_update_fed_by_the_prioritized_ring():
    from drqv2_amd.replay import VecDeviceReplay
    N, Au, Bu, nstep = 3, 3, 16, 3
    fb = int(np.prod(OBS))
    vs = VecDeviceReplay(R, N, OBS, Au, nstep, 0.99, "cuda", seed=5, priority_alpha=0.6)
    vp = VP.VecPEROracle(R, N, Au, fb, nstep, 0.99, guard_rows=8, alpha=0.6, beta=vs.priority_beta, eps=vs.priority_eps)
    feeder = make_agent(Au)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    for t in range(12):
        row = device_row(g, N, Au, feeder, t)
        vs.add(*row)
        vp.add(*(x.cpu().numpy().reshape(N, -1) for x in row[:4]), row[4].cpu().numpy())
    assert same_tree(store_tree(vs), vp.tree)
    # priorities away from the initial plateau, so that the weights differ from 1
    warm = vs.sample(Bu)
    td0 = torch.linspace(0.01, 30.0, Bu, device="cuda")
    warm.update_priorities(td0)
    renew(vs, vp, warm._pos.cpu().numpy(), td0.cpu().numpy())
    b = vs.sample(Bu)
    torch.cuda.synchronize()
    assert float(b.weights.min()) < 1.0 == float(b.weights.max())
    plain = WIndexed((b[0], b[1], b[2], b[3], b[4]))
    plain.frames, plain.weights = b.frames, b.weights
    outs = []
    for batch in (plain, b):                                       # the plain one first: the tree is still what it was
        ag = make_agent(Au)
        reseed()
        m = ag.update(iter([batch]), 0)
        outs.append((m,) + engine_state(ag) + (ag._engine.last_td_abs.clone(),))
    (m0, *s0), (m1, *s1) = outs
    assert m0 == m1 and len(m1) == 8 and all(np.isfinite(v) for v in m1.values())
    for x, y in zip(s0, s1):
        assert torch.equal(x, y)
    td = s1[-1].cpu().numpy()
    written = renew(vs, vp, b._pos.cpu().numpy(), td)
    assert len(written) == len(set(b._pos.tolist()))               # no add in between: every position still drawable


def test_uniform_ring_is_untouched():
    """priority_alpha=None: no tree, plain IndexedBatch objects, and the draws of a seed are VecOracle's (one
    random_sample((B, 4)) per batch), as tests/test_hip_vec_replay.py::test_store_draws_equal_the_oracle_across_wraps
    holds them"""
    from drqv2_amd.replay import IndexedBatch, PrioritizedBatch, VecDeviceReplay
    N, nstep, gamma, Bs, K = 3, 3, 0.9, 40, 4
    vs = VecDeviceReplay(R, N, (FB,), A, nstep, gamma, "cuda", seed=21)
    assert vs.tree is None and vs.priority_alpha is None
    vo = V.VecOracle(R, N, A, FB, nstep, gamma, guard_rows=8)
    twin, r = np.random.RandomState(21), rs_(2)
    for _ in range(2 * R + 3):
        row = random_row(r, N)
        vo.add(*row)
        vs.add(*(torch.from_numpy(x).cuda() for x in row))
        lo, hi = vo.bounds()
        if hi < lo:
            continue
        b = vs.sample(Bs)
        assert type(b) is IndexedBatch and not isinstance(b, PrioritizedBatch) and not hasattr(b, "weights")
        want = vo.sample(twin.random_sample((Bs, K)))
        compare(dict(idx=vs.last_index, act=b[1], rew=b[2], disc=b[3], steps=vs.last_steps), want)
    assert vs.tree is None and vs.T == 2 * R + 3
