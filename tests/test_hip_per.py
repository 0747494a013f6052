"""Prioritized replay on the GPU: the three sum-tree entries and drq_td_mse_w on poisoned, guarded memory against the
float64 restatement of tests/per_oracle.py, whole weighted updates against the plain update (weights 1: bit for bit) and
against PEROracleAgent (random weights), the prioritized store, the loader feeding update(), and the refusals.

Bounds.  Tree: leaves and sums are IEEE double operations the restatement performs in the same order, so positions,
inner nodes and fills are compared bit for bit; pow is held to 1e-12 relative (two fp64 implementations), the weights
to 1e-6 relative (one float32 rounding, 6e-8, plus the device pow).  drq_td_mse_w: what tests/test_hip_entries.py
holds drq_td_mse to (2e-6 normwise, the fixed-order summation bound).  Whole updates: the bounds of
tests/test_hip_step.py::test_update_matches_oracle at the same case; td_abs, which that test has no counterpart of, is
held to the rule it applies to the critic's gradients -- max(2 e_o32, 2e-5) normwise, e_o32 the fp32 restatement's own
distance from fp64 -- because dq, the quantity those gradients start from, is the same difference Q - y."""
import numpy as np
import pytest
import torch

from drqv2_amd import synth
from tests import per_oracle as P
from tests import poison
from tests import test_hip_step as S
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, f32, nerr, out, p, rs_, same_bits, sum_bound
from tests.test_hip_replay import OBS, episode

pytestmark = pytest.mark.gpu
EARG = -1


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_per_sample" in _lib.PROTOTYPES, "the prioritized-replay entries are missing"
    return _lib.load()


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def random_tree(capacity, seed, zero_frac=0.3, top=3.7):
    r = rs_(seed)
    L = P.leaves_of(capacity)
    leaves = np.zeros(L)
    leaves[:capacity] = 10.0 ** r.uniform(-6, 2, capacity)
    leaves[:capacity][r.uniform(size=capacity) < zero_frac] = 0.0
    t = P.build(leaves)
    t[0] = top
    return t


def inner_ok(t):
    L = t.size // 2
    k = np.arange(1, L)
    return np.array_equal(bits64(t[k]), bits64(t[2 * k] + t[2 * k + 1]))


# ------------------------------------------------------------------------------------------------ drq_per_fill
@pytest.mark.parametrize("capacity", [300, 2 ** 20 + 3])
def test_per_fill(lib, capacity):
    """a single slot, a range that crosses several subtrees, the last slots of the store, lo == hi; both modes.  The
    whole tree is read back after every call: leaves exact, every inner node the float64 sum of its children, every node
    outside the range and its ancestors untouched (all three are the restatement's tree, bit for bit)"""
    ref = random_tree(capacity, 7)
    L = ref.size // 2
    assert L == (512 if capacity == 300 else 2 ** 21)
    tree = dev(f64(ref), "tree")
    ranges = [(5, 6, 1), (L // 8 - 3, L // 2 + L // 16 + 1, 1), (capacity - 7, capacity, 0), (11, 11, 1), (9, 10, 0),
              (L // 4 - 1, L // 4 + 2, 0), (capacity - 2, capacity, 1), (0, 1, 1), (L - 2, L, 1)]
    for lo, hi, mode in ranges:
        assert lib.drq_per_fill(p(tree), L, lo, hi, mode, None) == 0
        P.fill(ref, lo, hi, mode)
        got = tree.cpu().numpy()
        assert np.array_equal(bits64(got), bits64(ref)), (lo, hi, mode)
        assert inner_ok(got)
        if hi > lo:
            assert (got[L + lo:L + hi] == (3.7 if mode else 0.0)).all()
    before = tree.clone()
    for bad in ((None, L, 0, 4, 0), (p(tree), L - 1, 0, 4, 0), (p(tree), L, -1, 4, 0), (p(tree), L, 5, 4, 0),
                (p(tree), L, 0, L + 1, 0), (p(tree), L, 0, 4, 2)):
        assert lib.drq_per_fill(*bad, None) == EARG
    torch.cuda.synchronize()
    assert torch.equal(before, tree)


# ------------------------------------------------------------------------------------------------ drq_per_sample
def sample_tree(kind):
    if kind == "mixed":
        return random_tree(300, 21, zero_frac=0.5), 300
    if kind == "single":
        leaves = np.zeros(512)
        leaves[177] = 0.25
        return P.build(leaves), 300
    L = 2 ** 21                                           # two non-zero leaves 2^20 slots apart: depth, index width
    leaves = np.zeros(L)
    leaves[5], leaves[5 + 2 ** 20] = 3.0, 1e-3
    return P.build(leaves), 2 ** 20 + 3


@pytest.mark.parametrize("kind", ["mixed", "single", "far"])
@pytest.mark.parametrize("B", [1, 6, 64, 257, 1100])
def test_per_sample(lib, B, kind):
    ref, capacity = sample_tree(kind)
    L = ref.size // 2
    nstep, beta = 3, 0.4
    n_valid = int((ref[L:] > 0).sum())
    tree = dev(f64(ref), "tree")
    r = rs_(B)
    edge = np.nextafter(1.0, 0.0)
    us = [r.random_sample(B), np.zeros(B), np.full(B, edge)]
    us[0][0], us[0][-1] = 0.0, edge                        # the first row at the very start, the last at the very end
    for u in us:
        idx, w = out(3, B, dtype=torch.int64, name="idx"), out(B, name="weights")
        assert lib.drq_per_sample(p(tree), L, p(dev(f64(u), "u")), B, nstep, n_valid, beta, p(idx), p(w), None) == 0
        back = tree.cpu().numpy()
        assert np.array_equal(bits64(back), bits64(ref))   # the draw does not write the tree
        pos = P.descend(back, u)
        got = idx.cpu().numpy()
        assert np.array_equal(got[2], pos), (kind, B)
        assert np.array_equal(got[0], pos - 1) and np.array_equal(got[1], pos + nstep - 1)
        assert (back[L + got[2]] > 0).all()
        want = P.weights(back, pos, n_valid, beta)
        wh = w.cpu().numpy().astype(np.float64)
        rel = float(np.abs(wh / want - 1).max())
        print(f"per_sample {kind} B={B}: weights max rel err {rel:.3e}, min weight {wh.min():.4g}")
        assert rel <= 1e-6
        assert wh.max() == 1.0
    bad_i, bad_w = (poison.alloc(s, d, "cuda", name="refused", kind="refused") for s, d in
                    (((3, B), torch.int64), ((B,), torch.float32)))
    u = dev(f64(us[0]), "u")
    for args in ((None, L, p(u), B, nstep, n_valid, beta, p(bad_i), p(bad_w)),
                 (p(tree), L, None, B, nstep, n_valid, beta, p(bad_i), p(bad_w)),
                 (p(tree), L, p(u), B, nstep, n_valid, beta, None, p(bad_w)),
                 (p(tree), L, p(u), B, nstep, n_valid, beta, p(bad_i), None),
                 (p(tree), L, p(u), 0, nstep, n_valid, beta, p(bad_i), p(bad_w)),
                 (p(tree), L - 1, p(u), B, nstep, n_valid, beta, p(bad_i), p(bad_w))):
        assert lib.drq_per_sample(*args, None) == EARG


# ------------------------------------------------------------------------------------------------ drq_per_update
@pytest.mark.parametrize("B,scale", [(6, 0.5), (257, 5.0), (1100, 5.0)])
def test_per_update(lib, B, scale):
    """the same position in rows 0, 5 and B-1 (and, at B = 1100 on 2,890 slots, many chance repeats): the highest row
    wins.  scale 0.5: every new leaf is below the old running maximum, which must then stay"""
    alpha, eps = 0.6, 1e-6
    ref = P.new_tree(3000)
    L = ref.size // 2
    ref[0] = 1.25
    P.fill(ref, 10, 2900, 1)
    r = rs_(3 * B)
    pos = r.randint(10, 2900, B)
    pos[0] = pos[5] = pos[B - 1] = 1234
    td = (r.uniform(0, scale, B)).astype(np.float32)
    td[1] = 0.0
    tree = dev(f64(ref), "tree")
    assert lib.drq_per_update(p(tree), L, p(dev(i64(pos), "pos")), p(dev(f32(td), "td")), B, alpha, eps, None) == 0
    got = tree.cpu().numpy()
    want = ref.copy()
    written = P.update(want, pos, td, alpha, eps)
    named = np.array(sorted(written), np.int64)
    rel = float(np.abs(got[L + named] / want[L + named] - 1).max())
    print(f"per_update B={B}: leaves max rel err {rel:.3e}")
    assert rel <= 1e-12
    v_last = (np.float64(td[B - 1]) + eps) ** alpha
    assert abs(got[L + 1234] / v_last - 1) <= 1e-12 and td[B - 1] != td[0] and (B == 6 or td[B - 1] != td[5])
    others = np.setdiff1d(np.arange(L), named)
    assert np.array_equal(bits64(got[L + others]), bits64(ref[L + others]))          # leaves not named: untouched
    assert inner_ok(got)                                                             # sums of the device's own leaves
    assert np.array_equal(bits64(got[1:L]), bits64(P.build(got[L:])[1:L]))
    assert got[0] == max(1.25, got[L + named].max())
    assert (got[0] == 1.25) == (scale < 1)
    before = tree.clone()
    pp, tt = dev(i64(pos), "pos"), dev(f32(td), "td")
    for bad in ((None, L, p(pp), p(tt), B, alpha, eps), (p(tree), L, None, p(tt), B, alpha, eps),
                (p(tree), L, p(pp), None, B, alpha, eps), (p(tree), L, p(pp), p(tt), 0, alpha, eps),
                (p(tree), L + 1, p(pp), p(tt), B, alpha, eps), (p(tree), L, p(pp), p(tt), B, 0.0, eps)):
        assert lib.drq_per_update(*bad, None) == EARG
    torch.cuda.synchronize()
    assert torch.equal(before, tree)


# ------------------------------------------------------------------------------------------------ drq_td_mse_w
@pytest.mark.parametrize("B", [1, 6, 257])
def test_td_mse_w(lib, B):
    r = rs_(77 * B)
    reward, disc = f32(r.uniform(0, 1, B)), f32(np.where(r.uniform(size=B) < 0.1, 0.0, 0.99))
    tq1, tq2 = f32(5 + r.standard_normal(B)), f32(5 + r.standard_normal(B))
    tq2[::3] = tq1[::3]
    q1, q2 = f32(11 + 0.3 * r.standard_normal(B)), f32(-1 + 0.3 * r.standard_normal(B))
    w = f32(r.uniform(0.25, 1.0, B))
    inv = float(np.float32(1.0 / B))
    marker = torch.arange(10.0, 18.0)
    ins = [dev(t) for t in (tq1, tq2, q1, q2, reward, disc)]

    def run(wt):
        dq1, dq2, td, sums = out(B, name="dq1"), out(B, name="dq2"), out(B, name="td_abs"), dev(marker, "sums")
        assert lib.drq_td_mse_w(*(p(t) for t in ins), p(dev(wt, "w")), p(dq1), p(dq2), p(td), p(sums), B, inv, None) == 0
        return dq1, dq2, td, sums

    dq1, dq2, td, sums = run(w)
    d = lambda t: t.double()
    y = d(reward) + d(disc) * torch.minimum(d(tq1), d(tq2))
    e1, e2 = d(q1) - y, d(q2) - y
    errs = nerr(dq1, 2 * d(w) * e1 * inv), nerr(dq2, 2 * d(w) * e2 * inv), nerr(td, 0.5 * (e1.abs() + e2.abs()))
    print(f"td_mse_w B={B}: dq1 {errs[0]:.3e} dq2 {errs[1]:.3e} td_abs {errs[2]:.3e}")
    assert max(errs) <= 2e-6
    s = sums.cpu().double()
    for i, term in enumerate((d(reward), y, d(q1), d(q2), d(w) * (e1 * e1 + e2 * e2))):
        err, bound = abs(float(s[i] - term.sum())), sum_bound(B, term)
        print(f"td_mse_w B={B} sums[{i}]: |hip - fp64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (i, float(s[i]), float(term.sum()))
    assert same_bits(sums[5:], marker[5:])
    # unit weights: drq_td_mse's dq and sums, bit for bit
    u1, u2, utd, usums = run(torch.ones(B))
    p1, p2, psums = out(B, name="dq1"), out(B, name="dq2"), dev(marker, "sums")
    assert lib.drq_td_mse(*(p(t) for t in ins), p(p1), p(p2), p(psums), B, inv, None) == 0
    assert same_bits(u1, p1) and same_bits(u2, p2) and same_bits(usums, psums) and same_bits(utd, td)
    bad = [poison.alloc((B,), torch.float32, "cuda", name="refused", kind="refused") for _ in range(3)]
    wd = dev(w, "w")
    ok = [p(t) for t in ins] + [p(wd), p(bad[0]), p(bad[1]), p(bad[2]), p(sums)]
    for k in range(len(ok)):
        args = list(ok)
        args[k] = None
        assert lib.drq_td_mse_w(*args, B, inv, None) == EARG, k
    assert lib.drq_td_mse_w(*ok, 0, inv, None) == EARG


# ------------------------------------------------------------------------------------------------ whole updates
CASE_NAMES = ("cheetah_b8", "cartpole_b32", "small_h64_b6")


class WBatch(tuple):
    """a batch type of the caller's own: the reference's 5-tuple with a `weights` attribute"""


def run_weighted(ag, cfg, u, w):
    batch = synth.make_batch(cfg["B"], cfg["A"], cfg["C"], seed=cfg["bseed"] + u, smooth=cfg["smooth"])
    draws = synth.make_draws(cfg["B"], cfg["A"], seed=cfg["bseed"] + u)
    ag._draw_hook = lambda n, A: tuple(t.float().cuda() for t in draws)
    b = WBatch(tuple(x.numpy() for x in batch))
    b.weights = w
    return ag.update(iter([b]), cfg["step0"] + 2 * u), batch, draws


def state(ag):
    eng = ag._engine
    torch.cuda.synchronize()
    return eng.params.clone(), eng.grads.clone(), eng.adam_m.clone(), eng.adam_v.clone()


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_unit_weights_are_the_plain_update_bit_for_bit(name, flags):
    cfg = S.CASES[name]
    plain, per = S.make_agent(cfg), S.make_agent(cfg)
    plain._engine.step_flags = per._engine.step_flags = flags
    ones = torch.ones(cfg["B"], device="cuda")
    for u in range(cfg["updates"]):
        m0, _, _ = S.run_hip(plain, cfg, u)
        m1, _, _ = run_weighted(per, cfg, u, ones)
        assert m0 == m1, (u, m0, m1)
        for x, y in zip(state(plain), state(per)):
            assert torch.equal(x, y), u
        td = per._engine.last_td_abs
        assert td is not None and td.shape == (cfg["B"],) and bool(torch.isfinite(td).all()) and bool((td >= 0).all())
        assert plain._engine.last_td_abs is None


def per_oracle_agent(cfg, dtype):
    enc, actor, critic = synth.make_weights(cfg["C"], cfg["A"], cfg["F"], cfg["H"], cfg["wseed"])
    return P.PEROracleAgent(enc, actor, critic, cfg["lr"], stddev_schedule=cfg["sched"], dtype=dtype)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_weighted_update_matches_restatement(name, flags):
    """test_update_matches_oracle with weights drawn from [0.25, 1]: the same injections (the encoder inputs and the ReLU
    decisions of the HIP step), the same bounds; parameters as test_params_after_update_match_oracle_with_same_grads
    holds them: the oracle's Adam fed with the HIP gradients gives the HIP parameters bit for bit"""
    from oracle import drq_oracle as O
    cfg = S.CASES[name]
    ag = S.make_agent(cfg)
    ag._engine.step_flags = flags
    o32, o64 = per_oracle_agent(cfg, torch.float32), per_oracle_agent(cfg, torch.float64)
    B = cfg["B"]
    for u in range(cfg["updates"]):
        step = cfg["step0"] + 2 * u
        if u > 0:
            S.sync_oracle_state(o32, ag)
            S.sync_oracle_state(o64, ag)
        before = {n: {k: v.detach().cpu().clone() for k, v in getattr(ag, n).named_parameters()}
                  for n in ("encoder", "critic", "actor")}
        moments = ag._engine.adam_m.cpu().clone(), ag._engine.adam_v.cpu().clone()
        w = f32(rs_(500 + u).uniform(0.25, 1.0, B))
        m, batch, (sh_o, sh_n, n_c, n_a) = run_weighted(ag, cfg, u, w.cuda())
        xin = S.check_encoder_inputs_bitwise(ag, cfg, batch, sh_o, sh_n)
        acts, crit_masks = S.hip_masks(ag, cfg)
        kw = dict(enc_in_override=(xin[:B], xin[B:]), relu_masks=acts, critic_relu_masks=crit_masks, weights=w)
        m32 = o32.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
        m64 = o64.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
        assert list(m.keys()) == list(m64.keys())
        for k in m64:
            print(f"{name} flags={flags} u={u} {k}: hip {m[k]:.9g} fp32 {m32[k]:.9g} fp64 {m64[k]:.9g}")
        for k in m64:
            assert m[k] == pytest.approx(m64[k], rel=1e-5, abs=1e-5), (u, k, m[k], m32[k], m64[k])
        for nm, mod, key in (("enc", ag.encoder, "g_enc"), ("critic", ag.critic, "g_critic"),
                             ("actor", ag.actor, "g_actor")):
            for (pn, prm), g64, g32 in zip(mod.named_parameters(), o64.last[key].values(), o32.last[key].values()):
                e_hip, e_o32 = S.nerr(prm.grad, g64), S.nerr(g32, g64)
                lim = max(2.0 * e_o32, 2e-5 if nm != "actor" else 2e-3)
                print(f"{name} flags={flags} u={u} {nm} {pn}: hip {e_hip:.3e} fp32 restatement {e_o32:.3e}")
                assert e_hip <= lim, (u, nm, pn, e_hip, e_o32)
        td = ag._engine.last_td_abs
        e_hip, e_o32 = S.nerr(td, o64.last["td_abs"]), S.nerr(o32.last["td_abs"], o64.last["td_abs"])
        print(f"{name} flags={flags} u={u} td_abs: hip {e_hip:.3e} fp32 restatement {e_o32:.3e}")
        assert e_hip <= max(2.0 * e_o32, 2e-5), (u, e_hip, e_o32)
        # parameters: Adam on the HIP gradients, from the state before the update
        eng = ag._engine
        t = {"encoder": ag.encoder_opt.t, "critic": ag.critic_opt.t, "actor": ag.actor_opt.t}
        for n, net in (("encoder", "enc"), ("critic", "critic"), ("actor", "actor")):
            for (k, prm), off in zip(getattr(ag, n).named_parameters(), eng.layout[net]):
                p0 = before[n][k].clone()
                cnt = p0.numel()
                mm, vv = (a[off:off + cnt].view(p0.shape).clone() for a in moments)
                O.adam_step(p0, prm.grad.detach().cpu(), mm, vv, t[n], cfg["lr"])
                assert torch.equal(prm.detach().cpu(), p0), (u, n, k)


# ------------------------------------------------------------------------------------------------ the store
def device_tree(rp):
    torch.cuda.synchronize()
    return rp.tree.cpu().numpy()


def test_store_keeps_exactly_the_drawable_positions():
    from drqv2_amd.replay import DeviceReplay, PrioritizedBatch
    A, nstep, cap = 2, 3, 300
    rp = DeviceReplay(cap, OBS, A, nstep, 0.99, "cuda", seed=9, indexed=True, priority_alpha=0.6)
    L = rp.tree_leaves
    assert L == 512
    r = rs_(4)
    wraps = draws = 0
    last_start = -1
    while wraps < 2 or draws < 200:
        start = rp.add_episode(episode(int(r.randint(3, 40)), A, seed=int(r.randint(1 << 20))))     # 4 .. 40 steps
        wraps += start < last_start
        last_start = start
        t = device_tree(rp)
        want = P.drawable(rp.episodes, nstep)
        nz = set(np.nonzero(t[L:])[0].tolist())
        assert nz == want, (sorted(nz ^ want), rp.episodes)
        assert inner_ok(t) and rp.n_valid == len(want)
        for _ in range(4):
            b = rp.sample(8)
            assert isinstance(b, PrioritizedBatch)
            pos = (b[0] + 1).cpu().numpy()
            assert set(pos.tolist()) <= want, (pos, rp.episodes)
            assert np.array_equal(b[4].cpu().numpy(), pos + nstep - 1)
            b.update_priorities(torch.from_numpy(r.uniform(0, 4, 8).astype(np.float32)).cuda())
            draws += 1
        t = device_tree(rp)
        assert set(np.nonzero(t[L:])[0].tolist()) == want and inner_ok(t)


def test_uniform_store_draws_what_it_always_drew():
    """priority_alpha=None: the positions of a seed are those of the uniform store (restated here: episode uniform, then
    idx uniform in [1, len - nstep + 1], one randint and one random_sample call per batch)"""
    from drqv2_amd.replay import DeviceReplay, IndexedBatch, PrioritizedBatch
    A, nstep = 2, 3
    rp = DeviceReplay(300, OBS, A, nstep, 0.99, "cuda", seed=31, indexed=True)
    assert rp.tree is None
    for i, T in enumerate((12, 30, 2, 25)):         # the third is too short to draw from
        rp.add_episode(episode(T, A, seed=i))
    rng = np.random.RandomState(31)
    starts = np.array([s for s, n in rp.episodes if n - 1 >= nstep])
    lens = np.array([n - 1 for s, n in rp.episodes if n - 1 >= nstep])
    for _ in range(3):
        b = rp.sample(16)
        assert isinstance(b, IndexedBatch) and not isinstance(b, PrioritizedBatch) and not hasattr(b, "weights")
        e = rng.randint(0, len(starts), size=16)
        idx = (rng.random_sample(16) * (lens[e] - nstep + 1)).astype(np.int64) + 1
        assert np.array_equal((b[0] + 1).cpu().numpy(), starts[e] + idx)


def test_priorities_of_an_overtaken_batch_are_dropped():
    from drqv2_amd.replay import DeviceReplay
    A = 2
    rp = DeviceReplay(120, OBS, A, 3, 0.99, "cuda", seed=2, indexed=True, priority_alpha=0.6)
    for i, T in enumerate((40, 40, 30)):
        rp.add_episode(episode(T, A, seed=i))
    b = rp.sample(16)
    rp.add_episode(episode(35, A, seed=9))                        # wraps to slot 0: evicts what b was drawn from
    after_add = device_tree(rp).copy()
    b.update_priorities(torch.full((16,), 50.0, device="cuda"))
    assert np.array_equal(bits64(device_tree(rp)), bits64(after_add))
    b2 = rp.sample(16)
    b2.update_priorities(torch.full((16,), 50.0, device="cuda"))
    assert device_tree(rp)[0] == pytest.approx((50.0 + 1e-6) ** 0.6, rel=1e-12)


# ------------------------------------------------------------------------------------------------ end to end
class Spec:
    def __init__(self, name, shape, dtype):
        self.name, self.shape, self.dtype = name, shape, dtype


class Step(dict):
    def last(self):
        return self["_last"]


class Recording:
    """the loader's iterator with every batch it hands out kept for the test"""

    def __init__(self, it):
        self.it, self.seen = it, []

    def __next__(self):
        self.seen.append(next(self.it))
        return self.seen[-1]

    def prefetch(self):
        self.it.prefetch()


@pytest.mark.parametrize("indexed,updates", [(True, 20), (False, 4)])
def test_loader_feeds_prioritized_updates(tmp_path, indexed, updates):
    import drqv2
    import replay_buffer as rb
    from drqv2_amd.replay import IndexedBatch, PrioritizedBatch
    cfg = S.CASES["cheetah_b8"]
    A, B, nstep, alpha, eps = cfg["A"], cfg["B"], 3, 0.6, 1e-6
    specs = (Spec("observation", OBS, np.uint8), Spec("action", (A,), np.float32), Spec("reward", (1,), np.float32),
             Spec("discount", (1,), np.float32))
    st = rb.ReplayBufferStorage(specs, tmp_path / "buffer")
    loader = rb.make_replay_loader(tmp_path / "buffer", 500, B, 4, False, nstep, 0.99, seed=1, indexed=indexed,
                                   priority_alpha=alpha, priority_eps=eps)

    def add(seed, T=20):
        ep = episode(T, A, seed=seed)
        for t in range(T + 1):
            st.add(Step(observation=ep["observation"][t], action=ep["action"][t], reward=ep["reward"][t],
                        discount=ep["discount"][t], _last=(t == T)))

    for e in range(3):
        add(e)
    rp = rb._entry(tmp_path / "buffer")["store"]
    L = rp.tree_leaves
    torch.manual_seed(5)
    ag = drqv2.DrQV2Agent(OBS, (A,), "cuda", cfg["lr"], cfg["F"], cfg["H"], 0.01, 2000, 2, cfg["sched"], 0.3, True)
    torch.manual_seed(6); torch.cuda.manual_seed_all(6)
    it = Recording(iter(loader))
    for u in range(updates):
        n_eps = len(rp.episodes)
        if u == 2:
            add(50, T=15)                                          # waits for the next draw (the order of the docstring)
            assert len(rp.episodes) == n_eps
        m = ag.update(it, 2 * u)
        assert len(m) == 8 and all(np.isfinite(v) for v in m.values()), (u, m)
        b = it.seen[-1]
        assert isinstance(b, PrioritizedBatch) and isinstance(b, IndexedBatch) == indexed
        assert b.weights.dtype == torch.float32 and b.weights.shape == (B,) and float(b.weights.max()) == 1.0
        td = ag._engine.last_td_abs.cpu().numpy()
        pos = b._pos.cpu().numpy()
        t = device_tree(rp)
        last = {int(q): float(x) for q, x in zip(pos, td)}        # the highest row of a repeated position
        for q, x in last.items():
            assert t[L + q] == pytest.approx((np.float64(np.float32(x)) + eps) ** alpha, rel=1e-12), (u, q)
        assert inner_ok(t)
        if u == 2:                                                 # the draw ahead placed the episode: at the maximum
            assert len(rp.episodes) == n_eps + 1
            s, n = rp.episodes[-1]
            assert (t[L + s + 1:L + s + n - nstep + 1] == t[0]).all() and t[L + s] == 0 and t[L + s + n - 1] == 0
            assert t[0] >= 1.0
    assert set(np.nonzero(device_tree(rp)[L:])[0].tolist()) == P.drawable(rp.episodes, nstep)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from drqv2_amd import _lib
    cfg = S.CASES["small_h64_b6"]
    ag = S.make_agent(cfg)
    B = cfg["B"]
    ones = torch.ones(B, device="cuda")
    t0 = (ag.critic_opt.t, ag.encoder_opt.t, ag.actor_opt.t)
    ag._engine.pg = object()                                       # what enable_data_parallel leaves
    try:
        with pytest.raises(_lib.DrqError, match="data parallelism"):
            run_weighted(ag, cfg, 0, ones)
    finally:
        ag._engine.pg = None
    ag.set_compute_dtype("bf16")
    with pytest.raises(_lib.DrqError, match="bf16"):
        run_weighted(ag, cfg, 0, ones)
    ag.set_compute_dtype("fp32")
    ag.set_behavior_cloning(2.5)
    with pytest.raises(_lib.DrqError, match="behaviour cloning"):
        run_weighted(ag, cfg, 0, ones)
    ag.set_behavior_cloning(None)
    for bad in (torch.ones(B + 1, device="cuda"), torch.ones(B, 1, device="cuda"), torch.ones(B),
                torch.ones(B, device="cuda", dtype=torch.float64)):
        with pytest.raises(_lib.DrqError, match="loss weights"):
            run_weighted(ag, cfg, 0, bad)
    assert (ag.critic_opt.t, ag.encoder_opt.t, ag.actor_opt.t) == t0      # a refused update moved nothing
    m, _, _ = run_weighted(ag, cfg, 0, ones)
    assert len(m) == 8
    ag.set_behavior_cloning(2.5)                                   # afterwards BC still works, on a uniform batch
    m, _, _ = S.run_hip(ag, cfg, 1)
    assert "actor_bc_loss" in m and all(np.isfinite(v) for v in m.values())
