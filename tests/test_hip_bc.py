"""DrQ+BC on the GPU (DrQV2Agent.set_behavior_cloning): the four new C entries on poisoned, guarded memory against the
fp64 closed form, whole updates against the restatement of tests/bc_oracle.py, and the invariants of the feature (the
critic side does not move, off is off, the manual sequence and the device replay give the same update, long runs).

Bounds are the ones the suite already holds the plain forms of these kernels to: normwise 2e-6 for elementwise results
and the Q output layer's input gradient, 3e-6 for GEMM-shaped sums (tests/test_hip_ops.py), the fixed-order summation
bound of tests/test_hip_entries.py for the metric sums; whole updates: metrics rel = abs = 1e-5 against fp64, actor
gradients max(2 e_o32, 2e-3) normwise with e_o32 the fp32 restatement's own error (test_update_matches_oracle)."""
import ctypes

import numpy as np
import pytest
import torch

from drqv2_amd import synth
from tests import bc_oracle, poison
from tests import test_hip_step as S
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, f32, is_sent, nerr, out, p, rnd, rs_, same_bits, sum_bound, wide

pytestmark = pytest.mark.gpu
EARG = -1
BS, AS = (6, 32, 256, 2048), (1, 3, 6, 21)


@pytest.fixture(autouse=True)
def feature_present():
    import drqv2
    assert callable(getattr(drqv2.DrQV2Agent, "set_behavior_cloning", None)), "DrQV2Agent.set_behavior_cloning is missing"


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def parr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ------------------------------------------------------------------------------------------------ op tests
def loss_problem(B, A, centre, Fd=50, std=0.37):
    """Q values around `centre` with exact ties on every third row; the sampled action in columns [Fd, Fd+A) of a wider
    poisoned buffer, the behavioural action in columns [3, 3+A) of another"""
    r = rs_(91 * B + A)
    q1, q2 = f32(centre + r.standard_normal(B)), f32(centre + r.standard_normal(B))
    q2[::3] = q1[::3]
    mu = torch.tanh(f32(r.standard_normal((B, A))))
    a = (mu + f32(r.standard_normal((B, A))) * std).clamp(-1 + 1e-6, 1 - 1e-6)
    ab = f32(r.uniform(-1, 1, (B, A)))
    ha, hb = wide(B, Fd + A, "ha"), wide(B, A + 5, "a_beh")
    ha[:, Fd:] = a.cuda()
    hb[:, 3:3 + A] = ab.cuda()
    return q1, q2, mu, a, ab, ha, hb, Fd, std


def loss_reference(q1, q2, mu, a, ab, std, alpha, inv):
    d = lambda t: t.double()
    qmin = torch.minimum(d(q1), d(q2))
    g = -(alpha / qmin.abs().mean()) * inv
    zero = torch.zeros_like(qmin)
    dq1 = torch.where(q1 < q2, g, torch.where(q1 == q2, 0.5 * g, zero))
    dq2 = torch.where(q2 < q1, g, torch.where(q1 == q2, 0.5 * g, zero))
    lp = torch.distributions.Normal(d(mu), float(np.float32(std))).log_prob(d(a))
    terms = {5: (-qmin, q1.numel()), 6: (lp, a.numel()), 9: ((d(a) - d(ab)) ** 2, a.numel()), 10: (qmin.abs(), q1.numel())}
    return dq1, dq2, terms


def check_sums(tag, sums, marker, terms):
    s = sums.cpu().double()
    for i, (term, n) in terms.items():
        err, bound = abs(float(s[i] - term.sum())), sum_bound(n, term)
        print(f"{tag} sums[{i}]: |hip - fp64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (i, float(s[i]), float(term.sum()), err, bound)
    keep = [i for i in range(marker.numel()) if i not in terms]
    assert same_bits(sums[keep], marker[keep])                   # slots 0..4, 7, 8 and 11.. are not this kernel's


@pytest.mark.parametrize("centre,alpha", [(5.0, 2.5), (0.0, 0.7)])
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("B", BS)
def test_actor_loss_bc(lib, B, A, centre, alpha):
    q1, q2, mu, a, ab, ha, hb, Fd, std = loss_problem(B, A, centre)
    inv = float(np.float32(1.0 / B))
    alpha32 = float(np.float32(alpha))
    marker = torch.arange(10.0, 26.0)
    runs = []
    for _ in range(2):
        dq1, dq2, sums = out(B, name="dq1"), out(B, name="dq2"), dev(marker, "sums")
        rc = lib.drq_actor_loss_bc(p(dev(q1)), p(dev(q2)), ha[:, Fd:].data_ptr(), Fd + A, hb[:, 3:].data_ptr(), A + 5,
                                   p(dev(mu)), std, alpha, p(dq1), p(dq2), p(sums), B, A, inv, None)
        assert rc == 0
        runs.append((dq1, dq2, sums))
    (dq1, dq2, sums), second = runs
    assert all(same_bits(x, y) for x, y in zip(runs[0], second))
    r1, r2, terms = loss_reference(q1, q2, mu, a, ab, std, alpha32, inv)
    e1, e2 = nerr(dq1, r1), nerr(dq2, r2)
    print(f"actor_loss_bc B={B} A={A}: dq1 {e1:.3e} dq2 {e2:.3e}")
    assert e1 <= 2e-6 and e2 <= 2e-6
    assert bool(((dq1 != 0) | (dq2 != 0)).all()) and int((q1 == q2).sum()) == (B + 2) // 3
    assert same_bits(dq1[::3], dq2[::3])                          # ties: half each
    check_sums(f"actor_loss_bc B={B} A={A}", sums, marker, terms)
    assert bool(is_sent(ha[:, :Fd]).all()) and bool(is_sent(hb[:, :3]).all()) and bool(is_sent(hb[:, 3 + A:]).all())
    bad = poison.alloc((B,), torch.float32, "cuda", name="refused", kind="refused")
    assert lib.drq_actor_loss_bc(p(dev(q1)), p(dev(q2)), ha[:, Fd:].data_ptr(), Fd + A, hb[:, 3:].data_ptr(), A + 5,
                                 p(dev(mu)), std, 0.0, p(bad), p(bad), p(sums), B, A, inv, None) == EARG
    assert bool(is_sent(bad).all())


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("B", BS)
def test_qout_bwd_actor_bc(lib, B, A):
    """the fused form: the Q output layer's input gradient with the BC loss inside, both workgroup shapes (64 columns
    below 1,024 rows, 16 from there on), H ragged against both; dq, lambda and the sums must be those of the separate
    loss kernel BIT FOR BIT (every workgroup adds |Qmin| in the same order), which is what makes update() and the
    manual sequence the same update"""
    alpha, H = 2.5, 100
    q1, q2, mu, a, ab, ha, hb, Fd, std = loss_problem(B, A, 5.0)
    inv = float(np.float32(1.0 / B))
    hs = [rnd(B, H, seed=i).clamp_min(0) for i in range(2)]
    ws_ = [rnd(H, seed=10 + i, scale=H ** -0.5) for i in range(2)]
    hd, wd = [dev(t) for t in hs], [dev(t) for t in ws_]
    marker = torch.arange(10.0, 26.0)
    runs = []
    for _ in range(2):
        dh, sums = [out(B, H, name=f"dh{i}") for i in range(2)], dev(marker, "sums")
        rc = lib.drq_qout_bwd_actor_bc(p(dev(q1)), p(dev(q2)), ha[:, Fd:].data_ptr(), Fd + A, hb[:, 3:].data_ptr(), A + 5,
                                       p(dev(mu)), std, alpha, A, inv, p(sums), parr(hd), parr(wd), parr(dh), B, H, None)
        assert rc == 0
        runs.append((dh[0], dh[1], sums))
    assert all(same_bits(x, y) for x, y in zip(*runs))
    dh0, dh1, sums = runs[0]
    r1, r2, terms = loss_reference(q1, q2, mu, a, ab, std, alpha, inv)
    for k, (dh, dq, h, w) in enumerate(((dh0, r1, hs[0], ws_[0]), (dh1, r2, hs[1], ws_[1]))):
        e = nerr(dh, torch.outer(dq, w.double()) * (h > 0).double())
        print(f"qout_bwd_actor_bc B={B} A={A} head {k}: dh {e:.3e}")
        assert e <= 2e-6
    # the sums of a 1024-thread tree against the bound of the 256-thread one (more, shorter chains: the bound holds)
    check_sums(f"qout_bwd_actor_bc B={B} A={A}", sums, marker, terms)
    # the separate loss kernel on the same inputs: the same lambda, hence the same dq, bit for bit
    dq1, dq2, sums2 = out(B, name="dq1"), out(B, name="dq2"), dev(marker, "sums2")
    assert lib.drq_actor_loss_bc(p(dev(q1)), p(dev(q2)), ha[:, Fd:].data_ptr(), Fd + A, hb[:, 3:].data_ptr(), A + 5,
                                 p(dev(mu)), std, alpha, p(dq1), p(dq2), p(sums2), B, A, inv, None) == 0
    assert same_bits(sums[10], sums2[10])
    for dh, dq, h, w in ((dh0, dq1, hd[0], wd[0]), (dh1, dq2, hd[1], wd[1])):
        assert same_bits(dh, torch.where(h > 0, dq[:, None] * w[None, :], torch.zeros((), device="cuda")))


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("B", BS)
def test_actor_dmu_bc(lib, B, A):
    col0, ld = 50, 50 + A + 3
    d1, d2 = wide(B, ld, "dha1"), wide(B, ld, "dha2")
    a1, a2 = rnd(B, A, seed=1), rnd(B, A, seed=2)
    d1[:, col0:col0 + A], d2[:, col0:col0 + A] = a1.cuda(), a2.cuda()
    mu = torch.tanh(rnd(B, A, seed=3))
    a, ab = rnd(B, A, seed=4).clamp(-1, 1), f32(rs_(5).uniform(-1, 1, (B, A)))
    ha, hb = wide(B, 20 + A, "a"), wide(B, A + 2, "a_beh")
    ha[:, 20:], hb[:, :A] = a.cuda(), ab.cuda()
    scale = float(np.float32(2.0 / (B * A))) * 1000.0             # x1000: the pull is as large as da, not lost beside it
    scale = float(np.float32(scale))
    runs = []
    for _ in range(2):
        dpre = out(B, A, name="dpre")
        assert lib.drq_actor_dmu_bc(p(d1), p(d2), ld, col0, p(dev(mu)), ha[:, 20:].data_ptr(), 20 + A, p(hb), A + 2, scale,
                                    p(dpre), B, A, None) == 0
        runs.append(dpre)
    assert same_bits(*runs)
    want = (a1.double() + a2.double() + scale * (a.double() - ab.double())) * (1 - mu.double() ** 2)
    e = nerr(runs[0], want)
    print(f"actor_dmu_bc B={B} A={A}: {e:.3e}")
    assert e <= 2e-6
    assert bool(is_sent(ha[:, :20]).all()) and bool(is_sent(hb[:, A:]).all())
    assert lib.drq_actor_dmu_bc(p(d1), p(d2), ld, col0, p(dev(mu)), None, 20 + A, p(hb), A + 2, scale, p(runs[0]), B, A,
                                None) == EARG
    assert lib.drq_actor_dmu_bc(p(d1), p(d2), ld, col0, p(dev(mu)), ha[:, 20:].data_ptr(), A - 1, p(hb), A + 2, scale,
                                p(runs[0]), B, A, None) == EARG


@pytest.mark.parametrize("form", ["columns", "partials"])
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("B", BS)
def test_policy_out_bwd_bc(lib, B, A, form):
    """the fused output-layer backward: dpre in LDS (B A <= 11264, beyond that the entry refuses and the update takes
    the elementwise form), da as columns of wide buffers or as split-K partial records; 16 columns per workgroup at
    H >= 256, 64 below"""
    H = 64 if B == 6 else 256
    fits = B * A <= 11264
    splitk = 3
    a1, a2 = rnd(B, A, seed=1), rnd(B, A, seed=2)
    mu = torch.tanh(rnd(B, A, seed=3))
    a, ab = rnd(B, A, seed=4).clamp(-1, 1), f32(rs_(5).uniform(-1, 1, (B, A)))
    p2, w = rnd(B, H, seed=6).clamp_min(0), rnd(A, H, seed=7, scale=H ** -0.5)
    ha, hb = wide(B, 20 + A, "a"), wide(B, A + 2, "a_beh")
    ha[:, 20:], hb[:, :A] = a.cuda(), ab.cuda()
    scale = float(np.float32(float(np.float32(2.0 / (B * A))) * 1000.0))
    if form == "columns":
        col0, ld = 50, 50 + A + 3
        d1, d2 = wide(B, ld, "da1"), wide(B, ld, "da2")
        d1[:, col0:col0 + A], d2[:, col0:col0 + A] = a1.cuda(), a2.cuda()
        da = (p(d1), p(d2), ld, col0)
        part, sk = None, 0
        s1, s2 = a1.double(), a2.double()
    else:
        recs = rnd(2 * splitk, B, A, seed=8)
        part, sk = dev(recs, "partials"), splitk
        da = (None, None, A, 0)
        s1, s2 = recs[:splitk].double().sum(0), recs[splitk:].double().sum(0)
    args = lambda dp2, dw, db: (*da, p(dev(mu)), ha[:, 20:].data_ptr(), 20 + A, p(hb), A + 2, scale, p(dev(p2)), p(dev(w)),
                                p(dp2), p(dw), p(db), B, H, A, p(part), sk, None)
    if not fits:
        bad = [poison.alloc(s, torch.float32, "cuda", name="refused", kind="refused") for s in ((B, H), (A, H), (A,))]
        assert lib.drq_policy_out_bwd_bc(*args(*bad)) == EARG
        return
    runs = []
    for _ in range(2):
        o = out(B, H, name="dp2"), out(A, H, name="dw"), out(A, name="db")
        assert lib.drq_policy_out_bwd_bc(*args(*o)) == 0
        runs.append(o)
    assert all(same_bits(x, y) for x, y in zip(*runs))
    dp2, dw, db = runs[0]
    dpre = (s1 + s2 + scale * (a.double() - ab.double())) * (1 - mu.double() ** 2)
    e = (nerr(dp2, (dpre @ w.double()) * (p2 > 0).double()), nerr(dw, dpre.t() @ p2.double()), nerr(db, dpre.sum(0)))
    print(f"policy_out_bwd_bc B={B} A={A} {form}: dp2 {e[0]:.3e} dw {e[1]:.3e} db {e[2]:.3e}")
    assert e[0] <= 3e-6 and e[1] <= 3e-6 and e[2] <= 3e-6
    assert bool(is_sent(ha[:, :20]).all()) and bool(is_sent(hb[:, A:]).all())


# ------------------------------------------------------------------------------------------------ whole updates
BIG = dict(C=9, A=12, F=50, H=1024, B=1024, lr=1e-4, sched="linear(1.0,0.1,500000)", wseed=11, bseed=110, updates=1,
           step0=0, smooth=True)                                  # B A = 12288 > 11264: the elementwise dmu form
UPDATE_CASES = {"cheetah_b8": S.CASES["cheetah_b8"], "cartpole_b32": S.CASES["cartpole_b32"],
                "small_h64_b6": S.CASES["small_h64_b6"], "cheetah_b256": S.WIDE["cheetah_b256"], "quadruped_b1024": BIG}
UPDATE_RUNS = [(n, fl, al) for n in ("cheetah_b8", "cartpole_b32", "small_h64_b6") for fl, al in ((0, 2.5), (1, 2.5), (0, 0.7))]
UPDATE_RUNS += [(n, fl, al) for n in ("cheetah_b256", "quadruped_b1024") for fl, al in ((0, 2.5), (1, 0.7))]


def bc_agent(cfg, alpha, flags=0):
    ag = S.make_agent(cfg)
    ag._engine.step_flags = flags
    return ag.set_behavior_cloning(alpha)


def bc_oracle_agent(cfg, dtype, alpha):
    enc, actor, critic = synth.make_weights(cfg["C"], cfg["A"], cfg["F"], cfg["H"], cfg["wseed"])
    return bc_oracle.BCOracleAgent(enc, actor, critic, cfg["lr"], stddev_schedule=cfg["sched"], dtype=dtype, alpha=alpha)


@pytest.mark.parametrize("name,flags,alpha", UPDATE_RUNS)
def test_bc_update_matches_restatement(name, flags, alpha):
    """test_update_matches_oracle with BC on: the same injections (encoder inputs, ReLU decisions of the HIP step), the
    same bounds; both the fused schedule (flags 0) and the separate row launches (flags 1)."""
    cfg = UPDATE_CASES[name]
    ag = bc_agent(cfg, alpha, flags)
    o32, o64 = bc_oracle_agent(cfg, torch.float32, alpha), bc_oracle_agent(cfg, torch.float64, alpha)
    B = cfg["B"]
    for u in range(min(cfg["updates"], 2)):
        step = cfg["step0"] + 2 * u
        if u > 0:
            S.sync_oracle_state(o32, ag)
            S.sync_oracle_state(o64, ag)
        m, batch, (sh_o, sh_n, n_c, n_a) = S.run_hip(ag, cfg, u)
        xin = S.check_encoder_inputs_bitwise(ag, cfg, batch, sh_o, sh_n)
        acts, crit_masks = S.hip_masks(ag, cfg)
        kw = dict(enc_in_override=(xin[:B], xin[B:]), relu_masks=acts, critic_relu_masks=crit_masks)
        m32 = o32.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
        m64 = o64.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
        assert list(m.keys()) == list(m64.keys()) and list(m)[-2:] == ["actor_bc_loss", "actor_bc_lambda"]
        for k in m64:
            print(f"{name} flags={flags} alpha={alpha} u={u} {k}: hip {m[k]:.9g} fp32 {m32[k]:.9g} fp64 {m64[k]:.9g}")
        for k in m64:
            assert m[k] == pytest.approx(m64[k], rel=1e-5, abs=1e-5), (u, k, m[k], m32[k], m64[k])
        for (pn, prm), g64, g32 in zip(ag.actor.named_parameters(), o64.last["g_actor"].values(),
                                       o32.last["g_actor"].values()):
            e_hip, e_o32 = S.nerr(prm.grad, g64), S.nerr(g32, g64)
            print(f"{name} flags={flags} alpha={alpha} u={u} actor {pn}: hip {e_hip:.3e} fp32 restatement {e_o32:.3e}")
            assert e_hip <= max(2.0 * e_o32, 2e-3), (u, pn, e_hip, e_o32)
        # the critic side is the plain update's: its gradients against the same oracle, the existing bound
        for nm, mod, key in (("enc", ag.encoder, "g_enc"), ("critic", ag.critic, "g_critic")):
            for (pn, prm), g64, g32 in zip(mod.named_parameters(), o64.last[key].values(), o32.last[key].values()):
                assert S.nerr(prm.grad, g64) <= max(2.0 * S.nerr(g32, g64), 2e-5), (u, nm, pn)


def full_state(ag):
    eng = ag._engine
    torch.cuda.synchronize()
    return eng.params.clone(), eng.grads.clone(), eng.adam_m.clone(), eng.adam_v.clone()


@pytest.mark.parametrize("name", ["cheetah_b8", "cheetah_b256"])
def test_critic_side_does_not_move(name):
    """two agents, same seed, same draws and batch, one with BC: encoder / critic gradients, stepped encoder, critic
    and target parameters, their Adam moments and the first five metric sums are bit-identical; the actor differs"""
    cfg = UPDATE_CASES[name]
    plain, bc = S.make_agent(cfg), bc_agent(cfg, 2.5)
    S.run_hip(plain, cfg, 0)
    S.run_hip(bc, cfg, 0)
    seg = plain._engine.layout["seg"]
    sp, sb = full_state(plain), full_state(bc)
    for net in ("enc", "critic", "target"):
        b, e = seg[net]
        for x, y in zip(sp, sb):
            assert torch.equal(x[b:e], y[b:e]), net
    b, e = seg["actor"]
    assert not torch.equal(sp[1][b:e], sb[1][b:e]) and not torch.equal(sp[0][b:e], sb[0][b:e])
    assert torch.equal(plain._engine.sums[:5], bc._engine.sums[:5])
    assert torch.equal(plain._engine.sums[5:7], bc._engine.sums[5:7])      # sum -Qmin and the log-prob sum: the same a


def test_turning_bc_off_again():
    """set_behavior_cloning(None) after BC updates: the next update is bit-identical to that of an agent that never had
    BC and was given the same state"""
    import pickle
    cfg = UPDATE_CASES["cheetah_b8"]
    ag = bc_agent(cfg, 2.5)
    for u in range(2):
        S.run_hip(ag, cfg, u)
    torch.cuda.synchronize()
    st = ag.__getstate__()
    st.pop("bc_alpha")
    import drqv2
    twin = object.__new__(drqv2.DrQV2Agent)
    twin.__setstate__(pickle.loads(pickle.dumps(st)))
    twin._engine.store_aug_next = True
    assert twin._engine.bc_alpha is None
    ag.set_behavior_cloning(None)
    ma, _, _ = S.run_hip(ag, cfg, 2)
    mb, _, _ = S.run_hip(twin, cfg, 2)
    assert ma == mb and "actor_bc_loss" not in ma
    for x, y in zip(full_state(ag), full_state(twin)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["cheetah_b8", "cartpole_b32"])
def test_manual_sequence_with_bc_equals_update(name):
    """encode -> update_critic -> update_actor with BC on is update() bit for bit, generator state included (modelled
    on test_update_critic_update_actor_as_separate_calls_equal_update); update_actor uses the action update_critic got"""
    import utils
    cfg = UPDATE_CASES[name]
    batches = [synth.make_batch(cfg["B"], cfg["A"], cfg["C"], seed=cfg["bseed"] + u, smooth=cfg["smooth"]) for u in range(2)]
    outs = []
    for manual in (False, True):
        ag = bc_agent(cfg, 2.5)
        ag._engine.fused_rng = False
        torch.manual_seed(123)
        torch.cuda.manual_seed_all(123)
        ms = []
        for u, batch in enumerate(batches):
            step = cfg["step0"] + 2 * u
            if not manual:
                ms.append(ag.update(iter([tuple(x.numpy() for x in batch)]), step))
                continue
            obs, action, reward, discount, next_obs = utils.to_torch(tuple(x.numpy() for x in batch), ag.device)
            m = {"batch_reward": float(reward.float().mean())}
            f_obs, f_next = ag.encode(obs, next_obs, step)
            m.update(ag.update_critic(f_obs, action, reward, discount, f_next, step))
            action.fill_(float("nan"))                # the caller's tensor is not needed any more
            del action
            m.update(ag.update_actor(f_obs.detach(), step))
            utils.soft_update_params(ag.critic, ag.critic_target, ag.critic_target_tau)
            ms.append(m)
        torch.cuda.synchronize()
        eng = ag._engine
        outs.append((ms, eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.cuda.get_rng_state()))
    (m0, p0, am0, av0, r0), (m1, p1, am1, av1, r1) = outs
    assert torch.equal(r0, r1)
    assert torch.equal(p0, p1) and torch.equal(am0, am1) and torch.equal(av0, av1)
    for a, b in zip(m0, m1):
        assert list(a) == list(b) and list(a)[-2:] == ["actor_bc_loss", "actor_bc_lambda"]
        for k in a:
            assert a[k] == pytest.approx(b[k], rel=1e-6, abs=1e-7), k
        assert a["actor_bc_lambda"] == b["actor_bc_lambda"]      # the same bits of sum |Qmin| in both loss kernels


def test_device_replay_with_bc():
    """update() fed by an IndexedBatch equals the materialised batch bit for bit with BC on (the iterator draws the next
    batch beside the running update: the behavioural action of the running one must not be its victim)"""
    import drqv2
    from drqv2_amd.replay import DeviceReplay, IndexedBatch
    from tests.test_hip_replay import OBS, episode
    A, B = 6, 64
    outs = []
    for indexed in (False, True):
        rp = DeviceReplay(400, OBS, A, 3, 0.99, "cuda", seed=5, indexed=indexed)
        for i, T in enumerate((40, 25, 60)):
            rp.add_episode(episode(T, A, seed=20 + i))
        rp.batch_size = B
        torch.manual_seed(3)
        ag = drqv2.DrQV2Agent(OBS, (A,), "cuda", 1e-4, 50, 1024, 0.01, 2000, 2, "linear(1.0,0.1,500000)", 0.3, True)
        ag.set_behavior_cloning(2.5)
        torch.manual_seed(11); torch.cuda.manual_seed_all(11)
        it = iter(rp)
        ms = [ag.update(it, 2 * u) for u in range(4)]
        torch.cuda.synchronize()
        assert isinstance(next(it), IndexedBatch) == indexed
        eng = ag._engine
        outs.append((ms, eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
    (m0, *a0), (m1, *a1) = outs
    assert m0 == m1 and all("actor_bc_loss" in m for m in m0)
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)


def test_metrics_on_device_with_bc():
    cfg = UPDATE_CASES["small_h64_b6"]
    a, b = bc_agent(cfg, 2.5), bc_agent(cfg, 2.5)
    b.metrics_on_device = True
    for u in range(2):
        ma, _, _ = S.run_hip(a, cfg, u)
        mb, _, _ = S.run_hip(b, cfg, u)
        assert list(ma.keys()) == list(mb.keys()) and len(ma) == 10
        assert all(torch.is_tensor(v) and v.dim() == 0 for v in mb.values())
        assert all(v.is_cuda for k, v in mb.items() if k != "actor_ent")
        for k in ma:
            assert float(mb[k].item()) == pytest.approx(ma[k], rel=1e-6, abs=1e-7), (u, k)
    assert torch.equal(a._engine.params, b._engine.params)


def test_long_run_stable_and_finite():
    """20 BC updates: two agents bit-identical (metrics and state); 100: every metric finite"""
    cfg = UPDATE_CASES["small_h64_b6"]
    a, b = bc_agent(cfg, 2.5), bc_agent(cfg, 2.5)
    for u in range(100):
        ma, _, _ = S.run_hip(a, cfg, u)
        assert len(ma) == 10 and all(np.isfinite(v) for v in ma.values()), (u, ma)
        if u < 20:
            mb, _, _ = S.run_hip(b, cfg, u)
            assert ma == mb, u
        if u == 19:
            for x, y in zip(full_state(a), full_state(b)):
                assert torch.equal(x, y)
