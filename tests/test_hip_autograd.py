"""Autograd through the modules (drqv2_amd/autograd.py): Encoder, Actor, Critic and RandomShiftsAug forwards are
differentiable on the HIP kernels.  Gradients are held to the fp64 oracle under torch autograd with the rule of
test_hip_step.py: error vs fp64 <= max(2 x the fp32 oracle's own error, floor), with the HIP path's ReLU decisions
handed to the oracle (a flipped near-zero pre-activation is an O(1) change of its gradient path, not an error)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from drqv2_amd import ops, synth

pytestmark = pytest.mark.gpu

CASES = {
    # name: C, A, F, H, B, weight seed, batch seed
    "small_h64_b6": dict(C=9, A=3, F=20, H=64, B=6, wseed=3, bseed=30),
    "cheetah_b8": dict(C=9, A=6, F=50, H=1024, B=8, wseed=0, bseed=0),
    "humanoid_b4": dict(C=9, A=21, F=100, H=1024, B=4, wseed=1, bseed=10),
    "cheetah_b256": dict(C=9, A=6, F=50, H=1024, B=256, wseed=7, bseed=70),
    "ragged_a1_f37_h96_b5": dict(C=9, A=1, F=37, H=96, B=5, wseed=11, bseed=110),
}
FORBIDDEN = {"ConvolutionBackward0", "MmBackward0", "AddmmBackward0", "NativeLayerNormBackward0", "TanhBackward0",
             "ReluBackward0", "ThresholdBackward0"}


def nerr(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def make_agent(cfg, lr=1e-4, sched="linear(1.0,0.1,500000)"):
    import drqv2
    ag = drqv2.DrQV2Agent((cfg["C"], 84, 84), (cfg["A"],), "cuda", lr, cfg["F"], cfg["H"], 0.01, 2000, 2, sched, 0.3,
                          True)
    enc, actor, critic = synth.make_weights(cfg["C"], cfg["A"], cfg["F"], cfg["H"], cfg["wseed"])
    ag.encoder.load_state_dict(enc)
    ag.actor.load_state_dict(actor)
    ag.critic.load_state_dict(critic)
    ag.critic_target.load_state_dict(critic)
    return ag


def oracle_grads(fn, params, inputs, upstream, dtype):
    """d(sum_k <out_k, upstream_k>) / d(params, inputs) of fn(P, *inputs) in `dtype` on the CPU."""
    P = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in params.items()}
    X = [t.detach().cpu().to(dtype).requires_grad_(True) for t in inputs]
    outs = fn(P, *X)
    outs = outs if isinstance(outs, tuple) else (outs,)
    loss = sum((o * u.detach().cpu().to(dtype)).sum() for o, u in zip(outs, upstream))
    g = torch.autograd.grad(loss, list(P.values()) + X)
    return dict(zip(P, g[:len(P)])), list(g[len(P):])


def check_bound(got, g64, g32, floor, what):
    e_hip, e_o32 = nerr(got, g64), nerr(g32, g64)
    lim = max(2.0 * e_o32, floor)
    assert e_hip <= lim, (what, e_hip, e_o32)


def params_of(mod):
    return {k: p.detach() for k, p in mod.named_parameters()}


def zero_all(ag):
    for opt in (ag.encoder_opt, ag.actor_opt, ag.critic_opt):
        opt.zero_grad()


# ---- 1. per-module gradients against the fp64 oracle ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_module_gradients_match_oracle(name):
    from oracle import drq_oracle as O
    cfg = CASES[name]
    B, A = cfg["B"], cfg["A"]
    ag = make_agent(cfg)
    obs = synth.make_batch(B, A, cfg["C"], seed=cfg["bseed"])[0].cuda()
    gen = torch.Generator().manual_seed(cfg["bseed"])
    zero_all(ag)

    # encoder: parameter gradients (uint8 input)
    feat = ag.encoder(obs)
    saved = feat.grad_fn.saved_tensors
    x, acts = saved[0], saved[1:5]
    g_feat = torch.randn(feat.shape, generator=gen).cuda()
    feat.backward(g_feat)
    masks = [a.cpu() > 0 for a in acts]
    enc_fn = lambda P, xin: O.encoder_forward(P, xin, normalized=True, relu_masks=masks)
    r64, _ = oracle_grads(enc_fn, params_of(ag.encoder), [x], [g_feat], torch.float64)
    r32, _ = oracle_grads(enc_fn, params_of(ag.encoder), [x], [g_feat], torch.float32)
    for k, p in ag.encoder.named_parameters():
        check_bound(p.grad, r64[k], r32[k], 2e-5, ("encoder", k))

    # actor: trunk + policy + tanh, and the gradient of its input features
    f = feat.detach().clone().requires_grad_(True)
    mu = ag.actor(f, 0.2).mean
    _, _, _, _, h1, h2, _ = mu.grad_fn.saved_tensors
    pm = (h1.cpu() > 0, h2.cpu() > 0)
    g_mu = torch.randn(mu.shape, generator=gen).cuda()
    mu.backward(g_mu)
    act_fn = lambda P, fin: torch.tanh(O.mlp3(P, "policy", O.trunk_forward(P, fin), masks=pm))
    r64, (rf64,) = oracle_grads(act_fn, params_of(ag.actor), [f], [g_mu], torch.float64)
    r32, (rf32,) = oracle_grads(act_fn, params_of(ag.actor), [f], [g_mu], torch.float32)
    for k, p in ag.actor.named_parameters():
        check_bound(p.grad, r64[k], r32[k], 2e-3, ("actor", k))
    check_bound(f.grad, rf64, rf32, 2e-3, ("actor", "features"))

    # critic: trunk + two Q heads, gradients of the features and of the action (the actor loss needs it)
    f = feat.detach().clone().requires_grad_(True)
    act = (torch.rand((B, A), generator=gen) * 2 - 1).cuda().requires_grad_(True)
    q1, q2 = ag.critic(f, act)
    cm = {q: tuple(t.cpu() > 0 for t in qq.grad_fn.saved_tensors[4:6]) for q, qq in (("Q1", q1), ("Q2", q2))}
    g1, g2 = torch.randn(q1.shape, generator=gen).cuda(), torch.randn(q2.shape, generator=gen).cuda()
    torch.autograd.backward([q1, q2], [g1, g2])
    cr_fn = lambda P, fin, ain: O.critic_q(P, fin, ain, masks=cm)
    r64, (rf64, ra64) = oracle_grads(cr_fn, params_of(ag.critic), [f, act], [g1, g2], torch.float64)
    r32, (rf32, ra32) = oracle_grads(cr_fn, params_of(ag.critic), [f, act], [g1, g2], torch.float32)
    for k, p in ag.critic.named_parameters():
        check_bound(p.grad, r64[k], r32[k], 2e-5, ("critic", k))
    check_bound(f.grad, rf64, rf32, 2e-5, ("critic", "features"))
    check_bound(act.grad, ra64, ra32, 2e-5, ("critic", "action"))


# ---- 2. input gradients --------------------------------------------------------------------------------------------
def test_encoder_float_input_gradient():
    from oracle import drq_oracle as O
    cfg = CASES["cheetah_b8"]
    ag = make_agent(cfg)
    obs = synth.make_batch(cfg["B"], cfg["A"], 9, seed=3)[0].float().cuda().requires_grad_(True)
    feat = ag.encoder(obs)
    masks = [a.cpu() > 0 for a in feat.grad_fn.saved_tensors[1:5]]
    g = torch.randn(feat.shape, generator=torch.Generator().manual_seed(4)).cuda()
    feat.backward(g)
    fn = lambda P, o: O.encoder_forward(P, o, relu_masks=masks)
    _, (r64,) = oracle_grads(fn, params_of(ag.encoder), [obs], [g], torch.float64)
    _, (r32,) = oracle_grads(fn, params_of(ag.encoder), [obs], [g], torch.float32)
    check_bound(obs.grad, r64, r32, 2e-5, "obs")
    # a stride-2 3x3 layer on 84 pixels never reads row / column 83
    assert torch.count_nonzero(obs.grad[:, :, 83, :]) == 0 and torch.count_nonzero(obs.grad[:, :, :, 83]) == 0
    assert torch.count_nonzero(obs.grad[:, :, :83, :83]) > 0


def test_conv1_input_gradient_kernel_against_conv_transpose():
    """drq_conv1_dgrad alone: dy [B,32,41,41] (in the zero-padded layout) -> dx, against fp64 conv_transpose2d."""
    gen = torch.Generator().manual_seed(5)
    dy = torch.randn((3, 32, 41, 41), generator=gen)
    w = torch.randn((32, 9, 3, 3), generator=gen) * 0.1
    dx = ops.conv1_dgrad(ops.relu_mask_pad(dy.cuda(), None), w.cuda()).cpu()
    ref = F.conv_transpose2d(dy.double(), w.double(), stride=2, output_padding=1)
    assert ref.shape == dx.shape
    assert nerr(dx, ref) <= 1e-6
    assert torch.count_nonzero(dx[:, :, 83]) == 0 and torch.count_nonzero(dx[:, :, :, 83]) == 0


def test_aug_float_input_gradient():
    from oracle import drq_oracle as O
    cfg = CASES["small_h64_b6"]
    ag = make_agent(cfg)
    corners = [(0, 0), (8, 8), (0, 8), (8, 0), (4, 4), (0, 4), (4, 0), (8, 4), (4, 8), (2, 7), (5, 1), (3, 6)]
    sh = torch.tensor(corners, dtype=torch.float32)
    n = sh.shape[0]
    x = synth.make_batch(n, 3, 9, seed=6, smooth=False)[0].float().cuda().requires_grad_(True)
    ag.aug.draw = lambda n_, device, dtype=torch.float32: sh.view(n_, 1, 1, 2).to(device=device, dtype=dtype)
    y = ag.aug(x)
    assert torch.equal(y.detach(), ops.random_shifts_aug(x.detach(), sh.cuda(), 4))
    g = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).cuda()
    y.backward(g)
    fn = lambda P, xin: O.random_shifts_aug(xin, sh.long(), 4)
    _, (r64,) = oracle_grads(fn, {}, [x], [g], torch.float64)
    _, (r32,) = oracle_grads(fn, {}, [x], [g], torch.float32)
    check_bound(x.grad, r64, r32, 2e-5, "aug input")
    for b in range(n):       # per frame as well: every shift, corners included, carries its own weight
        check_bound(x.grad[b], r64[b], r32[b], 2e-5, ("aug input", corners[b]))


# ---- 3. no torch kernels in the backward graph ----------------------------------------------------------------------
def graph_nodes(t):
    seen, stack, names = set(), [t.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        stack.extend(nf for nf, _ in fn.next_functions)
    return names


def test_backward_graph_has_no_torch_conv_or_linear_nodes():
    cfg = CASES["small_h64_b6"]
    ag = make_agent(cfg)
    obs = synth.make_batch(cfg["B"], cfg["A"], 9, seed=8)[0].float().cuda().requires_grad_(True)
    feat = ag.encoder(ag.aug(obs))
    dist = ag.actor(feat, 0.2)
    a = dist.sample(clip=0.3)
    q1, q2 = ag.critic(feat, a)
    loss = -torch.min(q1, q2).mean() + dist.log_prob(a).sum(-1).mean() + feat.pow(2).mean()
    names = graph_nodes(loss)
    assert not (names & FORBIDDEN), names & FORBIDDEN
    for fn in ("RandomShiftsAugFnBackward", "EncoderFnBackward", "TrunkFnBackward", "MLP3FnBackward"):
        assert fn in names, (fn, names)
    loss.backward()
    assert obs.grad is not None and torch.isfinite(obs.grad).all()


# ---- 4. forward values unchanged, nothing kept without grad --------------------------------------------------------
def test_forward_unchanged_and_nothing_saved_without_grad():
    cfg = dict(CASES["cheetah_b8"], B=64)
    ag = make_agent(cfg)
    obs = synth.make_batch(64, cfg["A"], 9, seed=9)[0].cuda()
    act = torch.rand((64, cfg["A"]), generator=torch.Generator().manual_seed(9)).cuda() * 2 - 1
    sh = torch.randint(0, 9, (64, 1, 1, 2), generator=torch.Generator().manual_seed(10)).float()
    ag.aug.draw = lambda n_, device, dtype=torch.float32: sh.to(device=device, dtype=dtype)

    def run():
        xa = ag.aug(obs.float())
        f = ag.encoder(obs)
        fa = ag.encoder(xa)
        mu = ag.actor(f, 0.2).mean
        q1, q2 = ag.critic(f, act)
        return xa, f, fa, mu, q1, q2

    with_grad = run()
    assert all(t.grad_fn is not None for t in with_grad[1:])
    with torch.no_grad():
        no_grad = run()
    assert all(t.grad_fn is None for t in no_grad)
    for a, b in zip(with_grad, no_grad):
        assert torch.equal(a.detach(), b)
    # the values of the forward before this change: the ops it issued, called directly
    x = ops.u8_normalize(obs)
    for li, i in enumerate((0, 2, 4, 6)):
        c = ag.encoder.convnet[i]
        x = ops.conv3x3_fwd(x, c.weight.data, c.bias.data, 2 if li == 0 else 1, relu=True)
    assert torch.equal(x.view(64, -1), no_grad[1])
    # what the encoder keeps: its four activations and its input with grad, nothing without
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    with torch.no_grad():
        f = ag.encoder(obs)
    m_nograd = torch.cuda.memory_allocated() - m0
    del f
    m0 = torch.cuda.memory_allocated()
    f = ag.encoder(obs)
    m_grad = torch.cuda.memory_allocated() - m0
    assert len(f.grad_fn.saved_tensors) == 9
    out_bytes = 64 * 39200 * 4
    assert m_nograd <= out_bytes + (2 << 20), m_nograd
    assert m_grad >= out_bytes + 64 * (9 * 84 * 84 + 32 * (41 * 41 + 39 * 39 + 37 * 37)) * 4, m_grad


# ---- 5. capstone: the reference's update restated on the agent's modules ------------------------------------------
def reference_update(ag, batch, step, snaps):
    """DrQV2Agent.update / update_critic / update_actor of the reference, written against this agent's modules and
    optimisers (autograd + zero_grad / backward / step).  snaps receives the gradients right after each backward."""
    import utils
    obs, action, reward, discount, next_obs = (torch.as_tensor(t, device="cuda") for t in batch)
    obs = ag.aug(obs.float())
    next_obs = ag.aug(next_obs.float())
    obs = ag.encoder(obs)
    with torch.no_grad():
        next_obs = ag.encoder(next_obs)
    m = {"batch_reward": reward.mean().item()}
    std = utils.schedule(ag.stddev_schedule, step)
    with torch.no_grad():
        next_action = ag.actor(next_obs, std).sample(clip=ag.stddev_clip)
        tq1, tq2 = ag.critic_target(next_obs, next_action)
        target_q = reward + discount * torch.min(tq1, tq2)
    q1, q2 = ag.critic(obs, action)
    snaps["critic_masks"] = {q: tuple(t.cpu() > 0 for t in qq.grad_fn.saved_tensors[4:6]) for q, qq in
                             (("Q1", q1), ("Q2", q2))}
    snaps["enc_masks"] = [t.cpu() > 0 for t in obs.grad_fn.saved_tensors[1:5]]
    snaps["enc_in"] = obs.grad_fn.saved_tensors[0].cpu()
    critic_loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
    m.update(critic_target_q=target_q.mean().item(), critic_q1=q1.mean().item(), critic_q2=q2.mean().item(),
             critic_loss=critic_loss.item())
    ag.encoder_opt.zero_grad(set_to_none=True)
    ag.critic_opt.zero_grad(set_to_none=True)
    critic_loss.backward()
    snaps["g_enc"] = {k: p.grad.detach().cpu().clone() for k, p in ag.encoder.named_parameters()}
    snaps["g_critic"] = {k: p.grad.detach().cpu().clone() for k, p in ag.critic.named_parameters()}
    ag.critic_opt.step()
    ag.encoder_opt.step()
    obs = obs.detach()
    dist = ag.actor(obs, std)
    action = dist.sample(clip=ag.stddev_clip)
    log_prob = dist.log_prob(action).sum(-1, keepdim=True)
    aq1, aq2 = ag.critic(obs, action)
    actor_loss = -torch.min(aq1, aq2).mean()
    ag.actor_opt.zero_grad(set_to_none=True)
    actor_loss.backward()
    snaps["g_actor"] = {k: p.grad.detach().cpu().clone() for k, p in ag.actor.named_parameters()}
    ag.actor_opt.step()
    m.update(actor_loss=actor_loss.item(), actor_logprob=log_prob.mean().item(),
             actor_ent=dist.entropy().sum(dim=-1).mean().item())
    utils.soft_update_params(ag.critic, ag.critic_target, ag.critic_target_tau)
    return m


def sync_oracle_state(o, ag):
    dt = o.dtype
    eng = ag._engine
    for name, mod in (("enc", ag.encoder), ("actor", ag.actor), ("critic", ag.critic)):
        dst = getattr(o, name)
        for (k, p), off in zip(mod.named_parameters(), eng.layout[name]):
            n = p.numel()
            dst[k] = p.detach().cpu().to(dt).clone()
            o.m[name][k] = eng.adam_m[off:off + n].view(p.shape).cpu().to(dt).clone()
            o.v[name][k] = eng.adam_v[off:off + n].view(p.shape).cpu().to(dt).clone()
    for k, p in ag.critic_target.named_parameters():
        o.critic_target[k] = p.detach().cpu().to(dt).clone()
    o.t = {"enc": ag.encoder_opt.t, "actor": ag.actor_opt.t, "critic": ag.critic_opt.t}


def agent_state(ag):
    eng = ag._engine
    st = {}
    for name, mod in (("enc", ag.encoder), ("actor", ag.actor), ("critic", ag.critic)):
        for (k, p), off in zip(mod.named_parameters(), eng.layout[name]):
            n = p.numel()
            st[(name, k)] = (p.detach().cpu().clone(), eng.adam_m[off:off + n].view(p.shape).cpu().clone(),
                             eng.adam_v[off:off + n].view(p.shape).cpu().clone())
    st["target"] = {k: p.detach().cpu().clone() for k, p in ag.critic_target.named_parameters()}
    return st


@pytest.mark.parametrize("name", ["small_h64_b6", "cheetah_b8"])
def test_reference_update_through_autograd_matches_oracle(name):
    from oracle import drq_oracle as O
    from torch.distributions.utils import _standard_normal
    cfg = CASES[name]
    B, A = cfg["B"], cfg["A"]
    lr, sched = 1e-4, "linear(1.0,0.1,500000)"
    ag = make_agent(cfg, lr, sched)
    mk = lambda dt: O.OracleAgent(*synth.make_weights(cfg["C"], A, cfg["F"], cfg["H"], cfg["wseed"]), lr,
                                  stddev_schedule=sched, dtype=dt)
    o32, o64 = mk(torch.float32), mk(torch.float64)
    for u in range(3):
        step = 2 * u
        sync_oracle_state(o32, ag)
        sync_oracle_state(o64, ag)
        before = agent_state(ag)
        t_before = {"enc": ag.encoder_opt.t, "critic": ag.critic_opt.t, "actor": ag.actor_opt.t}
        batch = synth.make_batch(B, A, cfg["C"], seed=cfg["bseed"] + u)
        snaps = {}
        torch.manual_seed(500 + u)
        m = reference_update(ag, tuple(x.numpy() for x in batch), step, snaps)
        # the draws the reference's calls consumed, replayed from the same generator state
        torch.manual_seed(500 + u)
        sh_o = torch.randint(0, 9, size=(B, 1, 1, 2), device="cuda", dtype=torch.float32)
        sh_n = torch.randint(0, 9, size=(B, 1, 1, 2), device="cuda", dtype=torch.float32)
        n_c = _standard_normal((B, A), dtype=torch.float32, device="cuda")
        n_a = _standard_normal((B, A), dtype=torch.float32, device="cuda")
        sh_o, sh_n = sh_o.view(B, 2).cpu().long(), sh_n.view(B, 2).cpu().long()
        n_c, n_a = n_c.cpu(), n_a.cpu()
        # encoder inputs as the HIP path formed them (aug + /255 - 0.5), so both sides see identical upstream tensors
        nxt = torch.as_tensor(batch[4]).cuda().float()
        xin_next = (ops.random_shifts_aug(nxt, sh_n.float().cuda(), 4) / 255.0 - 0.5).cpu()
        kw = dict(enc_in_override=(snaps["enc_in"], xin_next), keep=True, relu_masks=snaps["enc_masks"],
                  critic_relu_masks=snaps["critic_masks"])
        m32 = o32.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
        m64 = o64.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
        assert set(m) == set(m64)
        for k in m64:
            assert m[k] == pytest.approx(m64[k], rel=1e-5, abs=1e-5), (u, k, m[k], m32[k], m64[k])
        for key, floor in (("g_enc", 2e-5), ("g_critic", 2e-5), ("g_actor", 2e-3)):
            for k, g in snaps[key].items():
                check_bound(g, o64.last[key][k], o32.last[key][k], floor, (u, key, k))
        # parameters after the steps: the oracle's Adam fed the snapshotted gradients, then Polyak, bit for bit
        for name_, mod, gk in (("enc", ag.encoder, "g_enc"), ("critic", ag.critic, "g_critic"),
                               ("actor", ag.actor, "g_actor")):
            assert getattr(ag, {"enc": "encoder_opt", "critic": "critic_opt", "actor": "actor_opt"}[name_]).t == \
                t_before[name_] + 1
            for k, p in mod.named_parameters():
                p0, m0, v0 = (t.clone() for t in before[(name_, k)])
                O.adam_step(p0, snaps[gk][k], m0, v0, t_before[name_] + 1, lr)
                assert torch.equal(p.detach().cpu(), p0), (u, name_, k)
        crit = dict(ag.critic.named_parameters())
        for k, t in ag.critic_target.named_parameters():
            t0 = before["target"][k].clone()
            O.polyak(crit[k].detach().cpu(), t0, ag.critic_target_tau)
            assert torch.equal(t.detach().cpu(), t0), (u, k)


# ---- 6. optimiser state across fused and autograd steps ------------------------------------------------------------
def test_step_counters_coherent_between_fused_update_and_autograd_steps():
    from oracle import drq_oracle as O
    cfg = CASES["small_h64_b6"]
    B, A = cfg["B"], cfg["A"]
    ag = make_agent(cfg)
    opts = (ag.encoder_opt, ag.critic_opt, ag.actor_opt)
    for u in range(4):
        batch = synth.make_batch(B, A, 9, seed=40 + u)
        if u % 2 == 0:
            ag.update(iter([tuple(x.numpy() for x in batch)]), 2 * u)
        else:
            before = agent_state(ag)
            snaps = {}
            torch.manual_seed(u)
            reference_update(ag, tuple(x.numpy() for x in batch), 2 * u, snaps)
            # the autograd step continued the fused update's Adam: moments and the bias correction of step u + 1
            for k, p in ag.actor.named_parameters():
                p0, m0, v0 = (t.clone() for t in before[("actor", k)])
                O.adam_step(p0, snaps["g_actor"][k], m0, v0, u + 1, ag.actor_opt.lr)
                assert torch.equal(p.detach().cpu(), p0), (u, k)
        assert [o.t for o in opts] == [u + 1] * 3
    st = ag.export_reference_state()
    assert float(st["actor_opt"]["state"][0]["step"]) == 4.0
    assert torch.isfinite(ag._engine.params).all()


# ---- 7. double backward ---------------------------------------------------------------------------------------------
def test_double_backward_raises():
    cfg = CASES["small_h64_b6"]
    ag = make_agent(cfg)
    obs = synth.make_batch(cfg["B"], cfg["A"], 9, seed=11)[0].cuda()
    feat = ag.encoder(obs)
    w = ag.encoder.convnet[0].weight
    (gw,) = torch.autograd.grad(feat.pow(2).sum(), w, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gw.sum().backward()
    mu = ag.actor(feat.detach(), 0.2).mean
    (gp,) = torch.autograd.grad(mu.pow(2).sum(), ag.actor.policy[0].weight, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gp.sum().backward()


def test_module_zero_grad_then_backward_reaches_the_arena():
    """nn.Module.zero_grad() sets .grad to None; autograd then assigns fresh tensors, which step() folds back in."""
    cfg = CASES["small_h64_b6"]
    ag = make_agent(cfg)
    obs = synth.make_batch(cfg["B"], cfg["A"], 9, seed=12)[0].cuda()
    feat = ag.encoder(obs).detach()
    ag.actor.zero_grad()
    assert all(p.grad is None for p in ag.actor.parameters())
    ag.actor(feat, 0.2).mean.pow(2).sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in ag.actor.named_parameters()}
    before = agent_state(ag)
    ag.actor_opt.step()
    eng = ag._engine
    from oracle import drq_oracle as O
    for (k, p), off in zip(ag.actor.named_parameters(), eng.layout["actor"]):
        assert p.grad.data_ptr() == eng.grads.data_ptr() + 4 * off
        assert torch.equal(p.grad, grads[k])
        p0, m0, v0 = (t.clone() for t in before[("actor", k)])
        O.adam_step(p0, grads[k].cpu(), m0, v0, 1, ag.actor_opt.lr)
        assert torch.equal(p.detach().cpu(), p0), k
