"""FlatAdam on the arenas for the reference's own loop (zero_grad / backward / step), without a GPU."""
import torch


def make_cpu_agent():
    import drqv2
    return drqv2.DrQV2Agent((9, 84, 84), (3,), "cpu", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, False)


def arena_view(ag, net, i, p):
    off = ag._engine.layout[net][i]
    return ag._engine.grads[off:off + p.numel()]


def test_zero_grad_zeroes_the_segment_and_reattaches_views():
    ag = make_cpu_agent()
    eng = ag._engine
    seg = eng.layout["seg"]
    for net, mod, opt in (("enc", ag.encoder, ag.encoder_opt), ("critic", ag.critic, ag.critic_opt),
                          ("actor", ag.actor, ag.actor_opt)):
        b, e = seg[net]
        with torch.no_grad():
            eng.grads.fill_(3.0)
        mod.zero_grad()                         # nn.Module.zero_grad(): .grad -> None
        assert all(p.grad is None for p in mod.parameters())
        opt.zero_grad(set_to_none=True)
        assert torch.count_nonzero(eng.grads[b:e]) == 0
        assert torch.count_nonzero(eng.grads[:b]) == b and torch.count_nonzero(eng.grads[e:]) == eng.grads.numel() - e
        for i, p in enumerate(mod.parameters()):
            assert p.grad is not None
            assert p.grad.data_ptr() == arena_view(ag, net, i, p).data_ptr()
            assert p.grad.shape == p.shape


def test_backward_accumulates_into_the_arena_in_place():
    """autograd adds into a defined .grad in place: a CPU-side loss over the arena-backed parameters lands in the
    gradient arena (the HIP modules' backwards reach it the same way)."""
    ag = make_cpu_agent()
    ag.critic_opt.zero_grad()
    w = ag.critic.Q1[4].weight
    view = w.grad
    (w * 2.0).sum().backward()
    (w * 3.0).sum().backward()
    assert w.grad is view
    assert torch.equal(w.grad, torch.full_like(w, 5.0))
    i = [p is w for p in ag.critic.parameters()].index(True)
    assert torch.equal(arena_view(ag, "critic", i, w), torch.full((w.numel(),), 5.0))


def test_fold_replaced_and_missing_grads_into_the_arena():
    ag = make_cpu_agent()
    opt = ag.actor_opt
    opt.zero_grad()
    with torch.no_grad():
        ag._engine.grads.fill_(7.0)
    params = list(ag.actor.parameters())
    params[0].grad = torch.ones_like(params[0])          # replaced by the user
    params[1].grad = None                                # dropped
    opt._fold_grads()
    assert torch.equal(arena_view(ag, "actor", 0, params[0]), torch.ones(params[0].numel()))
    assert torch.count_nonzero(arena_view(ag, "actor", 1, params[1])) == 0
    assert torch.equal(arena_view(ag, "actor", 2, params[2]), torch.full((params[2].numel(),), 7.0))
    for i, p in enumerate(params):
        assert p.grad.data_ptr() == arena_view(ag, "actor", i, p).data_ptr()
