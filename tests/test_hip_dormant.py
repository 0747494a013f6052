"""DrM building blocks on the GPU: drq_dormant_scores / drq_dormant_count / drq_lerp_flat on poisoned, guarded memory
against the numpy restatement of tests/dormant_oracle.py, and DrQV2Agent.dormant_ratio() / perturb() against the oracle's
modules and the restated lerp.

Bounds.  Scores of the op test: (rows + 2) * 2^-24 relative per unit, the bound of a sum of `rows` non-negative terms
(dormant_oracle.score_bound).  Counts, the layer mean and the lerp: equality, bit for bit.  Scores of dormant_ratio(): 2e-6
of the layer's largest score against the fp64 forward (the bound test_act_matches_oracle holds the same forward to);
its counts: equality, on inputs whose fp64 scores all keep a margin from the threshold that this bound cannot bridge --
asserted on the oracle's numbers before the GPU's are looked at."""
import functools
import pickle

import numpy as np
import pytest
import torch

from drqv2_amd import synth
from tests import dormant_oracle as DO
from tests import poison
from tests import test_hip_step as S
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import bits, cap, dev, f32, is_sent, out, p, rnd, rs_, same_bits, wide  # noqa: F401

pytestmark = pytest.mark.gpu
EARG = -1
TOL = 2e-6
CASE_NAMES = ("cheetah_b8", "cartpole_b32", "small_h64_b6")
# the weight seed of each case, chosen on the fp64 oracle alone: the seeds (of 0..11) whose scores keep the largest
# margin from the threshold at BOTH values of tau, in multiples of what margin_ok() asks for -- cheetah 5.1 / 12.1 (the
# case's own seed 0: 4.1 / 0.11), cartpole 6.4 / 7.4 (its own seed 2: 1.1 / 9.7), small 14.2 / 65.8 (its own)
WSEED = {"cheetah_b8": 2, "cartpole_b32": 3, "small_h64_b6": 3}
TAUS = (0.025, 0.5)


@pytest.fixture(autouse=True)
def feature_present():
    import drqv2
    from drqv2_amd import _lib
    assert "drq_dormant_scores" in _lib.PROTOTYPES, "the dormant-ratio entries are missing"
    assert callable(getattr(drqv2.DrQV2Agent, "dormant_ratio", None)), "DrQV2Agent.dormant_ratio is missing"
    assert callable(getattr(drqv2.DrQV2Agent, "perturb", None)), "DrQV2Agent.perturb is missing"


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ drq_dormant_scores
@pytest.mark.parametrize("rows,units,ld", [(1, 1, 1), (6, 50, 50), (7, 64, 70), (257, 1024, 1024), (1024, 6, 56),
                                           (1030, 33, 40)])
def test_dormant_scores(lib, rows, units, ld):
    x = rnd(rows, units, seed=rows + units, mean=0.3).numpy()
    x[:, ::5] *= 1e-3                                          # columns of very different scale
    if units > 2:
        x[:, 2] = 0.0                                          # a dead unit: its score is exactly 0
    src = wide(rows, ld, "act")
    src[:, :units] = f32(x).cuda()
    runs = []
    for _ in range(2):
        score = out(units, name="score")
        assert lib.drq_dormant_scores(p(src), ld, rows, units, p(score), None) == 0
        runs.append(score)
    assert same_bits(*runs)
    ref = DO.scores(x)
    got = runs[0].cpu().numpy()
    err, bound = np.abs(got.astype(np.float64) - ref), DO.score_bound(rows, ref)
    print(f"dormant_scores {rows}x{units}: worst |hip - fp64| / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (float(err.max()), int((err > bound).sum()))
    assert units <= 2 or got[2] == 0.0
    assert bool(is_sent(src[:, units:]).all())                 # the gap between the rows is neither read into a result ...
    # NaN: its own column only
    src[rows // 2, units - 1] = float("nan")
    score = poison.partial(out(units, name="score_nan"))
    assert lib.drq_dormant_scores(p(src), ld, rows, units, p(score), None) == 0
    assert bool(torch.isnan(score[units - 1])) and same_bits(score[:units - 1], runs[0][:units - 1])
    assert not bool(is_sent(score).any())
    refused = poison.alloc((units,), torch.float32, "cuda", name="refused", kind="refused")
    for bad in ((ld, 0, units), (ld, rows, 0), (units - 1, rows, units)):
        assert lib.drq_dormant_scores(p(src), bad[0], bad[1], bad[2], p(refused), None) == EARG


# ------------------------------------------------------------------------------------------------ drq_dormant_count
@pytest.mark.parametrize("units", [1, 50, 64, 1024, 1030])
def test_dormant_count(lib, units):
    cases = [(0.25, *DO.known_scores(units, 0.25))]
    if units == 1:
        cases.append((1.0, *DO.known_scores(units, 1.0)))
    r = rs_(units)
    general = (r.uniform(0.0, 1.0, units) * 10.0 ** r.uniform(-6, 2, units) * (r.uniform(size=units) < 0.8)).astype(np.float32)
    for tau in (0.0, 0.025, 0.3, 1.0):
        cases.append((tau, general, None))
    cases.append((0.025, np.zeros(units, np.float32), units))  # all zero: every unit
    for tau, s, known in cases:
        want, _, m = DO.count(s, tau)
        assert known is None or want == known
        runs = []
        for _ in range(2):
            cnt, mean = dev(i32([0, 0]), "count"), out(1, name="mean")
            assert lib.drq_dormant_count(p(dev(f32(s), "score")), units, tau, p(cnt), p(mean), None) == 0
            runs.append((cnt, mean))
        assert all(same_bits(a, b) for a, b in zip(*runs))
        cnt, mean = runs[0]
        assert cnt.tolist() == [want, units], (units, tau, cnt.tolist(), want)
        assert mean.cpu().numpy().tobytes() == np.float32(m).tobytes(), (units, tau)
    # three layers into one pair, on top of what it held; no mean asked for
    cnt, total = dev(i32([5, 7]), "count3"), [5, 7]
    for tau, s, _ in cases[:1] + cases[-3:-1]:
        assert lib.drq_dormant_count(p(dev(f32(s), "score")), units, tau, p(cnt), None, None) == 0
        total = [total[0] + DO.count(s, tau)[0], total[1] + units]
    assert cnt.tolist() == total
    refused = poison.alloc((2,), torch.int32, "cuda", name="refused", kind="refused")
    sc = dev(f32(general), "score")
    assert lib.drq_dormant_count(p(sc), units, -0.5, p(refused), None, None) == EARG
    assert lib.drq_dormant_count(p(sc), 0, 0.5, p(refused), None, None) == EARG
    assert lib.drq_dormant_count(p(sc), units, float("nan"), p(refused), None, None) == EARG


# ------------------------------------------------------------------------------------------------ drq_lerp_flat
ALPHAS = (0.0, 1.0, 0.5, 0.9, 1e-3)


def lerp_case(lib, n, a, off_p, off_p0, special=False):
    """p and p0 start off_p / off_p0 floats into their allocations: the elements before them must not move"""
    x, x0 = rnd(n + off_p, seed=n + 1).numpy(), rnd(n + off_p0, seed=n + 2, scale=3.0).numpy()
    if special and n >= 8:
        x[off_p:off_p + 4] = (0.0, -0.0, np.inf, -np.inf)
        x0[off_p0 + 4:off_p0 + 6] = (0.0, -0.0)
    want = DO.lerp(x[off_p:], x0[off_p0:], a)
    pd, qd = dev(f32(x), f"p n={n}"), dev(f32(x0), f"p0 n={n}")
    assert lib.drq_lerp_flat(pd[off_p:].data_ptr(), qd[off_p0:].data_ptr(), n, a, None) == 0
    got = pd.cpu().numpy()
    assert got[off_p:].tobytes() == want.tobytes(), (n, a, off_p, off_p0, int((got[off_p:].view(np.int32) != want.view(np.int32)).sum()))
    assert got[:off_p].tobytes() == x[:off_p].tobytes() and qd.cpu().numpy().tobytes() == x0.tobytes()
    if a == 1.0:
        assert got.tobytes() == x.tobytes()
    if a == 0.0:
        assert got[off_p:].tobytes() == x0[off_p0:].tobytes()


@pytest.mark.parametrize("a", ALPHAS)
def test_lerp_flat(lib, a, cap):
    for n in (0, 1, 3, 4, 5, 1023, 1025):
        lerp_case(lib, n, a, 0, 0, special=True)
        lerp_case(lib, n, a, 1, 1)                              # both 4 bytes past a 16-byte boundary: scalar head of 3
        lerp_case(lib, n, a, 1, 0)                              # misaligned against each other: scalar throughout
        lerp_case(lib, n, a, 2, 3)
    if a == 0.9:
        lerp_case(lib, 4 * cap + 4 * 300 + 3, a, 3, 3)          # more 16-byte vectors than one pass of the grid covers
        lerp_case(lib, cap + 300, a, 0, 1)                      # ... and more scalars
    x = rnd(64, seed=9)
    pd, qd = dev(x, "p refused"), dev(rnd(64, seed=10), "p0")
    for n, bad in ((64, 1.5), (64, -0.25), (64, float("nan")), (-1, 0.5)):
        assert lib.drq_lerp_flat(p(pd), p(qd), n, bad, None) == EARG
    assert lib.drq_lerp_flat(p(pd) + 2, p(qd), 8, 0.5, None) == EARG
    assert same_bits(pd, x)


def test_ops_wrappers():
    from drqv2_amd import _lib, ops
    x = rnd(40, 33, seed=4)
    s = ops.dormant_scores(dev(x))
    ref = DO.scores(x.numpy())
    assert (np.abs(s.cpu().numpy().astype(np.float64) - ref) <= DO.score_bound(40, ref)).all()
    s20 = ops.dormant_scores(dev(x), units=20)
    assert same_bits(s20, s[:20])
    cnt = dev(i32([0, 0]))
    mean = ops.dormant_count(s, 0.5, cnt)
    want, units, m = DO.count(s.cpu().numpy(), 0.5)
    assert cnt.tolist() == [want, units] and mean.cpu().numpy().tobytes() == np.float32(m).tobytes()
    a, b = dev(rnd(77, seed=5)), dev(rnd(77, seed=6))
    before = a.cpu().numpy().copy()
    assert ops.lerp_flat(a, b, 0.25) is a
    assert a.cpu().numpy().tobytes() == DO.lerp(before, b.cpu().numpy(), 0.25).tobytes()
    with pytest.raises(_lib.DrqError):
        ops.lerp_flat(a, b, 1.5)
    with pytest.raises(_lib.DrqError):
        ops.lerp_flat(a, b[:50], 0.5)


# ------------------------------------------------------------------------------------------------ dormant_ratio()
def case_cfg(name):
    return dict(S.CASES[name], wseed=WSEED[name])


def case_inputs(cfg):
    batch = synth.make_batch(cfg["B"], cfg["A"], cfg["C"], seed=cfg["bseed"], smooth=cfg["smooth"])
    return batch[0], batch[1]


@functools.lru_cache(maxsize=None)
def oracle_layers(name):
    """the fp64 forward of a case, computed once and shared"""
    cfg = case_cfg(name)
    enc, actor, critic = synth.make_weights(cfg["C"], cfg["A"], cfg["F"], cfg["H"], cfg["wseed"])
    obs, action = case_inputs(cfg)
    return DO.forward_layers(enc, actor, critic, obs, action, ("actor", "critic"))


def margin_ok(layers, tau):
    """every fp64 score is further from its layer's threshold than scores within TOL of the layer's largest can move
    the comparison: the score by TOL smax, the mean (hence the threshold) by tau TOL smax; twice that is asked for"""
    for name, act in layers.items():
        s = np.abs(act.numpy()).mean(0)
        thr, room = tau * s.mean(), 2 * (1 + tau) * TOL * s.max()
        if s.mean() == 0 or float(np.abs(s - thr).min()) <= room:
            return False
    return True


def check_against_oracle(ag, layers, tau, nets):
    """per-layer scores within TOL of the layer's largest, counts and the ratio equal to the oracle's"""
    _, per = DO.ratio_of({k: v for k, v in layers.items() if k.split(".")[0] in nets}, tau)
    # the ratio as the agent forms it: two integers, exact as float32, one float32 division
    want_ratio = np.float32(sum(d for d, _, _, _ in per.values())) / np.float32(sum(u for _, u, _, _ in per.values()))
    assert list(ag.last_dormant) == list(per) == list(ag.last_dormant_scores)
    for name, (d, u, m, s) in per.items():
        got = ag.last_dormant_scores[name].cpu().numpy().astype(np.float64)
        s64 = np.abs(layers[name].numpy()).mean(0)
        err = float(np.abs(got - s64).max() / s64.max())
        print(f"dormant_ratio {name}: score error {err:.3e} of the largest score, {d} of {u} dormant")
        assert err <= TOL, (name, err)
        gd, gu, gm = ag.last_dormant[name]
        assert (int(gd), int(gu)) == (d, u), (name, int(gd), d)
        assert abs(float(gm) - float(s64.mean())) <= TOL * s64.max()
    return want_ratio


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_dormant_ratio_matches_oracle(name, tau):
    cfg = case_cfg(name)
    layers = oracle_layers(name)
    assert margin_ok(layers, tau), "the reference's own scores lie too close to a threshold: pick another weight seed"
    ag = S.make_agent(cfg)
    obs, action = (t.cuda() for t in case_inputs(cfg))
    F, H = cfg["F"], cfg["H"]
    ratio = ag.dormant_ratio(obs, action, tau=tau, nets=("actor", "critic"))
    assert ratio.is_cuda and ratio.dim() == 0 and ratio.dtype == torch.float32
    want = check_against_oracle(ag, layers, tau, ("actor", "critic"))
    assert sum(int(u) for _, u, _ in ag.last_dormant.values()) == F + 2 * H + F + 4 * H
    assert float(ratio) == float(want) and 0.0 <= float(ratio) <= 1.0
    # the actor alone (the default): its three layers, the same numbers
    ratio_a = ag.dormant_ratio(obs, tau=tau)
    want_a = check_against_oracle(ag, layers, tau, ("actor",))
    assert list(ag.last_dormant) == ["actor.trunk", "actor.policy.0", "actor.policy.2"]
    assert sum(int(u) for _, u, _ in ag.last_dormant.values()) == F + 2 * H and float(ratio_a) == float(want_a)
    # the order of nets does not matter, a single row works
    assert float(ag.dormant_ratio(obs, action, tau=tau, nets=("critic", "actor"))) == float(ratio)
    one = ag.dormant_ratio(obs[:1], tau=tau)
    assert 0.0 <= float(one) <= 1.0


def test_dormant_ratio_hand_built():
    """a hidden unit whose incoming weights and bias are zero is counted; scaling a layer leaves its count unchanged"""
    name, tau = "small_h64_b6", 0.025
    cfg = case_cfg(name)
    ag = S.make_agent(cfg)
    obs, action = case_inputs(cfg)
    enc, actor, critic = synth.make_weights(cfg["C"], cfg["A"], cfg["F"], cfg["H"], cfg["wseed"])
    ag.dormant_ratio(obs.cuda(), tau=tau)
    base = {k: (int(d), ag.last_dormant_scores[k].clone()) for k, (d, u, m) in ag.last_dormant.items()}
    j = int(base["actor.policy.0"][1].argmax())                 # the liveliest unit of the first hidden layer
    with torch.no_grad():
        ag.actor.policy[0].weight[j].zero_()
        ag.actor.policy[0].bias[j].zero_()
    actor["policy.0.weight"][j] = 0.0
    actor["policy.0.bias"][j] = 0.0
    layers = DO.forward_layers(enc, actor, critic, obs, None, ("actor",))
    assert margin_ok(layers, tau)
    ag.dormant_ratio(obs.cuda(), tau=tau)
    check_against_oracle(ag, layers, tau, ("actor",))
    assert float(ag.last_dormant_scores["actor.policy.0"][j]) == 0.0
    assert int(ag.last_dormant["actor.policy.0"][0]) == base["actor.policy.0"][0] + 1
    # x4 on the weights and bias of a ReLU layer is x4 on its output, exactly: the same count, four times the scores
    before = (int(ag.last_dormant["actor.policy.0"][0]), ag.last_dormant_scores["actor.policy.0"].clone())
    with torch.no_grad():
        ag.actor.policy[0].weight.mul_(4.0)
        ag.actor.policy[0].bias.mul_(4.0)
    ag.dormant_ratio(obs.cuda(), tau=tau)
    assert int(ag.last_dormant["actor.policy.0"][0]) == before[0]
    assert same_bits(ag.last_dormant_scores["actor.policy.0"], before[1] * 4.0)


def test_dormant_ratio_moves_nothing():
    """no generator, no optimiser state, no weight moves; the updates around the call are the updates without it"""
    cfg = case_cfg("small_h64_b6")
    obs, action = (t.cuda() for t in case_inputs(cfg))
    outs = []
    for probe in (False, True):
        ag = S.make_agent(cfg)
        eng = ag._engine
        ms = []
        for u in range(2):
            if probe:
                state = (torch.cuda.get_rng_state(), torch.random.get_rng_state(), eng.params.clone(), eng.adam_m.clone(),
                         eng.adam_v.clone(), (ag.encoder_opt.t, ag.actor_opt.t, ag.critic_opt.t))
                ag.dormant_ratio(obs, action, nets=("actor", "critic"))
                after = (torch.cuda.get_rng_state(), torch.random.get_rng_state(), eng.params, eng.adam_m, eng.adam_v,
                         (ag.encoder_opt.t, ag.actor_opt.t, ag.critic_opt.t))
                assert all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(state, after))
            ms.append(S.run_hip(ag, cfg, u)[0])
        torch.cuda.synchronize()
        outs.append((ms, eng.params.clone(), eng.grads.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
    (m0, *a0), (m1, *a1) = outs
    assert m0 == m1
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)


def test_dormant_ratio_refusals():
    from drqv2_amd._lib import DrqError
    cfg = case_cfg("small_h64_b6")
    ag = S.make_agent(cfg)
    obs, action = (t.cuda() for t in case_inputs(cfg))
    for bad in (obs.float(), obs.cpu(), obs[:, :6], obs[:0], obs.permute(0, 1, 3, 2), obs[0]):
        with pytest.raises(DrqError):
            ag.dormant_ratio(bad)
    for bad in (action[:2], action.double(), action.cpu(), action[:, :1], action.t().contiguous().t()):
        with pytest.raises(DrqError):
            ag.dormant_ratio(obs, bad, nets=("critic",))
    assert ag.last_dormant is None


# ------------------------------------------------------------------------------------------------ perturb()
def agent_arena(ag):
    return ag._engine.params.detach().cpu().numpy().copy()


def fresh_p0(cfg, seed, nets):
    """the fresh weights perturb() draws from a generator seeded `seed`, rebuilt here: the same constructors in the same
    order under the same seed -> {net: {parameter name: tensor}}"""
    import drqv2
    dims = (32 * 35 * 35, (cfg["A"],), cfg["F"], cfg["H"])
    make = {"encoder": lambda: drqv2.Encoder((cfg["C"], 84, 84)), "actor": lambda: drqv2.Actor(*dims),
            "critic": lambda: drqv2.Critic(*dims)}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        return {n: dict(make[n]().named_parameters()) for n in ("encoder", "actor", "critic") if n in nets}


def expected_arena(ag, before, p0, alpha):
    """the whole parameter arena after perturb(): every parameter of the named nets (and the target's, from the
    critic's p0) is oracle.lerp(before, p0); everything else -- other nets, the gaps between tensors -- keeps its bits"""
    eng = ag._engine
    want = before.copy()
    mods = {"encoder": ("enc", ag.encoder), "actor": ("actor", ag.actor), "critic": ("critic", ag.critic)}
    for net, fresh in p0.items():
        key, mod = mods[net]
        for seg in ((key, "target") if net == "critic" else (key,)):
            for (k, prm), off in zip(mod.named_parameters(), eng.layout[seg]):
                n = prm.numel()
                want[off:off + n] = DO.lerp(before[off:off + n], fresh[k].detach().numpy().reshape(-1), alpha)
    return want


@pytest.mark.parametrize("name,alpha,nets", [("small_h64_b6", 0.5, ("encoder", "actor", "critic")),
                                             ("small_h64_b6", 0.9, ("actor",)), ("small_h64_b6", 1e-3, ("critic",)),
                                             ("cheetah_b8", 0.8, ("encoder", "actor", "critic"))])
def test_perturb_is_the_lerp_toward_fresh_weights(name, alpha, nets):
    cfg = case_cfg(name)
    ag = S.make_agent(cfg)
    eng = ag._engine
    S.run_hip(ag, cfg, 0)                                       # Adam moments, and a target that is not the critic
    torch.cuda.synchronize()
    before = agent_arena(ag)
    moments = (eng.adam_m.clone(), eng.adam_v.clone(), (ag.encoder_opt.t, ag.actor_opt.t, ag.critic_opt.t))
    glob = (torch.random.get_rng_state(), torch.cuda.get_rng_state())
    g = torch.Generator().manual_seed(77)
    assert ag.perturb(alpha, nets=nets, generator=g) is ag
    assert not torch.equal(g.get_state(), torch.Generator().manual_seed(77).get_state())      # the draw came from g
    assert torch.equal(glob[0], torch.random.get_rng_state()) and torch.equal(glob[1], torch.cuda.get_rng_state())
    want = expected_arena(ag, before, fresh_p0(cfg, 77, nets), alpha)
    got = agent_arena(ag)
    assert got.tobytes() == want.tobytes(), int((got.view(np.int32) != want.view(np.int32)).sum())
    assert (got != before).any()
    assert torch.equal(eng.adam_m, moments[0]) and torch.equal(eng.adam_v, moments[1])
    assert (ag.encoder_opt.t, ag.actor_opt.t, ag.critic_opt.t) == moments[2]
    # the modules' state_dict()s are views of the arena: they show the new values
    for mod, key in ((ag.encoder, "enc"), (ag.actor, "actor"), (ag.critic, "critic"), (ag.critic_target, "target")):
        for (k, v), off in zip(mod.state_dict().items(), eng.layout[key]):
            assert v.data_ptr() == eng.params[off:].data_ptr()
            assert v.cpu().numpy().tobytes() == want[off:off + v.numel()].tobytes()
    # training goes on
    m = S.run_hip(ag, cfg, 1)[0]
    assert all(np.isfinite(v) for v in m.values()) and bool(torch.isfinite(eng.params).all())


def test_perturb_global_generator_and_alpha_edges():
    import drqv2
    cfg = case_cfg("small_h64_b6")
    ag = S.make_agent(cfg)
    S.run_hip(ag, cfg, 0)
    torch.cuda.synchronize()
    before = agent_arena(ag)
    # alpha = 1: nothing moves, nothing is drawn
    g = torch.Generator().manual_seed(5)
    gs, glob = g.get_state(), torch.random.get_rng_state()
    ag.perturb(1.0, generator=g)
    ag.perturb(1.0)
    assert agent_arena(ag).tobytes() == before.tobytes()
    assert torch.equal(g.get_state(), gs) and torch.equal(torch.random.get_rng_state(), glob)
    # no generator: the global one, advanced exactly as the three constructors advance it
    dims = (39200, (cfg["A"],), cfg["F"], cfg["H"])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(123)
        ag.perturb(0.25)
        after_state = torch.random.get_rng_state()
        torch.manual_seed(123)
        drqv2.Encoder((9, 84, 84)), drqv2.Actor(*dims), drqv2.Critic(*dims)
        assert torch.equal(torch.random.get_rng_state(), after_state)
    want = expected_arena(ag, before, fresh_p0(cfg, 123, ("encoder", "actor", "critic")), 0.25)
    assert agent_arena(ag).tobytes() == want.tobytes()
    # alpha = 0: a re-initialisation -- the state_dict()s of an agent constructed under the same seed
    ag.perturb(0.0, generator=torch.Generator().manual_seed(31))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(31)
        new = drqv2.DrQV2Agent((cfg["C"], 84, 84), (cfg["A"],), "cuda", cfg["lr"], cfg["F"], cfg["H"], 0.01, 2000, 2,
                               cfg["sched"], 0.3, True)
    for n in ("encoder", "actor", "critic", "critic_target"):
        a, b = getattr(ag, n).state_dict(), getattr(new, n).state_dict()
        assert list(a) == list(b) and all(same_bits(a[k], b[k]) for k in a), n


def test_perturb_flush_pickle_and_data_parallel_refusal():
    from drqv2_amd._lib import DrqError
    cfg = case_cfg("small_h64_b6")
    arenas = []
    for flush in (False, True):
        ag = S.make_agent(cfg)
        S.run_hip(ag, cfg, 0)
        if flush:
            ag.flush()
        ag.perturb(0.5, generator=torch.Generator().manual_seed(9))
        arenas.append(agent_arena(ag))
    assert arenas[0].tobytes() == arenas[1].tobytes()           # a deferred optimiser step lands before the lerp
    back = pickle.loads(pickle.dumps(ag))
    for n in ("encoder", "actor", "critic", "critic_target"):
        a, b = getattr(ag, n).state_dict(), getattr(back, n).state_dict()
        assert all(same_bits(a[k], b[k]) for k in a), n
    assert agent_arena(back).tobytes() == arenas[1].tobytes()
    ag._engine.pg = object()                                    # a data-parallel engine: refused, nothing moves
    try:
        g = torch.Generator().manual_seed(1)
        gs = g.get_state()
        with pytest.raises(DrqError, match="data parallelism"):
            ag.perturb(0.5, generator=g)
        with pytest.raises(DrqError, match="data parallelism"):
            ag._engine.perturb(0.5, {})
        assert torch.equal(g.get_state(), gs)
    finally:
        ag._engine.pg = None
    assert agent_arena(ag).tobytes() == arenas[1].tobytes()
