"""DrQV2Agent.act_batch on the GPU: parity with the float64 oracle, the generator contract, fresh weights after an
update, no interference with training, routing of large batches, input / output forms."""
import io

import numpy as np
import pytest
import torch
from torch.distributions.utils import _standard_normal

import utils
from drqv2_amd import synth
from drqv2_amd._lib import DrqError
from oracle import drq_oracle as O
from tests.test_hip_step import CASES, make_agent, nerr, run_hip

pytestmark = pytest.mark.gpu

CONFIGS = ("cheetah_b8", "humanoid_b4", "small_h64_b6")
ROWS = (1, 2, 3, 7, 16, 64)
# (max |a - ref|, normwise error) against the float64 oracle: the bounds the suite already applies to this quantity
# (test_act_matches_oracle: 2e-6; test_module_forwards_and_soft_update: 5e-6).  Where the parent path
# (engine.act_forward, same inputs, same oracle) itself exceeds them the bound is twice the parent's measured maximum
# over ROWS.  Measured on an MI355X (maxima over ROWS, abs / normwise): the parent stays inside both bounds at every
# config, so no bound is widened.
BOUNDS = {
    "cheetah_b8": (2e-6, 5e-6),      # parent 1.35e-7 / 4.7e-7, act_batch 1.45e-7 / 6.9e-7
    "humanoid_b4": (2e-6, 5e-6),     # parent 1.72e-7 / 5.5e-7, act_batch 1.69e-7 / 4.8e-7
    "small_h64_b6": (2e-6, 5e-6),    # parent 4.28e-7 / 8.5e-7, act_batch 3.57e-7 / 8.8e-7
}
_cache = {}


def _setup(name):
    """One agent per config, 64 frames and their float64 mean actions.  The engine routes batches above
    ACT_FUSED_MAX_ROWS to the training kernels; these agents raise the limit so that every n below runs csrc/act.hip
    (routing itself has tests of its own at the end of the file)."""
    if name not in _cache:
        cfg = CASES[name]
        ag = make_agent(cfg)
        ag._engine.ACT_FUSED_MAX_ROWS = 64
        obs = synth.make_batch(64, cfg["A"], 9, seed=11)[0]
        enc, actor, _ = synth.make_weights(cfg["C"], cfg["A"], cfg["F"], cfg["H"], cfg["wseed"])
        mu64 = _oracle_mu(enc, actor, obs)
        _cache[name] = (cfg, ag, obs, mu64)
    return _cache[name]


def _oracle_mu(enc_sd, actor_sd, obs):
    d = lambda sd: {k: v.detach().double().cpu() for k, v in sd.items()}
    return O.actor_mu(d(actor_sd), O.encoder_forward(d(enc_sd), obs.double()))


def _errs(a, ref):
    a = a.detach().double().cpu()
    return float((a - ref).abs().max()), nerr(a, ref)


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", CONFIGS)
def test_mean_matches_oracle(name, n):
    cfg, ag, obs, mu64 = _setup(name)
    dev = obs[:n].cuda()
    a = ag.act_batch(dev, 5000, True)
    assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (n, cfg["A"])
    new = _errs(a, mu64[:n])
    parent = _errs(ag._engine.act_forward(dev), mu64[:n])
    print(f"act_batch parity {name} n={n}: new abs {new[0]:.3e} nerr {new[1]:.3e} | parent abs {parent[0]:.3e} "
          f"nerr {parent[1]:.3e}")
    assert new[0] <= BOUNDS[name][0] and new[1] <= BOUNDS[name][1]


@pytest.mark.parametrize("name,n", [("cheetah_b8", 7), ("humanoid_b4", 16), ("small_h64_b6", 64)])
def test_sample_matches_oracle_and_consumes_one_normal_draw(name, n):
    cfg, ag, obs, mu64 = _setup(name)
    step = 5000
    assert step >= ag.num_expl_steps
    torch.manual_seed(17)
    noise = _standard_normal((n, cfg["A"]), dtype=torch.float32, device=torch.device("cuda"))
    state = torch.cuda.get_rng_state()
    torch.manual_seed(17)
    a = ag.act_batch(obs[:n].cuda(), step, False)
    assert torch.equal(torch.cuda.get_rng_state(), state)
    std = utils.schedule(cfg["sched"], step)
    ref = O.trunc_normal_sample(mu64[:n], noise.double().cpu(), std, None)
    err = _errs(a, ref)
    print(f"act_batch sample parity {name} n={n}: abs {err[0]:.3e} nerr {err[1]:.3e}")
    assert err[0] <= BOUNDS[name][0] and err[1] <= BOUNDS[name][1]
    assert float(a.abs().max()) <= float(np.float32(1.0 - 1e-6))
    assert not torch.equal(a, ag.act_batch(obs[:n].cuda(), step, True))


def test_one_frame_consumes_the_generator_like_act():
    cfg, ag, obs, _ = _setup("cheetah_b8")
    frame = obs[0].numpy()
    for step in (5000, 10):                      # sampling; sampling + the uniform exploration override
        torch.manual_seed(5)
        want = ag.act(frame, step, False)
        state = torch.cuda.get_rng_state()
        torch.manual_seed(5)
        got = ag.act_batch(frame[None], step, False)
        assert torch.equal(torch.cuda.get_rng_state(), state)
        assert got.shape == (1, cfg["A"]) and np.abs(got[0] - want).max() <= 2 * BOUNDS["cheetah_b8"][0]


@pytest.mark.parametrize("n", [1, 5, 64])
def test_exploration_branch_is_torchs_uniform_after_the_normal_draw(n):
    cfg, ag, obs, _ = _setup("cheetah_b8")
    assert 10 < ag.num_expl_steps
    dev = torch.device("cuda")
    torch.manual_seed(23)
    _standard_normal((n, cfg["A"]), dtype=torch.float32, device=dev)
    want = torch.empty(n, cfg["A"], device=dev).uniform_(-1.0, 1.0)
    torch.manual_seed(23)
    got = ag.act_batch(obs[:n].cuda(), 10, False)
    assert torch.equal(got, want)


def test_weights_are_read_fresh_after_an_update():
    cfg = CASES["cheetah_b8"]
    ag = make_agent(cfg)
    obs = synth.make_batch(4, cfg["A"], 9, seed=12)[0]        # fused size
    a1 = ag.act_batch(obs.cuda(), 5000, True)
    run_hip(ag, cfg, 0)
    a2 = ag.act_batch(obs.cuda(), 5000, True)
    ref = _oracle_mu(ag.encoder.state_dict(), ag.actor.state_dict(), obs)
    err = _errs(a2, ref)
    print(f"act_batch after update: abs {err[0]:.3e} nerr {err[1]:.3e}; moved {float((a2 - a1).abs().max()):.3e}")
    assert err[0] <= BOUNDS["cheetah_b8"][0] and err[1] <= BOUNDS["cheetah_b8"][1]
    assert not torch.equal(a1, a2)


def test_acting_between_encode_and_update_critic_changes_nothing():
    cfg = CASES["cheetah_b8"]
    batch = synth.make_batch(cfg["B"], cfg["A"], cfg["C"], seed=cfg["bseed"], smooth=cfg["smooth"])
    frames = synth.make_batch(4, cfg["A"], 9, seed=13)[0].cuda()       # fused size: own scratch
    outs = []
    for acting in (False, True):
        ag = make_agent(cfg)
        ag._engine.fused_rng = False
        if acting:
            ag.act_batch(frames, 5000, True)          # its scratch exists before the update starts, too
        torch.manual_seed(123)
        torch.cuda.manual_seed_all(123)
        obs, action, reward, discount, next_obs = utils.to_torch(tuple(x.numpy() for x in batch), ag.device)
        f_obs, f_next = ag.encode(obs, next_obs, 0)
        if acting:
            ag.act_batch(frames, 5000, True)
        m = dict(ag.update_critic(f_obs, action, reward, discount, f_next, 0))
        if acting:
            ag.act_batch(frames[:3], 5000, True)
        m.update(ag.update_actor(f_obs.detach(), 0))
        utils.soft_update_params(ag.critic, ag.critic_target, ag.critic_target_tau)
        torch.cuda.synchronize()
        eng = ag._engine
        outs.append((m, eng.params.clone(), eng.adam_m.clone(), eng.adam_v.clone()))
    (m0, p0, am0, av0), (m1, p1, am1, av1) = outs
    assert m0 == m1
    assert torch.equal(p0, p1) and torch.equal(am0, am1) and torch.equal(av0, av1)


def test_acting_between_updates_changes_nothing():
    cfg = CASES["cheetah_b8"]
    frames = synth.make_batch(4, cfg["A"], 9, seed=14)[0].cuda()
    ends = []
    for acting in (False, True):
        ag = make_agent(cfg)
        ms = []
        for u in range(3):
            if acting:
                ag.act_batch(frames, 5000 + u, False)
            ms.append(run_hip(ag, cfg, u)[0])
        if acting:
            ag.act_batch(frames, 5000, True)
        torch.cuda.synchronize()
        ends.append((ms, ag._engine.params.clone()))
    assert ends[0][0] == ends[1][0]
    assert torch.equal(ends[0][1], ends[1][1])


def test_large_batches_are_routed_through_the_training_kernels():
    """n above StepEngine.ACT_FUSED_MAX_ROWS with a B = 8 step workspace: chunks of 16 rows through drq_act_forward.
    (The fused path takes every (A, F, H) the engine accepts, so there is no excluded shape to route.)"""
    cfg = CASES["cheetah_b8"]
    ag = make_agent(cfg)
    run_hip(ag, cfg, 0)
    n = 200
    assert n > ag._engine.ACT_FUSED_MAX_ROWS and ag._engine._ws_B == cfg["B"]
    obs = synth.make_batch(n, cfg["A"], 9, seed=15)[0]
    ref = _oracle_mu(ag.encoder.state_dict(), ag.actor.state_dict(), obs)
    a = ag.act_batch(obs.cuda(), 5000, True)
    err = _errs(a, ref)
    print(f"act_batch routed n={n}: abs {err[0]:.3e} nerr {err[1]:.3e}")
    assert tuple(a.shape) == (n, cfg["A"]) and err[0] <= BOUNDS["cheetah_b8"][0] and err[1] <= BOUNDS["cheetah_b8"][1]
    assert ag._engine._ws_B == cfg["B"]                     # the step workspace was not re-sized
    assert ag._engine._act_ws is None                       # ... and the fused path never ran on this agent
    a16 = ag.act_batch(obs[:16].cuda(), 5000, True)         # the shipped crossover: 16 rows are routed as well
    assert ag._engine._act_ws is None and _errs(a16, ref[:16])[0] <= BOUNDS["cheetah_b8"][0]
    a4 = ag.act_batch(obs[:4].cuda(), 5000, True)           # ... and 4 rows are not
    assert ag._engine._act_ws is not None and _errs(a4, ref[:4])[0] <= BOUNDS["cheetah_b8"][0]
    torch.manual_seed(3)
    noise = _standard_normal((n, cfg["A"]), dtype=torch.float32, device=torch.device("cuda"))
    torch.manual_seed(3)
    s = ag.act_batch(obs.cuda(), 5000, False)
    sref = O.trunc_normal_sample(ref, noise.double().cpu(), utils.schedule(cfg["sched"], 5000), None)
    assert _errs(s, sref)[0] <= BOUNDS["cheetah_b8"][0]


def test_input_and_output_forms():
    cfg, ag, obs, mu64 = _setup("small_h64_b6")
    A = cfg["A"]
    a_np = ag.act_batch(obs[:4].numpy(), 5000, True)
    assert isinstance(a_np, np.ndarray) and a_np.dtype == np.float32 and a_np.shape == (4, A)
    a_host = ag.act_batch(obs[:4], 5000, True)                 # host tensor: as numpy
    assert isinstance(a_host, np.ndarray) and np.array_equal(a_host, a_np)
    a_dev = ag.act_batch(obs[:4].cuda(), 5000, True)
    assert isinstance(a_dev, torch.Tensor) and a_dev.is_cuda and np.array_equal(a_dev.cpu().numpy(), a_np)
    strided = obs[:8][::2]                                     # non-contiguous input is made contiguous
    assert np.array_equal(ag.act_batch(strided.cuda(), 5000, True).cpu().numpy(),
                          ag.act_batch(strided.contiguous().cuda(), 5000, True).cpu().numpy())
    with pytest.raises(DrqError):
        ag.act_batch(obs[:4].float().cuda(), 5000, True)
    with pytest.raises(DrqError):
        ag.act_batch(obs[:4, :, :80].cuda(), 5000, True)
    with pytest.raises(DrqError):
        ag.act_batch(obs[0].cuda(), 5000, True)                # one frame needs its leading axis
    with pytest.raises(DrqError):
        ag._engine.act_batch_forward(obs[:4])                  # the engine takes device tensors only
    with pytest.raises(DrqError):
        ag._engine.act_batch_forward(obs[:4].cuda(), torch.zeros(4, A + 1, device="cuda"), 0.1)


def test_pickle_roundtrip_keeps_acting():
    cfg, ag, obs, _ = _setup("small_h64_b6")
    before = ag.act_batch(obs[:3].cuda(), 5000, True)
    buf = io.BytesIO()
    torch.save({"agent": ag}, buf)
    buf.seek(0)
    ag2 = torch.load(buf, weights_only=False)["agent"]
    assert ag2._engine._act_ws is None
    assert torch.equal(ag2.act_batch(obs[:3].cuda(), 5000, True), before)
