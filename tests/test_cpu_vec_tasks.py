"""Tasks and action repeat of the device environment (drq_vec_task_step, VecReach(action_repeat=), VecPointMass): everything
that needs no GPU.  The numpy restatement tests/vec_tasks_oracle.py against the older one (tests/vec_env_oracle.py) at
repeat 1 and against that one folded by the wrapper rule at repeat k, the point mass by hand, the public surface, the
DRQ_EARG cases (all are decided before any launch), the constructors and the state dicts, and the condition on the inputs
of the GPU tests (tests/test_hip_vec_tasks.py), which is a property of the oracle's run alone."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_env_oracle as E
from tests import vec_skeleton_oracle as S
from tests import vec_tasks_oracle as T
from tests.vec_skeleton_oracle import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "drq_vec_task_step"
F = np.float32


def same_state(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        same_bits(got[k], want[k], (what, k))


def wild(r, o, A, s):
    return T.wild_actions(r, o, A, s)


# ------------------------------------------------------------------------------------------------ the oracle, reach
def test_reach_at_repeat_1_is_the_reach_oracle_bit_for_bit():
    """300 steps, N = 5, episode_length 9: frames, reward, discount, first and the state after every step; substeps is 1
    on a step row and 0 on a reset row.  Actions hold NaN, +-inf and |a| > 1; two environments home, so targets are hit"""
    N, A, L, SEED = 5, 3, 9, 21
    new, old = T.TaskOracle("reach", N, episode_length=L, seed=SEED, repeat=1), E.ReachOracle(N, episode_length=L, seed=SEED)
    same_bits(new.reset(), old.reset(), "first frame")
    same_state(new.state(), old.state(), "reset")
    r = np.random.RandomState(1)
    seen = np.zeros(3, bool)
    for s in range(300):
        a = wild(r, old, A, s)
        seen |= [np.isnan(a[:, :2]).any(), np.isinf(a[:, :2]).any(), (np.abs(a[:, :2][np.isfinite(a[:, :2])]) > 1).any()]
        got, want = new.step(a), old.step(a)
        for name, g, w in zip(("frame", "reward", "discount", "first"), got, want):
            same_bits(g, w, (s, name))
        same_bits(got[4], (1 - want[3]).astype(np.int32), (s, "substeps"))
        same_state(new.state(), old.state(), s)
    assert seen.all() and old.reached >= 1 and old.timed_out >= 1
    assert (new.reached, new.timed_out, new.cut_by_target, new.cut_by_limit) == (old.reached, old.timed_out, 0, 0)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_reach_at_repeat_k_is_the_single_step_oracle_folded_by_the_wrapper_rule(k):
    """N = 1, four seeds, 60 macro steps each, episode_length 7.  The fold, dmc.py:40-50: reward and discount start at 0
    and 1; up to k single steps under the same action, reward += r * discount, discount *= d, and it stops at the step
    that ended the episode -- the next macro step is then the reset row, one single step() whose outputs pass through"""
    L, A = 7, 2
    cut_target = cut_limit = full = 0
    for seed in (1, 2, 3, 4):
        new, one = T.TaskOracle("reach", 1, episode_length=L, seed=seed, repeat=k), E.ReachOracle(1, episode_length=L, seed=seed)
        same_bits(new.reset(), one.reset(), "first frame")
        r = np.random.RandomState(100 + seed)
        for s in range(60):
            a = wild(r, one, A, s)
            if one.over[0]:
                frame, reward, discount, first = one.step(a)
                n = 0
                assert first[0] == 1 and reward[0] == 0 and discount[0] == 1
            else:
                reward, discount, first, n = np.zeros(1, F), np.ones(1, F), np.zeros(1, np.uint8), 0
                for _ in range(k):
                    frame, r1, d1, f1 = one.step(a)
                    assert f1[0] == 0
                    reward[0] = F(reward[0] + F(r1[0] * discount[0]))
                    discount[0] = F(discount[0] * d1[0])
                    n += 1
                    if one.over[0]:
                        break
                if n == k:
                    full += 1
                elif discount[0] == 0:
                    cut_target += 1
                else:
                    cut_limit += 1
            got = new.step(a)
            for name, g, w in zip(("frame", "reward", "discount", "first"), got, (frame, reward, discount, first)):
                same_bits(g, w, (seed, s, name))
            assert got[4].dtype == np.int32 and got[4].tolist() == [n], (seed, s)
            same_state(new.state(), one.state(), (seed, s))
        assert new.t[0] <= L
    assert cut_target >= 1 and cut_limit >= 1 and full >= 1, "the fold must have stopped early both ways"
    # No task's d is other than 1 before its last sub-step, so no run above multiplies a reward by a discount below 1.  A
    # rule that halves it, on the same skeleton: reward = 1 + 1/2 + .. + 2^-(k-1), discount = 2^-k, both exact
    class Halving(S.SkeletonOracle):
        new_episode = sanitise = lambda self, *a: None
        substep = lambda self, e, act: (F(1), F(0.5), False)
    o = Halving(1, L, 0, k, frames=False)
    o.reset()
    _, reward, discount, first, n = o.step(np.zeros((1, A), F))
    assert (reward[0], discount[0], first[0], n[0]) == (2 - 0.5 ** (k - 1), 0.5 ** k, 0, k)


# ------------------------------------------------------------------------------------------------ the oracle, point mass
def mass_at(pos, target, vel, L=50, repeat=1):
    o = T.TaskOracle("pointmass", 1, episode_length=L, seed=1, repeat=repeat)
    o.reset()
    o.pos[:], o.target[:], o.vel[:] = np.asarray(pos, F), np.asarray(target, F), np.asarray(vel, F)
    return o


def test_point_mass_velocity_is_in_no_frame_but_in_the_next():
    a, b = mass_at([0.0, 0.0], [0.5, 0.5], [0.0, 0.0]), mass_at([0.0, 0.0], [0.5, 0.5], [0.1, -0.1])
    same_bits(a.frames(), b.frames(), "two states that differ only in vel")
    same_bits(a.frames()[0], E.render(a.pos[0], a.target[0]), "the frame rule is reach's")
    fa, fb = a.step(np.zeros((1, 2), F))[0], b.step(np.zeros((1, 2), F))[0]
    assert not np.array_equal(fa, fb)
    same_bits(fa, mass_at([0.0, 0.0], [0.5, 0.5], [0.0, 0.0]).frames(), "at rest, no action: nothing moves")
    # by hand: v = 0.1 * 0.9 + 0 * 0.02, pos = 0 + v
    v = F(F(F(0.1) * F(0.9)) + F(F(0) * F(0.02)))
    assert b.vel[0, 0] == v and b.pos[0, 0] == v and b.vel[0, 1] == -v and b.pos[0, 1] == -v and b.t[0] == 1
    # the action accelerates: from rest a = 1 gives v = 0.02, pos = 0.02; NaN counts as 0, 5 as 1
    c = mass_at([0.0, 0.0], [0.5, 0.5], [0.0, 0.0])
    c.step(np.array([[5.0, np.nan]], F))
    assert c.vel[0].tolist() == [F(0.02), 0] and c.pos[0].tolist() == [F(0.02), 0]


def test_point_mass_wall_stops_the_axis_that_hit_it():
    o = mass_at([0.95, -0.95], [0.0, 0.0], [0.1, 0.01])
    o.step(np.zeros((1, 2), F))
    assert o.pos[0, 0] == F(1) and o.vel[0, 0] == 0                          # 0.95 + 0.09 > 1
    assert o.vel[0, 1] == F(F(0.01) * F(0.9)) and o.pos[0, 1] == F(F(-0.95) + o.vel[0, 1])     # the other axis goes on
    o = mass_at([0.0, -0.95], [0.0, 0.0], [0.0, -0.1])
    o.step(np.zeros((1, 2), F))
    assert o.pos[0, 1] == F(-1) and o.vel[0, 1] == 0 and o.pos[0, 0] == 0


def test_point_mass_never_ends_early():
    """homing actions carry the point onto its target (rows that end with d2 <= 0.01, where reach would end): discount is
    1 on every row, and an episode ends at t == episode_length only"""
    N, L, k = 3, 30, 2
    o = T.TaskOracle("pointmass", N, episode_length=L, seed=7, repeat=k)
    o.reset()
    on_target = 0
    for s in range(100):
        t_before, over_before = o.t.copy(), o.over.copy()
        a = np.clip((o.target - o.pos) / F(0.1), -1, 1).astype(F)
        _, reward, discount, first, n = o.step(a)
        assert (discount == 1).all(), s
        on_target += int(((((o.pos - o.target) ** 2).sum(1) <= 0.01) & (first == 0) & (o.over == 0)).sum())
        for e in range(N):
            assert first[e] == over_before[e] and o.over[e] == (first[e] == 0 and o.t[e] == L)
            assert n[e] == (0 if first[e] else min(k, L - t_before[e]))
    assert on_target >= 1 and o.reached == 0 and o.timed_out >= N and o.cut_by_target == 0


def test_inputs_of_the_gpu_tests_cover_what_they_claim():
    """the condition tests/test_hip_vec_tasks.py asserts before it compares, on every one of its configurations"""
    from tests.test_hip_vec_tasks import CONFIGS, L, REPEATS, SEED, STEPS
    for task in T.TASKS:
        for N, A in CONFIGS:
            for k in REPEATS:
                run = S.run_of(T, (task, N, A, k, SEED, STEPS, L), frames=False)
                assert T.covers(run, task, k), (task, N, A, k)


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototype_contract_symbol_and_abi_version():
    header = abi.text()
    abi.assert_prototype(NAME)
    assert len(_lib.PROTOTYPES[NAME][1]) == 20 and NAME not in _lib.NO_STREAM
    assert NAME in abi.stream_entries()
    enums = abi.enumerators()
    assert enums["DRQ_TASK_REACH"] == 0 and enums["DRQ_TASK_POINTMASS"] == 1 and abi.define("DRQ_TASK_MAX_REPEAT") == 16
    for text in ("reward = reward + r_i * discount", "discount = discount * d_i", "v = v * 0.9f;  v = v + a * 0.02f;  p = pos + v",
                 "p < -1: pos = -1, v = 0;  p > 1: pos = 1, v = 0", "substeps = 0", "dmc.py:35-50"):
        assert text in header, text                                        # the macro step is part of the contract
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()        # additive: the version stays
    from drqv2_amd import build, envs
    assert build.FILE_FLAGS["vecenv.hip"] == ["-ffp-contract=off"]         # the new kernel lives in the same file
    with open(os.path.join(build.CSRC, "vecenv.hip")) as f:
        assert NAME in f.read()
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    assert _lib.load().drq_abi_version() == 7 and hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert (envs.VecReach.TASK_ID, envs.VecPointMass.TASK_ID) == (0, 1) and envs.MAX_ACTION_REPEAT == 16
    assert (envs.VecReach.TASK, envs.VecPointMass.TASK) == T.TASKS


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_tasks.py repeats them on poisoned outputs.)"""
    lib = _lib.load()
    S.all_refused(((lib.drq_vec_task_step, T.refused_calls(0x10000, 0x20000, 0x30000, 0x40000)),))


# ------------------------------------------------------------------------------------------------ the classes, no GPU
@pytest.mark.parametrize("name", ["VecReach", "VecPointMass"])
def test_action_repeat_is_checked_in_the_constructor_before_any_device(name):
    from drqv2_amd import envs
    cls = getattr(envs, name)
    for bad in (0, 17, 2.5, -1, "2", None, True, 2.0):
        with pytest.raises(ValueError, match="action_repeat"):
            cls(3, "cpu", action_repeat=bad)
    env = cls(3, "cpu", action_dim=4, episode_length=7, seed=1, action_repeat=2)
    assert env.action_repeat == 2 and cls(3, "cpu").action_repeat == 1 and cls(3, "cpu", action_repeat=16).action_repeat == 16
    assert env.last_substeps is None
    for method in ("reset", "step", "render", "image", "state", "state_dict", "load_state_dict"):
        assert callable(getattr(cls, method)), method
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        env.reset()
    with pytest.raises(ValueError, match=r"step\(\): action"):
        env.step(torch.zeros(3, 2))
    s = env.state()
    assert ("vel" in s) == (name == "VecPointMass") and set(s) - {"vel"} == {"pos", "target", "t", "episode", "over"}
    if name == "VecPointMass":
        assert s["vel"].shape == (3, 2) and s["vel"].dtype == np.float32
    assert envs.VecReach.__mro__[1] is envs.VecPointMass.__mro__[1]        # one base holds the code of both


def loads(env, sd):
    """load_state_dict() on a CPU environment: the checks pass, then the device is refused"""
    with pytest.raises(_lib.DrqError, match="GPU"):
        env.load_state_dict(sd)


def test_state_dicts_carry_task_and_repeat_and_the_old_format_loads():
    from drqv2_amd.envs import VecPointMass, VecReach
    kw = dict(num_envs=3, device="cpu", action_dim=2, episode_length=5, seed=3)
    reach, mass = VecReach(**kw), VecPointMass(action_repeat=2, **kw)
    sd, sm = reach.state_dict(), mass.state_dict()
    assert sd["kind"] == "VecReach" and sd["config"]["task"] == "reach" and sd["config"]["action_repeat"] == 1 and "vel" not in sd
    assert sm["kind"] == "VecPointMass" and sm["config"]["task"] == "pointmass" and sm["config"]["action_repeat"] == 2
    assert sm["vel"].shape == (3, 2) and sm["vel"].dtype == torch.float32 and sm["vel"].device.type == "cpu"
    loads(VecReach(**kw), sd)
    loads(VecPointMass(action_repeat=2, **kw), sm)
    # a VecReach dict written before there were tasks: no "task", no "action_repeat" -- it is reach at repeat 1
    old = dict(sd, config={k: v for k, v in sd["config"].items() if k not in ("task", "action_repeat")})
    assert set(old["config"]) == {"N", "A", "episode_length", "seed"}
    loads(VecReach(**kw), old)
    assert set(old["config"]) == {"N", "A", "episode_length", "seed"}       # the caller's dict is not edited
    with pytest.raises(ValueError, match=r"\baction_repeat: saved 1, here 2"):
        VecReach(action_repeat=2, **kw).load_state_dict(old)
    with pytest.raises(ValueError, match=r"\baction_repeat: saved 1, here 3"):
        VecReach(action_repeat=3, **kw).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\baction_repeat: saved 2, here 1"):
        VecPointMass(**kw).load_state_dict(sm)
    with pytest.raises(ValueError, match="kind"):                          # the task is the class
        VecReach(action_repeat=2, **kw).load_state_dict(sm)
    with pytest.raises(ValueError, match="kind"):
        VecPointMass(**kw).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        VecPointMass(**kw).load_state_dict(old)
    with pytest.raises(ValueError, match=r"\btask: saved 'pointmass', here 'reach'"):
        VecReach(**kw).load_state_dict(dict(sd, config=dict(sd["config"], task="pointmass")))
    with pytest.raises(ValueError, match=r"\btask: saved '<absent>'"):     # only the old VecReach format may omit it
        VecPointMass(action_repeat=2, **kw).load_state_dict(
            dict(sm, config={k: v for k, v in sm["config"].items() if k != "task"}))
    with pytest.raises(ValueError, match="vel: no tensor saved"):
        VecPointMass(action_repeat=2, **kw).load_state_dict({k: v for k, v in sm.items() if k != "vel"})


def test_checkpoint_file_round_trip_of_a_point_mass_state(tmp_path):
    """drqv2_amd.checkpoint takes either class with no special case: the file holds the dict as it is"""
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecPointMass
    env = VecPointMass(3, "cpu", episode_length=5, seed=3, action_repeat=2)
    env.vel[1, 0] = 0.25
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=env, extra={"step": 4})
    ck = torch.load(path, weights_only=True)
    assert ck["env"]["kind"] == "VecPointMass" and ck["env"]["config"]["action_repeat"] == 2
    assert torch.equal(ck["env"]["vel"], env.vel) and ck["extra"] == {"step": 4}
    with pytest.raises(ValueError, match="action_repeat: saved 2, here 1"):
        checkpoint.load(path, env=VecPointMass(3, "cpu", episode_length=5, seed=3))
