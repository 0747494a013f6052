"""The reacher of the device environment (drq_vec_reacher_step / _render, drqv2_amd.envs.VecReacher): everything that needs
no GPU.  The public surface and the DRQ_EARG cases (all are decided before any launch), the properties of the numpy
restatement tests/vec_reacher_oracle.py that make it a damped two-link arm with a sparse reward -- the unit vectors stay
unit, rest is a fixed point, the mirror symmetry, the loss of energy, targets within reach, a scripted controller that
collects reward where doing nothing collects none -- and the condition on the inputs of the GPU tests
(tests/test_hip_vec_reacher.py), which is a property of the oracle's runs alone.  No assertion here has a tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_reacher_oracle as O
from tests import vec_skeleton_oracle as S
from tests.vec_skeleton_oracle import same_bits

F = np.float32
STEP, RENDER = "drq_vec_reacher_step", "drq_vec_reacher_render"
ULP1 = 2.0 ** -23                   # the spacing of float32 at 1


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN or O.PHYSICS without its frames: computed once, never modified"""
    return S.run_of(O, cfg, frames=False)


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build_flags():
    header = abi.text()
    for name, nargs in ((STEP, 20), (RENDER, 6)):
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs and name not in _lib.NO_STREAM and name in abi.stream_entries()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for text in ("Reacher.", "c12 = c1 * c2 - s1 * s2;  s12 = s1 * c2 + c1 * s2",
                 "M11 = 0.75f + 0.5f * c2;  M12 = 0.25f + 0.25f * c2;  h = 0.25f * s2", "cor = (2 * w1) * w2 + w2 * w2",
                 "tau1 = (a1 * 2 - 0.5f * w1) + h * cor;  tau2 = (a2 * 2 - 0.5f * w2) - h * (w1 * w1)",
                 "det = M11 * 0.25f - M12 * M12", "al1 = (0.25f * tau1 - M12 * tau2) / det;  al2 = (M11 * tau2 - M12 * tau1) / det",
                 "w1 = clamp(w1 + al1 * 0.01f, -16, 16)", "k == 0: (c, s) stay as they are",
                 "r_i = d2 <= target_radius * target_radius ? 1 : 0", "r_i = 1 / (1 + 4 * d2)",
                 "u = clamp(v * 1.1111112f, -1, 1);  x = 1 - 2 * |u|;  y = 1 - |x|, negated for u < 0",
                 "x * x + y * y < 0.25f: (1, 0)", "f = 0.5f + v_3 * 0.5f;  rho = (1 - target_radius) * f",
                 "TX = (int)floorf((ax + c12 * 288) + 672.5f)", "GR = (int)floorf(target_radius * 576 + 0.5f)"):
        assert text in header, text                                        # the rule is part of the contract
    from drqv2_amd import build, envs
    assert "vecreacher.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecreacher.hip"))
    assert build.FILE_FLAGS["vecreacher.hip"] == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    assert envs.VecReacher.TASK == "reacher" and issubclass(envs.VecReacher, envs._VecTask)
    assert envs.VecReacher._MIN_ACTION_DIM == 2
    with open(os.path.join(build.CSRC, "vecreacher.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("sinf", "cosf", "expf", "__shared__", "atomic"):        # no libm rounding, no LDS, no atomics
        assert banned not in src, banned
    assert "sqrtf" in src and "launch_env_step<Reacher>" in src and "launch_env_render<Reacher>" in src


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_reacher.py repeats them on poisoned outputs.)"""
    lib = _lib.load()
    calls, renders = O.refused_calls(0x10000, 0x20000, 0x30000, 0x40000), O.refused_renders(0x10000, 0x30000)
    S.all_refused(((lib.drq_vec_reacher_step, calls), (lib.drq_vec_reacher_render, renders)))
    ok = [0x10000, 0x10100, 0x10200, 0x10300, 0x10400, 5, 2, 0x20000, 7, 9, 2, 0, 0.15, 1, 0x30000, 0x40000, 0x40100,
          0x40200, 0x40300]
    sub = lambda k, v: ok[:k] + [v] + ok[k + 1:]
    for a in ([None] + ok[1:], sub(0, 0x10002), sub(1, None), sub(1, 0x10102), sub(6, 1), sub(10, 0), sub(10, 17), sub(11, 2),
              sub(7, None), sub(12, 0.0199), sub(12, 0.301), sub(12, float("nan")), sub(13, 2)):    # the cases the issue lists
        assert repr(a) in map(repr, calls), a                              # by text: a NaN equals no NaN
    for a in ([None, 0x10100, 3, 0.15, 0x30000], [0x10000, 0x10102, 3, 0.15, 0x30000], [0x10000, 0x10100, 3, 0.0199, 0x30000],
              [0x10000, 0x10100, 3, 0.301, 0x30000]):
        assert repr(a) in map(repr, renders), a
    # the task entry still knows reach and the point mass only
    assert lib.drq_vec_task_step(3, *([0x10000] * 6), 5, 2, 0x20000, 7, 9, 2, 0, 0x30000, *([0x40000] * 4), None) == -1


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_constructor_state_and_state_dict_without_a_device(tmp_path):
    from drqv2_amd.envs import VecCartpole, VecReacher
    env = VecReacher(3, "cpu")
    assert (env.A, env.episode_length, env.action_repeat, env.target_radius, env.sparse) == (2, 1000, 1, 0.15, True)
    with pytest.raises(ValueError, match="action_dim >= 2"):
        VecReacher(3, "cpu", action_dim=1)
    for bad in (0.0199, 0.301, float("nan"), "0.1", None, True):
        with pytest.raises(ValueError, match="target_radius"):
            VecReacher(3, "cpu", target_radius=bad)
    for bad in (2, "yes", None, 0.5):
        with pytest.raises(ValueError, match="sparse"):
            VecReacher(3, "cpu", sparse=bad)
    kw = dict(action_dim=3, episode_length=7, seed=1, action_repeat=2, target_radius=0.05, sparse=False)
    env = VecReacher(3, "cpu", **kw)
    with pytest.raises(ValueError, match=r"step\(\): action"):
        env.step(torch.zeros(3, 2))
    s = env.state()
    assert list(s) == ["phys", "target", "t", "episode", "over"] and s["phys"].shape == (3, 6) and s["target"].shape == (3, 2)
    assert s["phys"].dtype == s["target"].dtype == np.float32
    sd = env.state_dict()
    assert sd["kind"] == "VecReacher" and sd["config"] == {"N": 3, "A": 3, "episode_length": 7, "seed": 1, "task": "reacher",
                                                            "action_repeat": 2, "target_radius": 0.05, "sparse": False}
    with pytest.raises(_lib.DrqError, match="GPU"):                        # the checks pass, then the device is refused
        VecReacher(3, "cpu", **kw).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\btarget_radius: saved 0.05, here 0.15"):
        VecReacher(3, "cpu", **dict(kw, target_radius=0.15)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        VecReacher(3, "cpu", **dict(kw, sparse=True)).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        VecCartpole(3, "cpu", action_dim=3, episode_length=7, seed=1, action_repeat=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="target: no tensor saved"):
        VecReacher(3, "cpu", **kw).load_state_dict({k: v for k, v in sd.items() if k != "target"})
    # what no task decides: action_repeat, the methods, no CPU fallback, the skeleton's words, the checkpoint file
    ck = S.class_without_a_device(VecReacher, env, tmp_path, ("phys", (1, 5), 0.25), methods=("background_key",))
    assert ck["env"]["config"]["target_radius"] == 0.05 and ck["env"]["config"]["sparse"] is False


# ------------------------------------------------------------------------------------------------ the oracle's properties
def test_both_unit_vectors_stay_within_1_ulp_of_one_over_the_physics_runs():
    """c^2 + s^2, evaluated in float64, within 1 float32 ulp of 1 (2^-23) for both joints after every macro step of the
    PHYSICS runs, which turn both joints through all four quadrants and spin two arms at the clamp"""
    worst = 0.0
    for cfg in O.PHYSICS:
        for st in run_of(cfg)["states"]:
            p = st["phys"].astype(np.float64)
            worst = max(worst, np.abs(p[:, 0] ** 2 + p[:, 1] ** 2 - 1).max(), np.abs(p[:, 3] ** 2 + p[:, 4] ** 2 - 1).max())
    print(f"worst |c^2 + s^2 - 1| = {worst:.3e} = {worst / ULP1:.3f} ulp of 1")
    assert worst <= ULP1, worst / ULP1


def test_an_arm_at_rest_under_zero_action_stays_at_rest_bit_for_bit():
    starts = [O.reset_state(7, e, 1, F(0.15))[0] for e in range(8)]
    starts += [tuple(F(v) for v in pose[0][:2]) + (F(0),) + tuple(F(v) for v in pose[0][3:5]) + (F(0),) for pose in O.POSES]
    for start in starts:
        for a in (F(0), F(-0.0)):
            p = start
            for _ in range(50):
                p, cut = O.substep(p, a, a)
                assert cut == 0
                same_bits(np.array(p), np.array(start), (start, a))
    # ... and the smallest torque moves it
    p, _ = O.substep(starts[0], F(1e-3), F(0))
    assert p[2] != 0 and p[5] != 0 and p[0:2] != starts[0][0:2]


def test_the_mirror_state_under_the_mirror_action_gives_the_mirrored_trajectory_bit_for_bit():
    """s1, s2, w1, w2 and the target's y negated, both torques negated: the mirrored run, rewards included, both forms"""
    r = np.random.RandomState(3)
    mirror = lambda p: (p[0], -p[1], -p[2], p[3], -p[4], -p[5])
    d1, d2, d3 = O.normalise(F(0.3), F(-0.7)), O.normalise(F(-0.9), F(0.2)), O.normalise(F(-0.1), F(-1))
    for start, target in (((*d1, F(1.5), *d2, F(-3)), (F(0.3), F(-0.4))), ((*d3, F(-12), *d1, F(15)), (F(-0.6), F(0.1)))):
        p, m, mtarget = start, mirror(start), (target[0], -target[1])
        for i in range(600):
            a1, a2 = O.clamp1(F(r.uniform(-1.5, 1.5))), O.clamp1(F(r.uniform(-1.5, 1.5)))
            p, cp = O.substep(p, a1, a2)
            m, cm = O.substep(m, F(-a1), F(-a2))
            assert cp == cm
            same_bits(np.array(m), np.array(mirror(p)), i)
            for sparse in (True, False):
                same_bits(O.reward_of(m, mtarget, F(0.3), sparse), O.reward_of(p, target, F(0.3), sparse), (i, "reward"))


def kinetic_energy(p):
    """of the two unit masses, in float64: (M11 w1^2 + 2 M12 w1 w2 + M22 w2^2) / 2"""
    c2, w1, w2 = float(p[3]), float(p[2]), float(p[5])
    return 0.5 * ((0.75 + 0.5 * c2) * w1 * w1 + 2 * (0.25 + 0.25 * c2) * w1 * w2 + 0.25 * w2 * w2)


def test_a_spinning_arm_under_zero_action_loses_energy():
    for start in ((F(1), F(0), F(3), F(0), F(1), F(-5)), (*O.normalise(F(-0.5), F(0.5)), F(-2), F(-1), F(0), F(6)),
                  (F(0), F(-1), F(8), F(1), F(0), F(8))):
        p = start
        for _ in range(500):
            p, _ = O.substep(p, F(0), F(0))
        assert all(np.isfinite(v) and v.dtype == np.float32 for v in p)
        assert 0 <= kinetic_energy(p) < kinetic_energy(start)


def test_after_a_reset_the_whole_target_disc_lies_within_reach():
    """256 (environment, episode) pairs at the two named radii and both ends of the range: |target| + radius <= 1 in
    float64, the joints' vectors are unit vectors and the arm is at rest; and the targets do differ"""
    for radius in (0.02, 0.05, 0.15, 0.3):
        seen = set()
        for e in range(16):
            for ep in range(1, 17):
                p, target = O.reset_state(11, e, ep, F(radius))
                assert np.hypot(float(target[0]), float(target[1])) + float(F(radius)) <= 1.0
                assert p[2] == 0 and p[5] == 0
                for c, s in (p[0:2], p[3:5]):
                    assert abs(float(c) ** 2 + float(s) ** 2 - 1) <= ULP1
                seen.add((float(target[0]), float(target[1]), float(p[0]), float(p[3])))
        assert len(seen) == 256
    # the direction of a draw: every quadrant, both ends of the range, and the stated threshold
    quadrants = {O.quadrant(*O.direction(F(v))) for v in np.linspace(-0.9, 0.9, 41, dtype=F)}
    assert quadrants == {0, 1, 2, 3}
    same_bits(np.array(O.direction(F(0))), np.array((F(1), F(0))), "u = 0")
    assert O.direction(F(0.9))[0] == -1 and O.direction(F(-0.9))[0] == -1


# ------------------------------------------------------------------------------------------------ sparse and solvable
@pytest.mark.parametrize("radius", [0.15, 0.05])
def test_a_scripted_controller_collects_reward_in_every_environment_and_zero_action_does_not(radius):
    """Inverse kinematics in float64, a PD law on the joint angles, fed through the float32 step: reward > 0 in each of 16
    environments within one episode of 1,000 steps -- what K = 2 and b = 0.5 were held to.  Under zero action at least one
    of the 16 returns exactly 0: the reward is sparse"""
    got = [O.controlled_episode(0, e, radius) for e in range(16)]
    print(f"radius {radius}: returns {[int(g[0]) for g in got]}, first rewarded step {[g[1] for g in got]}")
    assert all(total > 0 for total, _ in got)
    idle = [O.controlled_episode(0, e, radius, controlled=False)[0] for e in range(16)]
    print(f"radius {radius}: returns under zero action {[int(v) for v in idle]}")
    assert any(v == 0.0 for v in idle)


# ------------------------------------------------------------------------------------------------ the shared drive
def test_inputs_of_the_gpu_tests_cover_what_they_claim():
    """The runs and poses tests/test_hip_vec_reacher.py compares on the GPU, on the oracle alone"""
    rewarded = unrewarded = 0
    for cfg in O.DRIVEN:
        run = run_of(cfg)
        acts = np.stack(run["actions"])[:, :, :2]
        assert np.isnan(acts).any() and np.isinf(acts).any() and (np.abs(acts[np.isfinite(acts)]) > 1).any(), cfg
        firsts = np.stack([o[3] for o in run["out"]])
        # a repeat of 16 ends every episode of seven steps in its first row, whatever t was: only there all reset together
        assert firsts.any() and (cfg[2] > O.EPISODE_LENGTH or not (firsts.all(1) | ~firsts.any(1)).all()), "no stagger"
        assert run["reset_rows"] >= 1 and (cfg[2] == 1 or run["cut_by_limit"] >= 1), cfg     # a time limit inside a repeat
        assert all((o[2] == 1).all() for o in run["out"])                  # the discount is 1 on every row
        rewards = np.stack([o[1] for o in run["out"]])
        if cfg[3]:      # sparse: exact small integers
            assert (rewards == np.round(rewards)).all() and rewards.min() >= 0 and rewards.max() <= cfg[2]
            rewarded, unrewarded = rewarded + run["rewarded"], unrewarded + run["unrewarded"]
            assert (rewards[firsts == 0] == 0).any(), cfg
        else:
            assert (rewards[firsts == 0] > 0).all()
    assert rewarded >= 1 and unrewarded >= 1, (rewarded, unrewarded)
    for cfg in O.PHYSICS:
        run = run_of(cfg)
        assert run["quadrants"][0] == run["quadrants"][1] == {0, 1, 2, 3}, run["quadrants"]
        assert run["clamped"] >= 1 and run["reset_rows"] == 0
        assert (np.abs(np.stack(run["actions"])[:, :, 0]) > 1).all()
    # the poses: the arm along each axis, folded, stretched, the fingertip over the target, the target under the upper arm
    unit = lambda c, s: (int(np.rint(c)), int(np.rint(s)))
    stretched = {unit(*p[0][0:2]) for p in O.POSES if p[0][3] == 1}
    assert stretched == {(1, 0), (0, 1), (-1, 0), (0, -1)}
    assert any(p[0][3] == -1 for p in O.POSES)
    over = [p for p in O.POSES if O.distance2(tuple(p[0]), tuple(p[1])) == 0]
    assert over and all((O.render(*p)[:, 42 - 36:42 + 36, :] == 255).any() for p in over)
    under = 0
    for phys, target, radius in O.POSES:
        EX, EY, TX, TY, GX, GY, GR = O.points(phys, target, F(radius))
        both = O.disc(GX, GY, GR) & O.capsule(O.CENTRE, O.CENTRE, EX, EY, O.ARM_R)
        under += bool(both.any() and (O.disc(GX, GY, GR) & ~both).any() and not O.disc(TX, TY, O.TIP_R)[O.disc(GX, GY, GR)].any())
        frame = O.render(phys, target, radius)
        shape = (frame != O.BACKGROUND).any(0)
        assert set(np.unique(frame[:, shape])) == {64, 255} and not (frame == 0xA5).any()
        assert not ((frame[0] == frame[1]) & (frame[1] == frame[2]))[shape].any()     # never VecDistract's background key
        assert not shape[0].any() and not shape[-1].any() and not shape[:, 0].any() and not shape[:, -1].any()   # all inside
        colours = {tuple(v) for v in frame[:, shape].T}
        assert O.TIP_RGB in colours and (phys[3] == -1 or O.UPPER_RGB in colours)     # folded: the forearm hides the upper arm
    assert under >= 1
    assert {p[2] for p in O.POSES} >= {0.02, 0.05, 0.15, 0.3}
