"""The finger of the device environment (drq_vec_finger_step / _render, drqv2_amd.envs.VecFinger): everything that needs no
GPU.  The public surface and the DRQ_EARG cases (all are decided before any launch); the conditions the constants of the
rule were chosen under -- rest is rest, no start in penetration, no tunnelling, contacts that take energy out, everything
in the frame, and a task that a script solves where random actions earn nothing -- on the numpy restatement
tests/vec_finger_oracle.py; and what the inputs of the GPU tests (tests/test_hip_vec_finger.py) cover, which is a property
of the oracle's runs alone.  Comparisons of bits have no tolerance; a bound on a float64 quantity is stated where it
stands."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_finger_oracle as O
from tests import vec_skeleton_oracle as S

F = np.float32
STEP, RENDER = "drq_vec_finger_step", "drq_vec_finger_render"
RESET_SEED = 11                  # the fixed resets: environments 0 .. 63 of this seed, their first episode
MODES = ((0, O.TURN_EASY_RADIUS, "spin"), (1, O.TURN_EASY_RADIUS, "turn_easy"), (1, O.TURN_HARD_RADIUS, "turn_hard"))


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN or O.PHYSICS without its frames: computed once, never modified"""
    return S.run_of(O, cfg, frames=False)


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build_flags():
    from drqv2_amd import build, envs
    assert "vecfinger.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecfinger.hip"))
    assert build.FILE_FLAGS["vecfinger.hip"] == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    header = abi.text()
    for name, nargs in ((STEP, 21), (RENDER, 7)):
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs and name not in _lib.NO_STREAM and name in abi.stream_entries()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for text in ("Finger.", "the\n *   finger's two links pass over the rod, the hinge and each other",
                 "proj = qx * cs + qy * ss;  u = clamp(proj, 0, 0.3f);  rx = cs * u;  ry = ss * u",
                 "e2 == 0: e = 0, (nx, ny) = (0, 1)", "j1 = ny * tx - nx * ty;  j2 = ny * fx - nx * fy;  js = rx * ny - ry * nx",
                 "qx * qx + qy * qy >= 0.0169f: (cs, ss) = normalise(-qx, -qy)", "(c1, s1, c2, s2) = (0, 1, 1, 0)",
                 "M11 = 0.41f + 0.24f * c2;  M12 = 0.09f + 0.12f * c2;  h = 0.12f * s2", "ws = ws * 0.97f",
                 "gap = e - 0.11f;  lim = -(max(gap, 0) * 100);  vn = (j1 * w1 + j2 * w2) - js * ws",
                 "vn < lim and den > 0:  lam = (lim - vn) / den;  w1 = w1 + u1 * lam;  w2 = w2 + u2 * lam;  ws = ws - (js * 20) * lam",
                 "ws = clamp(ws, -10, 10)", "den = (j1 * j1) * 2.5f + (js * js) * 20;  den >= 0.01f:  mu = (0.11f - e) / den",
                 "sparse: r_i = ws >= 2 ? 1 : 0;  dense: r_i = clamp(ws / 2, 0, 1)", "0.11 - 0.011",
                 "SX = (int)floorf(cs * 201.6f + 672.5f);  SY = (int)floorf(672.5f - (ss * 201.6f - 134.4f))"):
        assert text in header, text                                        # the rule is part of the contract
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    cls = envs.VecFinger
    assert cls.TASK == "finger" and issubclass(cls, envs._VecTask)
    assert cls._MIN_ACTION_DIM == 2 and cls._STATE == ("phys", "target", "t", "episode", "over")
    assert cls._STATE_SPEC["phys"] == ((9,), torch.float32) and cls._STATE_SPEC["target"] == ((2,), torch.float32)
    assert (cls.TURN_EASY_RADIUS, cls.TURN_HARD_RADIUS, cls.SPIN_SPEED) == (O.TURN_EASY_RADIUS, O.TURN_HARD_RADIUS, O.SPIN_SPEED)
    assert (cls.MIN_TARGET_RADIUS, cls.MAX_TARGET_RADIUS) == (O.MIN_RADIUS, O.MAX_RADIUS)
    with open(os.path.join(build.CSRC, "vecfinger.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("sinf", "cosf", "expf", "__shared__", "atomic"):        # no libm rounding, no LDS, no atomics
        assert banned not in src, banned
    assert "sqrtf" in src and "launch_env_step<Finger>" in src and "launch_env_render<Finger>" in src


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_finger.py repeats them on poisoned outputs.)"""
    lib = _lib.load()
    calls, renders = O.refused_calls(0x10000, 0x20000, 0x30000, 0x40000), O.refused_renders(0x10000, 0x30000)
    S.all_refused(((lib.drq_vec_finger_step, calls), (lib.drq_vec_finger_render, renders)))
    ok = [0x10000, 0x10100, 0x10200, 0x10300, 0x10400, 5, 2, 0x20000, 7, 9, 2, 0, 1, 0.1, 1, 0x30000, 0x40000, 0x40100, 0x40200,
          0x40300]
    for a in ([None] + ok[1:], S.sub(ok, 1, 0x10102), S.sub(ok, 6, 1), S.sub(ok, 10, 17), S.sub(ok, 7, None), S.sub(ok, 12, 2),
              S.sub(ok, 12, -1), S.sub(ok, 13, 0.201), S.sub(ok, 13, float("nan")), S.sub(ok, 14, 2), S.sub(ok, 15, 0x30008)):
        assert repr(a) in map(repr, calls), a                              # by text: a NaN equals no NaN
    for a in ([None, 0x10100, 3, 1, 0.1, 0x30000], [0x10000, 0x10102, 3, 1, 0.1, 0x30000], [0x10000, 0x10100, 0, 1, 0.1, 0x30000],
              [0x10000, 0x10100, 3, 2, 0.1, 0x30000], [0x10000, 0x10100, 3, 1, 0.0199, 0x30000], [0x10000, 0x10100, 3, 1, 0.1, None]):
        assert repr(a) in map(repr, renders), a
    assert (len(calls), len(renders)) == (46, 15)


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_constructor_state_and_state_dict_without_a_device(tmp_path):
    from drqv2_amd.envs import VecFinger, VecReacher
    env = VecFinger(3, "cpu")
    assert (env.A, env.episode_length, env.action_repeat, env.mode, env.target_radius, env.sparse) == (2, 1000, 1, "spin", 0.1, True)
    with pytest.raises(ValueError, match="action_dim >= 2"):
        VecFinger(3, "cpu", action_dim=1)
    for bad in (0.0199, 0.201, float("nan"), float("inf"), "0.1", None, True):
        with pytest.raises(ValueError, match="target_radius"):
            VecFinger(3, "cpu", target_radius=bad)
    for bad in (0, 1, True, None, "flick", "finger_spin"):
        with pytest.raises(ValueError, match="task"):
            VecFinger(3, "cpu", task=bad)
    for bad in (2, -1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="sparse"):
            VecFinger(3, "cpu", sparse=bad)
    for radius in (0.02, 0.2, O.TURN_HARD_RADIUS):                         # both ends are valid
        assert VecFinger(3, "cpu", task="turn", target_radius=radius).target_radius == radius
    kw = dict(action_dim=4, episode_length=7, seed=1, action_repeat=2, task="turn", target_radius=0.04, sparse=False)
    env = VecFinger(3, "cpu", **kw)
    with pytest.raises(ValueError, match=r"step\(\): action"):
        env.step(torch.zeros(3, 2))
    s = env.state()
    assert list(s) == ["phys", "target", "t", "episode", "over"] and s["phys"].shape == (3, 9) and s["target"].shape == (3, 2)
    sd = env.state_dict()
    assert sd["kind"] == "VecFinger" and sd["config"] == {"N": 3, "A": 4, "episode_length": 7, "seed": 1, "task": "finger",
                                                           "action_repeat": 2, "mode": "turn", "target_radius": 0.04, "sparse": False}
    with pytest.raises(_lib.DrqError, match="GPU"):                        # the checks pass, then the device is refused
        VecFinger(3, "cpu", **kw).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bmode: saved 'turn', here 'spin'"):
        VecFinger(3, "cpu", **dict(kw, task="spin")).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\btarget_radius: saved 0.04, here 0.1"):
        VecFinger(3, "cpu", **dict(kw, target_radius=0.1)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        VecFinger(3, "cpu", **dict(kw, sparse=True)).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        VecReacher(3, "cpu", action_dim=4, episode_length=7, seed=1, action_repeat=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="phys: no tensor saved"):
        VecFinger(3, "cpu", **kw).load_state_dict({k: v for k, v in sd.items() if k != "phys"})
    # what no task decides: action_repeat, the methods, no CPU fallback, the skeleton's words, the checkpoint file
    ck = S.class_without_a_device(VecFinger, env, tmp_path, ("phys", (1, 5), 0.25), methods=("background_key",))
    assert ck["env"]["config"]["mode"] == "turn"


# ------------------------------------------------------------------------------------------------ the conditions on the constants
def test_1_rest_is_rest():
    """64 fixed resets, 1,000 steps of the zero action: every state word keeps its bits"""
    start, _ = O.reset_states(RESET_SEED, range(64))
    phys, zero = start, np.zeros((64, 2), F)
    for s in range(1000):
        phys = O.substep_many(phys, zero)
        assert phys.tobytes() == start.tobytes(), s
    assert len({p.tobytes() for p in start}) >= 60


def test_2_no_episode_starts_in_penetration_or_rewarded():
    """the 64 fixed resets and 10,000 (e, episode) pairs: the fingertip's centre is at least 0.13 (to rounding) from the
    rod's axis, so no contact and no speculative impulse at rest; every vector is a unit vector, every velocity 0; the
    target's angle is at least 44.9 degrees from the rod's.  Both shifts of the reset rule occur"""
    counts = {"away": 0, "upright": 0}
    both = [O.reset_state(RESET_SEED, e, 1) for e in range(64)] + [O.reset_state(7, e, ep, counts) for e in range(100) for ep in range(1, 101)]
    phys, target = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    gap = O.gap_many(phys)[0]
    assert gap.min() >= 0.13 - 1e-6 > float(O.TOUCH), gap.min()
    assert (phys[:, [2, 5, 8]] == 0).all() and counts["away"] >= 1 and counts["upright"] >= 1
    for c, s in ((phys[:, 0], phys[:, 1]), (phys[:, 3], phys[:, 4]), (phys[:, 6], phys[:, 7]), (target[:, 0], target[:, 1])):
        assert np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1).max() <= 2.0 ** -23
    cos = phys[:, 6].astype(np.float64) * target[:, 0] + phys[:, 7].astype(np.float64) * target[:, 1]
    assert cos.max() <= np.cos(np.radians(44.9))
    for mode, radius, _ in MODES[1:]:
        assert (O.reward_many(phys, target, mode, radius, True) == 0).all()


def test_3_no_tunnelling():
    """By construction: in one simulator step the fingertip's centre moves at most (L1 + L2) W1 dt + L2 W2 dt and a point
    of the rod's axis at most Ls Ws dt, from the lengths and the three clamps; together less than the touching distance.
    Beside it, 20,000 simulator steps of 8 environments under S.wild_actions (a new row every fourth step): after every
    sub-step the centre is no closer to the axis than touching minus the skin, the skin is at most a tenth of touching, and
    no fingertip changes the side of the rod it is on, with its projection inside the rod before and after, in a step
    without an impulse or a separation"""
    dt = float(O.DT)
    finger = (float(O.L1) + float(O.L2)) * float(O.MAX_W) * dt + float(O.L2) * float(O.MAX_W) * dt
    rod = float(O.LS) * float(O.MAX_WS) * dt
    touching = O.TIP_RADIUS + O.ROD_RADIUS
    assert abs(touching - float(O.TOUCH)) < 1e-7 and finger + rod < touching and O.SKIN <= touching / 10 + 1e-12
    print(f"largest relative displacement {finger:.3f} + {rod:.3f} = {finger + rod:.3f} < {touching}")
    r = np.random.RandomState(3)
    phys, _ = O.reset_states(RESET_SEED, range(8))
    events, worst, a = dict.fromkeys(O.EVENTS, 0), 9.0, None
    for s in range(20000):
        if s % 4 == 0:
            a = np.array([[S.sanitise(v) for v in row] for row in S.wild_actions(r, 8, 2)], F)
        trace = {}
        _, side0, proj0 = O.gap_many(phys)
        phys = O.substep_many(phys, a, events, trace)
        gap, side1, proj1 = O.gap_many(phys)
        worst = min(worst, float(gap.min()))
        assert gap.min() >= touching - O.SKIN, (s, gap.min())
        crossed = (side0 * side1 < 0) & (proj0 > 0) & (proj0 < float(O.LS)) & (proj1 > 0) & (proj1 < float(O.LS))
        assert not (crossed & ~(trace["impulse"] | trace["separation"])).any(), s
    print(f"closest {worst:.6f} of {touching}; {events}")
    assert events["impulse"] >= 100 and events["separation"] >= 50 and events["side"] and events["cap"] and events["hinge_end"]


def test_4_contacts_take_energy_out_and_the_clamps_hold():
    """8 environments, 10,000 simulator steps of actions held for 25 steps at +-1 (the hardest pushing there is), from
    resets and from the hand-set states of the physics runs.  In float64, from the states around the two contact parts of
    every sub-step: the impulse never raises the kinetic energy 0.5 w^T M w + 0.5 I ws^2 by more than 1e-5 (1 + E) -- a
    rounding allowance: the three velocities are float32 sums of a few products, each relative 2^-24, of magnitudes up
    to E -- and the separation leaves it exactly as it is, because it moves neither a velocity nor the elbow.  After every
    sub-step |w1|, |w2| <= 6, |ws| <= 10, and c^2 + s^2 of all three unit vectors is within 2^-23 of 1 (the reacher's bound)"""
    r = np.random.RandomState(5)
    phys = np.concatenate([O.reset_states(RESET_SEED, range(4))[0], O.physics_start()])
    phys[7, 8] = F(9.5)                                                  # inside its clamp: this test starts from states of the rule
    events, a, worst = dict.fromkeys(O.EVENTS, 0), None, -1.0
    for s in range(10000):
        if s % 25 == 0:
            a = r.choice([-1.0, 1.0], (8, 2)).astype(F)
        trace = {}
        phys = O.substep_many(phys, a, events, trace)
        before, after = O.energy_many(trace["before_impulse"]), O.energy_many(trace["after_impulse"])
        worst = max(worst, float(((after - before) / (1 + before)).max()))
        assert (after <= before + 1e-5 * (1 + before)).all(), s
        assert (O.energy_many(trace["after_separation"]) == O.energy_many(trace["before_separation"])).all(), s
        assert np.abs(phys[:, [2, 5]]).max() <= 6 and np.abs(phys[:, 8]).max() <= 10
        for k in (0, 3, 6):
            assert np.abs(phys[:, k].astype(np.float64) ** 2 + phys[:, k + 1].astype(np.float64) ** 2 - 1).max() <= 2.0 ** -23
    print(f"largest relative gain of an impulse {worst:.2e}; {events}")
    assert events["impulse"] >= 100 and events["separation"] >= 10 and events["clamp_w1"] + events["clamp_w2"] >= 1


def test_5_everything_stays_in_the_frame():
    """from the constants: the reach of every shape, radii included, in world units and in the frame's integers"""
    root, hinge = float(O.ROOT_Y), float(O.HINGE_Y)
    reach = float(O.L1) + float(O.L2) + O.TIP_RADIUS
    assert reach <= 1 and root + reach <= 1 and root - reach >= -1                       # the finger, from (0, root)
    for r in (float(O.LS) + O.ROD_RADIUS, float(O.LS) + O.MAX_RADIUS, O.HINGE_R / 672):  # the rod, the target's disc, the hinge
        assert r <= 1 and hinge + r <= 1 and hinge - r >= -1
    assert O.ROOT_PY == int(np.floor(672.5 - root * 672)) and O.HINGE_PY == int(np.floor(672.5 - hinge * 672))
    assert O.TIP_R == int(O.TIP_RADIUS * 672) and O.ROD_R == round(O.ROD_RADIUS * 672) and 0 <= 672 - 672 * 0.7 - O.TIP_R
    assert O.ROOT_PY - (268.8 + 201.6) - O.TIP_R >= 0 and O.HINGE_PY + 201.6 + 672 * O.MAX_RADIUS + 1 <= 1344
    assert float(O.DROP) == root - hinge


@pytest.mark.parametrize("mode,radius,name", MODES, ids=[m[2] for m in MODES])
def test_6_there_is_a_task_to_learn(mode, radius, name):
    """1,000 simulator steps, the sparse reward, the first episode of environments 0 .. 15 of the fixed seed.  Uniformly
    random actions, 16 seeds: the mean return of every seed is at most 10 % of the maximum of 1,000.  The script (flick()
    for spin, turn_to() for turn): a mean return of at least 50 % in spin and turn_easy, at least 25 % in turn_hard"""
    script = O.episode_returns(RESET_SEED, range(16), mode, radius, O.scripted(mode))
    random = []
    for seed in range(16):
        r = np.random.RandomState(seed)
        random.append(O.episode_returns(RESET_SEED, range(16), mode, radius, lambda p, g, s: r.uniform(-1, 1, (len(p), 2)).astype(F)))
    random = np.array(random)
    print(f"{name}: script mean {script.mean():.1f} ({script.min():.0f} .. {script.max():.0f}), random mean {random.mean():.2f}, "
          f"largest seed mean {random.mean(1).max():.2f}, largest episode {random.max():.0f}")
    assert random.mean(1).max() <= 100
    assert script.mean() >= (250 if name == "turn_hard" else 500)


# ------------------------------------------------------------------------------------------------ the shared drive
def test_inputs_of_the_gpu_tests_cover_what_they_claim():
    """The runs and poses tests/test_hip_vec_finger.py compares on the GPU, on the oracle alone"""
    assert {(c[0], c[1]) for c in O.DRIVEN} == {(3, 2), (5, 4)} and {c[2] for c in O.DRIVEN} == {1, 2, 16}
    assert {(c[3], c[5]) for c in O.DRIVEN} == {(0, True), (0, False), (1, True), (1, False)} and len(O.DRIVEN) == 24
    for cfg in O.DRIVEN:
        run = run_of(cfg)
        acts = np.stack(run["actions"])[:, :, :2]
        assert np.isnan(acts).any() and np.isinf(acts).any() and (np.abs(acts[np.isfinite(acts)]) > 1).any(), cfg
        firsts = np.stack([o[3] for o in run["out"]])
        assert firsts.any() and (cfg[2] > O.EPISODE_LENGTH or not (firsts.all(1) | ~firsts.any(1)).all()), "no stagger"
        assert run["reset_rows"] >= 1 and (cfg[2] == 1 or run["cut_by_limit"] >= 1), cfg     # a time limit inside a repeat
        assert all((o[2] == 1).all() for o in run["out"])                  # the discount is 1 on every row
        rewards = np.stack([o[1] for o in run["out"]])
        assert (rewards >= 0).all() and rewards.max() <= cfg[2]
        if cfg[3] == 1 and not cfg[5]:
            assert (rewards[firsts == 0] > 0).all()                        # the dense turn reward is positive on every step
    for cfg in O.PHYSICS:
        run = run_of(cfg)
        other = "turn_" if cfg[3] == 0 else "spin_"
        for name in O.EVENTS:
            assert run["events"][name] >= 1 or name.startswith(other), (name, run["events"])
        assert run["reset_rows"] == 0 and np.isfinite(np.stack([s["phys"] for s in run["states"]])).all()
    saved = run_of(O.PHYSICS[0])["states"][O.CUT - 1]["phys"]             # where the checkpoint test cuts: in contact, in motion
    assert O.gap_many(saved[:1])[0][0] <= float(O.TOUCH) + 1e-4 and (saved[0, [2, 5, 8]] != 0).all()
    # the poses: every shape's colour, never VecDistract's background key, and what the GPU test's docstring lists
    colours = set()
    for pose in O.POSES:
        frame = O.render(pose)
        shape = (frame != O.BACKGROUND).any(0)
        assert set(np.unique(frame[:, shape])) == {64, 255} and not (frame == 0xA5).any()
        assert not ((frame[0] == frame[1]) & (frame[1] == frame[2]))[shape].any()
        assert not shape[0].any() and not shape[-1].any() and not shape[:, 0].any() and not shape[:, -1].any()
        assert all(m.any() for m, _ in O.masks(pose)) and len(O.masks(pose)) == 6 + pose[2]
        colours |= {tuple(v) for v in frame[:, shape].T}
    assert colours == {O.TARGET_RGB, O.HINGE_RGB, O.ROD_RGB, O.UPPER_RGB, O.FORE_RGB, O.TIP_RGB}
    phys = np.stack([p[0] for p in O.POSES])
    assert {(1, 0), (0, 1), (-1, 0), (0, -1)} <= {(float(p[6]), float(p[7])) for p in phys}          # the rod along each axis
    assert ((phys[:, 1] == 0) & (phys[:, 4] == 0) & (phys[:, 0] != 0)).any() and ((phys[:, 0] == 0) & (phys[:, 4] == 0) & (phys[:, 1] != 0)).any()
    assert {O.MIN_RADIUS, O.MAX_RADIUS} <= {p[3] for p in O.POSES} and {0, 1} == {p[2] for p in O.POSES}
    points = [O.points(p[0], p[1], p[3]) for p in O.POSES]
    assert any((pt[2], pt[3]) == (O.CENTRE, O.HINGE_PY) for pt in points)                  # the fingertip over the hinge
    assert any(abs(pt[2] - pt[4]) <= 1 and abs(pt[3] - pt[5]) <= 1 for pt in points)       # ... over the rod's tip
    assert any((pt[0], pt[1]) == (O.CENTRE, O.ROOT_PY) and (pt[4], pt[5]) == (O.CENTRE, O.HINGE_PY) for pt in points)      # length 0
    # ... and every frame of a physics run and a driven run: never the key
    for run in (S.run_of(O, O.PHYSICS[1]), S.run_of(O, O.DRIVEN[-1])):
        for out in run["out"]:
            f = out[0].transpose(1, 0, 2, 3)
            shape = (out[0] != O.BACKGROUND).any(1)
            assert not ((f[0] == f[1]) & (f[1] == f[2]))[shape].any()
