"""The walker of the device environment (drq_vec_walker_step / _render, drqv2_amd.envs.VecWalker): everything that needs no
GPU.  The public surface and the DRQ_EARG cases (all are decided before any launch); the conditions the constants of the
rule were chosen under -- a body that stands at rest, holds together under any action, never flips a joint, stays in the
frame, and can be run by a scripted gait where random actions get nowhere -- on the numpy restatement
tests/vec_walker_oracle.py; and what the inputs of the GPU tests (tests/test_hip_vec_walker.py) cover, which is a property of
the oracle's runs alone.  Comparisons of bits have no tolerance; a bound on a float64 quantity is stated where it stands."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_skeleton_oracle as S
from tests import vec_walker_oracle as O
from tests.vec_skeleton_oracle import same_bits

F = np.float32
STEP, RENDER = "drq_vec_walker_step", "drq_vec_walker_render"
RESET_SEED = 11                  # the fixed resets: environments 0 .. 63 of this seed, their first episode


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN or O.PHYSICS without its frames: computed once, never modified"""
    return S.run_of(O, cfg, frames=False)


def middle(phys):
    return (phys[:, 0].astype(np.float64) + phys[:, 4]) / 2


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build_flags():
    from drqv2_amd import build, envs
    assert "vecwalker.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecwalker.hip"))
    assert build.FILE_FLAGS["vecwalker.hip"] == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    header = abi.text()
    for name, nargs in ((STEP, 18), (RENDER, 4)):
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs and name not in _lib.NO_STREAM and name in abi.stream_entries()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for text in ("Walker.", "vx = vx * 0.9f;  vy = vy * 0.9f - 0.1f;  ox = x;  oy = y;  x = x + vx * 0.01f",
                 "T_m = mid_m + a_m * half_m", "d2 == 0: d = 0, (nx, ny) = (0, 1)",
                 "h = c * 0.5f;  hx = nx * h;  hy = ny * h;  x_i = x_i + hx;  y_i = y_i + hy",
                 "s < 4: c = clamp((d - T_m) * 0.5f, -0.004f, 0.004f)", "q = d - c;  q < lo_m: c = d - lo_m;  else q > hi_m: c = d - hi_m",
                 "vx = (x - ox) * 100;  vy = (y - oy) * 100;  y == 0: vx = vx * 0.1f",
                 "s2 > 4: k = 2 / sqrt(s2);  vx = vx * k;  vy = vy * k",
                 "mid = (x_0 + x_1) * 0.5f;  mid >= 2: every x_i = x_i - 4;  else mid < -2: every x_i = x_i + 4",
                 "stand = clamp01((height - 0.1f) * 10) * clamp01((upright - 0.5f) * 2.5f)",
                 "move = clamp01(v / speed);  r_i = stand * (1 + 5 * move) / 6",
                 "tilt = v_0 * 0.05f;  n = sqrt(tilt * tilt + 1);  ux = 1 / n;  uy = tilt / n",
                 "C = (int)floorf((x_0 + x_1) * 0.5f * 672)", "X_i = (int)floorf(x_i * 672 + 0.5f) - C + 672;  Y_i = (int)floorf(1008.5f - y_i * 672)"):
        assert text in header, text                                        # the rule is part of the contract
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    cls = envs.VecWalker
    assert cls.TASK == "walker" and issubclass(cls, envs._VecTask)
    assert cls._MIN_ACTION_DIM == 4 and cls._STATE == ("phys", "t", "episode", "over")
    assert cls._STATE_SPEC["phys"] == ((24,), torch.float32)
    assert (cls.MAX_SPEED, cls.WALK_SPEED, cls.RUN_SPEED) == (O.MAX_SPEED, O.WALK_SPEED, O.RUN_SPEED) and O.RUN_SPEED == 2 * O.WALK_SPEED
    with open(os.path.join(build.CSRC, "vecwalker.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("sinf", "cosf", "expf", "__shared__", "atomic"):        # no libm rounding, no LDS, no atomics
        assert banned not in src, banned
    assert "sqrtf" in src and "launch_env_step<Walker>" in src and "launch_env_render<Walker>" in src


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_walker.py repeats them on poisoned outputs.)"""
    lib = _lib.load()
    calls, renders = O.refused_calls(0x10000, 0x20000, 0x30000, 0x40000), O.refused_renders(0x10000, 0x30000)
    S.all_refused(((lib.drq_vec_walker_step, calls), (lib.drq_vec_walker_render, renders)))
    ok = [0x10000, 0x10100, 0x10200, 0x10300, 5, 4, 0x20000, 7, 9, 2, 0, 0.3, 0x30000, 0x40000, 0x40100, 0x40200, 0x40300]
    sub = lambda k, v: ok[:k] + [v] + ok[k + 1:]
    for a in ([None] + ok[1:], sub(0, 0x10002), sub(5, 3), sub(5, 0), sub(9, 0), sub(9, 17), sub(10, 2), sub(6, None), sub(11, -0.001),
              sub(11, 2.001), sub(11, float("nan")), sub(12, 0x30008)):
        assert repr(a) in map(repr, calls), a                              # by text: a NaN equals no NaN
    for a in ([None, 3, 0x30000], [0x10002, 3, 0x30000], [0x10000, 0, 0x30000], [0x10000, 3, None], [0x10000, 3, 0x30008]):
        assert repr(a) in map(repr, renders), a
    assert (len(calls), len(renders)) == (N_REFUSED_CALLS, N_REFUSED_RENDERS)


N_REFUSED_CALLS, N_REFUSED_RENDERS = 10 + 21 + 3 + 7, 2 + 3 + 2 + 1      # pointers, scalars, the frame, words; the render's


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_constructor_state_and_state_dict_without_a_device(tmp_path):
    from drqv2_amd.envs import VecCatch, VecWalker
    env = VecWalker(3, "cpu")
    assert (env.A, env.episode_length, env.action_repeat, env.speed) == (4, 1000, 1, O.WALK_SPEED)
    with pytest.raises(ValueError, match="action_dim >= 4"):
        VecWalker(3, "cpu", action_dim=3)
    for bad in (-0.001, 2.001, float("nan"), float("inf"), "0.3", None, True):
        with pytest.raises(ValueError, match="speed"):
            VecWalker(3, "cpu", speed=bad)
    for speed in (0, 0.0, 2.0, O.RUN_SPEED):                               # both ends are valid
        assert VecWalker(3, "cpu", speed=speed).speed == speed
    kw = dict(action_dim=5, episode_length=7, seed=1, action_repeat=2, speed=0.6)
    env = VecWalker(3, "cpu", **kw)
    with pytest.raises(ValueError, match=r"step\(\): action"):
        env.step(torch.zeros(3, 4))
    s = env.state()
    assert list(s) == ["phys", "t", "episode", "over"] and s["phys"].shape == (3, 24) and s["phys"].dtype == np.float32
    sd = env.state_dict()
    assert sd["kind"] == "VecWalker" and sd["config"] == {"N": 3, "A": 5, "episode_length": 7, "seed": 1, "task": "walker",
                                                           "action_repeat": 2, "speed": 0.6}
    with pytest.raises(_lib.DrqError, match="GPU"):                        # the checks pass, then the device is refused
        VecWalker(3, "cpu", **kw).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bspeed: saved 0.6, here 0.3"):
        VecWalker(3, "cpu", **dict(kw, speed=0.3)).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        VecCatch(3, "cpu", action_dim=5, episode_length=7, seed=1, action_repeat=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="phys: no tensor saved"):
        VecWalker(3, "cpu", **kw).load_state_dict({k: v for k, v in sd.items() if k != "phys"})
    # what no task decides: action_repeat, the methods, no CPU fallback, the skeleton's words, the checkpoint file
    ck = S.class_without_a_device(VecWalker, env, tmp_path, ("phys", (1, 5), 0.25), methods=("background_key",))
    assert ck["env"]["config"]["speed"] == 0.6


# ------------------------------------------------------------------------------------------------ the two restatements
def wild(r, n, s, held):
    """S.wild_actions with 1e30 and +-1 flips among them; held: None on the seven steps of eight that keep the action"""
    if held and s % 8:
        return None
    a = S.wild_actions(r, n, 4)
    kind = r.randint(0, 16, a.shape)
    a[kind == 0] = F(1e30)
    a[kind == 1] = np.where(r.randint(0, 2, a.shape) == 0, F(-1), F(1))[kind == 1]
    return O.sanitise_many(a)


def test_the_array_rule_equals_the_scalar_rule_bit_for_bit():
    """300 steps of 8 resets under wild actions, and the five hand-set states of the physics runs: substep_many() and
    substep() agree in every bit of every state, and sanitise_many() with S.sanitise"""
    r = np.random.RandomState(0)
    raw = S.wild_actions(r, 64, 4)
    same_bits(O.sanitise_many(raw), np.array([[S.sanitise(v) for v in row] for row in raw], F), "sanitise")
    for phys in (O.reset_states(RESET_SEED, range(8)), np.stack(list(O.physics_start().values()))):
        scalar = [tuple(p) for p in phys]
        for s in range(300):
            a = wild(r, len(phys), s, False)
            phys, shift = O.substep_many(phys, a)
            scalar = [O.substep(p, tuple(a[e]))[0] for e, p in enumerate(scalar)]
            same_bits(phys, np.array(scalar, F), s)
            assert set(np.unique(shift)) <= {-4.0, 0.0, 4.0}


def test_after_a_reset_the_body_stands_on_a_foot_inside_its_limits():
    """256 (environment, episode) pairs: rods exact to rounding, muscle distances inside the muscles' own range, the lowest
    knee or foot exactly on the ground and nothing below it, the torso's middle at x = 0, nothing moves, and the states differ"""
    phys = np.array([O.reset_state(RESET_SEED, e, ep) for e in range(16) for ep in range(1, 17)], F)
    rods, muscles = O.lengths(phys)
    assert (np.abs(rods - [float(r[2]) for r in O.RODS]) < 1e-6).all()
    mid, half = np.array([float(v) for v in O.MID]), np.array([float(v) for v in O.HALF])
    assert (np.abs(muscles - mid) <= 0.25 * half + 1e-6).all()
    assert (phys[:, 2::4] == 0).all() and (phys[:, 3::4] == 0).all()
    assert (phys[:, 9::4].min(1) == 0).all() and (phys[:, 1::4] >= 0).all()
    assert (np.abs(middle(phys)) < 1e-7).all() and len({p.tobytes() for p in phys}) == 256
    assert (O.joint_signs(phys) == O.joint_signs(phys[:1])).all()          # every reset bends its joints the same way
    O.check_states(phys)


# ------------------------------------------------------------------------------------------------ the conditions on the constants
def test_the_body_stands_at_rest_under_the_zero_action():
    """64 fixed resets, 1,000 steps of the zero action.  After every step, from the first, on every environment: stand == 1,
    the torso's height where stand's height term is 1 and the torso upright enough for it; the torso's middle within a
    tenth of the torso's length of where it started, the largest drift taken over all steps; over the last 100 steps no
    particle is faster than 1e-3"""
    phys = O.reset_states(RESET_SEED, range(64))
    start, zero, fastest, drift = middle(phys), np.zeros((64, 4), F), 0.0, 0.0
    assert all(O.stand_of(p) == 1 for p in phys)
    for s in range(1000):
        phys, _ = O.substep_many(phys, zero)
        assert all(O.stand_of(p) == 1 for p in phys), s
        assert ((phys[:, 1] + phys[:, 5]) / 2 >= O.STAND_HEIGHT).all() and ((phys[:, 0] - phys[:, 4]) * 2.5 >= 0.9).all(), s
        drift = max(drift, float(np.abs(middle(phys) - start).max()))
        if s >= 900:
            fastest = max(fastest, float(np.abs(phys[:, 2::4]).max()), float(np.abs(phys[:, 3::4]).max()))
    print(f"drift {drift:.4f} of {0.1 * float(O.TORSO)}, fastest {fastest:.2e}, height {phys[:, 1].min():.4f} .. {phys[:, 1].max():.4f}")
    assert drift < 0.1 * float(O.TORSO) and fastest < 1e-3
    O.check_states(phys)


@pytest.mark.parametrize("held", [False, True], ids=["per_step", "held"])
def test_the_body_holds_together_never_flips_a_joint_and_stays_in_the_frame(held):
    """64 fixed resets, 2,000 steps of wild actions (+-1 flips, NaN, +-inf, 1e30, uniform beyond the clamp; drawn every step,
    or held for 8).  After every step (O.check_states): every state word finite; every y >= 0 exactly; every rod within
    1 % of its length; every muscle distance inside its joint's hard limits, with no slack; the sign of each joint's
    cross product as at the reset; every particle within the frame's half width of the camera and below the frame's top.
    O.check_states asserts all of it; the worst figures are only printed beside it"""
    r = np.random.RandomState(17 + held)
    phys = O.reset_states(RESET_SEED, range(64))
    signs = O.joint_signs(phys)
    assert (signs != 0).all()
    a, worst_rod, worst_limit, top = None, 0.0, -1.0, 0.0
    for s in range(2000):
        new = wild(r, 64, s, held)
        a = a if new is None else new
        phys, _ = O.substep_many(phys, a)
        O.check_states(phys, signs)
        rods, muscles = O.lengths(phys)
        worst_rod = max(worst_rod, float(np.abs(rods / [float(v[2]) for v in O.RODS] - 1).max()))
        worst_limit = max(worst_limit, float((np.array(O.LO, float) - O.SKIN - muscles).max()), float((muscles - np.array(O.HI, float) - O.SKIN).max()))
        top = max(top, float(phys[:, 1::4].max()))
    print(f"worst rod error {worst_rod:.5f}, worst distance beyond a hard limit {worst_limit:.5f}, highest particle {top:.3f}")


def gait_run(phys, speed, steps=1000):
    """the states phys under O.gait for `steps`: the displacement of the torso's middle, wraps undone, and the mean move"""
    start, wraps, move = middle(phys), np.zeros(len(phys)), 0.0
    for s in range(steps):
        phys, shift = O.substep_many(phys, np.repeat(O.gait(s)[None], len(phys), 0))
        wraps -= shift
        move += np.clip((phys[:, 2].astype(np.float64) + phys[:, 6]) / 2 / speed, 0, 1) / steps
    O.check_states(phys)
    return middle(phys) + wraps - start, move


def random_run(phys, r, hold, steps=1000):
    start, wraps, a = middle(phys), np.zeros(len(phys)), None
    for s in range(steps):
        if s % hold == 0:
            a = r.uniform(-1, 1, (len(phys), 4)).astype(F)
        phys, shift = O.substep_many(phys, a)
        wraps -= shift
    return middle(phys) + wraps - start


def test_the_gait_runs_where_random_actions_get_nowhere():
    """speed = the walk speed, 1,000 simulator steps: O.gait moves the torso forward by at least 3 torso lengths on each of
    8 fixed resets, at least 4 times the largest absolute displacement of uniformly random actions on 64 resets, drawn per
    step and held for 8 steps; the gait's mean move term is at least 0.5"""
    forward, move = gait_run(O.reset_states(RESET_SEED, range(8)), O.WALK_SPEED)
    r = np.random.RandomState(2)
    random = max(float(np.abs(random_run(O.reset_states(RESET_SEED, range(64)), r, hold)).max()) for hold in (1, 8))
    print(f"gait {np.round(forward, 3).tolist()}, mean move {np.round(move, 3).tolist()}, random at most {random:.3f}")
    assert (forward >= 3 * float(O.TORSO)).all() and (forward >= 4 * random).all() and (move >= 0.5).all()


def test_the_wrap_keeps_the_body_and_the_ground_under_it():
    """a body carried across +2 and one across -2 (reset poses beside the seam, every particle at +-1.5): the step shifts
    every x by -+4, the rods keep their lengths within the rod tolerance on that step and on the 50 after it, and the frame
    of the shifted state equals the frame of the same state not shifted, in every pixel: the camera's integer moved by
    4 * 672 = 8 * 336, a whole number of periods, so the ground stripes under the body have the same phase"""
    assert float(O.WORLD) * O.UNIT == 8 * O.PERIOD
    for sign in (1, -1):
        phys = O.reset_states(RESET_SEED, range(4))
        phys[:, 0::4] += F(sign * 1.99)
        phys[:, 2::4] = F(sign * 1.5)
        after, shift = O.substep_many(phys, np.zeros((4, 4), F))
        assert (shift == -4 * sign).all() and (np.abs(middle(after) - middle(phys) + 4 * sign) < 0.02).all()
        O.check_states(after)
        assert np.abs(O.lengths(after)[0] - O.lengths(phys)[0]).max() <= O.ROD_TOLERANCE * float(O.LIMB)
        unshifted = after.copy()
        unshifted[:, 0::4] -= shift[:, None]
        for e in range(4):
            assert O.points(unshifted[e])[0] - O.points(after[e])[0] == sign * 8 * O.PERIOD
            same_bits(O.render(after[e]), O.render(unshifted[e]), ("the frame across the seam", sign, e))
        for s in range(50):
            after, _ = O.substep_many(after, np.repeat(O.gait(s)[None], 4, 0))
            O.check_states(after)


# ------------------------------------------------------------------------------------------------ the shared drive
def test_inputs_of_the_gpu_tests_cover_what_they_claim():
    """The runs and poses tests/test_hip_vec_walker.py compares on the GPU, on the oracle alone.  Every state of every
    driven run has passed O.check_states inside the oracle"""
    for cfg in O.DRIVEN:
        run = run_of(cfg)
        acts = np.stack(run["actions"])[:, :, :4]
        assert np.isnan(acts).any() and np.isinf(acts).any() and (np.abs(acts[np.isfinite(acts)]) > 1).any(), cfg
        firsts = np.stack([o[3] for o in run["out"]])
        assert firsts.any() and (cfg[2] > O.EPISODE_LENGTH or not (firsts.all(1) | ~firsts.any(1)).all()), "no stagger"
        assert run["reset_rows"] >= 1 and (cfg[2] == 1 or run["cut_by_limit"] >= 1), cfg     # a time limit inside a repeat
        assert all((o[2] == 1).all() for o in run["out"])                  # the discount is 1 on every row
        rewards = np.stack([o[1] for o in run["out"]])
        assert (rewards[firsts == 0] > 0).all() and rewards.max() <= cfg[2]      # a standing body is paid on every step
        assert run["events"]["force_clamp"] >= 1 and run["events"]["ground_front_foot"] + run["events"]["ground_back_foot"] >= 1
    for cfg in O.PHYSICS:
        run = run_of(cfg)
        for name in O.EVENTS:
            assert run["events"][name] >= 1 or (cfg[3] == 0 and name.startswith("move_")), (name, run["events"])
        assert run["reset_rows"] == 0 and (np.abs(np.stack(run["actions"])[:, 2, :]) > 1).any()
        states = np.stack([s["phys"] for s in run["states"]])
        assert np.isfinite(states).all() and (states[:, :, 1::4] >= 0).all()
        for e in (0, 1):                                                   # the two that start from a reset pose hold together
            O.check_states(states[:, e])
    # the poses: every shape its own colour, never VecDistract's background key, and what the GPU test's docstring lists
    colours = set()
    for phys in O.POSES:
        frame = O.render(phys)
        shape = (frame != O.BACKGROUND).any(0)
        assert set(np.unique(frame[:, shape])) == {64, 255} and not (frame == 0xA5).any()
        assert not ((frame[0] == frame[1]) & (frame[1] == frame[2]))[shape].any()
        assert shape[64:].all() and not shape[:, 0][:40].any() and not shape[0].any()      # the ground band is full; the body inside
        for m, _ in O.masks(phys):
            assert m.any()
        colours |= {tuple(v) for v in frame[:, shape].T}
    assert colours == {O.TORSO_RGB, O.FRONT_RGB, O.BACK_RGB, O.STRIPE_A_RGB, O.STRIPE_B_RGB}
    x, y = np.stack([p[0::4] for p in O.POSES]), np.stack([p[1::4] for p in O.POSES])
    cam = [O.points(p)[0] for p in O.POSES]
    assert (y == 0).all(1).any() and (y == 0).any(1).sum() >= 3           # lying flat; a particle exactly at y = 0
    assert ((y[:, 0] == y[:, 1]) & (x[:, 0] == x[:, 2]) & (x[:, 2] == x[:, 3]) & (y[:, 2] == y[:, 3])).any()
    assert (x[:, 0] > 2).any() and (x[:, 0] < -1.7).any() and min(cam) < 0 and 336 in cam and -336 in cam
    assert any(c % O.PERIOD not in (0,) and c < 0 for c in cam)           # a negative offset that is no whole period
    # ... and every frame of a physics run and a driven run: never the key, the ground band full
    for run in (S.run_of(O, O.PHYSICS[1]), S.run_of(O, O.DRIVEN[-1])):
        for out in run["out"]:
            f = out[0].transpose(1, 0, 2, 3)
            shape = (out[0] != O.BACKGROUND).any(1)
            assert not ((f[0] == f[1]) & (f[1] == f[2]))[shape].any() and shape[:, 64:].all()
