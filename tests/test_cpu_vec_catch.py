"""The catch of the device environment (drq_vec_catch_step / _render, drqv2_amd.envs.VecCatch): everything that needs no GPU.
The public surface and the DRQ_EARG cases (all are decided before any launch); the conditions the constants of the rule
were chosen under -- no tunnelling, the ball inside the world, rest that stays rest, a scripted controller that catches
the ball where a random policy never does -- on the numpy restatement tests/vec_catch_oracle.py; and what the inputs of the
GPU tests (tests/test_hip_vec_catch.py) cover, which is a property of the oracle's runs alone.  Comparisons of bits have no
tolerance; a bound on a float64 quantity is derived where it stands."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_catch_oracle as O
from tests import vec_skeleton_oracle as S
from tests.vec_skeleton_oracle import same_bits

F = np.float32
STEP, RENDER = "drq_vec_catch_step", "drq_vec_catch_render"


def run_of(cfg):
    """the oracle's run of a configuration of O.DRIVEN or O.PHYSICS without its frames: computed once, never modified"""
    return S.run_of(O, cfg, frames=False)


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build_flags():
    from drqv2_amd import build, envs
    assert "veccatch.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "veccatch.hip"))
    assert build.FILE_FLAGS["veccatch.hip"] == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    header = abi.text()
    for name, nargs in ((STEP, 19), (RENDER, 5)):
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs and name not in _lib.NO_STREAM and name in abi.stream_entries()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for text in ("Catch.", "v = clamp(v * 0.9f + a * 0.3f, -1.5f, 1.5f);  q = c + v * 0.01f",
                 "vby = vby - 0.04f;  s2 = vbx * vbx + vby * vby", "s2 > 16: k = 4 / sqrt(s2);  vbx = vbx * k;  vby = vby * k",
                 "ay = cy + 0.02f;  dx = bx - cx;  dy = by - ay;  d2 = dx * dx + dy * dy",
                 "d2 > 0.25f: d = sqrt(d2);  nx = dx / d;  ny = dy / d;  bx = cx + nx * 0.5f;  by = ay + ny * 0.5f",
                 "vn = (vbx - vcx) * nx + (vby - vcy) * ny;  vn > 0: vbx = vbx - vn * nx;  vby = vby - vn * ny",
                 "ex = bx - T.x;  ey = by - T.y;  e2 = ex * ex + ey * ey;  e2 < 0.0049f", "e2 == 0: (nx, ny) = (0, 1)",
                 "vn < 0: vbx = vbx - vn * nx;  vby = vby - vn * ny", "uy = by - (cy + 0.085f);  d2 = ux * ux + uy * uy;  r_i = 1 / (1 + 4 * d2)",
                 "o = v_2 * 0.25f;  n = sqrt(o * o + 1)", "bx = cx + (o / n) * 0.5f;  by = ay - (1 / n) * 0.5f",
                 "X(x) = (int)floorf(x * 672 + 672.5f);  Y(y) = (int)floorf(672.5f - y * 672)"):
        assert text in header, text                                        # the rule is part of the contract
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    assert envs.VecCatch.TASK == "catch" and issubclass(envs.VecCatch, envs._VecTask)
    assert envs.VecCatch._MIN_ACTION_DIM == 2 and envs.VecCatch._STATE == ("phys", "t", "episode", "over")
    assert envs.VecCatch._STATE_SPEC["phys"] == ((8,), torch.float32)
    assert (envs.VecCatch.MIN_CUP_WIDTH, envs.VecCatch.MAX_CUP_WIDTH) == (O.MIN_WIDTH, O.MAX_WIDTH)
    with open(os.path.join(build.CSRC, "veccatch.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("sinf", "cosf", "expf", "__shared__", "atomic"):        # no libm rounding, no LDS, no atomics
        assert banned not in src, banned
    assert "sqrtf" in src and "launch_env_step<Catch>" in src and "launch_env_render<Catch>" in src


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_catch.py repeats them on poisoned outputs.)"""
    lib = _lib.load()
    calls, renders = O.refused_calls(0x10000, 0x20000, 0x30000, 0x40000), O.refused_renders(0x10000, 0x30000)
    S.all_refused(((lib.drq_vec_catch_step, calls), (lib.drq_vec_catch_render, renders)))
    ok = [0x10000, 0x10100, 0x10200, 0x10300, 5, 2, 0x20000, 7, 9, 2, 0, 0.3, 1, 0x30000, 0x40000, 0x40100, 0x40200, 0x40300]
    sub = lambda k, v: ok[:k] + [v] + ok[k + 1:]
    for a in ([None] + ok[1:], sub(0, 0x10002), sub(5, 1), sub(9, 0), sub(9, 17), sub(10, 2), sub(6, None), sub(11, 0.1599),
              sub(11, 0.401), sub(11, float("nan")), sub(12, 2), sub(13, 0x30008)):
        assert repr(a) in map(repr, calls), a                              # by text: a NaN equals no NaN
    for a in ([None, 3, 0.3, 0x30000], [0x10002, 3, 0.3, 0x30000], [0x10000, 3, 0.1599, 0x30000], [0x10000, 3, 0.401, 0x30000],
              [0x10000, 3, float("nan"), 0x30000]):
        assert repr(a) in map(repr, renders), a


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_constructor_state_and_state_dict_without_a_device(tmp_path):
    from drqv2_amd.envs import VecCartpole, VecCatch
    env = VecCatch(3, "cpu")
    assert (env.A, env.episode_length, env.action_repeat, env.cup_width, env.sparse) == (2, 1000, 1, 0.3, True)
    with pytest.raises(ValueError, match="action_dim >= 2"):
        VecCatch(3, "cpu", action_dim=1)
    for bad in (0.1599, 0.401, float("nan"), float("inf"), "0.3", None, True):
        with pytest.raises(ValueError, match="cup_width"):
            VecCatch(3, "cpu", cup_width=bad)
    for bad in (2, "yes", None, 0.5):
        with pytest.raises(ValueError, match="sparse"):
            VecCatch(3, "cpu", sparse=bad)
    for width in (0.16, 0.4):                                              # both ends are valid (on the device: the GPU test's poses)
        assert VecCatch(3, "cpu", cup_width=width).cup_width == width
    kw = dict(action_dim=3, episode_length=7, seed=1, action_repeat=2, cup_width=0.18, sparse=False)
    env = VecCatch(3, "cpu", **kw)
    with pytest.raises(ValueError, match=r"step\(\): action"):
        env.step(torch.zeros(3, 2))
    s = env.state()
    assert list(s) == ["phys", "t", "episode", "over"] and s["phys"].shape == (3, 8) and s["phys"].dtype == np.float32
    sd = env.state_dict()
    assert sd["kind"] == "VecCatch" and sd["config"] == {"N": 3, "A": 3, "episode_length": 7, "seed": 1, "task": "catch",
                                                          "action_repeat": 2, "cup_width": 0.18, "sparse": False}
    with pytest.raises(_lib.DrqError, match="GPU"):                        # the checks pass, then the device is refused
        VecCatch(3, "cpu", **kw).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bcup_width: saved 0.18, here 0.3"):
        VecCatch(3, "cpu", **dict(kw, cup_width=0.3)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"\bsparse: saved False, here True"):
        VecCatch(3, "cpu", **dict(kw, sparse=True)).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        VecCartpole(3, "cpu", action_dim=3, episode_length=7, seed=1, action_repeat=2).load_state_dict(sd)
    with pytest.raises(ValueError, match="phys: no tensor saved"):
        VecCatch(3, "cpu", **kw).load_state_dict({k: v for k, v in sd.items() if k != "phys"})
    # what no task decides: action_repeat, the methods, no CPU fallback, the skeleton's words, the checkpoint file
    ck = S.class_without_a_device(VecCatch, env, tmp_path, ("phys", (1, 5), 0.25), methods=("background_key",))
    assert ck["env"]["config"]["cup_width"] == 0.18 and ck["env"]["config"]["sparse"] is False


# ------------------------------------------------------------------------------------------------ the conditions on the constants
def test_no_tunnelling_and_the_ball_stays_in_the_world():
    """in float64 on the oracle's float32 constants: the largest relative displacement of ball and cup in one step is less
    than the distance at which they touch; the reach of the ball and the cup's widest form fit the world on both axes;
    a ball in contact cannot be at the tether's length; the integer radii of the frame are the rounded world radii"""
    c = {k: float(getattr(O, k)) for k in ("DT", "MAX_CUP_V", "MAX_BALL_V", "RANGE", "TETHER", "WALL", "CAPSULE_R", "BALL_R",
                                            "TOUCH", "TOUCH2", "TETHER2", "MAX_BALL_V2", "MID_Y", "RESET_XY", "GDT")}
    assert (c["MAX_BALL_V"] + c["MAX_CUP_V"] * np.sqrt(2)) * c["DT"] < c["BALL_R"] + c["CAPSULE_R"]
    assert c["RANGE"] + c["CAPSULE_R"] + c["TETHER"] + c["BALL_R"] <= 1          # y: the anchor is 0.02 above cy; x has less
    assert c["RANGE"] + O.MAX_WIDTH / 2 + c["CAPSULE_R"] <= 1 and c["RANGE"] + c["WALL"] + c["CAPSULE_R"] <= 1
    assert O.TOUCH == F(O.BALL_R + O.CAPSULE_R) and abs(c["TOUCH2"] - c["TOUCH"] ** 2) < 1e-9
    assert O.TETHER2 == F(O.TETHER * O.TETHER) and O.MAX_BALL_V2 == F(O.MAX_BALL_V * O.MAX_BALL_V) and O.GDT == F(F(4) * O.DT)
    assert c["MID_Y"] == pytest.approx((c["CAPSULE_R"] + c["WALL"]) / 2, abs=1e-7) and c["RESET_XY"] * 0.9 <= c["RANGE"]
    assert np.hypot(O.MAX_WIDTH / 2, c["WALL"]) + c["CAPSULE_R"] + c["TOUCH"] < c["TETHER"]
    assert O.MIN_WIDTH - 2 * c["CAPSULE_R"] > 2 * c["BALL_R"]                     # the ball fits the narrowest cup
    assert O.MIN_WIDTH <= O.HARD_WIDTH < O.WIDTH <= O.MAX_WIDTH
    assert (O.CUP_R, O.BALL_PIX) == (round(c["CAPSULE_R"] * 672), round(c["BALL_R"] * 672)) and O.TETHER_R < O.CUP_R


def test_after_a_reset_the_ball_hangs_at_rest_at_the_tethers_length():
    """256 (environment, episode) pairs: the cup inside its range, the ball below the anchor within the tether's length up
    to the stated slack (O.check_state), nothing moves, and the states do differ"""
    seen = set()
    for e in range(16):
        for ep in range(1, 17):
            p = O.reset_state(11, e, ep)
            O.check_state(p, O.half_width(O.MAX_WIDTH))
            assert all(v == 0 for v in (p[2], p[3], p[6], p[7])) and all(v.dtype == np.float32 for v in p)
            ay = float(F(p[1] + O.CAPSULE_R))
            assert float(p[5]) < ay - 0.48 and abs(float(p[4]) - float(p[0])) <= 0.5 * 0.225 / np.sqrt(1 + 0.225 ** 2) + 1e-6
            assert np.hypot(float(p[4]) - float(p[0]), float(p[5]) - ay) >= 0.5 - 2 * 2.0 ** -23
            seen.add(tuple(float(v) for v in p))
    assert len(seen) == 256


def energy(p):
    """of the ball, in float64: 4 by + |vb|^2 / 2"""
    return 4.0 * float(p[5]) + 0.5 * (float(p[6]) ** 2 + float(p[7]) ** 2)


@pytest.mark.parametrize("where", ["floor", "tether"])
def test_rest_is_quiet(where):
    """a ball lying on the floor of a still cup, and one hanging on the taut tether under it: 1,000 steps under zero action.
    The cup does not move at all.  The ball keeps its x to the bit and stays within 2 float32 ulps of 1 of where it lay (the
    push-out and the projection each end in one add of numbers below 1); on the floor it is in the cup on every step.  Its
    energy never exceeds the start's by more than the 4 * 2 ulps that bound on y allows, and its velocity is 0 after every
    step: what gravity adds, the contact or the string removes"""
    for cx, cy in ((0, 0), (0.25, -0.125), (-0.4, 0.4), (0.3333, 0.1111)):
        cx, cy = F(cx), F(cy)
        ay = F(cy + O.CAPSULE_R)
        by = F(cy + O.TOUCH) if where == "floor" else F(ay - O.TETHER)
        bx = F(cx + F(0.03)) if where == "floor" else cx
        start = (cx, cy, F(0), F(0), bx, by, F(0), F(0))
        hw = O.half_width(O.WIDTH)
        p, e0 = start, energy(start)
        for i in range(1000):
            p, ev = O.substep(p, F(0), F(0), hw)
            O.check_state(p, hw)
            same_bits(np.array(p[:5]), np.array(start[:5]), (where, i))
            assert abs(float(p[5]) - float(by)) <= 2 * 2.0 ** -23 and p[6] == 0 and p[7] == 0, (where, i, p)
            assert energy(p) <= e0 + 8 * 2.0 ** -23
            if where == "floor":
                assert O.in_cup(p, hw) and ev["floor"] == 1 and ev["slack"] == 1
            else:
                assert ev["taut"] == 1 and not O.in_cup(p, hw)


def test_a_swinging_ball_under_a_still_cup_loses_energy():
    """a pendulum released from the horizontal and a ball dropped into the cup from above: after 1,000 steps under zero
    action the ball's energy is below the start's, and every state on the way passed O.check_state"""
    hw = O.half_width(O.WIDTH)
    for start in ((0, 0, 0, 0, 0.5, 0.02, 0, 0), (0.1, -0.2, 0, 0, 0.12, 0.25, 0.2, 0), (0, 0.3, 0, 0, -0.3, -0.08, -1, 2)):
        p = tuple(F(v) for v in start)
        e0 = energy(p)
        for _ in range(1000):
            p, _ = O.substep(p, F(0), F(0), hw)
            O.check_state(p, hw)
        assert all(np.isfinite(v) and v.dtype == np.float32 for v in p) and energy(p) < e0


# ------------------------------------------------------------------------------------------------ sparse and solvable
EXPERT_SEED, EXPERT_EPISODE = 3, 1       # the eight reset states: environments 0 .. 7 of this seed, their first episode


def test_the_expert_catches_the_ball_on_all_eight_resets_and_a_random_policy_does_not():
    """default cup_width, 1,000 steps: under O.expert() the ball is in the cup on every one of the last 100 steps, on all
    eight resets; a seeded uniform-random policy's sparse return on the same resets is under 1 % of the expert's"""
    expert = [O.episode(EXPERT_SEED, e, EXPERT_EPISODE, lambda p, i: O.expert(p)) for e in range(8)]
    print(f"expert returns {[int(r) for r, _ in expert]}, first step in the cup {[ins.index(True) for _, ins in expert]}")
    for total, inside in expert:
        assert len(inside) == 1000 and all(inside[-100:]) and total >= 100
    r = np.random.RandomState(0)
    rand = [O.episode(EXPERT_SEED, e, EXPERT_EPISODE, lambda p, i: r.uniform(-1, 1, 2).astype(F))[0] for e in range(8)]
    print(f"random returns {[int(v) for v in rand]}")
    assert sum(rand) < 0.01 * sum(total for total, _ in expert)
    assert all(v < 0.01 * total for v, (total, _) in zip(rand, expert))


# ------------------------------------------------------------------------------------------------ the shared drive
def test_inputs_of_the_gpu_tests_cover_what_they_claim():
    """The runs and poses tests/test_hip_vec_catch.py compares on the GPU, on the oracle alone.  Every state of every run
    has passed O.check_state inside the oracle: the ball within the tether's length of the anchor up to 2 ulps of 1, the
    ball inside the world, the cup inside its range"""
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
        assert run["events"]["taut"] >= 1 and run["events"]["slack"] >= 1, cfg
        if cfg[3]:      # sparse: exact small integers
            assert (rewards == np.round(rewards)).all() and rewards.min() >= 0 and rewards.max() <= cfg[2]
        else:
            assert (rewards[firsts == 0] > 0).all()
    for cfg in O.PHYSICS:
        run = run_of(cfg)
        for name in O.EVENTS:                                              # the tether both ways, every contact from every
            assert run["events"][name] >= 1, (name, run["events"])         # side, the degenerate normal, stops, clamps
        assert run["longest_rest"] >= 50 and run["rewarded"] >= 1 and run["unrewarded"] >= 1 and run["reset_rows"] == 0
        assert (np.abs(np.stack(run["actions"])[:, 0, :]) > 1).any()
        rewards = np.stack([o[1] for o in run["out"]])
        if cfg[3]:
            assert rewards.max() == cfg[2] and rewards.min() == 0 and (rewards == np.round(rewards)).all()
    # the poses: every shape inside the frame, its own colour, never VecDistract's background key
    colours = set()
    for phys, width in O.POSES:
        O.check_state(tuple(phys), O.half_width(width))
        frame = O.render(phys, width)
        shape = (frame != O.BACKGROUND).any(0)
        assert set(np.unique(frame[:, shape])) == {64, 255} and not (frame == 0xA5).any()
        assert not ((frame[0] == frame[1]) & (frame[1] == frame[2]))[shape].any()
        assert not shape[0].any() and not shape[-1].any() and not shape[:, 0].any() and not shape[:, -1].any()   # all inside
        for m, _ in O.masks(phys, width):
            assert m.any() and not (m & ~shape).any()
        colours |= {tuple(v) for v in frame[:, shape].T}
        assert {O.BALL_RGB, O.FLOOR_RGB} <= {tuple(v) for v in frame[:, shape].T}
    assert colours == {O.TETHER_RGB, O.LEFT_RGB, O.RIGHT_RGB, O.FLOOR_RGB, O.BALL_RGB}
    rel = [(float(p[4]) - float(p[0]), float(p[5]) - float(F(p[1] + O.CAPSULE_R))) for p, _ in O.POSES]
    assert any(abs(dx) == 0.5 and dy == 0 for dx, dy in rel) and any(dx == 0 and abs(dy + 0.5) < 1e-6 for dx, dy in rel)
    assert any(dx == 0 and dy == 0 for dx, dy in rel)                      # horizontal, vertical, zero length
    assert {(float(p[0]), float(p[1])) for p, _ in O.POSES} >= {(F(x).item(), F(y).item()) for x in (-0.4, 0.4) for y in (-0.4, 0.4)}
    assert {w for _, w in O.POSES} >= {O.MIN_WIDTH, O.HARD_WIDTH, O.WIDTH, O.MAX_WIDTH}
    # ... and every frame of a physics run and a driven run: inside, and never the key
    for run in (S.run_of(O, O.PHYSICS[0]), S.run_of(O, O.DRIVEN[-1])):
        for out in run["out"]:
            shape = (out[0] != O.BACKGROUND).any(1)
            assert not shape[:, 0].any() and not shape[:, -1].any() and not shape[:, :, 0].any() and not shape[:, :, -1].any()
            f = out[0].transpose(1, 0, 2, 3)
            assert not ((f[0] == f[1]) & (f[1] == f[2]))[shape].any()
