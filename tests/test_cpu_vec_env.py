"""The device environment (VecReach, drq_vec_reach_step / drq_vec_reach_image): everything that needs no GPU.  The numpy
restatement tests/vec_env_oracle.py against hand-computed cases, the public surface (header, prototype table, build list
and flags, exported symbols, ABI version), the DRQ_EARG cases that are decided before any launch, and the argument
errors and the CPU refusal of the class."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_env_oracle as E
from tests import vec_render_oracle as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"drq_vec_reach_step": 16, "drq_vec_reach_image": 6}
F = np.float32


# ------------------------------------------------------------------------------------------------ the oracle
def test_fmix32_on_known_inputs():
    """the murmur3 finaliser: 0 is its fixed point, the other three are the values of the reference implementation"""
    assert E.fmix32(0) == 0
    assert E.fmix32(1) == 0x514E28B7
    assert E.fmix32(0x12345678) == 0xE37CD1BC
    assert E.fmix32(0xFFFFFFFF) == 0x81F16F39


def test_draws_are_on_the_24_bit_grid_inside_the_square():
    seen = set()
    for e in (0, 1, 64, 4095):
        for episode in (1, 2, 2 ** 32 - 1):
            for k in range(4):
                v = E.draw(12345, e, episode, k)
                assert v.dtype == F and -0.9 <= float(v) <= 0.9
                seen.add(float(v))
    assert len(seen) == 48                                  # environment, episode and k all enter the hash
    # by hand: seed 0, e 0, episode 1, k 0 hashes fmix32(0x85EBCA6B)
    h = E.fmix32(0x85EBCA6B)
    assert E.draw(0, 0, 1, 0) == F(F(F(F(h >> 8) * F(2.0 ** -24)) * F(2) - F(1)) * F(0.9))
    assert E.draw(2 ** 32 + 5, 3, 1, 2) == E.draw(5, 3, 1, 2)   # the seed is taken mod 2^32


def test_disc_pixel_counts_and_the_frame():
    """lattice points with x^2 + y^2 <= 25: 81; <= 16: 49"""
    assert int(E.disc(40, 30, 25).sum()) == 81 and int(E.disc(40, 30, 16).sum()) == 49
    assert int(E.disc(0, 0, 25).sum()) == 26                # a corner keeps the quarter with its two axes
    assert E.centre(F(-1)) == 0 and E.centre(F(1)) == 83 and E.centre(F(0)) == 42
    pos, target = np.array([-0.5, 0.5], F), np.array([0.5, -0.5], F)        # centres (21, 62) and (62, 21): far apart
    f = E.render(pos, target)
    assert f.shape == (3, 84, 84) and f.dtype == np.uint8
    assert (E.centre(pos[0]), E.centre(pos[1]), E.centre(target[0]), E.centre(target[1])) == (21, 62, 62, 21)
    agent, goal = (f[0] == 255), (f[1] == 255)
    assert int(agent.sum()) == 49 and int(goal.sum()) == 81 and not (agent & goal).any()
    assert agent[62, 21] and agent[62, 25] and not agent[62, 26]             # row = y, column = x
    assert goal[21, 62] and goal[26, 62] and not goal[27, 62] and goal[24, 66] and not goal[25, 66]
    assert f[:, 62, 21].tolist() == [255, 64, 64] and f[:, 21, 62].tolist() == [64, 255, 64]
    assert f[:, 0, 0].tolist() == [32] * 3 and f[:, 83, 83].tolist() == [73] * 3 and f[:, 3, 1].tolist() == [33] * 3
    bg = ~(agent | goal)
    assert all(np.array_equal(f[c][bg], (32 + ((E._II + E._JJ) >> 2))[bg]) for c in range(3))
    # the agent is drawn over the target
    g = E.render(np.array([0.0, 0.0], F), np.array([0.0, 0.0], F))
    assert int((g[0] == 255).sum()) == 49 and int((g[1] == 255).sum()) == 81 - 49


def env_at(pos, target, N=1, L=5):
    o = E.ReachOracle(N, episode_length=L, seed=1)
    o.reset()
    o.pos[:], o.target[:] = np.asarray(pos, F), np.asarray(target, F)
    return o


def test_step_moves_clamps_and_ignores_nan():
    o = env_at([0.25, 0.95], [-0.8, -0.8])
    _, r, d, first = o.step(np.array([[0.5, 2.0, 9.0]], F))                  # a third column is not read
    assert o.pos[0, 0] == F(F(0.25) + F(F(0.5) * F(0.1)))
    assert o.pos[0, 1] == F(1)                                               # 0.95 + clamp(2) * 0.1 = 1.05 -> the wall
    assert first[0] == 0 and d[0] == 1 and o.t[0] == 1 and r[0] == 0         # d2 > 1: the reward is clipped at 0
    before = o.pos.copy()
    o.step(np.array([[np.nan, -7.0]], F))
    assert o.pos[0, 0] == before[0, 0] and o.pos[0, 1] == F(F(1) + F(F(-1) * F(0.1)))
    o = env_at([-0.95, 0.0], [0.8, 0.8])
    o.step(np.array([[-1.0, 0.0]], F))
    assert o.pos[0, 0] == F(-1)
    # the reward, by hand: pos (0.5, 0), target (0, 0) after a zero action -> 1 - 0.25
    o = env_at([0.5, 0.0], [0.0, 0.0])
    assert o.step(np.zeros((1, 2), F))[1][0] == F(0.75)


def test_reached_target_ends_with_discount_0_and_the_next_step_is_a_reset_row():
    o = env_at([[0.15, 0.0], [0.5, 0.5]], [[0.0, 0.0], [-0.5, -0.5]], N=2)
    frame, r, d, first = o.step(np.array([[-1.0, 0.0], [0.0, 0.0]], F))      # e 0: 0.15 - 0.1: d2 = 0.0025 <= 0.01
    assert d.tolist() == [0.0, 1.0] and o.over.tolist() == [1, 0] and first.tolist() == [0, 0]
    assert r[0] == F(F(1) - F(F(o.pos[0, 0] * o.pos[0, 0]) + F(0))) and o.reached == 1 and o.timed_out == 0
    ep = o.episode.copy()
    frame, r, d, first = o.step(np.full((2, 2), np.nan, F))                  # the action of a reset row is not read
    assert first.tolist() == [1, 0] and r[0] == 0 and d[0] == 1 and o.t.tolist() == [0, 2] and o.over.tolist() == [0, 0]
    assert o.episode.tolist() == [ep[0] + 1, ep[1]]
    assert o.pos[0].tolist() == [E.draw(1, 0, 2, 0), E.draw(1, 0, 2, 1)]
    assert o.target[0].tolist() == [E.draw(1, 0, 2, 2), E.draw(1, 0, 2, 3)]
    assert np.array_equal(frame[0], E.render(o.pos[0], o.target[0]))
    # exactly on the bound: d2 == float32(0.01) counts as reached, one ulp above does not
    for d2, reached in ((F(0.01), True), (np.nextafter(F(0.01), F(1)), False)):
        assert (d2 <= F(0.01)) == reached


def test_time_limit_ends_with_discount_1():
    o = env_at([0.9, 0.9], [-0.9, -0.9], L=3)
    for k in range(3):
        _, r, d, first = o.step(np.zeros((1, 2), F))
        assert d[0] == 1 and first[0] == 0 and o.over[0] == (k == 2) and o.t[0] == k + 1
    assert o.timed_out == 1 and o.reached == 0
    _, r, d, first = o.step(np.zeros((1, 2), F))
    assert first[0] == 1 and o.t[0] == 0 and o.episode[0] == 2 and d[0] == 1 and r[0] == 0


def test_replicated_image_and_its_area_average():
    """image(S, C) of the oracle: k x k copies of every pixel, channels last, alpha 255 -- and the resize rule of
    add_render() (tests/vec_render_oracle.py) gives the frame back exactly"""
    o = E.ReachOracle(3, seed=4)
    frames = o.reset()
    for S in (84, 168, 252, 336):
        for C in (3, 4):
            img = E.replicate(frames, S, C)
            k = S // 84
            assert img.shape == (3, S, S, C) and img.dtype == np.uint8
            assert np.array_equal(img[:, ::k, ::k, :3].transpose(0, 3, 1, 2), frames)
            assert np.array_equal(img[:, k - 1::k, k - 1::k, :3].transpose(0, 3, 1, 2), frames)
            assert C == 3 or (img[..., 3] == 255).all()
            assert np.array_equal(VR.resize(img), frames)


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_build_list_symbols_and_abi_version():
    header = abi.text()
    assert "device environment" in header
    for name, nargs in NAMES.items():
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs, name
    for text in ("fmix32(seed ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ k * 0xC2B2AE35)", "d2 <= 0.01f",
                 "(int)floorf((x + 1) * 41.5f + 0.5f)", "32 + ((i + j) >> 2)"):
        assert text in header, text                                        # the task is part of the contract
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()        # additive: the version stays
    from drqv2_amd import build
    assert "vecenv.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecenv.hip"))
    assert build.FILE_FLAGS["vecenv.hip"] == ["-ffp-contract=off"]         # single float32 operations, never fused
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    lib = _lib.load()
    assert lib.drq_abi_version() == 7
    for name in NAMES:
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name


def test_refusals_that_need_no_gpu():
    """argument errors are reported before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them"""
    lib = _lib.load()
    S0, ACT, FR, SC = 0x10000, 0x20000, 0x30000, 0x40000
    #     pos target      t           episode     over        N  A  action seed L reset frame reward discount   first
    ok = [S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, S0 + 0x400, 5, 2, ACT, 7, 9, 0, FR, SC, SC + 0x100, SC + 0x200]
    bad = []
    for k in (0, 1, 2, 3, 4, 7, 11, 12, 13, 14):                          # every pointer; action only without reset_all
        bad.append(ok[:k] + [None] + ok[k + 1:])
    for k, vals in ((5, (0, -1, 2 ** 31)), (6, (1, 0, -2)), (9, (0, -5)), (10, (2, -1))):      # N, A, episode_length, reset_all
        for v in vals:
            bad.append(ok[:k] + [v] + ok[k + 1:])
    for mis in (1, 4, 8):
        bad.append(ok[:11] + [FR + mis] + ok[12:])                         # frame not 16-byte aligned
    for k in (0, 1, 2, 3, 7, 12, 13):
        bad.append(ok[:k] + [ok[k] + 2] + ok[k + 1:])                      # a float / int array not 4-byte aligned
    for a in bad:
        assert lib.drq_vec_reach_step(*a, None) == -1, a
    assert len(bad) == 10 + 3 + 3 + 2 + 2 + 3 + 7
    oki = [FR, FR + 0x100000, 3, 168, 4]
    badi = [[None] + oki[1:], oki[:1] + [None] + oki[2:], [FR + 8] + oki[1:], oki[:1] + [oki[1] + 4] + oki[2:]]
    for k, vals in ((2, (0, -1, 2 ** 31)), (3, (0, 83, 85, 128, 420, -84)), (4, (0, 1, 2, 5))):   # N, S, C
        for v in vals:
            badi.append(oki[:k] + [v] + oki[k + 1:])
    for a in badi:
        assert lib.drq_vec_reach_image(*a, None) == -1, a
    assert len(badi) == 4 + 3 + 6 + 4


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_vec_reach_argument_errors_and_cpu_refusal():
    from drqv2_amd.envs import VecReach
    for kw in (dict(num_envs=0), dict(num_envs=3, action_dim=1), dict(num_envs=3, episode_length=0)):
        with pytest.raises(ValueError):
            VecReach(device="cpu", **kw)
    N, A = 3, 4
    env = VecReach(N, "cpu", action_dim=A, episode_length=5, seed=2 ** 32 + 3)
    assert env.seed == 3 and env.N == N and env.A == A
    bad = {"numpy": np.zeros((N, A), np.float32), "list": [[0.0] * A] * N, "rows": torch.zeros(N + 1, A),
           "columns": torch.zeros(N, 2), "rank": torch.zeros(N), "rank3": torch.zeros(N, A, 1),
           "float64": torch.zeros(N, A, dtype=torch.float64), "int": torch.zeros(N, A, dtype=torch.int32)}
    for name, a in bad.items():
        with pytest.raises(ValueError, match=r"step\(\): action"):
            env.step(a)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="is on"):
            env.step(torch.zeros(N, A, device="cuda"))
    for size, channels in ((128, 3), (83, 3), (420, 4), (84, 2), (84, 5)):
        with pytest.raises(ValueError, match=r"image\(\): size"):
            env.image(size, channels)
    # well-formed calls on a CPU environment: refused like the stores, after the argument checks
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        env.reset()
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        env.step(torch.zeros(N, A))
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        env.image(168, 4)
    s = env.state()                                                        # nothing ran: the initial state
    assert s["episode"].dtype == np.uint32 and not s["episode"].any() and s["pos"].shape == (N, 2)
    assert s["t"].dtype == np.int32 and s["over"].dtype == np.uint8
