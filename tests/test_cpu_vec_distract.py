"""Distractions (drq_vec_distract, drqv2_amd.distract): everything that needs no GPU.  The public surface and every
DRQ_EARG case (all are decided before any launch), the constructor's and apply()'s ValueErrors, the presets, state dicts
on CPU objects, the properties of the numpy restatement tests/vec_distract_oracle.py -- the identity settings, the ranges
of what it draws -- and what the inputs of the GPU tests (tests/test_hip_vec_distract.py) cover, which is a property of
the oracle's runs alone."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_distract_oracle as O

ENTRY = "drq_vec_distract"


def distract():
    from drqv2_amd import distract as D
    return D


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build():
    header = abi.text()
    abi.assert_prototype(ENTRY)
    assert len(_lib.PROTOTYPES[ENTRY][1]) == 20 and ENTRY not in _lib.NO_STREAM and ENTRY in abi.stream_entries()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY)
    for text in ("---- distractions.", "draw(k) = fmix32(seed ^ e * 0x9E3779B9 ^ episode * 0x85EBCA6B ^ (256 + k) * 0xC2B2AE35)",
                 "tri(v, m) for v >= 0", "ox = tri(draw(0) % (2P + 1) + (draw(2) % 3) * (tau / camera_period), 2P) - P",
                 "f_c = clamp(((s_c * gain_c + 128) >> 8) + off_c, 0, 255)", "n_c = (top * (12 - fy) + bot * fy + 72) / 144",
                 "f = tri(draw(11) % F + tau, F - 1)", "b_c = (a * n_c + (256 - a) * s_c + 128) >> 8",
                 "Identity: camera = 0, color = 0, bg_mode = 0 writes frame_in back bit for bit", "hold = 1 draws the frame of the state AS IT IS"):
        assert text in header, text                                        # the rule is part of the contract
    assert (abi.define("DRQ_DISTRACT_MAX_CAMERA"), abi.define("DRQ_DISTRACT_MAX_COLOR"), abi.define("DRQ_DISTRACT_MAX_BANK")) \
        == (O.MAX_CAMERA, O.MAX_COLOR, O.MAX_BANK) == (distract().MAX_CAMERA, distract().MAX_COLOR, distract().MAX_BANK)
    from drqv2_amd import build
    assert "vecdistract.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecdistract.hip"))
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    with open(os.path.join(build.CSRC, "vecdistract.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("atomic", "asm", "float", "printf"):                    # integers alone, plain HIP C++
        assert banned not in src, banned
    assert "__shared__" in src and "uint4" in src and "DRQ_LAUNCH_CHECK" in src


def test_every_refusal_needs_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_vec_distract.py repeats them on poisoned memory.)"""
    lib = _lib.load()
    calls = O.refused_calls(0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000)
    assert len(calls) == 42 and len({why for why, _ in calls}) == 42
    for why, a in calls:
        assert lib.drq_vec_distract(*a, None) == -1, why


# ------------------------------------------------------------------------------------------------ the classes, no GPU
def test_constructor_value_errors_say_why():
    D = distract()
    make = lambda **kw: D.FrameDistractor(**dict(dict(num_envs=3, device="cpu"), **kw))
    key = torch.zeros(3, 84, 84, dtype=torch.uint8)
    bank = torch.zeros(2, 3, 3, 84, 84, dtype=torch.uint8)
    with pytest.raises(ValueError, match="num_envs"):
        make(num_envs=0)
    for name, bads in (("camera", (-1, 9, True, 2.0)), ("camera_period", (0, -1, 1.5)), ("color", (-1, 129, "4")),
                       ("background_alpha", (-1, 257, None))):
        for bad in bads:
            with pytest.raises(ValueError, match=rf"\b{name} must be an int in"):
                make(**{name: bad})
    for bad in (2, "yes", None):
        with pytest.raises(ValueError, match="dynamic"):
            make(dynamic=bad)
    for bad in ("clouds", None, 3):
        with pytest.raises(ValueError, match="background must be"):
            make(background=bad, key=key)
    with pytest.raises(ValueError, match=r"a bank is \[M, F, 3, 84, 84\]"):                 # the wrong rank
        make(background=bank[0], key=key)
    with pytest.raises(ValueError, match=r"a bank is \[M, F, 3, 84, 84\]"):
        make(background=torch.zeros(2, 3, 3, 64, 64, dtype=torch.uint8), key=key)
    with pytest.raises(ValueError, match=r"a bank is \[M, F, 3, 84, 84\]"):
        make(background=bank[:0], key=key)
    with pytest.raises(ValueError, match="bank must be torch.uint8"):
        make(background=bank.float(), key=key)
    with pytest.raises(ValueError, match="the bank must be contiguous"):
        make(background=bank[:, ::2], key=key)
    with pytest.raises(ValueError, match="the bank is on meta, the distractor on cpu"):     # the wrong device
        make(background=bank.to("meta"), key=key)
    for background in ("noise", bank):
        with pytest.raises(ValueError, match="without a key"):
            make(background=background)
    for bad in ("frame", torch.zeros(3, 84, 84), torch.zeros(84, 84, dtype=torch.uint8), 7):
        with pytest.raises(ValueError, match="key must be None"):
            make(key=bad)
    with pytest.raises(ValueError, match="key is on meta"):
        make(key=key.to("meta"))
    d = make(camera=8, color=128, background=bank, background_alpha=0, key=key, dynamic=False, seed=-1)
    assert (d.camera, d.color, d.background, d.background_alpha, d.dynamic, d.seed) == (8, 128, "bank", 0, False, 0xFFFFFFFF)
    assert make(key=None).key is None and make(background="noise", key="env").key_from_env


def test_apply_checks_its_arguments_then_refuses_the_cpu():
    D = distract()
    d = D.FrameDistractor(3, "cpu", camera=2)
    frame = torch.zeros(3, 3, 84, 84, dtype=torch.uint8)
    for bad, why in ((frame.numpy(), "must be a tensor"), (frame[:2], "shape"), (frame.float(), "must be torch.uint8"),
                     (frame.to("meta"), "is on meta")):
        with pytest.raises(ValueError, match=rf"apply\(\): frame.*{why}"):
            d.apply(bad)
    for bad, why in ((torch.zeros(2, dtype=torch.uint8), "shape"), (torch.zeros(3), "must be torch.uint8 or torch.bool"),
                     ([0, 0, 1], "must be a tensor")):
        with pytest.raises(ValueError, match=rf"apply\(\): first.*{why}"):
            d.apply(frame, bad)
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):            # after the checks
        d.apply(frame, torch.zeros(3, dtype=torch.bool))
    with pytest.raises(_lib.DrqError, match=r"render\(\): call apply"):
        d.render(frame)
    with pytest.raises(ValueError, match='key="env"'):                     # never bound to an environment
        D.FrameDistractor(3, "cpu", background="noise", key="env").apply(frame)


def test_presets_are_three_fixed_triples_within_range():
    D = distract()
    assert list(D.PRESETS) == ["easy", "medium", "hard"]
    last = (0, 0, 0)
    for name in D.PRESETS:
        kw = D.FrameDistractor.difficulty(name)
        assert set(kw) == {"camera", "color", "background", "background_alpha"} and kw["background"] == "noise"
        triple = (kw["camera"], kw["color"], kw["background_alpha"])
        assert triple == D.PRESETS[name] and all(a < b for a, b in zip(last, triple))       # each stronger than the one before
        assert 0 < kw["camera"] <= O.MAX_CAMERA and 0 < kw["color"] <= O.MAX_COLOR and 0 < kw["background_alpha"] <= 256
        d = D.FrameDistractor(2, "cpu", key="env", **kw)                   # the constructor takes them
        assert (d.camera, d.color, d.background_alpha) == triple
        assert D.parse_spec(name) == kw
        last = triple
    with pytest.raises(ValueError, match="difficulty 'extreme': one of easy, medium, hard"):
        D.FrameDistractor.difficulty("extreme")
    with open(os.path.join(os.path.dirname(abi.HEADER), "..", "INTEGRATION.md")) as f:
        text = f.read()
    for name, (camera, color, alpha) in D.PRESETS.items():                 # written down where a user looks
        assert f"| `{name}` | {camera} | {color} | {alpha} |" in text, name


def test_parse_spec():
    D = distract()
    assert D.parse_spec("camera=4,color=32,background=noise") == {"camera": 4, "color": 32, "background": "noise"}
    assert D.parse_spec(" camera_period=2, alpha=77 ,dynamic=0") == {"camera_period": 2, "background_alpha": 77, "dynamic": False}
    for bad in ("", "camera", "camera=4,camera=5", "zoom=2", "camera=x", "background=clouds", "dynamic=2", "Hard"):
        with pytest.raises(ValueError, match="distractions"):
            D.parse_spec(bad)


def test_state_dicts_round_trip_and_a_mismatch_is_named_and_changes_nothing(tmp_path):
    D = distract()
    from drqv2_amd import checkpoint
    from drqv2_amd.envs import VecCartpole, VecReach
    key = torch.from_numpy(O.ramp())
    bank = torch.zeros(2, 3, 3, 84, 84, dtype=torch.uint8)
    kw = dict(seed=5, camera=3, camera_period=2, color=9, background=bank, background_alpha=200, key=key, dynamic=False)
    d = D.FrameDistractor(3, "cpu", **kw)
    d.episode.copy_(torch.tensor([1, -2, 3], dtype=torch.int32))           # -2: the uint32 4294967294
    d.t.copy_(torch.tensor([7, 0, 9], dtype=torch.int32))
    d._started = True
    sd = d.state_dict()
    assert sd["format"] == 1 and sd["kind"] == "FrameDistractor" and sd["started"] is True
    assert sd["config"] == {"N": 3, "seed": 5, "camera": 3, "camera_period": 2, "color": 9, "background": "bank", "bank_clips": 2,
                            "bank_frames": 3, "background_alpha": 200, "keyed": True, "dynamic": False}
    assert set(sd) == {"format", "kind", "config", "started", "episode", "t"}              # neither the bank nor the key
    assert d.state()["episode"].tolist() == [1, 4294967294, 3]
    fresh = D.FrameDistractor(3, "cpu", **kw)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.episode, d.episode) and torch.equal(fresh.t, d.t) and fresh._started
    assert fresh.episode.data_ptr() != sd["episode"].data_ptr()
    # a mismatch names every field that differs and changes nothing
    other = D.FrameDistractor(3, "cpu", **dict(kw, camera=4, background="noise", seed=6))
    other.t.fill_(5)
    with pytest.raises(ValueError, match=r"seed: saved 5, here 6; camera: saved 3, here 4.*background: saved 'bank', here 'noise'; "
                                         r"bank_clips: saved 2, here 0; bank_frames: saved 3, here 0"):
        other.load_state_dict(sd)
    assert other.t.tolist() == [5, 5, 5] and not other._started
    with pytest.raises(ValueError, match="keyed: saved True, here False"):
        D.FrameDistractor(3, "cpu", **dict(kw, background="none", key=None)).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"N: saved 3, here 4.*episode: saved torch.int32 \(3,\), here torch.int32 \(4,\)"):
        D.FrameDistractor(4, "cpu", **kw).load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        fresh.load_state_dict(dict(sd, kind="SimHashBonus"))
    with pytest.raises(ValueError, match="t: no tensor saved"):
        fresh.load_state_dict({k: v for k, v in sd.items() if k != "t"})

    # the wrapper: the same attributes, nested dicts, and a checkpoint file takes it as env= with no special case
    env = VecReach(3, "cpu", action_dim=4, episode_length=9, seed=2, action_repeat=2)
    w = D.VecDistract(env, d)
    assert (w.N, w.A, w.device, w.episode_length, w.action_repeat, w.last_substeps) == (3, 4, torch.device("cpu"), 9, 2, None)
    for method in ("reset", "step", "render", "image", "state", "state_dict", "load_state_dict"):
        assert callable(getattr(w, method)), method
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        w.reset()
    with pytest.raises(ValueError, match=r"image\(\): size"):
        w.image(100)
    wsd = w.state_dict()
    assert wsd["kind"] == "VecDistract" and wsd["env"]["kind"] == "VecReach" and wsd["distractor"]["config"] == sd["config"]
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=w, extra={"step": 3})
    ck = torch.load(path, weights_only=True)
    assert ck["env"]["kind"] == "VecDistract" and torch.equal(ck["env"]["distractor"]["t"], d.t)
    assert ck["env"]["env"]["config"]["task"] == "reach"
    # a mismatch in either part changes neither: the distractor's part is checked before the environment restores itself
    w2 = D.VecDistract(VecReach(3, "cpu", action_dim=4, episode_length=9, seed=2, action_repeat=2),
                       D.FrameDistractor(3, "cpu", **dict(kw, color=10)))
    w2.env.t.fill_(4)
    with pytest.raises(ValueError, match="FrameDistractor.*color: saved 9, here 10"):
        w2.load_state_dict(wsd)
    assert w2.env.t.tolist() == [4, 4, 4]
    w3 = D.VecDistract(VecReach(3, "cpu", action_dim=4, episode_length=8, seed=2, action_repeat=2), D.FrameDistractor(3, "cpu", **kw))
    with pytest.raises(ValueError, match="VecReach.*episode_length: saved 9, here 8"):
        w3.load_state_dict(wsd)
    assert w3.distractor.t.tolist() == [0, 0, 0] and not w3.distractor._started
    with pytest.raises(ValueError, match="kind"):
        w3.load_state_dict(sd)
    # what the wrapper refuses to wrap
    with pytest.raises(ValueError, match="steps 2 environments, the distractor 3"):
        D.VecDistract(VecReach(2, "cpu"), d)
    with pytest.raises(ValueError, match="must be a FrameDistractor"):
        D.VecDistract(env, env)
    # key="env": the wrapper asks the environment
    w4 = D.VecDistract(VecCartpole(2, "cpu"), D.FrameDistractor(2, "cpu", background="noise", key="env"))
    assert torch.equal(w4.distractor.key, torch.from_numpy(O.ramp()))


def test_background_key_is_the_ramp_of_every_built_in_task():
    from drqv2_amd.envs import VecCartpole, VecPointMass, VecReach
    for cls in (VecReach, VecPointMass, VecCartpole):
        key = cls(2, "cpu").background_key()
        assert key.dtype == torch.uint8 and tuple(key.shape) == (3, 84, 84) and key.is_contiguous()
        assert key.numpy().tobytes() == O.ramp().tobytes()
    i, j = 5, 77
    assert int(O.ramp()[1, i, j]) == 32 + ((i + j) >> 2) and O.ramp().max() == 32 + (166 >> 2)


# ------------------------------------------------------------------------------------------------ the oracle's properties
def test_require_branches_fails_before_anything_is_drawn_and_names_what_is_missing():
    o = O.DistractOracle(1, key=O.ramp(), bg_mode=1)
    with pytest.raises(AssertionError, match="never took: tri_rising, tri_falling, clamp_left"):
        o.require_branches()
    o.apply(O.ramp()[None], reset_all=True)
    o.require_branches("background", "reset_row")
    with pytest.raises(AssertionError, match="never took: foreground, step_row$"):
        o.require_branches("background", "foreground", "reset_row", "step_row")


def test_identity_settings_return_the_frame_bit_for_bit():
    """camera = 0, color = 0, bg_mode = 0 writes the frame back, with or without a key and for any alpha; so does alpha 0
    over noise and over a bank; the state words still step"""
    r = np.random.RandomState(0)
    key = r.randint(0, 256, O.FRAME).astype(np.uint8)
    bank = r.randint(0, 256, (2, 3) + O.FRAME).astype(np.uint8)
    for kw in (dict(), dict(key=key), dict(key=key, bg_alpha=77), dict(key=key, bg_mode=1, bg_alpha=0),
               dict(key=key, bank=bank, bg_mode=2, bg_alpha=0, dynamic=False)):
        o = O.DistractOracle(2, seed=3, **kw)
        for s in range(6):
            frame = np.stack([O.scene(r, key) for _ in range(2)])
            out = o.apply(frame, np.array([0, s == 4], np.uint8), reset_all=s == 0)
            assert out.dtype == np.uint8 and out.tobytes() == frame.tobytes(), (kw, s)
        assert o.episode.tolist() == [1, 2] and o.t.tolist() == [5, 1]
        if "key" in kw:
            o.require_branches("background", "foreground")
    # and each strength alone does change the frame
    for kw in (dict(camera=8), dict(color=128), dict(key=key, bg_mode=1), dict(key=key, bank=bank, bg_mode=2)):
        o = O.DistractOracle(1, seed=3, **kw)
        frame = O.scene(r, key)[None]
        assert o.apply(frame, reset_all=True).tobytes() != frame.tobytes(), kw


def test_hold_draws_the_frame_of_the_state_again_and_static_distractions_stay_put():
    r = np.random.RandomState(1)
    key = r.randint(0, 256, O.FRAME).astype(np.uint8)
    frame = np.stack([O.scene(r, key) for _ in range(2)])
    o = O.DistractOracle(2, seed=9, camera=8, camera_period=1, color=60, bg_mode=1, key=key)
    o.apply(frame, reset_all=True)
    out = o.apply(frame)
    state = (o.episode.copy(), o.t.copy())
    assert o.frames(frame).tobytes() == out.tobytes() and (o.episode == state[0]).all() and (o.t == state[1]).all()
    assert o.apply(frame).tobytes() != out.tobytes()                       # dynamic: the next step moves
    static = O.DistractOracle(2, seed=9, camera=8, camera_period=1, color=60, bg_mode=1, key=key, dynamic=False)
    first = static.apply(frame, reset_all=True)
    for _ in range(5):
        assert static.apply(frame).tobytes() == first.tobytes()           # within an episode nothing moves
    assert static.apply(frame, np.array([1, 0], np.uint8))[0].tobytes() != first[0].tobytes()       # a new episode draws anew


def test_the_draws_of_the_distractions_are_not_the_environments_own():
    """draw(k) hashes (256 + k): under one seed, environment and episode none of the thirteen equals one of the first 256
    draws an environment may make for itself"""
    base = 7 ^ (2 * O.K1 & O.MASK) ^ (5 * O.K2 & O.MASK)
    own = {O.fmix32(base ^ (k * O.K3 & O.MASK)) for k in range(256)}
    ours = {O.fmix32(base ^ ((256 + k) * O.K3 & O.MASK)) for k in range(13)}
    assert len(ours) == 13 and not own & ours


# ------------------------------------------------------------------------------------------------ the shared runs
def test_inputs_of_the_gpu_tests_cover_every_branch():
    """The runs tests/test_hip_vec_distract.py compares on the GPU, on the oracle alone: together they take every branch
    the oracle records; every lane sees at least two episodes and the resets stagger; the scenes hold 0 and 255; the
    identity scenarios return their input"""
    fresh = O.DistractOracle(1)
    with pytest.raises(AssertionError, match="never took"):                # before anything is drawn it can fail
        fresh.require_branches()
    total = O.DistractOracle(1)
    for name in O.SCENARIOS:
        run = O.run_of(name)
        for k, v in run["oracle"].seen.items():
            total.seen[k] += v
        assert (run["states"][-1][0] >= 3).all(), name                     # three episodes per lane
        firsts = np.stack(run["firsts"][1:])
        assert firsts.any(0).all() and (run["N"] == 1 or not (firsts.all(1) | ~firsts.any(1)).all()), name
        assert all(f.min() == 0 and f.max() == 255 for f in run["frames"])
        same = all(a.tobytes() == b.tobytes() for a, b in zip(run["frames"], run["outs"]))
        assert same == (name in O.IDENTITY), name
    total.require_branches()
    assert {O.SCENARIOS[n][0] for n in O.SCENARIOS} == {1, 3}
    assert {O.SCENARIOS[n][1].get("bg_alpha", 256) for n in O.SCENARIOS} >= {0, 77, 256}
    # the scenario the issue names for each: both fold directions and all four clamps at camera 8 / period 1, both colour
    # clamps at colour 128, X and Y below zero under noise, the reversal of a bank of 3 frames
    O.run_of("camera8-colour128-unkeyed")["oracle"].require_branches(
        "tri_rising", "tri_falling", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "colour_clamp_0", "colour_clamp_255")
    O.run_of("noise-alpha77")["oracle"].require_branches("negative_X", "negative_Y", "background", "foreground")
    O.run_of("bank")["oracle"].require_branches("bank_reversal", "tri_rising", "tri_falling")
