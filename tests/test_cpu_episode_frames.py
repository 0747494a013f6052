"""Single frames in the episode store (DeviceReplay(single_frames=True), drq_nstep_gather_frames): everything that needs no
GPU.  The slot rule of tests/episode_frames_oracle.py against the frame-stack simulator on layouts that wrap and evict,
the public surface, the frame-stack check and the constructor's validation, and the argument errors the library reports
before any launch."""
import inspect
import os

import numpy as np
import pytest

from drqv2_amd import _lib
from tests import abi
from tests import episode_frames_oracle as EF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "drq_nstep_gather_frames"
NSTEP = 3
SMALL = (3, 2, 2)


def single_store(**kw):
    from drqv2_amd.replay import DeviceReplay
    return DeviceReplay(40, (9, 84, 84), 2, NSTEP, 0.99, "cpu", seed=0, single_frames=True, **kw)


# ------------------------------------------------------------------------------------------------ the surface
def test_header_prototype_export_and_abi_version():
    abi.assert_prototype(NAME)
    assert len(_lib.PROTOTYPES[NAME][1]) == 18
    assert "single frames in the episode store" in abi.text()
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()        # additive: the version stays
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "vecframes.hip")) as f:
        src = f.read()
    assert NAME in src and "ring_stack_slots(a.first, a.R, 1," in src     # the rule is used, not restated
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert hasattr(lib, NAME) and lib.drq_abi_version() == 7


def test_loader_and_store_signatures():
    import replay_buffer
    from drqv2_amd.replay import DeviceReplay
    for fn in (replay_buffer.make_replay_loader, DeviceReplay.__init__):
        prm = inspect.signature(fn).parameters
        assert prm["single_frames"].default is False and prm["check_stacks"].default is True
    # the reference's positional signature is where it was
    assert list(inspect.signature(replay_buffer.make_replay_loader).parameters)[:7] == [
        "replay_dir", "max_size", "batch_size", "num_workers", "save_snapshot", "nstep", "discount"]


# ------------------------------------------------------------------------------------------------ the slot rule
def check_layout(lay):
    """at every slot of every live episode the oracle's stack from single frames + flags is the simulator's observation,
    and no slot outside the episode was named"""
    n = 0
    for s, m in lay.episodes:
        for q in range(s, s + m):
            slots = EF.stack_slots(lay.first, q)
            assert all(s <= x <= q for x in slots), (s, m, q, slots)
            assert np.array_equal(EF.stack_at(lay.frames, lay.first, q), lay.stacked[q]), (s, m, q)
            n += 1
    return n


@pytest.mark.parametrize("garbage", [None, 7])
def test_rule_equals_the_simulator_on_every_live_slot(garbage):
    """episode lengths 1, 2, 3 and nstep + 2 among others; an episode at slot 0; one that ends on the last slot; a wrap
    to slot 0 that evicts; the stale frames and flags of the evicted range left in place (garbage = 7: slots never
    written hold random flags as well)"""
    r = np.random.RandomState(1)
    R = 23
    lay = EF.Layout(R, 2, SMALL, seed=garbage)
    for n in (1, 2, 3, NSTEP + 2, 5, 7):                                   # 1 + 2 + 3 + 5 + 5 + 7 = 23: ends on slot R - 1
        lay.add(EF.episode(r, n, 2, SMALL))
        check_layout(lay)
    assert lay.episodes[0] == [0, 1] and lay.episodes[-1] == [16, 7] and lay.head == R
    assert sorted(lay.live_slots()) == list(range(R))
    start, evicted = lay.add(EF.episode(r, 4, 2, SMALL))                   # wraps, evicts the episodes on slots 0 .. 5
    assert start == 0 and evicted == [[0, 1], [1, 2], [3, 3]] and lay.first[0] == 1
    stale = [q for q in range(R) if q not in lay.live_slots()]
    assert stale == [4, 5] and lay.first[3] == 0                           # slot 3's old flag was overwritten, 4 and 5 kept
    assert check_layout(lay) == R - 2
    lay.first[stale] = 1                                                   # whatever the stale flags hold
    check_layout(lay)
    lay.first[stale] = 0
    check_layout(lay)
    for n in (3, 6, 2, 9, 1, 8, 23, 5, 5, 5, 5, 4):                        # more wraps, a whole-store episode, a tail left over
        lay.add(EF.episode(r, n, 2, SMALL))
        check_layout(lay)
    # all three branches of the rule at the start of an episode
    s, m = lay.episodes[-1]
    assert m >= 4
    assert EF.stack_slots(lay.first, s) == (s, s, s) and EF.stack_slots(lay.first, s + 1) == (s, s, s + 1)
    assert EF.stack_slots(lay.first, s + 2) == (s, s + 1, s + 2) and EF.stack_slots(lay.first, s + 3) == (s + 1, s + 2, s + 3)


def test_simulator_by_hand():
    ep = EF.episode(np.random.RandomState(0), 4, 2, SMALL)
    f, o = ep["frames"], ep["observation"]
    assert o.shape == (4, 9, 2, 2) and o.dtype == np.uint8
    assert np.array_equal(o[0], np.concatenate([f[0], f[0], f[0]])) and np.array_equal(o[1], np.concatenate([f[0], f[0], f[1]]))
    assert np.array_equal(o[2], np.concatenate([f[0], f[1], f[2]])) and np.array_equal(o[3], np.concatenate([f[1], f[2], f[3]]))


# ------------------------------------------------------------------------------------------------ the host logic
def test_frame_stack_check():
    from drqv2_amd.replay import newest_frames
    r = np.random.RandomState(2)
    ep = EF.episode(r, 6, 2)
    obs = ep["observation"]
    assert np.array_equal(newest_frames(obs), ep["frames"]) and newest_frames(obs).flags.c_contiguous
    assert newest_frames(ep["frames"]) is ep["frames"] or np.array_equal(newest_frames(ep["frames"]), ep["frames"])
    for t, c in ((0, 0), (0, 4), (1, 0), (3, 5), (5, 2)):                  # one altered byte among channels 0:6
        bad = obs.copy()
        bad[t, c, 17, 40] ^= 1
        with pytest.raises(ValueError, match="no (reset|frame) stack"):
            newest_frames(bad)
        assert np.array_equal(newest_frames(bad, check=False), ep["frames"])       # the caller said it knows the source
    for wrong in (obs.astype(np.int16), obs[:, :6], obs[:, :, :80], obs[0], obs.reshape(6, -1), ep["frames"].astype(np.float32)):
        with pytest.raises(ValueError, match="observation must be uint8"):
            newest_frames(wrong)


def test_store_validation_and_rejection_leaves_the_store_as_it_was():
    from drqv2_amd.replay import DeviceReplay
    for shape in ((9, 64, 64), (3, 84, 84), (12, 84, 84)):
        with pytest.raises(ValueError, match="single-frame store"):
            DeviceReplay(40, shape, 2, NSTEP, 0.99, "cpu", single_frames=True)
    st = single_store()
    assert st.frames.shape == (40, 21168) and st.frames.dtype.is_floating_point is False and st.frame_bytes == 21168
    assert st.stack_bytes == 63504 and st.obs_shape == (9, 84, 84) and st.single_frames and st.check_stacks
    assert st.first.shape == (40,) and st.first.tolist() == [0] * 40
    plain = DeviceReplay(40, (9, 84, 84), 2, NSTEP, 0.99, "cpu", seed=0)
    assert plain.frames.shape == (40, 63504) and plain.first is None and not plain.single_frames
    r = np.random.RandomState(3)
    eps = [EF.episode(r, n, 2) for n in (7, 5)]
    assert st.add_episode(EF.npz_fields(eps[0])) == 0                      # stacked input
    single = dict(EF.npz_fields(eps[1]), observation=eps[1]["frames"])
    assert st.add_episode(single) == 7                                     # single-frame input
    assert np.array_equal(st.frames[:7].numpy(), eps[0]["frames"].reshape(7, -1))
    assert np.array_equal(st.frames[7:12].numpy(), eps[1]["frames"].reshape(5, -1))
    assert st.first.tolist() == [1] + [0] * 6 + [1] + [0] * 4 + [0] * 28
    for e in eps:                                                          # the twin draws the same positions
        plain.add_episode(EF.npz_fields(e))
    assert plain.episodes == st.episodes and np.array_equal(plain.draw_positions(64), st.draw_positions(64))
    before = (len(st), [list(e) for e in st.episodes], st._head, st._placements, st.first.clone(), st.frames[:12].clone())
    bad = EF.npz_fields(EF.episode(r, 35, 2))                              # would wrap to slot 0 and evict both
    bad["observation"][9, 3, 0, 0] ^= 0x80
    with pytest.raises(ValueError, match=r"observation\[9\] is no frame stack"):
        st.add_episode(bad)
    for shape in ((35, 6, 84, 84), (35, 9, 84, 80), (35, 63504)):
        with pytest.raises(ValueError, match="observation must be uint8"):
            st.add_episode(dict(bad, observation=np.zeros(shape, np.uint8)))
    with pytest.raises(ValueError, match="observation must be uint8"):
        st.add_episode(dict(bad, observation=np.zeros((35, 9, 84, 84), np.float32)))
    after = (len(st), st.episodes, st._head, st._placements, st.first, st.frames[:12])
    assert before[:4] == after[:4] and bool((before[4] == after[4]).all()) and bool((before[5] == after[5]).all())
    loose = single_store(check_stacks=False)
    assert loose.add_episode(bad) == 0 and len(loose) == 34
    with pytest.raises(_lib.DrqError):                                     # no CPU fallback for the batch assembly
        st.sample(4)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")
def test_argument_errors_before_any_launch():
    lib = _lib.load()
    x = 4096                                              # never dereferenced: every call below is refused on the host
    ok = [x, x, 23, x, x, x, x, 4, 2, 48, 3, 0.99, x, x, x, x, x]
    for k in (0, 1, 3, 4, 5, 6, 12, 13, 14, 15, 16):      # every pointer; obs or next_obs alone
        assert getattr(lib, NAME)(*(ok[:k] + [None] + ok[k + 1:]), None) == -1, k
    for k, v in ((2, 0), (2, -3), (7, 0), (7, -1), (8, 0), (8, -2), (9, 0), (9, 24), (9, -16), (10, 0), (10, -1)):
        assert getattr(lib, NAME)(*(ok[:k] + [v] + ok[k + 1:]), None) == -1, (k, v)
    for k, off in ((0, 8), (12, 4), (16, 8), (6, 4), (3, 2), (13, 1)):
        assert getattr(lib, NAME)(*(ok[:k] + [x + off] + ok[k + 1:]), None) == -1, (k, off)
