"""Evaluation for the vectorised loop without a GPU: the prototypes of the two entries against the header, the stack
oracle against the FrameStackWrapper and the ring's observation() oracle, the animated PNG writer and reader, and every
argument error of drqv2_amd.evaluate.  All comparisons are exact (integers)."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import abi
from tests import vec_eval_oracle as EO
from tests import vec_frames_oracle as FO

NAMES = ("drq_vec_stack_push", "drq_vec_video_record")


def test_the_new_entries_are_declared_and_prototyped():
    from drqv2_amd import _lib, build, ops
    assert "veceval.hip" in build.SOURCES
    for name in NAMES:
        abi.assert_prototype(name)
    assert callable(ops.vec_stack_push) and callable(ops.vec_video_record)
    lib = _lib.load()
    # argument errors are reported before anything is launched: no GPU needed
    assert lib.drq_vec_stack_push(None, None, None, None, 1, 1, None) == -1
    assert lib.drq_vec_stack_push(None, 4096, 8192, None, 0, 1, None) == -1                    # N = 0
    assert lib.drq_vec_stack_push(None, 4096, 1 << 20, None, 1, 0, None) == -1                 # no prev, no reset_all
    assert lib.drq_vec_stack_push(1 << 20, (1 << 20) + 16, 1 << 30, None, 1, 0, None) == -1    # prev overlaps next
    for k in (0, 5):
        assert lib.drq_vec_video_record(4096, 4096, 1, None, 0, 1 << 20, 1, 1, k, 1, None) == -1
    assert lib.drq_vec_video_record(4096, 4096, 5, None, 0, 1 << 20, 2, 2, 1, 8, None) == -1    # M > GH GW
    assert lib.drq_vec_video_record(4096, 4096, 0, None, 0, 1 << 20, 2, 2, 1, 8, None) == -1    # M < 1
    assert lib.drq_vec_video_record(None, 4096, 1, None, 0, 1 << 20, 1, 1, 1, 1, None) == -1


def test_stack_oracle_is_the_frame_stack_wrapper_and_the_rings_observation():
    """a random 10-row sequence of N = 3 with resets on consecutive rows: stack_push == one FrameStack per environment ==
    FrameStream.stacks, the observation() oracle of the single-frame ring"""
    N, rows = 3, 10
    r = np.random.RandomState(4)
    firsts = np.zeros((rows, N), np.uint8)
    firsts[3, 1] = firsts[4, 1] = 1                       # two resets in a row
    firsts[4, 0] = firsts[5, 2] = firsts[6, 2] = firsts[8] = 1
    stream, oracle = FO.FrameStream(16, N), EO.StackOracle(N)
    wrappers = [FO.FrameStack() for _ in range(N)]
    for t in range(rows):
        frame = r.randint(0, 256, (N, 3, 84, 84)).astype(np.uint8)
        first = np.zeros(N, np.uint8) if t == 0 else firsts[t]          # row 0 resets whatever the flags say
        want = stream.add(frame, first)
        got = oracle.push(frame, first)
        by_hand = np.stack([w.reset(frame[e]) if (t == 0 or first[e]) else w.step(frame[e]) for e, w in enumerate(wrappers)])
        assert got.dtype == np.uint8 and got.shape == (N, 9, 84, 84)
        assert np.array_equal(got, want) and np.array_equal(got, by_hand), t
    oracle.reset()
    assert np.array_equal(oracle.push(frame), np.concatenate([frame] * 3, axis=1))


def test_mosaic_oracle_on_a_case_worked_by_hand():
    frame = np.zeros((2, 3, 84, 84), np.uint8)
    frame[1, 0, 0, 1], frame[1, 2, 83, 83], frame[0, 1, 5, 7] = 200, 9, 77
    img = EO.mosaic(frame, [1, 0], (1, 3), 2, done=np.array([3, 0]), limit=2)
    assert img.shape == (168, 504, 3)
    assert (img[0:2, 2:4, 0] == 200).all() and img[0, 4, 0] == 0 and img[2, 2, 0] == 0
    assert (img[166:168, 166:168, 2] == 9).all()
    assert (img[10:12, 168 + 14:168 + 16, 1] == 77 >> 2).all()              # environment 0 is past its limit: dimmed
    assert not img[:, 336:].any()                                           # the third tile is empty


SHAPES = [(1, 5, 7), (3, 5, 7), (1, 168, 252), (3, 168, 252)]


@pytest.mark.parametrize("n,H,W", SHAPES)
def test_apng_round_trip_is_exact(tmp_path, n, H, W):
    from drqv2_amd import evaluate as E
    x = np.random.RandomState(n * H).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    path = str(tmp_path / "clip.png")
    size = E.write_apng(path, x, fps=25)
    assert os.path.getsize(path) == size and not os.path.exists(path + ".tmp")
    back, fps = E.read_apng(path)
    assert fps == 25 and back.dtype == np.uint8 and np.array_equal(back, x)

    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, at = [], 8
    while at < len(data):                                                   # every CRC, verified here and not by the module
        (length,) = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + length]
        assert struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0] == zlib.crc32(kind + payload) & 0xFFFFFFFF
        chunks.append((kind, payload))
        at += 12 + length
    assert at == len(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"acTL"] + [b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 8, 2, 0, 0, 0)
    assert struct.unpack(">II", chunks[1][1]) == (n, 0)
    seq = 0
    for kind, payload in chunks:                                            # the sequence numbers the format requires
        if kind == b"fcTL":
            assert struct.unpack(">IIIIIHHBB", payload) == (seq, W, H, 0, 0, 1, 25, 0, 0)
            seq += 1
        elif kind == b"fdAT":
            assert struct.unpack(">I", payload[:4])[0] == seq
            seq += 1
    # a plain PNG reader sees IHDR + IDAT: frame 0, every row with filter type 0
    raw = np.frombuffer(zlib.decompress(chunks[3][1]), np.uint8).reshape(H, 1 + 3 * W)
    assert not raw[:, 0].any() and np.array_equal(raw[:, 1:].reshape(H, W, 3), x[0])


def test_read_apng_rejects_what_it_did_not_write(tmp_path):
    from drqv2_amd import evaluate as E
    x = np.arange(2 * 4 * 4 * 3, dtype=np.uint8).reshape(2, 4, 4, 3)
    good = E.apng_bytes(x, fps=10)
    bad = bytearray(good)
    bad[40] ^= 1                                                            # inside acTL: its CRC no longer verifies
    for name, data in (("crc.png", bytes(bad)), ("cut.png", good[:-20]), ("sig.png", b"GIF89a" + good[6:])):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError):
            E.read_apng(path)
    for wrong in (x.astype(np.int32), x[0], x[:, :, :, :2], x[:0]):
        with pytest.raises(ValueError):
            E.apng_bytes(wrong)
    for fps in (0, 2.5, 70000):
        with pytest.raises(ValueError):
            E.apng_bytes(x, fps=fps)


def test_constructor_and_argument_errors():
    from drqv2_amd import evaluate as E
    from drqv2_amd._lib import DrqError
    from drqv2_amd.replay import VecEpisodeStats
    with pytest.raises(ValueError):
        E.VecFrameStack(0, "cpu")
    for kw in (dict(num_envs=0), dict(num_envs=4, scale=5), dict(num_envs=4, scale=0), dict(num_envs=4, max_frames=0),
               dict(num_envs=4, envs=[0, 0]), dict(num_envs=4, envs=[0, 4]), dict(num_envs=4, envs=[-1]),
               dict(num_envs=4, envs=[]), dict(num_envs=4, grid=(1, 3)), dict(num_envs=4, envs=[0, 1, 2], grid=(2, 1)),
               dict(num_envs=4, grid=(0, 4))):
        with pytest.raises(ValueError):
            E.VecVideo(device="cpu", **{"max_frames": 2, **kw})
    v = E.VecVideo(20, "cpu", max_frames=1)
    assert v.envs == tuple(range(16)) and v.grid == (4, 4) and v.scale == 2 and tuple(v.clip().shape) == (0, 672, 672, 3)
    assert E.VecVideo(5, "cpu", max_frames=1, scale=1).grid == (2, 3)        # GW = ceil(sqrt(5)), GH = ceil(5 / 3)
    assert E.VecVideo(4, "cpu", envs=[3, 1], grid=(1, 3), scale=1, max_frames=1).image_shape == (84, 252, 3)
    assert len(v) == 0 and v.dropped == 0
    with pytest.raises(DrqError):
        v.save("/nonexistent/clip.png")                                     # empty: nothing is written anywhere
    with pytest.raises(ValueError):
        v.save("clip.gif")

    # a CPU object: the argument checks come first, then DrqError
    s = E.VecFrameStack(3, "cpu")
    with pytest.raises(DrqError):
        s.observation()
    good = torch.zeros(3, 3, 84, 84, dtype=torch.uint8)
    for frame, first in ((torch.zeros(2, 3, 84, 84, dtype=torch.uint8), None), (good.float(), None), ([1, 2], None),
                         (good, torch.zeros(2, dtype=torch.uint8)), (good, torch.zeros(3))):
        with pytest.raises(ValueError):
            s.push(frame, first)
    with pytest.raises(DrqError):
        s.push(good, torch.zeros(3, dtype=torch.bool))
    v = E.VecVideo(3, "cpu", scale=1, max_frames=1)
    for frame, done, limit in ((good[:2], None, 0), (good, torch.zeros(3), 1), (good, None, -1)):
        with pytest.raises(ValueError):
            v.record(frame, done, limit)
    with pytest.raises(DrqError):
        v.record(good, torch.zeros(3, dtype=torch.int32), 1)

    # evaluate(): what is wrong with the arguments is said before the environment is touched
    class Env:
        def reset(self):
            raise AssertionError("the environment must not have been reset")

    with pytest.raises(ValueError):
        E.evaluate(None, Env(), episodes_per_env=2, stats=VecEpisodeStats(3, "cpu", max_episodes_per_env=1), max_steps=5)
    with pytest.raises(ValueError):
        E.evaluate(None, Env(), episodes_per_env=1)                         # no episode_length: max_steps is required
    with pytest.raises(ValueError):
        E.evaluate(None, Env(), episodes_per_env=0, max_steps=5)
