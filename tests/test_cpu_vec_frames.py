"""Single-frame step-major replay (VecFrameReplay, drq_vec_stack_gather, drq_conv1_aug_fwd_frames,
drq_update_phase_frames): everything that needs no GPU.  The public surface, the slot rule of tests/vec_frames_oracle.py
against its restatement of the reference's FrameStackWrapper on random flag streams, bounds() and the constructor's
validation, and the argument errors the library reports before any launch."""
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_frames_oracle as VF

NEW = ("drq_vec_stack_gather", "drq_conv1_aug_fwd_frames", "drq_conv1_aug_fwd_frames_bf16", "drq_update_phase_frames")


def test_header_prototypes_and_build_list():
    for name in NEW:
        abi.assert_prototype(name)
    from drqv2_amd import build
    assert "vecframes.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecframes.hip"))
    assert "single-frame step-major replay" in abi.text()


# ------------------------------------------------------------------------------------------------ the slot rule
@pytest.mark.parametrize("R,N,T,p_reset,seed", [(5, 1, 40, 0.3, 0), (7, 3, 60, 0.25, 1), (12, 3, 30, 0.15, 2),
                                                (4, 2, 50, 0.6, 3), (16, 3, 100, 0.0, 4)])
def test_slot_rule_equals_the_frame_stack_wrapper(R, N, T, p_reset, seed):
    """random flag streams, rings that wrap several times: after every add, for every row whose three slots are still in
    the ring, the frames at stack_slots() are the deque's observation.  The frame of (t, e) is its own name, 3 bytes"""
    r = np.random.RandomState(seed)
    fs = VF.FrameStream(R, N)
    cases = set()
    for t in range(T):
        frame = np.array([[[t % 256], [t // 256], [e]] for e in range(N)], np.uint8).reshape(N, 3, 1, 1)
        fs.add(frame, r.uniform(size=N) < p_reset)
        frames, first = fs.ring()
        for back in range(min(R - 2, t + 1)):            # rows t-back whose p1, p2 have not been overwritten
            tt = t - back
            for e in range(N):
                s = VF.stack_slots(first, R, N, (tt % R) * N + e)
                assert all(0 <= q < R * N for q in s)
                got = np.concatenate([frames[q] for q in s])
                assert np.array_equal(got, fs.stacks[tt][e].reshape(-1)), (t, tt, e, s)
                cases.add(len(set(s)) if R > 2 else 0)
    assert fs.T > 2 * R
    if 0 < p_reset < 0.5:
        assert cases == {1, 2, 3}                        # all three branches of the rule were met
    # the row-0 rule: the first rows never address a row below 0
    fs = VF.FrameStream(R, N)
    for t in range(2):
        fs.add(np.full((N, 3, 1, 1), t, np.uint8))
    frames, first = fs.ring()
    assert VF.stack_slots(first, R, N, 0) == (0, 0, 0) and VF.stack_slots(first, R, N, N) == (0, 0, N)


def test_wrapper_restatement_by_hand():
    """reset fills the deque with the first frame, step pushes one frame (dmc.py:98-109)"""
    w = VF.FrameStack()
    f = [np.full((3, 2, 2), i, np.uint8) for i in range(5)]
    assert np.array_equal(w.reset(f[0]), np.concatenate([f[0], f[0], f[0]]))
    assert np.array_equal(w.step(f[1]), np.concatenate([f[0], f[0], f[1]]))
    assert np.array_equal(w.step(f[2]), np.concatenate([f[0], f[1], f[2]]))
    assert np.array_equal(w.step(f[3]), np.concatenate([f[1], f[2], f[3]]))
    assert np.array_equal(w.reset(f[4]), np.concatenate([f[4], f[4], f[4]])) and w.observation().shape == (9, 2, 2)


# ------------------------------------------------------------------------------------------------ the store
def test_bounds_and_constructor_validation():
    from drqv2_amd.replay import FrameBatch, IndexedBatch, VecDeviceReplay, VecFrameReplay
    R, N, A, nstep, g = 12, 2, 3, 3, 2
    vs = VecFrameReplay(R, N, A, nstep, 0.99, "cpu", guard_rows=g)
    twin = VecDeviceReplay(R, N, (9, 84, 84), A, nstep, 0.99, "cpu", guard_rows=g + 2)
    assert vs.frames.shape == (R * N, 3 * 84 * 84) and vs.frame_bytes == 21168 and twin.frame_bytes == 3 * vs.frame_bytes
    assert vs.obs_shape == (9, 84, 84) and vs.frame_shape == (3, 84, 84) and vs.first.tolist() == [1] * (R * N)
    for T in range(0, 5 * R):
        vs.T = twin.T = T
        lo, hi = vs.bounds()
        assert (lo, hi) == VF.bounds(T, R, nstep, g) == twin.bounds()
        assert hi == T - nstep and lo == max(1, T - R + 1 + g + 2)
        assert len(vs) == max(0, hi - lo + 1) * N
        if hi >= lo:
            assert lo - 3 >= T + g - R or lo == 1      # the oldest frame of an obs stack survives g more adds
    vs.T = 0
    with pytest.raises(ValueError, match="frame_shape"):
        VecFrameReplay(R, N, A, nstep, 0.99, "cpu", frame_shape=(9, 84, 84))
    with pytest.raises(ValueError, match="frame_shape"):
        VecFrameReplay(R, N, A, nstep, 0.99, "cpu", frame_shape=(3, 64, 64))
    with pytest.raises(ValueError, match="guard_rows \\+ 4"):
        VecFrameReplay(nstep + g + 3, N, A, nstep, 0.99, "cpu", guard_rows=g)
    VecFrameReplay(nstep + g + 4, N, A, nstep, 0.99, "cpu", guard_rows=g)
    with pytest.raises(ValueError, match="indexed"):       # as on VecDeviceReplay: prioritized draws are indexed
        VecFrameReplay(R, N, A, nstep, 0.99, "cpu", guard_rows=g, indexed=False, priority_alpha=0.6)
    with pytest.raises(_lib.DrqError):                    # the tree lives on the GPU
        VecFrameReplay(R, N, A, nstep, 0.99, "cpu", guard_rows=g, priority_alpha=0.6)
    with pytest.raises(_lib.DrqError):                    # no CPU fallback, and no row yet
        vs.observation()
    with pytest.raises(_lib.DrqError):                    # no CPU fallback
        vs.add(np.zeros((N, 3, 84, 84), np.uint8), np.zeros((N, A), np.float32), np.zeros(N, np.float32),
               np.ones(N, np.float32))
    with pytest.raises(ValueError, match="obs of shape"):  # a stack where a frame belongs
        vs.add(np.zeros((N, 9, 84, 84), np.uint8), np.zeros((N, A), np.float32), np.zeros(N, np.float32),
               np.ones(N, np.float32))
    assert issubclass(FrameBatch, IndexedBatch)
    first = torch.ones(4, dtype=torch.uint8)
    b = FrameBatch(torch.zeros(4, 16, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), 1, 2, 3,
                   torch.ones(2, dtype=torch.int64), first, 2, 2)
    assert b.ring == (first, 2, 2) and len(b) == 5 and b[1:4] == (1, 2, 3)


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="library not built")
def test_argument_errors_before_any_launch():
    lib = _lib.load()
    x = 4096                                              # never dereferenced: every call below is refused on the host
    assert lib.drq_vec_stack_gather(None, x, 4, 2, 16, None, 0, 2, x, None) == -1
    assert lib.drq_vec_stack_gather(x, x, 4, 2, 24, None, 0, 2, x, None) == -1
    assert lib.drq_vec_stack_gather(x, x, 4, 2, 16, None, 0, 3, x, None) == -1
    assert lib.drq_vec_stack_gather(x, x, 4, 2, 16, None, -1, 2, x, None) == -1
    assert lib.drq_vec_stack_gather(x, x, 4, 2, 16, None, 0, 2, x + 8, None) == -1
    assert lib.drq_conv1_aug_fwd_frames(x, None, 4, 2, x, x, x, x, x, x, x, x, x, 2, 2, None) == -1
    assert lib.drq_conv1_aug_fwd_frames(x, x, 0, 2, x, x, x, x, x, x, x, x, x, 2, 2, None) == -1
    assert lib.drq_conv1_aug_fwd_frames_bf16(x, x, 4, 2, None, x, x, x, x, x, x, x, x, 2, 2, None) == -1
    assert lib.drq_update_phase_frames(None, -1, None, 4, 2, None, None) == -1
    d = _lib.DrqStep()
    assert lib.drq_update_phase_frames(d, -1, x, 0, 2, None, None) == -1
    assert lib.drq_update_phase_frames(d, -1, x, 4, 2, x, None) == -1
    assert lib.drq_update_phase_frames(d, -1, x, 4, 2, None, None) == -1      # missing indices
