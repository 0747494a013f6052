"""What the GPU tests of the device-environment family share (a helper module like tests/poison.py: not collected, not a
conftest): the bit-for-bit comparisons, the `lib` fixture, the poisoned output set of a step entry, and the loop that
holds a step entry to its oracle on poisoned, guarded memory."""
import numpy as np
import pytest
import torch

from tests import poison
from tests.test_hip_entries import dev, p

OUT = ("frame", "reward", "discount", "first", "substeps")
U8 = poison.sentinel_of(torch.uint8)


def lib_fixture(entry, missing):
    """the module's `lib` fixture: the loaded library, on a machine with a GPU, whose prototypes hold `entry`"""
    @pytest.fixture(scope="module")
    def lib():
        from drqv2_amd import _lib
        assert torch.cuda.is_available()
        assert entry in _lib.PROTOTYPES, missing
        return _lib.load()
    return lib


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, "
                             f"want {want[tuple(bad[0])]}")


def same_state(got, want, what="state", keys=None):
    """every word of `want` in `got`, and no other (keys: these words only)"""
    if keys is None:
        assert got.keys() == want.keys(), what
    for k in keys or want:
        same_bits(got[k], want[k], (what, k))


def alloc_outs(N, substeps=True):
    """a fresh output set of a step entry, full of the sentinel between guard bands"""
    outs = [poison.alloc((N, 3, 84, 84), torch.uint8, "cuda", name="frame"),
            poison.alloc(N, torch.float32, "cuda", name="reward"), poison.alloc(N, torch.float32, "cuda", name="discount"),
            poison.alloc(N, torch.uint8, "cuda", name="first")]
    return outs + [poison.alloc(N, torch.int32, "cuda", name="substeps")] if substeps else outs


def state_words(state, names):
    """the host copy of the state arrays `names`, episode as the uint32 it is"""
    got = {n: state[n].cpu().numpy() for n in names}
    got["episode"] = got["episode"].view(np.uint32)
    return got


def entry_on_poisoned_memory(step, run, N, steps=12, substeps=True, state=None, compared=(), after_reset=None, beside=None):
    """A step entry on guarded allocations full of the sentinel: the reset of all with a NULL action, then `steps` steps
    into fresh poisoned outputs each.  The outputs equal the oracle's, which never holds the byte sentinel 0xA5 (a frame
    is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one, so every byte was written; check() finds the guard bands
    of outputs, state and action untouched; the words `compared` of `state` equal the oracle's after every call.
    step(action, reset_all, outs) calls the entry on pointers and returns its status; after_reset() runs once behind
    the reset; beside(s, want) runs in front of every check()."""
    for s in range(-1, steps):
        outs = alloc_outs(N, substeps)
        action = None if s < 0 else dev(torch.from_numpy(run["actions"][s]), "action")
        assert step(p(action), int(s < 0), [p(t) for t in outs]) == 0
        if s < 0 and after_reset:
            after_reset()
        want = (run["frame0"], np.zeros(N, np.float32), np.ones(N, np.float32), np.ones(N, np.uint8),
                np.zeros(N, np.int32)) if s < 0 else run["out"][s]
        for name, t, w in zip(OUT, outs, want):
            got = t.cpu().numpy()
            same_bits(got, w, (s, name))
            if got.dtype == np.uint8:
                assert not (got == U8).any(), (s, name)
        if beside:
            beside(s, want)
        poison.check()
        if compared:
            same_state(state_words(state, compared), run["state0"] if s < 0 else run["states"][s], s)
