"""Strong augmentations on the GPU: drq_aug_overlay and drq_aug_random_conv raw on poisoned, guard-banded memory, and
drqv2_amd.augment (RandomOverlay, RandomConv, svea_batch) against the numpy restatement tests/strongaug_oracle.py.

Bounds.  Everything is compared bit for bit (assert_array_equal): the overlay is integer arithmetic, the convolution single
float32 operations in a fixed order with a correctly rounded division.

Shapes.  B in {1, 3} and C in {3, 9, 12}: one frame, several frames, and a sample stride (C x 7,056) that is no multiple of
the frame stride; a plane is 441 pieces of 16 pixels over 256 lanes, so every launch runs a full and a partial round, and
B = 3 is more than one workgroup.  The images are random bytes with one all-0 and one all-255 frame.  The oracle's outputs
are computed once per case, shared and never modified."""
import functools

import numpy as np
import pytest
import torch
from numpy.testing import assert_array_equal

from tests import poison
from tests import strongaug_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p

pytestmark = pytest.mark.gpu
SHAPES = [(1, 3), (3, 9), (3, 12), (1, 12)]
WEIGHTS = ("normal", "large", "zero", "nonfinite")


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_aug_overlay" in _lib.PROTOTYPES, "the strong-augmentation entries are missing"
    assert "drq_aug_random_conv" in _lib.PROTOTYPES, "the strong-augmentation entries are missing"
    return _lib.load()


@functools.lru_cache(None)
def images(B, C):
    """random bytes; with three frames or more the first frame of the first sample is all 0 and the last frame of the
    last sample all 255"""
    obs = np.random.RandomState(100 * B + C).randint(0, 256, (B, C, 84, 84)).astype(np.uint8)
    if B * C >= 9:
        obs[0, :3] = 0
        obs[-1, -3:] = 255
    obs.setflags(write=False)
    return obs


@functools.lru_cache(None)
def bank_of(M):
    bank = np.random.RandomState(7 + M).randint(0, 256, (M, 3, 84, 84)).astype(np.uint8)
    bank.setflags(write=False)
    return bank


def idx_of(B, M):
    return np.array([-1, M, M - 1][:B] if B > 1 else [M], np.int32)      # below, above and the last: the clamp works


@functools.lru_cache(None)
def weights(B, kind):
    r = np.random.RandomState(11 * B + len(kind))
    w = r.standard_normal((B, 3, 3, 3, 3)).astype(np.float32)
    if kind == "large":
        w *= np.float32(1e3)
    elif kind == "zero":
        w[:] = 0
    elif kind == "nonfinite":
        w[0, 0, 1, 2, 0], w[0, 2, 0, 0, 1] = np.inf, np.nan
    w.setflags(write=False)
    return w


@functools.lru_cache(None)
def conv_want(B, C, kind):
    out = O.random_conv(images(B, C), weights(B, kind))
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the entries on poisoned memory
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("B,C", SHAPES)
def test_overlay_matches_the_oracle_bit_for_bit_out_of_place_and_in_place(lib, B, C, M):
    obs_h, bank_h, idx_h = images(B, C), bank_of(M), idx_of(B, M)
    obs, bank, idx = dev(torch.from_numpy(obs_h.copy()), "obs"), dev(torch.from_numpy(bank_h.copy()), "bank"), dev(torch.from_numpy(idx_h), "idx")
    for alpha in (0, 1, 128, 255, 256):
        want = O.overlay(obs_h, bank_h, idx_h, alpha)
        out = poison.alloc((B, C, 84, 84), torch.uint8, "cuda", name=f"out alpha={alpha}")
        assert lib.drq_aug_overlay(p(obs), p(bank), p(idx), p(out), B, C, M, alpha, None) == 0
        assert_array_equal(out.cpu().numpy(), want)
        assert_array_equal(obs.cpu().numpy(), obs_h)                       # the input is only read
        if alpha == 0:
            assert out.cpu().numpy().tobytes() == obs_h.tobytes()
        if alpha == 256:
            assert_array_equal(out.cpu().numpy()[0, -3:], bank_h[np.clip(idx_h[0], 0, M - 1)])
        place = dev(torch.from_numpy(obs_h.copy()), "obs in place")
        assert lib.drq_aug_overlay(p(place), p(bank), p(idx), p(place), B, C, M, alpha, None) == 0
        assert_array_equal(place.cpu().numpy(), want)
        poison.check()


@pytest.mark.parametrize("kind", WEIGHTS)
@pytest.mark.parametrize("B,C", SHAPES)
def test_random_conv_matches_the_oracle_bit_for_bit(lib, B, C, kind):
    obs_h, w_h, want = images(B, C), weights(B, kind), conv_want(B, C, kind)
    obs, w = dev(torch.from_numpy(obs_h.copy()), "obs"), dev(torch.from_numpy(w_h.copy()), "w")
    out = poison.alloc((B, C, 84, 84), torch.uint8, "cuda", name="out")
    assert lib.drq_aug_random_conv(p(obs), p(w), p(out), B, C, None) == 0
    got = out.cpu().numpy()
    assert_array_equal(got, want)
    assert_array_equal(obs.cpu().numpy(), obs_h)
    if kind == "zero":
        assert (got == 128).all()
    if kind == "large":
        assert got.min() == 0 and got.max() == 255                         # both ends of the squash
    if kind == "nonfinite":
        assert (got[0, 0:C:3] == 128).all() and (got[0, 2:C:3] == 128).all() and not (got[0, 1:C:3] == 128).all()


def test_the_byte_sentinel_never_survives_a_full_write(lib):
    """a uint8 output cannot be checked for "written" by its value in general (poison.py); here it can: zero weights give
    128 and alpha 256 over a bank without the sentinel gives the bank, so a byte that is still 0xA5 was never written"""
    B, C, M = 3, 9, 2
    sent = poison.sentinel_of(torch.uint8)
    obs = dev(torch.from_numpy(images(B, C).copy()), "obs")
    out = poison.alloc((B, C, 84, 84), torch.uint8, "cuda", name="conv out")
    assert lib.drq_aug_random_conv(p(obs), p(dev(torch.zeros(B, 81), "w")), p(out), B, C, None) == 0
    assert not bool((out == sent).any()) and bool((out == 128).all())
    bank_h = np.where(bank_of(M) == sent, 0, bank_of(M)).astype(np.uint8)
    out = poison.alloc((B, C, 84, 84), torch.uint8, "cuda", name="overlay out")
    assert lib.drq_aug_overlay(p(obs), p(dev(torch.from_numpy(bank_h), "bank")), p(dev(torch.tensor([0, 1, 0], dtype=torch.int32), "idx")),
                               p(out), B, C, M, 256, None) == 0
    assert not bool((out == sent).any())


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases of the contract (tests/strongaug_oracle, all held to return the error without a GPU by
    tests/test_cpu_strongaug.py) on real allocations full of the sentinel: the error, and check() finds every byte still
    poison -- in-place convolution among them"""
    B, C, M = 3, 9, 2
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    obs, out, bank = al(B * C * O.PLANE, "obs"), al(B * C * O.PLANE, "out"), al(M * O.FRAME + O.FRAME, "bank")
    idx, w = al(256, "idx"), al(B * 81 * 4 + 16, "w")
    calls = O.overlay_refusals(p(obs), p(bank), p(idx), p(out), B, C, M)
    assert len(calls) == 24
    for why, a in calls:
        assert lib.drq_aug_overlay(*a, None) == -1, why
    calls = O.conv_refusals(p(obs), p(w), p(out), B, C)
    assert len(calls) == 19 and any(a[2] == a[0] for _, a in calls)        # out == obs is one of them
    for why, a in calls:
        assert lib.drq_aug_random_conv(*a, None) == -1, why
    poison.check()


# ------------------------------------------------------------------------------------------------ the classes
def test_random_overlay_follows_the_oracle_and_its_seed_and_resumes():
    from drqv2_amd.augment import RandomOverlay
    B, C, M = 3, 9, 2
    bank_h = bank_of(M)
    obs = torch.from_numpy(images(B, C).copy()).cuda()
    a, twin = RandomOverlay(bank_h, alpha=0.3, device="cuda", seed=5), RandomOverlay(torch.from_numpy(bank_h.copy()).cuda(), 0.3, "cuda", 5)
    assert a.alpha_q8 == 77 and a.bank.is_cuda and a.bank_crc == twin.bank_crc
    outs, drawn = [], set()
    for k in range(4):
        if k == 2:
            mid = a.state_dict()
        out = a(obs)
        assert out.dtype == torch.uint8 and out.shape == obs.shape and out.data_ptr() != obs.data_ptr()
        idx = a.last_idx.cpu().numpy()
        assert idx.dtype == np.int32 and idx.shape == (B,) and 0 <= idx.min() and idx.max() < M
        drawn |= set(idx.tolist())
        assert_array_equal(out.cpu().numpy(), O.overlay(images(B, C), bank_h, idx, 77))
        assert torch.equal(twin(obs), out) and torch.equal(twin.last_idx, a.last_idx)      # the same seed, the same sequence
        outs.append(out)
    assert drawn == {0, 1}
    fresh = RandomOverlay(bank_h, alpha=0.3, device="cuda", seed=5)
    fresh.load_state_dict(mid)                                             # mid-sequence: continues as the uninterrupted one
    for k in (2, 3):
        assert torch.equal(fresh(obs), outs[k])
    # in place, and into a buffer of the caller's
    buf = torch.empty_like(obs)
    assert twin(obs, out=buf) is buf
    place = obs.clone()
    assert a(place, out=place) is place and torch.equal(place, buf) and torch.equal(a.last_idx, twin.last_idx)
    assert_array_equal(obs.cpu().numpy(), images(B, C))
    # a view that is not contiguous is copied first
    wide = torch.zeros(B, C + 3, 84, 84, dtype=torch.uint8, device="cuda")
    wide[:, :C] = obs
    assert_array_equal(a(wide[:, :C]).cpu().numpy(), O.overlay(images(B, C), bank_h, a.last_idx.cpu().numpy(), 77))


def test_random_conv_follows_the_oracle_and_its_seed_and_resumes():
    from drqv2_amd.augment import RandomConv
    B, C = 3, 9
    obs = torch.from_numpy(images(B, C).copy()).cuda()
    a, twin = RandomConv("cuda", seed=9), RandomConv(device="cuda", seed=9)
    outs = []
    for k in range(3):
        if k == 1:
            mid = a.state_dict()
        out = a(obs)
        w = a.last_weights.cpu().numpy()
        assert w.dtype == np.float32 and w.shape == (B, 3, 3, 3, 3)
        if k == 0:
            assert_array_equal(out.cpu().numpy(), O.random_conv(images(B, C), w))
        assert torch.equal(twin(obs), out) and torch.equal(twin.last_weights, a.last_weights)
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])
    fresh = RandomConv("cuda", seed=9)
    fresh.load_state_dict(mid)
    for k in (1, 2):
        assert torch.equal(fresh(obs), outs[k])
    buf = torch.empty_like(obs)
    assert twin(obs, out=buf) is buf and torch.equal(buf, a(obs))
    with pytest.raises(ValueError, match="out must not be obs"):
        a(obs, out=obs)


def test_one_update_on_a_svea_batch():
    """agent.update() on the svea_batch of a materialised batch of 4 rows -- the update sees 8, the smallest sizes the
    whole-update tests run: it runs, its metrics are finite, the augmenter drew exactly once"""
    import drqv2
    from drqv2_amd import synth
    from drqv2_amd.augment import RandomOverlay, noise_bank, svea_batch
    B, A = 4, 3
    torch.manual_seed(2)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, True)
    batch = tuple(t.cuda() for t in synth.make_batch(B, A, 9, seed=1))
    strong = RandomOverlay(noise_bank(4, seed=1), alpha=0.5, device="cuda", seed=3)
    calls = []
    counted = lambda x: calls.append(1) or strong(x)
    state0 = strong.generator.get_state().clone()
    big = svea_batch(batch, counted)
    assert len(calls) == 1 and big[0].shape == (2 * B, 9, 84, 84) and big[4].shape == (2 * B, 9, 84, 84)
    assert torch.equal(big[0][:B], batch[0]) and torch.equal(big[4][B:], batch[4]) and not torch.equal(big[0][B:], batch[0])
    assert_array_equal(big[0][B:].cpu().numpy(), O.overlay(batch[0].cpu().numpy(), strong.bank.cpu().numpy(), strong.last_idx.cpu().numpy(), 128))
    after = strong.generator.get_state().clone()
    assert not torch.equal(after, state0)
    metrics = agent.update(iter([big]), 0)
    assert torch.equal(strong.generator.get_state(), after)                # update() draws nothing from it
    assert set(metrics) >= {"critic_loss", "actor_loss", "critic_q1", "batch_reward"}
    assert all(np.isfinite(float(v)) for v in metrics.values()), metrics
