"""Strong augmentations (drq_aug_overlay, drq_aug_random_conv, drqv2_amd.augment): everything that needs no GPU.  The public
surface and every DRQ_EARG case (all are decided before any launch), the identities of the numpy restatement
tests/strongaug_oracle.py, the classes' ValueErrors and then DrqError on a CPU device, state dicts, svea_batch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import strongaug_oracle as O

ENTRIES = {"drq_aug_overlay": 9, "drq_aug_random_conv": 6}


def augment():
    from drqv2_amd import augment as A
    return A


def frames(seed, B=2, C=6):
    return np.random.RandomState(seed).randint(0, 256, (B, C, 84, 84)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototypes_symbols_and_build():
    header = abi.text()
    for name, nargs in ENTRIES.items():
        abi.assert_prototype(name)
        assert len(_lib.PROTOTYPES[name][1]) == nargs and name not in _lib.NO_STREAM and name in abi.stream_entries()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    for text in ("---- strong augmentation.", "out[b][3g + c][p] = (x * (256 - alpha_q8) + y * alpha_q8 + 128) >> 8",
                 "y = bank[clamp(idx[b], 0, M - 1)][c][p]", "acc = acc + w[b][co][ci][ky][kx] * p",
                 "(float)obs[b][3g + ci][clamp(i + ky - 1, 0, 83)][clamp(j + kx - 1, 0, 83)] * 0.003921568859368563f",
                 "q = acc / (1.0f + fabsf(acc))", "q = 0 if q != q", "v = (0.5f + 0.5f * q) * 255.0f",
                 "(uint8_t)(int)(v + 0.5f)"):
        assert text in header, text                                        # the rule is part of the contract
    flowed = " ".join(header.replace("\n *", " ").split())
    assert "in the image of DMControl-GB's sigmoid(conv2d(x / 255)), not a port of it" in flowed
    from drqv2_amd import build
    assert "strongaug.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "strongaug.hip"))
    assert build.FILE_FLAGS["strongaug.hip"] == build.FILE_FLAGS["veccartpole.hip"] \
        == ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]
    assert _lib.load().drq_abi_version() == 7                              # additive: the version stays
    with open(os.path.join(build.CSRC, "strongaug.hip")) as f:
        src = "\n".join(line.split("//")[0] for line in f.read().splitlines())     # the code without its comments
    for banned in ("atomic", "asm", "printf", "fmaf", "expf"):              # plain HIP C++, nothing fused by hand
        assert banned not in src, banned
    assert "__shared__" in src and "uint4" in src and src.count("DRQ_LAUNCH_CHECK") == 2


def test_every_refusal_needs_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_strongaug.py repeats them on poisoned memory.)"""
    lib = _lib.load()
    calls = O.overlay_refusals(0x1000000, 0x2000000, 0x3000000, 0x4000000)
    assert len(calls) == 24 and len({why for why, _ in calls}) == 24
    for why, a in calls:
        assert lib.drq_aug_overlay(*a, None) == -1, why
    calls = O.conv_refusals(0x1000000, 0x3000000, 0x4000000)
    assert len(calls) == 19 and len({why for why, _ in calls}) == 19
    for why, a in calls:
        assert lib.drq_aug_random_conv(*a, None) == -1, why


# ------------------------------------------------------------------------------------------------ the oracle's identities
def test_overlay_alpha_0_is_obs_and_256_is_the_bank_image():
    obs, bank = frames(0, 3, 9), frames(1, 2, 3)
    idx = np.array([1, 0, 1])
    assert O.overlay(obs, bank, idx, 0).tobytes() == obs.tobytes()
    full = O.overlay(obs, bank, idx, 256)
    for b in range(3):
        for g in range(3):
            assert full[b, 3 * g:3 * g + 3].tobytes() == bank[idx[b]].tobytes()      # the same image over every frame
    half = O.overlay(obs, bank, idx, 128)
    want = (obs[2, 4].astype(int) * 128 + bank[1, 1].astype(int) * 128 + 128) >> 8
    assert half.dtype == np.uint8 and (half[2, 4] == want).all()
    # the index is clamped, never refused: -1 reads image 0, M reads image M - 1
    assert O.overlay(obs, bank, [-1, 2, 7], 256)[:, :3].tobytes() == bank[[0, 1, 1]].tobytes()
    # alpha 1 and 255 move a byte by at most one step towards the other image
    for a in (1, 255):
        d = O.overlay(obs, bank, idx, a).astype(int) - (obs if a == 1 else O.overlay(obs, bank, idx, 256)).astype(int)
        assert np.abs(d).max() == 1


def test_conv_zero_weights_give_128_and_non_finite_sums_do():
    obs = frames(2, 1, 3)
    w = np.zeros((1, 3, 3, 3, 3), np.float32)
    assert (O.random_conv(obs, w) == 128).all()
    w[0, 0, 0, 1, 1], w[0, 1, 2, 0, 0] = np.inf, np.nan
    obs[0, 0, 5, 5] = 0                                                    # inf * 0 is NaN already; inf / (1 + inf) is too
    out = O.random_conv(obs, w)
    assert (out[0, :2] == 128).all() and (out[0, 2] == 128).all()


def test_conv_single_positive_tap_saturates_monotonically():
    """w[co][co][1][1] = +big alone: the output is a non-decreasing function of the input byte that starts at 128 and
    reaches 255"""
    ramp = (np.arange(84 * 84) % 256).astype(np.uint8).reshape(84, 84)
    obs = np.stack([ramp, ramp, ramp])[None]
    w = np.zeros((1, 3, 3, 3, 3), np.float32)
    for co in range(3):
        w[0, co, co, 1, 1] = 1e3
    out = O.random_conv(obs, w)
    for co in range(3):
        by_value = np.array([out[0, co][ramp == x].max() for x in range(256)])
        assert all((out[0, co][ramp == x] == by_value[x]).all() for x in range(256))      # a function of the byte alone
        assert (np.diff(by_value.astype(int)) >= 0).all() and by_value[0] == 128 and by_value[-1] == 255
        assert by_value[1] > 128
    w *= -1
    assert O.random_conv(obs, w)[0, 0][ramp == 255].max() == 0


def test_conv_replicate_padding_at_the_corners_by_hand():
    """a frame that is 0 but for three pixels at the corners, all-ones weights from channel 0 to channel 0: a corner's sum
    counts its own pixel four times (the clamp replicates it into three padded positions), an edge neighbour's twice"""
    obs = np.zeros((1, 3, 84, 84), np.uint8)
    obs[0, 0, 0, 0], obs[0, 0, 0, 83], obs[0, 0, 83, 0] = 255, 51, 102
    w = np.zeros((1, 3, 3, 3, 3), np.float32)
    w[0, 0, 0] = 1.0
    out = O.random_conv(obs, w)

    def byte(total):      # sums of 1.0, 0.2 and 0.4 in float32, as the contract adds them
        acc = np.float32(0.0)
        for t in total:
            acc = np.float32(acc + np.float32(np.float32(t) * O.INV255))
        q = np.float32(acc / np.float32(np.float32(1.0) + acc))
        return int(np.float32(np.float32(np.float32(0.5) + np.float32(np.float32(0.5) * q)) * np.float32(255.0)) + np.float32(0.5))

    assert out[0, 0, 0, 0] == byte([255] * 4) and out[0, 0, 0, 1] == byte([255] * 2) and out[0, 0, 1, 1] == byte([255])
    assert out[0, 0, 0, 83] == byte([51] * 4) and out[0, 0, 1, 83] == byte([51] * 2)
    assert out[0, 0, 83, 0] == byte([102] * 4) and out[0, 0, 83, 1] == byte([102] * 2) and out[0, 0, 83, 83] == 128
    assert out[0, 0, 2, 2] == 128 and (out[0, 1:] == 128).all()
    # and the vectorised oracle is the contract's scalar loop, on random data, at corners, edges and inside
    obs, w = frames(3, 2, 6), np.random.RandomState(4).standard_normal((2, 3, 3, 3, 3)).astype(np.float32)
    out = O.random_conv(obs, w)
    for b, g, co, i, j in ((0, 0, 0, 0, 0), (1, 1, 2, 83, 83), (0, 1, 1, 0, 83), (1, 0, 0, 83, 0), (0, 0, 2, 40, 0), (1, 1, 1, 17, 63)):
        assert out[b, 3 * g + co, i, j] == O.conv_pixel(obs, w, b, g, co, i, j), (b, g, co, i, j)


# ------------------------------------------------------------------------------------------------ the classes, no GPU
def test_constructor_value_errors_say_why():
    A = augment()
    bank = torch.zeros(2, 3, 84, 84, dtype=torch.uint8)
    for bad in (-0.1, 1.5, "half", None, True):
        with pytest.raises(ValueError, match="alpha must be a number in"):
            A.RandomOverlay(bank, alpha=bad, device="cpu")
    for bad in (bank[0], bank[:0], torch.zeros(2, 3, 64, 64, dtype=torch.uint8), torch.zeros(2, 1, 84, 84, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"bank: uint8 \[M, 3, 84, 84\]"):
            A.RandomOverlay(bad, device="cpu")
    with pytest.raises(ValueError, match="bank must be torch.uint8"):
        A.RandomOverlay(bank.float(), device="cpu")
    for cls, args in ((A.RandomOverlay, (bank,)), (A.RandomConv, ())):
        for bad in (1.5, "0", None, True):
            with pytest.raises(ValueError, match="seed must be an int"):
                cls(*args, device="cpu", seed=bad)
    assert [A.RandomOverlay(bank, alpha=a, device="cpu").alpha_q8 for a in (0, 0.5, 1, 0.001, 0.002, 0.999)] == [0, 128, 256, 0, 1, 256]
    aug = A.RandomOverlay(bank.numpy(), device="cpu")                      # an array is taken as well, and copied
    assert aug.M == 2 and aug.bank.data_ptr() != bank.data_ptr() and aug.last_idx is None
    assert A.RandomConv(device="cpu").last_weights is None


@pytest.mark.parametrize("kind", ["overlay", "conv"])
def test_call_checks_its_arguments_then_refuses_the_cpu(kind):
    A = augment()
    aug = A.RandomOverlay(torch.zeros(2, 3, 84, 84, dtype=torch.uint8), device="cpu") if kind == "overlay" else A.RandomConv(device="cpu")
    name = type(aug).__name__
    obs = torch.zeros(2, 9, 84, 84, dtype=torch.uint8)
    before = aug.generator.get_state().clone()
    for bad, why in ((obs.numpy(), "must be a tensor"), (obs[0], "shape"), (obs[:, :5], "shape"), (obs[:0], "shape"),
                     (obs[:, :, :64], "shape"), (obs.float(), "must be torch.uint8"), (obs.to("meta"), "is on meta")):
        with pytest.raises(ValueError, match=rf"{name}\(\): obs.*{why}"):
            aug(bad)
    for bad, why in ((obs[:1], "shape"), (obs.int(), "must be torch.uint8"), (obs.to("meta"), "is on meta"), ([1], "must be a tensor"),
                     (torch.zeros(2, 84, 84, 9, dtype=torch.uint8).permute(0, 3, 1, 2), "must be contiguous")):
        with pytest.raises(ValueError, match=rf"{name}\(\): out.*{why}"):
            aug(obs, out=bad)
    if kind == "conv":
        with pytest.raises(ValueError, match="out must not be obs"):
            aug(obs, out=obs)
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):            # after the checks
        aug(obs)
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        aug(obs, out=torch.empty_like(obs))
    assert torch.equal(aug.generator.get_state(), before)                  # nothing was drawn by any of them


def test_state_dicts_round_trip_the_generator_and_name_a_mismatch():
    A = augment()
    bank = torch.from_numpy(frames(5, 2, 3))
    a = A.RandomOverlay(bank, alpha=0.25, device="cpu", seed=7)
    sd = a.state_dict()
    assert set(sd) == {"format", "kind", "config", "generator"} and sd["format"] == 1 and sd["kind"] == "RandomOverlay"
    assert sd["config"] == {"seed": 7, "alpha_q8": 64, "bank_shape": (2, 3, 84, 84), "bank_crc": a.bank_crc}      # not the bytes
    draw = lambda o: torch.randint(100, (5,), generator=o.generator)
    draw(a)
    mid = a.state_dict()
    assert not torch.equal(mid["generator"], sd["generator"])
    want = [draw(a), draw(a)]
    fresh = A.RandomOverlay(bank, alpha=0.25, device="cpu", seed=7)
    fresh.load_state_dict(mid)
    assert torch.equal(draw(fresh), want[0]) and torch.equal(draw(fresh), want[1])
    # a mismatch names every field that differs and changes nothing: the bank is configuration by shape and CRC
    other_bank = bank.clone()
    other_bank[1, 2, 3, 4] ^= 1
    other = A.RandomOverlay(other_bank, alpha=0.5, device="cpu", seed=8)
    state = other.generator.get_state().clone()
    with pytest.raises(ValueError, match=r"seed: saved 7, here 8; alpha_q8: saved 64, here 128; bank_crc: saved \d+, here \d+"):
        other.load_state_dict(mid)
    assert torch.equal(other.generator.get_state(), state)                 # nothing changed
    with pytest.raises(ValueError, match=r"bank_shape: saved \(2, 3, 84, 84\), here \(1, 3, 84, 84\)"):
        A.RandomOverlay(bank[:1], alpha=0.25, device="cpu", seed=7).load_state_dict(mid)
    c = A.RandomConv(device="cpu", seed=3)
    csd = c.state_dict()
    assert csd["kind"] == "RandomConv" and csd["config"] == {"seed": 3}
    with pytest.raises(ValueError, match="kind"):
        c.load_state_dict(mid)
    with pytest.raises(ValueError, match="kind"):
        a.load_state_dict(csd)
    with pytest.raises(ValueError, match="format"):
        c.load_state_dict(dict(csd, format=2))
    with pytest.raises(ValueError, match="generator: no tensor saved"):
        c.load_state_dict({k: v for k, v in csd.items() if k != "generator"})
    with pytest.raises(ValueError, match="generator: saved torch.uint8"):
        c.load_state_dict(dict(csd, generator=csd["generator"][:-1]))
    with pytest.raises(ValueError, match="a dict from state_dict"):
        c.load_state_dict(None)
    c2 = A.RandomConv(device="cpu", seed=3)
    draw(c)
    c2.load_state_dict(c.state_dict())
    assert torch.equal(draw(c2), draw(c))


def test_state_dict_goes_through_a_checkpoint_file_as_plain_data(tmp_path):
    A = augment()
    from drqv2_amd import checkpoint
    a = A.RandomOverlay(torch.from_numpy(frames(6, 2, 3)), device="cpu", seed=1)
    torch.randint(9, (3,), generator=a.generator)
    path = str(tmp_path / "ck.pt")
    checkpoint.save(path, extra={"step": 4, "svea": a.state_dict()})
    extra = checkpoint.load(path)
    b = A.RandomOverlay(torch.from_numpy(frames(6, 2, 3)), device="cpu", seed=1)
    b.load_state_dict(extra["svea"])
    assert torch.equal(b.generator.get_state(), a.generator.get_state())


def test_noise_bank():
    A = augment()
    bank = A.noise_bank(3, seed=2)
    assert bank.dtype == torch.uint8 and tuple(bank.shape) == (3, 3, 84, 84) and bank.device.type == "cpu"
    assert torch.equal(bank, A.noise_bank(3, seed=2)) and not torch.equal(bank, A.noise_bank(3, seed=3))
    assert not torch.equal(bank[0], bank[1]) and int(bank.max()) > 200 and int(bank.min()) < 55
    # smooth: neighbouring pixels differ by little (a grid of 6 points over 84 pixels: at most 255 * 5 / 83 a pixel)
    d = (bank[:, :, :, 1:].int() - bank[:, :, :, :-1].int()).abs().max()
    assert int(d) <= 17
    A.RandomOverlay(bank, device="cpu")                                    # the constructor takes it
    with pytest.raises(ValueError, match="noise_bank"):
        A.noise_bank(0)


def test_svea_batch_shapes_and_contents_with_a_stub():
    A = augment()
    B = 3
    r = np.random.RandomState(0)
    obs, nxt = torch.from_numpy(frames(7, B, 9)), torch.from_numpy(frames(8, B, 9))
    action = torch.from_numpy(r.standard_normal((B, 2)).astype(np.float32))
    reward, discount = torch.arange(B, dtype=torch.float32).view(B, 1), torch.full((B, 1), 0.97)
    calls = []

    def strong(x):
        calls.append(x)
        return 255 - x

    out = A.svea_batch((obs, action, reward, discount, nxt), strong)
    assert len(calls) == 1 and calls[0] is obs                             # one call, on the clean observations
    assert isinstance(out, tuple) and len(out) == 5
    assert [tuple(t.shape) for t in out] == [(2 * B, 9, 84, 84), (2 * B, 2), (2 * B, 1), (2 * B, 1), (2 * B, 9, 84, 84)]
    assert [t.dtype for t in out] == [torch.uint8, torch.float32, torch.float32, torch.float32, torch.uint8]
    assert torch.equal(out[0][:B], obs) and torch.equal(out[0][B:], 255 - obs)
    for got, src in zip(out[1:], (action, reward, discount, nxt)):        # the target's side is never augmented
        assert torch.equal(got[:B], src) and torch.equal(got[B:], src)
    for text in ("actor step also sees the augmented half", "independent random shifts"):
        assert text in " ".join(A.svea_batch.__doc__.split())
