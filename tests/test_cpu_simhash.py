"""The exploration bonus without a GPU: the numpy oracle (tests/simhash_oracle.py) against the words of the contract and
against statements that follow from them, and the host side of drqv2_amd/explore.py -- argument checks, the sparse state
dict, the checkpoint file, the registration of the entry.  tests/test_hip_simhash.py holds the kernels to this oracle."""
import os
import re

import numpy as np
import pytest
import torch

from tests import simhash_oracle as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAME = "drq_explore_simhash_step"


def test_module_imports_and_the_entry_is_registered():
    import drqv2_amd.explore as X
    from drqv2_amd import _lib, build
    assert X.MAX_BITS == S.MAX_BITS == 24
    assert "explore.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "explore.hip"))
    assert not any("fast" in f for flags in build.FILE_FLAGS.values() for f in flags)
    assert NAME in _lib.PROTOTYPES and NAME not in _lib.NO_STREAM
    with open(os.path.join(ROOT, "include", "drqv2_hip.h")) as f:
        hdr = f.read()
    assert "---- exploration bonus" in hdr and re.search(r"#define\s+DRQ_SIMHASH_MAX_BITS\s+24\b", hdr)
    for text in ("fmix32(seed ^ (j * 441 + i) * 0x9E3779B9) & 1", "v_i = 441 * s_i - sum_j s_j", "(p_j > 0) << j",
                 "beta / sqrt((float)c_n)", "bonus_n = beta for c_n = 0"):
        assert text in hdr, text
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    assert hasattr(_lib.load(), NAME)


def test_refusals_that_need_no_gpu():
    """every DRQ_EARG case is decided before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them.  (tests/test_hip_simhash.py repeats them on poisoned outputs.)"""
    from drqv2_amd import _lib
    lib = _lib.load()
    for a in S.refused_calls(0x10000, 0x20000, 0x30000, 0x40000):
        assert getattr(lib, NAME)(*a, None) == -1, a


# ------------------------------------------------------------------------------------------------ the oracle
def test_fmix32_and_the_sign_matrix():
    assert [S.fmix32(h) for h in (0, 1, 0x12345678, 0xFFFFFFFF)] == [0, 0x514E28B7, 0xE37CD1BC, 0x81F16F39]
    for bits, seed in ((1, 0), (8, 3), (24, 0xDEADBEEF)):
        a = S.signs(bits, seed)
        assert a.shape == (bits, 441) and a.dtype == np.int64 and set(np.unique(a)) == {-1, 1}
        for j, i in ((0, 0), (0, 440), (bits - 1, 0), (bits - 1, 440), (bits // 2, 217)):
            assert a[j, i] == S.sign(j, i, seed), (bits, seed, j, i)
        assert abs(int(a.sum())) < 6 * np.sqrt(a.size)          # a fair coin, six standard deviations


def test_cells_by_hand_and_centred_sums_to_zero():
    frame = np.zeros((2, 3, 84, 84), np.uint8)
    frame[0, 0, 0, 0] = 7            # cell (0, 0)
    frame[0, 2, 3, 3] = 5            # cell (0, 0), another channel, the far corner of the block
    frame[0, 1, 4, 3] = 9            # cell (1, 0)
    frame[0, 1, 83, 80] = 11         # cell (20, 20)
    frame[1] = 255
    s = S.cells(frame)
    assert s.shape == (2, 441) and s[0, 0] == 12 and s[0, 21] == 9 and s[0, 440] == 11 and s[0].sum() == 32
    assert (s[1] == 12240).all()
    v = S.centred(S.cells(S.random_frames(5, 1)))
    assert v.dtype == np.int64 and (v.sum(axis=1) == 0).all() and np.abs(v).max() <= 441 * 12240 < 2 ** 31


def test_the_largest_projection_by_hand():
    """the frame that is 255 on the +1 cells of bit 0 and 0 elsewhere: with k such cells p_0 = 12,240 k (882 - 2 k), the
    bound the header states; its mirror image gives -p_0 and bit 0"""
    a = S.signs(1, 0)[0].reshape(21, 21)
    k = int((a > 0).sum())
    plane = np.repeat(np.repeat(np.where(a > 0, 255, 0).astype(np.uint8), 4, axis=0), 4, axis=1)
    frame = np.stack([plane] * 3)[None]
    assert S.projections(frame, 1, 0)[0, 0] == 12240 * k * (882 - 2 * k) <= 1190217600
    assert S.codes(frame, 1, 0)[0] == 1 and S.codes(255 - frame, 1, 0)[0] == 0
    assert S.projections(255 - frame, 1, 0)[0, 0] == -12240 * (441 - k) * (882 - 2 * (441 - k))


@pytest.mark.parametrize("bits", [1, 8, 24])
def test_uniform_frames_give_code_zero(bits):
    frame = np.stack([np.full(S.FRAME_SHAPE, v, np.uint8) for v in (0, 1, 128, 255)])
    assert (S.projections(frame, bits, 5) == 0).all()
    assert (S.codes(frame, bits, 5) == 0).all()


def test_code_is_invariant_under_a_constant_where_nothing_saturates():
    frame = np.random.RandomState(2).randint(0, 200, size=(6,) + S.FRAME_SHAPE).astype(np.uint8)
    want = S.codes(frame, 24, 9)
    assert len(np.unique(want)) > 1
    for k in (1, 17, 55):
        assert int(frame.max()) + k <= 255
        assert np.array_equal(S.codes(frame + np.uint8(k), 24, 9), want), k
        assert np.array_equal(S.projections(frame + np.uint8(k), 24, 9), S.projections(frame, 24, 9))


def test_two_far_apart_cell_patterns_differ_for_the_chosen_seed():
    """one bright block in the top-left corner against one in the bottom-right corner, 16 bits: the seed is the first
    for which the oracle tells them apart, found here, so the statement is true of the oracle and not assumed"""
    a, b = np.full((1,) + S.FRAME_SHAPE, 40, np.uint8), np.full((1,) + S.FRAME_SHAPE, 40, np.uint8)
    a[0, :, 4:12, 4:12] = 250
    b[0, :, 68:76, 72:80] = 250
    seed = next(s for s in range(64) if S.codes(a, 16, s)[0] != S.codes(b, 16, s)[0])
    ca, cb = S.codes(a, 16, seed)[0], S.codes(b, 16, seed)[0]
    assert ca != cb and ca != 0 and cb != 0
    # v of a one-block pattern is +(441 - 4) d on the four cells of the block and -4 d elsewhere (d = 48 * 210): by hand
    va = S.centred(S.cells(a))[0]
    assert sorted(set(va.tolist())) == [-4 * 48 * 210, 437 * 48 * 210] and (va > 0).sum() == 4


def test_count_and_bonus_over_a_hand_written_sequence_of_codes():
    o = S.SimHashOracle(3, 0.5, 0)
    c, b = o.count([1, 1, 4])                  # a duplicate inside the step: both see 2
    assert c.tolist() == [2, 2, 1] and o.table.tolist() == [0, 2, 0, 0, 1, 0, 0, 0]
    assert b.dtype == F and b.tobytes() == np.array([F(0.5) / np.sqrt(F(2)), F(0.5) / np.sqrt(F(2)), F(0.5)], F).tobytes()
    c, b = o.count([4, 0, 1, 1, 1])
    assert c.tolist() == [2, 1, 5, 5, 5] and o.distinct() == 3
    assert b.tobytes() == S.bonus_of([2, 1, 5, 5, 5], 0.5).tobytes()
    assert b[2] == F(F(0.5) / np.sqrt(F(5)))
    before = o.table.copy()
    c, b = o.count([7, 1, 7], update=False)    # reading only: an unseen code has count 0 and the bonus beta
    assert c.tolist() == [0, 5, 0] and b[0] == F(0.5) == b[2] and np.array_equal(o.table, before)
    # the conversion rounds: 2^24 + 1 is no float32
    assert S.bonus_of([2 ** 24 + 1], 1.0)[0] == F(1.0) / np.sqrt(F(2 ** 24))
    code, c, b, total = S.SimHashOracle(8, 0.1, 1).step(S.random_frames(3, 0), np.array([1, -2, 0.25], F))
    assert total.dtype == F and total.tobytes() == (np.array([1, -2, 0.25], F) + b).astype(F).tobytes()


@pytest.mark.parametrize("n", [1, 3, 65])
def test_the_shared_sequences_hold_what_the_gpu_tests_need(n):
    """duplicates inside a step (n > 1), repeats across steps, at least two codes: on the oracle's own output"""
    frames, rewards = S.sequence(n, 11)
    for bits in (8, 24):
        out = S.run(n, bits, 0.1, 3, frames, rewards)
        assert S.covers(out, n)
        assert np.array_equal(out[2][0], out[0][0]) and (out[2][1] >= 2).all()          # step 2 repeats step 0
        assert out[1][0][0] == 0 and (n == 1 or out[1][0][1] == 0)                      # all 0, all 255
        if n > 1:
            assert out[3][0][n - 1] == out[3][0][0] and out[3][1][n - 1] == out[3][1][0] >= 2
        assert out[-1][4].sum() == 6 * n


# ------------------------------------------------------------------------------------------------ the class, no GPU
def test_constructor_and_step_arguments_are_checked_before_any_device():
    from drqv2_amd._lib import DrqError
    from drqv2_amd.explore import SimHashBonus
    for bad in (0, 25, -1, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="bits"):
            SimHashBonus(3, "cpu", bits=bad)
    with pytest.raises(ValueError, match="num_envs"):
        SimHashBonus(0, "cpu")
    for bad in (float("nan"), float("inf"), -0.1):
        with pytest.raises(ValueError, match="beta"):
            SimHashBonus(3, "cpu", beta=bad)
    b = SimHashBonus(3, "cpu", bits=8, beta=0.25, seed=-1)
    assert b.seed == 0xFFFFFFFF and b.table.shape == (256,) and b.table.dtype == torch.int32 and not b.table.any()
    assert b.codes is None and b.counts is None and int(b.distinct()) == 0
    frame, reward = torch.zeros((3, 3, 84, 84), dtype=torch.uint8), torch.zeros(3)
    for bad, what in ((frame.numpy(), "tensor"), (frame[:2], "shape"), (frame[:, :, :, :83], "shape"),
                      (frame.float(), "uint8"), (frame.reshape(3, -1), "shape")):
        with pytest.raises(ValueError, match=what):
            b.step(bad)
    for bad, what in (([0.0] * 3, "tensor"), (reward[:2], "shape"), (reward.double(), "float32"), (reward[:, None], "shape")):
        with pytest.raises(ValueError, match=what):
            b.step(frame, bad)
    with pytest.raises(DrqError, match="GPU"):           # well formed: only now the missing device matters
        b.step(frame, reward)
    assert b._out is None and not b.table.any()


def test_sparse_state_dict_round_trip_on_cpu_tensors():
    from drqv2_amd.explore import SimHashBonus
    b = SimHashBonus(4, "cpu", bits=24, beta=0.1, seed=7)
    b.table[[5, 70000, 2 ** 24 - 1]] = torch.tensor([3, 1, 2 ** 31 - 1], dtype=torch.int32)
    sd = b.state_dict()
    assert sd["format"] == 1 and sd["kind"] == "SimHashBonus"
    assert sd["config"] == {"N": 4, "bits": 24, "beta": 0.1, "seed": 7}
    assert sd["index"].tolist() == [5, 70000, 2 ** 24 - 1] and sd["index"].dtype == torch.int64
    assert sd["count"].tolist() == [3, 1, 2 ** 31 - 1] and sd["count"].dtype == torch.int32
    assert sum(t.numel() for t in sd.values() if torch.is_tensor(t)) == 6          # sparse: not 2^24 entries
    fresh = SimHashBonus(4, "cpu", bits=24, beta=0.1, seed=7)
    fresh.table[9] = 4                                                              # a used object: overwritten whole
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.table, b.table) and int(fresh.distinct()) == 3
    sd["index"][0] = 6                                                              # shares nothing with the object
    assert int(b.table[5]) == 3 and int(fresh.table[5]) == 3
    empty = SimHashBonus(4, "cpu", bits=24, beta=0.1, seed=7)
    fresh.load_state_dict(empty.state_dict())
    assert not fresh.table.any()
    b.reset()
    assert not b.table.any()


def test_load_state_dict_refuses_what_does_not_fit_and_changes_nothing():
    from drqv2_amd.explore import SimHashBonus
    b = SimHashBonus(4, "cpu", bits=8, beta=0.1, seed=7)
    b.table[3] = 2
    sd = b.state_dict()
    for field, other in (("N", SimHashBonus(5, "cpu", bits=8, beta=0.1, seed=7)),
                         ("bits", SimHashBonus(4, "cpu", bits=9, beta=0.1, seed=7)),
                         ("beta", SimHashBonus(4, "cpu", bits=8, beta=0.2, seed=7)),
                         ("seed", SimHashBonus(4, "cpu", bits=8, beta=0.1, seed=8))):
        other.table[1] = 9
        with pytest.raises(ValueError, match=rf"\b{field}: saved"):
            other.load_state_dict(sd)
        assert other.table.tolist().count(9) == 1 and int(other.distinct()) == 1
    target = SimHashBonus(4, "cpu", bits=8, beta=0.1, seed=7)
    target.table[1] = 9
    for bad in (dict(sd, kind="VecReach"), dict(sd, format=2), dict(sd, index=torch.tensor([256])),
                dict(sd, index=torch.tensor([-1])), dict(sd, index=sd["index"].int()), dict(sd, count=sd["count"].long()),
                dict(sd, index=torch.tensor([3, 3]), count=torch.tensor([1, 1], dtype=torch.int32)),
                dict(sd, count=torch.zeros(2, dtype=torch.int32)), {k: v for k, v in sd.items() if k != "index"}, None):
        with pytest.raises(ValueError):
            target.load_state_dict(bad)
        assert int(target.table[1]) == 9 and int(target.distinct()) == 1


def test_checkpoint_file_with_and_without_the_bonus(tmp_path):
    from drqv2_amd import checkpoint
    from drqv2_amd.explore import SimHashBonus
    mk = lambda: SimHashBonus(4, "cpu", bits=12, beta=0.1, seed=7)
    b = mk()
    b.table[[1, 4000]] = torch.tensor([5, 6], dtype=torch.int32)
    with_bonus, without = str(tmp_path / "with.pt"), str(tmp_path / "without.pt")
    checkpoint.save(with_bonus, bonus=b, extra={"step": 3})
    checkpoint.save(without, extra={"step": 4})
    fresh = mk()
    assert checkpoint.load(with_bonus, bonus=fresh) == {"step": 3}
    assert torch.equal(fresh.table, b.table)
    assert checkpoint.load(with_bonus) == {"step": 3}                    # a part not asked for is ignored
    assert checkpoint.load(without) == {"step": 4}                       # a file without it loads as before
    ck = torch.load(without, weights_only=True)
    assert "bonus" not in ck and "bonus" in torch.load(with_bonus, weights_only=True)
    untouched = mk()
    untouched.table[2] = 1
    with pytest.raises(ValueError, match="bonus"):                       # asked for, not in the file
        checkpoint.load(without, bonus=untouched)
    assert int(untouched.table[2]) == 1
    with pytest.raises(ValueError, match=r"\bbits: saved 12, here 13"):
        checkpoint.load(with_bonus, bonus=SimHashBonus(4, "cpu", bits=13, beta=0.1, seed=7))
