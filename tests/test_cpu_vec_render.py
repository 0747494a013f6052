"""Renderer images (VecFrameReplay.add_render, drq_vec_add_render): everything that needs no GPU.  The properties of the
resize rule on its numpy restatement tests/vec_render_oracle.py, the public surface (header, prototype table, build list,
exported symbol, ABI version), the DRQ_EARG cases that are decided before any launch, and the argument errors and the CPU
refusal of the store."""
import ctypes
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import vec_render_oracle as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "drq_vec_add_render"
SIZES = VR.SIZES
assert SIZES == (84, 85, 100, 128, 168, 252, 255, 336)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("S", SIZES)
def test_weights_sum_to_S_and_84_with_at_most_four_taps(S):
    w = VR.weights(S)
    assert w.shape == (84, S) and w.dtype == np.int64 and (w >= 0).all()
    assert (w.sum(axis=1) == S).all() and (w.sum(axis=0) == 84).all()
    assert int((w > 0).sum(axis=1).max()) <= 4
    # the non-zero entries of a row are one run: first .. last input pixel the output pixel overlaps
    for o in (0, 1, 41, 83):
        nz = np.flatnonzero(w[o])
        assert nz[0] == o * S // 84 and nz[-1] == ((o + 1) * S - 1) // 84 and len(nz) == nz[-1] - nz[0] + 1


def test_five_taps_exist_beyond_the_checked_sizes_and_never_six():
    """the 4-tap bound holds at the sizes above and for every S <= 256, not for every S <= 336: 257 is the first size
    with an output pixel over five input pixels (1/84 of the first, three whole ones, 1/84 of the fifth)"""
    taps = {S: int((VR.weights(S) > 0).sum(axis=1).max()) for S in range(84, 337)}
    assert max(taps.values()) == 5 and min(S for S, n in taps.items() if n == 5) == 257
    assert all(n <= 4 for S, n in taps.items() if S <= 256 or S % 84 == 0)


@pytest.mark.parametrize("S", SIZES)
def test_sums_fit_32_bits_and_constant_images_stay_constant(S):
    assert 255 * S * S + (S * S) // 2 < 2 ** 31
    for v in (0, 1, 127, 128, 254, 255):
        out = VR.resize(np.full((2, S, S, 3), v, np.uint8))
        assert out.shape == (2, 3, 84, 84) and out.dtype == np.uint8 and (out == v).all(), (S, v)


def test_size_84_is_the_transposition():
    img = np.random.RandomState(0).randint(0, 256, (3, 84, 84, 4)).astype(np.uint8)
    assert np.array_equal(VR.resize(img), img[..., :3].transpose(0, 3, 1, 2))
    assert np.array_equal(VR.resize(img[..., :3]), img[..., :3].transpose(0, 3, 1, 2))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_multiples_of_84_are_block_means_rounded_half_up(k):
    S = 84 * k
    img = np.random.RandomState(k).randint(0, 256, (2, S, S, 3)).astype(np.uint8)
    img[1, :k, :k] = [[[1, 0, 255]]]                              # block sums k^2, 0, 255 k^2
    blocks = img.astype(np.int64).reshape(2, 84, k, 84, k, 3).sum(axis=(2, 4))
    want = ((blocks + (k * k) // 2) // (k * k)).transpose(0, 3, 1, 2)
    got = VR.resize(img)
    assert np.array_equal(got, want)
    assert got[1, :, 0, 0].tolist() == [1, 0, 255]
    # exactly half rounds up, just below half rounds down
    half = np.zeros((1, S, S, 3), np.uint8)
    n = (k * k + 1) // 2                                          # the smallest block sum that rounds up to 1
    for q in range(n):
        half[0, q // k, q % k, 0] = 1
        half[0, q // k, q % k, 1] = q < n - 1
    out = VR.resize(half)
    assert out[0, 0, 0, 0] == 1 and out[0, 1, 0, 0] == 0 and out[0, 2, 0, 0] == 0


@pytest.mark.parametrize("S", SIZES)
def test_alpha_is_ignored(S):
    r = np.random.RandomState(S)
    a = r.randint(0, 256, (2, S, S, 4)).astype(np.uint8)
    b = a.copy()
    b[..., 3] = r.randint(0, 256, (2, S, S))
    assert not np.array_equal(a, b)
    assert np.array_equal(VR.resize(a), VR.resize(b)) and np.array_equal(VR.resize(a), VR.resize(a[..., :3]))


def test_oracle_equals_a_float64_area_average_where_that_is_exact():
    """an independent statement of the same average: the overlap lengths as fractions of an input pixel in float64,
    the weighted mean, rounded half up -- equal wherever the float mean is not within 1e-9 of a half"""
    S = 100
    img = np.random.RandomState(7).randint(0, 256, (1, S, S, 3)).astype(np.uint8)
    edges_o, edges_i = np.arange(85) * (S / 84.0), np.arange(S + 1, dtype=np.float64)
    w = np.maximum(0.0, np.minimum(edges_o[1:, None], edges_i[None, 1:]) - np.maximum(edges_o[:-1, None], edges_i[None, :-1]))
    mean = np.einsum("yi,xj,eijc->ecyx", w, w, img.astype(np.float64)) / (S / 84.0) ** 2
    safe = np.abs(mean - np.floor(mean) - 0.5) > 1e-9
    assert safe.mean() > 0.99
    assert np.array_equal(np.floor(mean + 0.5)[safe], VR.resize(img).astype(np.float64)[safe])


# ------------------------------------------------------------------------------------------------ public surface
def test_header_prototype_build_list_symbol_and_abi_version():
    header = abi.text()
    abi.assert_prototype(NAME)
    assert len(_lib.PROTOTYPES[NAME][1]) == 17
    for text in ("w(o, i) = max(0, min(S (o+1), 84 (i+1)) - max(S o, 84 i))", "< 2^31", "round half up"):
        assert text in header, text                                        # the rule is part of the contract
    with open(os.path.join(ROOT, "drqv2_amd", "csrc", "step.hip")) as f:
        assert "drq_abi_version(void) { return 7; }" in f.read()        # additive: the version stays
    from drqv2_amd import build
    assert "vecrender.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vecrender.hip"))
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    lib = _lib.load()
    assert lib.drq_abi_version() == 7 and hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)


def test_refusals_that_need_no_gpu():
    """argument errors are reported before any launch.  The pointers are made-up addresses with the required alignment:
    a refused call never looks behind them"""
    lib = _lib.load()
    F, SC, IMG, FIRST = 0x10000, 0x20000, 0x30000, 0x40000
    ok = [F, SC, SC + 0x1000, SC + 0x2000, SC + 0x3000, 8, 3, 2, 5, IMG, 128, 4, SC + 0x4000, SC + 0x5000, SC + 0x6000,
          FIRST]
    bad = []
    for k in (0, 1, 2, 3, 4, 9, 12, 13, 14):                             # every required pointer; src_first may be NULL
        bad.append(ok[:k] + [None] + ok[k + 1:])
    for k, vals in ((5, (0, -1)), (6, (0, -3, 2 ** 31 // 21 + 1)), (7, (0, -2)), (8, (-1,)),      # R, N, A, t
                    (10, (83, 0, -84, 337, 420, 1024)), (11, (0, 1, 2, 5, -3))):                 # S, Cin
        for v in vals:
            bad.append(ok[:k] + [v] + ok[k + 1:])
    for mis in (4, 8, 12, 1):
        bad.append([F + mis] + ok[1:])                                     # frames not 16-byte aligned
    for mis in (1, 2, 3):
        bad.append(ok[:9] + [IMG + mis] + ok[10:])                         # src_image not 4-byte aligned
    for a in bad:
        assert getattr(lib, NAME)(*a, None) == -1, a
    assert len(bad) == 9 + 2 + 3 + 2 + 1 + 6 + 5 + 4 + 3


# ------------------------------------------------------------------------------------------------ the store, no GPU
def test_add_render_argument_errors_and_cpu_refusal():
    from drqv2_amd.replay import VecDeviceReplay, VecFrameReplay
    assert not hasattr(VecDeviceReplay, "add_render")                      # no renderer produces stacks
    N, A = 3, 2
    st = VecFrameReplay(rows=16, num_envs=N, action_dim=A, nstep=3, discount=0.99, device="cpu", seed=0)
    img = np.zeros((N, 128, 128, 4), np.uint8)
    act, rew = np.zeros((N, A), np.float32), np.zeros(N, np.float32)
    disc, first = np.ones((N, 1), np.float32), np.zeros(N, bool)
    z = lambda *s, dt=np.uint8: np.zeros(s, dt)
    bad_images = {"rank": z(N, 128, 128), "rank5": z(N, 1, 128, 128, 3), "N": z(N + 1, 128, 128, 3),
                  "square": z(N, 128, 96, 3), "small": z(N, 83, 83, 3), "large": z(N, 337, 337, 4),
                  "channels1": z(N, 128, 128, 1), "channels5": z(N, 128, 128, 5), "chw": z(N, 3, 84, 84),
                  "float": z(N, 128, 128, 3, dt=np.float32), "int8": z(N, 128, 128, 3, dt=np.int8),
                  "list": img.tolist(), "tensor_dtype": torch.zeros((N, 84, 84, 3), dtype=torch.int32)}
    for name, bad in bad_images.items():
        with pytest.raises(ValueError, match=r"add_render\(\): image"):
            st.add_render(bad, act, rew, disc, first)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="is on"):
            st.add_render(torch.zeros((N, 84, 84, 3), dtype=torch.uint8, device="cuda"), act, rew, disc, first)
    # the other four arguments: add()'s checks and add()'s messages
    for bad in ((img, act[:, :1], rew, disc, first), (img, act.astype(np.int32), rew, disc, first),
                (img, act, np.zeros((N, 2), np.float32), disc, first), (img, act, rew, disc[:2], first),
                (img, act, rew, disc, np.zeros((N, 1), bool)), (img, act, rew, disc, np.zeros(N, np.float32)),
                (img, act.tolist(), rew, disc, first)):
        with pytest.raises(ValueError) as e_render:
            st.add_render(*bad)
        with pytest.raises(ValueError) as e_add:
            st.add(np.zeros((N, 3, 84, 84), np.uint8), *bad[1:])
        assert str(e_render.value) == str(e_add.value) and str(e_add.value).startswith("add(): ")
    assert st.T == 0
    # well-formed rows on a CPU store: refused like add(), after the argument checks; nothing is counted
    for good in ((img, act, rew, disc, first), (torch.zeros((N, 84, 84, 3), dtype=torch.uint8), act.astype(np.float64), rew[:, None], disc, None),
                 (np.zeros((N, 336, 336, 3), np.uint8)[:, ::1], act, rew, disc, first)):
        with pytest.raises(_lib.DrqError, match="no CPU fallback"):
            st.add_render(*good)
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        st.add(np.zeros((N, 3, 84, 84), np.uint8), act, rew, disc, first)
    assert st.T == 0 and st._render_stage is None
