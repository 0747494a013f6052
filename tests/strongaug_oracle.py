"""The strong augmentations of include/drqv2_hip.h ("strong augmentation") restated in numpy (a helper module like
tests/poison.py: not collected, no torch).  overlay() is integer arithmetic; random_conv() is np.float32 operations in
the written order -- arrays over the pixels, one IEEE operation per element and step, which is what the scalars of the
contract do.  Also the argument lists of the refusals, which both test files walk."""
import numpy as np

SIDE, PLANE, FRAME = 84, 84 * 84, 3 * 84 * 84
STACKS = (3, 6, 9, 12)
INV255 = np.float32(0.003921568859368563)


def overlay(obs, bank, idx, alpha_q8):
    """obs u8 [B, C, 84, 84], bank u8 [M, 3, 84, 84], idx int [B] (any value: clamped), alpha_q8 0 .. 256"""
    B, C = obs.shape[:2]
    assert C in STACKS and 0 <= alpha_q8 <= 256
    m = np.clip(np.asarray(idx, np.int64), 0, bank.shape[0] - 1)
    y = np.tile(bank[m].astype(np.int64), (1, C // 3, 1, 1))          # the same image over every frame of the stack
    return ((obs.astype(np.int64) * (256 - alpha_q8) + y * alpha_q8 + 128) >> 8).astype(np.uint8)


def random_conv(obs, w):
    """obs u8 [B, C, 84, 84], w f32 [B, 3, 3, 3, 3] = (sample, c_out, c_in, ky, kx)"""
    B, C = obs.shape[:2]
    assert C in STACKS and w.shape == (B, 3, 3, 3, 3) and w.dtype == np.float32
    out = np.empty_like(obs)
    half, one, scale = np.float32(0.5), np.float32(1.0), np.float32(255.0)
    with np.errstate(all="ignore"):
        for b in range(B):
            for g in range(C // 3):
                x = obs[b, 3 * g:3 * g + 3].astype(np.float32) * INV255          # p of every pixel: two operations
                xp = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="edge")            # the clamp of the source pixel
                for co in range(3):
                    acc = np.zeros((SIDE, SIDE), np.float32)
                    for ci in range(3):
                        for ky in range(3):
                            for kx in range(3):
                                acc = acc + w[b, co, ci, ky, kx] * xp[ci, ky:ky + SIDE, kx:kx + SIDE]
                    q = acc / (one + np.abs(acc))
                    q = np.where(q != q, np.float32(0.0), q)
                    v = (half + half * q) * scale
                    assert acc.dtype == q.dtype == v.dtype == np.float32
                    out[b, 3 * g + co] = (v + half).astype(np.int32).astype(np.uint8)
    return out


def conv_pixel(obs, w, b, g, co, i, j):
    """one output byte by the contract's scalar loop, word for word: what random_conv() is checked against"""
    acc = np.float32(0.0)
    clamp = lambda v: min(max(v, 0), SIDE - 1)
    with np.errstate(all="ignore"):
        for ci in range(3):
            for ky in range(3):
                for kx in range(3):
                    p = np.float32(obs[b, 3 * g + ci, clamp(i + ky - 1), clamp(j + kx - 1)]) * INV255
                    acc = np.float32(acc + np.float32(w[b, co, ci, ky, kx] * p))
        q = np.float32(acc / np.float32(np.float32(1.0) + np.abs(acc)))
        if q != q:
            q = np.float32(0.0)
        v = np.float32(np.float32(np.float32(0.5) + np.float32(np.float32(0.5) * q)) * np.float32(255.0))
        return int(np.float32(v + np.float32(0.5)))


# ------------------------------------------------------------------------------------------------ refusals
def overlay_refusals(obs, bank, idx, out, B=3, C=9, M=2):
    """[(why, args without the stream)] of every DRQ_EARG case of drq_aug_overlay; the pointers are integers, 16-byte
    aligned, of allocations that hold B x C frames, M images and B indices"""
    ok = (obs, bank, idx, out, B, C, M, 128)
    at = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
    calls = [("a null obs", at(0, None)), ("a null bank", at(1, None)), ("a null idx", at(2, None)), ("a null out", at(3, None)),
             ("obs not 16-byte aligned", at(0, obs + 8)), ("bank not 16-byte aligned", at(1, bank + 4)),
             ("out not 16-byte aligned", at(3, out + 1)), ("idx not 4-byte aligned", at(2, idx + 2)),
             ("B = 0", at(4, 0)), ("B < 0", at(4, -1)), ("B C 7,056 > INT32_MAX", at(4, (2 ** 31 - 1) // (C * PLANE) + 1)),
             ("M = 0", at(6, 0)), ("alpha_q8 < 0", at(7, -1)), ("alpha_q8 > 256", at(7, 257)),
             ("out overlapping obs without being obs", at(3, obs + 16)), ("out overlapping the bank", at(3, bank + FRAME))]
    return calls + [(f"C = {c}", at(5, c)) for c in (0, 1, 2, 4, 8, 10, 15, -3)]


def conv_refusals(obs, w, out, B=3, C=9):
    """the same for drq_aug_random_conv"""
    ok = (obs, w, out, B, C)
    at = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
    calls = [("a null obs", at(0, None)), ("a null w", at(1, None)), ("a null out", at(2, None)),
             ("obs not 16-byte aligned", at(0, obs + 4)), ("out not 16-byte aligned", at(2, out + 8)),
             ("w not 4-byte aligned", at(1, w + 1)), ("B = 0", at(3, 0)), ("B < 0", at(3, -7)),
             ("B C 7,056 > INT32_MAX", at(3, (2 ** 31 - 1) // (C * PLANE) + 1)),
             ("out == obs (in place)", at(2, obs)), ("out overlapping obs", at(2, obs + 16 * 1000))]
    return calls + [(f"C = {c}", at(4, c)) for c in (0, 1, 5, 7, 11, 13, 15, -9)]
