"""The resize rule of VecFrameReplay.add_render() / drq_vec_add_render (include/drqv2_hip.h, "renderer images") restated in
numpy (a helper module: not collected).  The whole weight matrix, one int64 einsum over both axes at once, + S^2 // 2,
// S^2: nothing of the kernel's separable order, its bands or its tap ranges appears here."""
import numpy as np

OUT = 84
SIZES = (84, 85, 100, 128, 168, 252, 255, 336)      # the sizes the properties are checked at


def weights(S):
    """int64 [84][S]: w(o, i) = max(0, min(S (o+1), 84 (i+1)) - max(S o, 84 i)), an axis measured in 1/84 input pixel"""
    o = np.arange(OUT, dtype=np.int64)[:, None]
    i = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum(S * (o + 1), OUT * (i + 1)) - np.maximum(S * o, OUT * i))


def resize(image):
    """uint8 [N][S][S][3 or 4] -> uint8 [N][3][84][84]; a fourth channel is dropped before anything is computed"""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 4 and image.shape[1] == image.shape[2] and image.shape[3] in (3, 4)
    S = image.shape[1]
    w = weights(S)
    total = np.einsum("yi,xj,eijc->ecyx", w, w, image[..., :3].astype(np.int64), optimize=True)
    out = (total + (S * S) // 2) // (S * S)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)
