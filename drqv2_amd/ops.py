"""Thin tensor-level wrappers over the C ABI (include/drqv2_hip.h): shape checks on the host, raw
device pointers into the library, work enqueued on the current device's current stream.  GPU tensors only."""
import torch

from . import _lib
from ._lib import check, ptr

ENC_H = (84, 41, 39, 37, 35)


def _alloc(shape, dtype, device, kind="out"):
    """Every result and workspace of this module comes from here (tests swap it for poisoned, guarded memory).
    kind: "out" = a result the launch writes in full, "ws" = scratch, "zero" = a zeroed buffer it writes partly."""
    if kind == "zero":
        return torch.zeros(shape, device=device, dtype=dtype)
    return torch.empty(shape, device=device, dtype=dtype)


_stream = _lib.current_stream   # for tests and tools that call an entry themselves


def launch(name, *args):
    """_lib.launch on the current device; the status goes through this module's `check`, which tests/poison.py replaces"""
    check(_lib.enqueue(name, *args), name)


def _need(t, dtype=torch.float32, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise _lib.DrqError(f"{name}: a GPU tensor is required (the HIP path has no CPU fallback)")
    if t.device.index != torch.cuda.current_device():
        # these wrappers launch on the current device's current stream (the update path guards the device itself)
        raise _lib.DrqError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}: "
                            "wrap the call in torch.cuda.device(...)")
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.DrqError(f"{name}: contiguous {dtype} required, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


def aug_base_grid(h, pad, device):
    """The table torch.linspace gives the reference on the same device (drqv2.py:24-29)."""
    S = h + 2 * pad
    eps = 1.0 / S
    return torch.linspace(-1.0 + eps, 1.0 - eps, S, device=device, dtype=torch.float32)[:h].contiguous()


def random_shifts_aug(x, shift, pad=4, base=None, fuse_norm=False):
    """x: u8 or f32 [n,c,h,h]; shift: f32 [n,1,1,2] or [n,2] (the torch.randint draw)."""
    n, c, h, w = x.shape
    assert h == w
    shift = _need(shift.reshape(n, 2), name="shift")
    base = aug_base_grid(h, pad, x.device) if base is None else _need(base, name="base")
    out = _alloc((n, c, h, w), torch.float32, x.device)
    if x.dtype == torch.uint8:
        _need(x, torch.uint8, "obs")
        launch("drq_aug_fwd", ptr(x), ptr(shift), ptr(base), ptr(out), n, c, h, pad, int(fuse_norm))
    else:
        _need(x, name="obs")
        if fuse_norm:
            raise _lib.DrqError("fuse_norm needs uint8 input")
        launch("drq_aug_fwd_f32", ptr(x), ptr(shift), ptr(base), ptr(out), n, c, h, pad)
    return out


def conv1_aug_fwd(obs, shift, obs1, shift1, w, b, n_store=None, base=None, bf16=False, y_nhwc=False):
    """Fused RandomShiftsAug + /255-0.5 + conv1 + ReLU on both views (drq_conv1_aug_fwd).
    Returns (y [2n,32,41,41], xaug [2n,9,84,84] with frames [0,n_store) written, the rest zero); y_nhwc (with bf16): y
    is bf16 [2n,41,41,32] (drq_conv1_aug_fwd_bf16_nhwc)."""
    n = obs.shape[0]
    _need(obs, torch.uint8, "obs")
    _need(obs1, torch.uint8, "obs1")
    if tuple(obs.shape[1:]) != (9, 84, 84) or obs1.shape != obs.shape:
        raise _lib.DrqError("conv1_aug_fwd: frames must be [n,9,84,84]")
    shift, shift1 = _need(shift.reshape(n, 2), name="shift"), _need(shift1.reshape(n, 2), name="shift1")
    base = aug_base_grid(84, 4, obs.device) if base is None else _need(base, name="base")
    n_store = n if n_store is None else n_store
    y = (_alloc((2 * n, 41, 41, 32), torch.bfloat16, obs.device) if y_nhwc else
         _alloc((2 * n, 32, 41, 41), torch.float32, obs.device))
    xaug = _alloc((2 * n, 9, 84, 84), torch.float32, obs.device, "zero")
    if y_nhwc and not bf16:
        raise _lib.DrqError("conv1_aug_fwd: the channel-contiguous bf16 output belongs to the bf16 form")
    launch("drq_conv1_aug_fwd" + ("_bf16_nhwc" if y_nhwc else "_bf16" if bf16 else ""), ptr(obs), ptr(shift), ptr(obs1),
           ptr(shift1), ptr(base), ptr(_need(w, name="w")), ptr(_need(b, name="b")), ptr(xaug), ptr(y), n, n_store)
    return y, xaug


def conv1_aug_fwd_indexed(frames, idx, shift, frames1, idx1, shift1, w, b, n_store=None, base=None):
    """drq_conv1_aug_fwd_indexed: the two views are rows idx / idx1 (int64) of frame stores [slots, 9*84*84] uint8."""
    n = idx.numel()
    shift, shift1 = _need(shift.reshape(n, 2), name="shift"), _need(shift1.reshape(n, 2), name="shift1")
    base = aug_base_grid(84, 4, frames.device) if base is None else _need(base, name="base")
    n_store = n if n_store is None else n_store
    y = _alloc((2 * n, 32, 41, 41), torch.float32, frames.device)
    xaug = _alloc((2 * n, 9, 84, 84), torch.float32, frames.device, "zero")
    launch("drq_conv1_aug_fwd_indexed", ptr(frames), ptr(idx), ptr(shift), ptr(frames1), ptr(idx1), ptr(shift1),
           ptr(base), ptr(_need(w, name="w")), ptr(_need(b, name="b")), ptr(xaug), ptr(y), n, n_store)
    return y, xaug


def conv1_aug_fwd_frames(frames, first, R, N, idx, shift, idx1, shift1, w, b, n_store=None, base=None, bf16=False):
    """drq_conv1_aug_fwd_frames(_bf16): both views are stacks of a single-frame ring (frames [R N, 3*84*84] uint8, first
    [R N] uint8), idx / idx1 (int64) the slots of their newest frames."""
    n = idx.numel()
    _need(frames, torch.uint8, "frames"), _need(first, torch.uint8, "first")
    shift, shift1 = _need(shift.reshape(n, 2), name="shift"), _need(shift1.reshape(n, 2), name="shift1")
    base = aug_base_grid(84, 4, frames.device) if base is None else _need(base, name="base")
    n_store = n if n_store is None else n_store
    y = _alloc((2 * n, 32, 41, 41), torch.float32, frames.device)
    xaug = _alloc((2 * n, 9, 84, 84), torch.float32, frames.device, "zero")
    launch("drq_conv1_aug_fwd_frames" + ("_bf16" if bf16 else ""), ptr(frames), ptr(first), R, N, ptr(idx), ptr(shift),
           ptr(idx1), ptr(shift1), ptr(base), ptr(_need(w, name="w")), ptr(_need(b, name="b")), ptr(xaug), ptr(y), n,
           n_store)
    return y, xaug


def vec_stack_gather(frames, first, R, N, slots=None, t=0):
    """drq_vec_stack_gather: the frame stacks [n, 3 * frame bytes] whose newest frames are `slots` (int64), or, without
    slots, those of the N environments of absolute row t, out of a single-frame ring (frames [R N, frame bytes])."""
    _need(frames, torch.uint8, "frames"), _need(first, torch.uint8, "first")
    n, fb = (N if slots is None else slots.numel()), frames.shape[1]
    out = _alloc((n, 3 * fb), torch.uint8, frames.device)
    launch("drq_vec_stack_gather", ptr(frames), ptr(first), R, N, fb, ptr(slots), t, n, ptr(out))
    return out


def vec_export_rows(frames, action, reward, discount, R, N, table, stack=1):
    """drq_vec_export_rows: the M steps (t, e, t0) of `table` (int32 [M, 3]) out of a step-major ring -> (obs uint8
    [M, stack * frame bytes], action [M, A], reward [M], discount [M]); stack = 3 puts the observation together from the
    frames of a single-frame ring, and a step with t == t0 gets the dummies 0, 0, 1."""
    _need(frames, torch.uint8, "frames"), _need(table, torch.int32, "table")
    for t, name in ((action, "action"), (reward, "reward"), (discount, "discount")):
        _need(t, torch.float32, name)
    if table.dim() != 2 or table.shape[1] != 3:
        raise _lib.DrqError(f"table: int32 [M, 3] required, got {tuple(table.shape)}")
    M, A, fb, dev = table.shape[0], action.shape[1], frames.shape[1], frames.device
    obs = _alloc((M, stack * fb), torch.uint8, dev)
    act, rew, disc = _alloc((M, A), torch.float32, dev), _alloc((M,), torch.float32, dev), _alloc((M,), torch.float32, dev)
    launch("drq_vec_export_rows", ptr(frames), ptr(action), ptr(reward), ptr(discount), R, N, A, fb, stack, ptr(table),
           M, ptr(obs), ptr(act), ptr(rew), ptr(disc))
    return obs, act, rew, disc


def vec_fill(frames, action, reward, discount, first, R, N, T, src_frames, src_action, src_reward, src_discount, src_first):
    """drq_vec_fill: rows T .. T + n - 1 of a step-major ring, in place, from step-major sources (src_frames uint8
    [n, N, frame bytes], src_action [n, N, A], src_reward, src_discount [n, N], src_first uint8 [n, N]): what n
    drq_vec_add calls would write, in one launch."""
    for t, name in ((frames, "frames"), (first, "first"), (src_frames, "src_frames"), (src_first, "src_first")):
        _need(t, torch.uint8, name)
    for t, name in ((action, "action"), (reward, "reward"), (discount, "discount"), (src_action, "src_action"),
                    (src_reward, "src_reward"), (src_discount, "src_discount")):
        _need(t, torch.float32, name)
    n, A, fb = src_first.shape[0], action.shape[1], frames.shape[1]
    if (src_frames.numel() != n * N * fb or src_action.numel() != n * N * A or src_reward.numel() != n * N
            or src_discount.numel() != n * N or src_first.numel() != n * N):
        raise _lib.DrqError(f"vec_fill: sources of {n} rows x {N} environments required")
    launch("drq_vec_fill", ptr(frames), ptr(action), ptr(reward), ptr(discount), ptr(first), R, N, A, fb, T, n,
           ptr(src_frames), ptr(src_action), ptr(src_reward), ptr(src_discount), ptr(src_first))


def vec_stack_push(prev, frame, first=None, reset_all=False):
    """drq_vec_stack_push: the frame stacks uint8 [N, 9, 84, 84] after `frame` (uint8 [N, 3, 84, 84]) has been pushed onto
    `prev` (None with reset_all) -- a reset environment (first[e], or all) holds its frame three times."""
    _need(frame, torch.uint8, "frame")
    if frame.dim() != 4 or tuple(frame.shape[1:]) != (3, 84, 84):
        raise _lib.DrqError(f"frame: uint8 [N, 3, 84, 84] required, got {tuple(frame.shape)}")
    N = frame.shape[0]
    if prev is not None and (_need(prev, torch.uint8, "prev").numel() != N * 9 * 84 * 84):
        raise _lib.DrqError(f"prev: uint8 [{N}, 9, 84, 84] required, got {tuple(prev.shape)}")
    if first is not None and _need(first, torch.uint8, "first").numel() != N:
        raise _lib.DrqError(f"first: uint8 [{N}] required, got {tuple(first.shape)}")
    out = _alloc((N, 9, 84, 84), torch.uint8, frame.device)
    launch("drq_vec_stack_push", ptr(prev), ptr(out), ptr(frame), ptr(first), N, int(bool(reset_all)))
    return out


def vec_video_record(frame, envs, grid, scale, done=None, limit=0):
    """drq_vec_video_record: the mosaic uint8 [GH 84 k, GW 84 k, 3] of the environments `envs` (int32 [M]) out of `frame`
    (uint8 [N, 3, 84, 84]), grid = (GH, GW), scale = k; with done (int32 [N]) and limit > 0 the tiles of environments
    with done >= limit are dimmed."""
    _need(frame, torch.uint8, "frame"), _need(envs, torch.int32, "envs")
    if frame.dim() != 4 or tuple(frame.shape[1:]) != (3, 84, 84):
        raise _lib.DrqError(f"frame: uint8 [N, 3, 84, 84] required, got {tuple(frame.shape)}")
    N, (GH, GW), k = frame.shape[0], grid, int(scale)
    if done is not None and _need(done, torch.int32, "done").numel() != N:
        raise _lib.DrqError(f"done: int32 [{N}] required, got {tuple(done.shape)}")
    out = _alloc((GH * 84 * k, GW * 84 * k, 3), torch.uint8, frame.device)
    launch("drq_vec_video_record", ptr(frame), ptr(envs), envs.numel(), ptr(done), int(limit), ptr(out), GH, GW, k, N)
    return out


def u8_normalize(x):
    _need(x, torch.uint8, "obs")
    y = _alloc(x.shape, torch.float32, x.device)
    launch("drq_u8_normalize", ptr(x), ptr(y), x.numel())
    return y


def conv3x3_fwd(x, w, b, stride, relu=True, bf16=False, wino=False):
    _need(x, name="x"), _need(w, name="w"), _need(b, name="b")
    nb, cin, hin, _ = x.shape
    hout = (hin - 3) // stride + 1
    y = _alloc((nb, 32, hout, hout), torch.float32, x.device)
    if wino:
        launch("drq_conv3x3_fwd_wino", ptr(x), ptr(w), ptr(b), ptr(y), nb, hin, int(relu), 32 * hout * hout,
               hout * hout, hout, 0)
        return y
    if bf16:
        launch("drq_conv3x3_fwd_bf16", ptr(x), ptr(w), ptr(b), ptr(y), nb, hin, int(relu), 32 * hout * hout,
               hout * hout, hout, 0)
        return y
    launch("drq_conv3x3_fwd", ptr(x), ptr(w), ptr(b), ptr(y), nb, cin, hin, stride, int(relu), 32 * hout * hout,
           hout * hout, hout, 0)
    return y


def conv3x3_dgrad(dy_pad, w, mask, bf16=False, wino=False, pad_out=False):
    """dy_pad [nb,32,hout+4,hout+4] (zero border of 2) -> dx [nb,32,hout+2,hout+2] * (mask>0).
    pad_out (Winograd form): dx is returned in the same padded layout, [nb,32,hout+6,hout+6] with a zero border of 2,
    ready to be the next (shallower) layer's dy_pad."""
    _need(dy_pad, name="dy_pad"), _need(w, name="w")
    nb, _, hp, _ = dy_pad.shape
    hout = hp - 4
    hin = hout + 2
    if mask is not None:
        _need(mask, name="mask")
        assert tuple(mask.shape) == (nb, 32, hin, hin)
    if pad_out:
        if not wino:
            raise _lib.DrqError("conv3x3_dgrad: pad_out is implemented for the Winograd form")
        hpi = hin + 4
        dx = _alloc((nb, 32, hpi, hpi), torch.float32, dy_pad.device, "zero")
        launch("drq_conv3x3_dgrad_wino", ptr(dy_pad), ptr(w), ptr(mask), ptr(dx), nb, hout, 32 * hpi * hpi, hpi * hpi,
               hpi, 2 * hpi + 2)
        return dx
    dx = _alloc((nb, 32, hin, hin), torch.float32, dy_pad.device)
    if wino:
        launch("drq_conv3x3_dgrad_wino", ptr(dy_pad), ptr(w), ptr(mask), ptr(dx), nb, hout, 32 * hin * hin, hin * hin,
               hin, 0)
        return dx
    if bf16:
        launch("drq_conv3x3_dgrad_bf16", ptr(dy_pad), ptr(w), ptr(mask), ptr(dx), nb, hout, 32 * hin * hin, hin * hin,
               hin, 0)
        return dx
    launch("drq_conv3x3_dgrad", ptr(dy_pad), ptr(w), ptr(mask), ptr(dx), nb, hout, 32 * hin * hin, hin * hin, hin, 0)
    return dx


def conv3x3_wgrad(x, dy, stride, bf16=False, wino=False, ws=None):
    """x [nb,cin,hin,hin], dy [nb,32,hout,hout] (any strides with unit x-stride) -> dw, db.
    ws: an fp32 workspace of at least drq_conv3x3_wgrad_ws_bytes() to use instead of a fresh one."""
    _need(x, name="x")
    if not (dy.is_cuda and dy.dtype == torch.float32 and dy.stride(3) == 1):
        raise _lib.DrqError("dy: GPU fp32 with unit innermost stride required")
    nb, cin, hin, _ = x.shape
    dw = _alloc((32, cin, 3, 3), torch.float32, x.device)
    db = _alloc((32,), torch.float32, x.device)
    nbytes = _lib.load().drq_conv3x3_wgrad_ws_bytes()
    if ws is None:
        ws = _alloc((nbytes // 4,), torch.float32, x.device, "ws")
    elif ws.numel() * 4 < nbytes:
        raise _lib.DrqError("conv3x3_wgrad: workspace too small")
    if wino:        # dy must be the interior view of a buffer zero-padded by 2 (the kernel reads the padding as zeros)
        launch("drq_conv3x3_wgrad_wino", ptr(x), dy.data_ptr(), ptr(dw), ptr(db), nb, hin, dy.stride(0), dy.stride(1),
               dy.stride(2), 0, ptr(ws), nbytes)
        return dw, db
    if bf16:
        launch("drq_conv3x3_wgrad_bf16", ptr(x), dy.data_ptr(), ptr(dw), ptr(db), nb, hin, dy.stride(0), dy.stride(1),
               dy.stride(2), 0, ptr(ws), nbytes)
        return dw, db
    launch("drq_conv3x3_wgrad", ptr(x), dy.data_ptr(), ptr(dw), ptr(db), nb, cin, hin, stride, dy.stride(0),
           dy.stride(1), dy.stride(2), 0, ptr(ws), nbytes)
    return dw, db


def to_nhwc_bf16(x):
    """fp32 [n,32,h,w] -> the bf16 channel-contiguous layout of the bf16 update ([n,h,w,32], include/drqv2_hip.h)."""
    return x.permute(0, 2, 3, 1).to(torch.bfloat16).contiguous()


def from_nhwc_bf16(y):
    """the inverse, as fp32 [n,32,h,w] (the bf16 values, exactly)."""
    return y.to(torch.float32).permute(0, 3, 1, 2).contiguous()


def conv3x3_fwd_bf16_nhwc(x, w, b, relu=True, y_nhwc=True):
    """x: fp32 [nb,32,hin,hin] or bf16 [nb,hin,hin,32] (layout above) -> y in that layout (bf16) or fp32 NCHW."""
    x_nhwc = x.dtype == torch.bfloat16
    nb = x.shape[0]
    hin = x.shape[1] if x_nhwc else x.shape[2]
    hout = hin - 2
    assert x.is_cuda and x.is_contiguous() and (x.shape[3] == 32 if x_nhwc else x.shape[1] == 32)
    y = (_alloc((nb, hout, hout, 32), torch.bfloat16, x.device) if y_nhwc else
         _alloc((nb, 32, hout, hout), torch.float32, x.device))
    launch("drq_conv3x3_fwd_bf16_nhwc", ptr(x), ptr(w), ptr(b), ptr(y), nb, hin, int(relu), int(x_nhwc), int(y_nhwc))
    return y


def conv3x3_dgrad_bf16_nhwc(dy_pad, w, mask_nhwc, dx_nhwc=False):
    """dy_pad: fp32 [nb,32,hout+4,hout+4] or bf16 [nb,hout+4,hout+4,32] (zero border of 2); the mask bf16 [nb,hin,hin,32].
    -> dx fp32 [nb,32,hin,hin], or (dx_nhwc) a zeroed bf16 [nb,hin+4,hin+4,32] buffer with dx in its interior."""
    _need(w, name="w")
    dy_nhwc = dy_pad.dtype == torch.bfloat16
    nb = dy_pad.shape[0]
    hp = dy_pad.shape[1] if dy_nhwc else dy_pad.shape[2]
    hout = hp - 4
    hin = hout + 2
    assert dy_pad.is_cuda and dy_pad.is_contiguous()
    assert mask_nhwc.dtype == torch.bfloat16 and tuple(mask_nhwc.shape) == (nb, hin, hin, 32) and mask_nhwc.is_contiguous()
    dx = (_alloc((nb, hin + 4, hin + 4, 32), torch.bfloat16, dy_pad.device, "zero") if dx_nhwc else
          _alloc((nb, 32, hin, hin), torch.float32, dy_pad.device))
    launch("drq_conv3x3_dgrad_bf16_nhwc", ptr(dy_pad), ptr(w), ptr(mask_nhwc), ptr(dx), nb, hout, int(dy_nhwc),
           int(dx_nhwc), 32 * hin * hin, hin * hin, hin, 0)
    return dx


def conv3x3_wgrad_bf16_nhwc(x_nhwc, dy):
    """x bf16 [nb,hin,hin,32]; dy: an fp32 strided view [nb,32,hout,hout] or the padded bf16 [nb,hout+4,hout+4,32] buffer."""
    nb, hin, _, _ = x_nhwc.shape
    assert x_nhwc.dtype == torch.bfloat16 and x_nhwc.is_contiguous() and x_nhwc.shape[3] == 32
    dw = _alloc((32, 32, 3, 3), torch.float32, dy.device)
    db = _alloc((32,), torch.float32, dy.device)
    nbytes = _lib.load().drq_conv3x3_wgrad_ws_bytes()
    ws = _alloc((nbytes // 4,), torch.float32, dy.device, "ws")
    if dy.dtype == torch.bfloat16:
        assert tuple(dy.shape) == (nb, hin + 2, hin + 2, 32) and dy.is_contiguous()
        launch("drq_conv3x3_wgrad_bf16_nhwc", ptr(x_nhwc), ptr(dy), ptr(dw), ptr(db), nb, hin, 1, 0, 0, 0, 0, ptr(ws),
               nbytes)
    else:
        launch("drq_conv3x3_wgrad_bf16_nhwc", ptr(x_nhwc), dy.data_ptr(), ptr(dw), ptr(db), nb, hin, 0, dy.stride(0),
               dy.stride(1), dy.stride(2), 0, ptr(ws), nbytes)
    return dw, db


def gemm(A, a_kc, B, b_kc, M, N, K, lda=None, ldb=None, bias=None, relu=False, aux=None, nbatch=1, a_bs=0,
         b_bs=0, c_bs=None, bias_bs=0, aux_bs=0, tile=0, splitk=0, out=None, ldc=None, ws=None):
    """ws: an fp32 split-K workspace to use (e.g. one kept across calls); None: a fresh 64 MB one."""
    dev = A.device
    lda = lda if lda is not None else (K if a_kc else M)
    ldb = ldb if ldb is not None else (K if b_kc else N)
    ldc = ldc if ldc is not None else N
    c_bs = c_bs if c_bs is not None else M * N
    if out is None:
        out = _alloc((nbatch, M, N) if nbatch > 1 else (M, N), torch.float32, dev)
    if ws is None:
        ws = _alloc((16 * 1024 * 1024,), torch.float32, dev, "ws")
    launch("drq_gemm_f32", ptr(A), lda, int(a_kc), ptr(B), ldb, int(b_kc), ptr(out), ldc, M, N, K, nbatch, a_bs, b_bs,
           c_bs, ptr(bias), bias_bs, int(relu), ptr(aux), (aux.shape[-1] if aux is not None else 0), aux_bs, 0, tile,
           splitk, ptr(ws), ws.numel() * 4)
    return out


def linear_fwd(x, w, b, relu=False, **kw):
    M, K = x.shape
    N = w.shape[0]
    return gemm(x, True, w, True, M, N, K, bias=b, relu=relu, **kw)


def linear_dgrad(dy, w, mask=None, **kw):
    M, K = dy.shape           # K = out features
    N = w.shape[1]
    return gemm(dy, True, w, False, M, N, K, aux=mask, **kw)


def linear_wgrad(dy, x, **kw):
    Brows, N = dy.shape
    K = x.shape[1]
    dw = gemm(dy, False, x, False, N, K, Brows, lda=N, ldb=K, **kw)
    db = _alloc((N,), torch.float32, dy.device)
    launch("drq_colsum", ptr(dy), N, 0, ptr(db), 0, Brows, N, 1)
    return dw, db


def ln_tanh_fwd(z, gamma, beta, save=True):
    rows, F = z.shape
    out = _alloc(z.shape, z.dtype, z.device)
    xhat = _alloc(z.shape, z.dtype, z.device) if save else None
    rstd = _alloc((rows,), torch.float32, z.device) if save else None
    launch("drq_ln_tanh_fwd", ptr(z), F, ptr(gamma), ptr(beta), ptr(out), F, ptr(xhat), ptr(rstd), rows, F)
    return out, xhat, rstd


def ln_tanh_bwd(dh, h, xhat, rstd, gamma):
    rows, F = dh.shape
    dz, dln = _alloc(dh.shape, dh.dtype, dh.device), _alloc(dh.shape, dh.dtype, dh.device)
    dg, db = _alloc(gamma.shape, gamma.dtype, gamma.device), _alloc(gamma.shape, gamma.dtype, gamma.device)
    launch("drq_ln_tanh_bwd", ptr(dh), F, None, 0, ptr(h), F, ptr(xhat), ptr(rstd), ptr(gamma), ptr(dz), ptr(dln),
           ptr(dg), ptr(db), rows, F)
    return dz, dg, db


def trunc_normal_sample(pre_tanh, noise, std, clip):
    B, A = pre_tanh.shape
    mu, a = (_alloc(pre_tanh.shape, pre_tanh.dtype, pre_tanh.device) for _ in range(2))
    launch("drq_trunc_normal_sample", ptr(pre_tanh), ptr(noise), float(std), float(clip if clip is not None else 0.0),
           int(clip is not None), ptr(mu), ptr(a), A, B, A)
    return mu, a


def adam_flat(p, g, m, v, lr, step, gscale=1.0, tgt=None, tau=0.0):
    launch("drq_adam_flat", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), int(step), float(gscale), ptr(tgt),
           float(tau))


def ema_flat(p, t, tau):
    launch("drq_ema_flat", ptr(p), ptr(t), p.numel(), float(tau))


def dormant_scores(act, units=None):
    """drq_dormant_scores: act [rows, ld] (the first `units` columns are the layer, default all) -> the mean absolute
    activation of every unit over the rows, float32 [units]."""
    _need(act, name="act")
    rows, ld = act.shape
    units = ld if units is None else int(units)
    score = _alloc((units,), torch.float32, act.device)
    launch("drq_dormant_scores", ptr(act), ld, rows, units, ptr(score))
    return score


def dormant_count(score, tau, count, layer_mean=None):
    """drq_dormant_count: ADDS the number of units with score <= tau * mean(score) to count[0] and the number of units
    to count[1] (count: int32 [2], zeroed by the caller before the first layer); the layer's mean goes to layer_mean
    (float32 [1], allocated when None), which is returned."""
    _need(score, name="score"), _need(count, torch.int32, "count")
    if count.numel() != 2:
        raise _lib.DrqError("dormant_count: count must hold two int32")
    if layer_mean is None:
        layer_mean = _alloc((1,), torch.float32, score.device)
    else:
        _need(layer_mean, name="layer_mean")
    launch("drq_dormant_count", ptr(score), score.numel(), float(tau), ptr(count), ptr(layer_mean))
    return layer_mean


def lerp_flat(p, p0, a):
    """drq_lerp_flat: p <- a p + (1 - a) p0 in place over two flat float32 tensors of one length."""
    _need(p, name="p"), _need(p0, name="p0")
    if p.numel() != p0.numel():
        raise _lib.DrqError(f"lerp_flat: {p.numel()} and {p0.numel()} elements")
    launch("drq_lerp_flat", ptr(p), ptr(p0), p.numel(), float(a))
    return p


def tanh(x):
    y = _alloc(x.shape, x.dtype, x.device)
    launch("drq_tanh", ptr(x), ptr(y), x.numel())
    return y


def tanh_bwd(y, dy):
    """dy * (1 - y^2): the gradient through y = tanh(x)."""
    _need(y, name="y"), _need(dy, name="dy")
    dx = _alloc(y.shape, y.dtype, y.device)
    launch("drq_tanh_bwd", ptr(y), ptr(dy), ptr(dx), y.numel())
    return dx


def relu_mask_pad(dy, mask, pad=2):
    """dy [n,c,h,h] -> [n,c,h+2pad,h+2pad]: dy where mask > 0 (mask None: all of it), zero elsewhere and on the border."""
    _need(dy, name="dy")
    n, c, h, _ = dy.shape
    if mask is not None:
        _need(mask, name="mask")
        assert mask.shape == dy.shape
    out = _alloc((n, c, h + 2 * pad, h + 2 * pad), torch.float32, dy.device)
    launch("drq_relu_mask_pad", ptr(dy), ptr(mask), ptr(out), n * c, h, pad)
    return out


def conv1_dgrad(dy_pad, w):
    """dy_pad [nb,32,45,45] (conv1's pre-activation gradient, zero border of 2), w [32,9,3,3] -> dx [nb,9,84,84]."""
    _need(dy_pad, name="dy_pad"), _need(w, name="w")
    nb = dy_pad.shape[0]
    if tuple(dy_pad.shape[1:]) != (32, 45, 45) or tuple(w.shape) != (32, 9, 3, 3):
        raise _lib.DrqError("conv1_dgrad: dy_pad [nb,32,45,45] and w [32,9,3,3] required")
    dx = _alloc((nb, 9, 84, 84), torch.float32, dy_pad.device)
    launch("drq_conv1_dgrad", ptr(dy_pad), ptr(w), ptr(dx), nb)
    return dx


def aug_bwd_f32(dy, shift, pad=4, base=None):
    """Input gradient of random_shifts_aug on a float frame: dy [n,c,h,h], shift [n,2] / [n,1,1,2] -> dx."""
    _need(dy, name="dy")
    n, c, h, w = dy.shape
    assert h == w
    shift = _need(shift.reshape(n, 2), name="shift")
    base = aug_base_grid(h, pad, dy.device) if base is None else _need(base, name="base")
    dx = _alloc(dy.shape, dy.dtype, dy.device)
    launch("drq_aug_bwd_f32", ptr(dy), ptr(shift), ptr(base), ptr(dx), n, c, h, pad)
    return dx


def _ptr_array(ts):
    """host array of device pointers (None entries allowed) for the batched entry points."""
    import ctypes
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def gemm_batched(As, a_kc, Bs, b_kc, M, N, K, lda, ldb, biases=None, relu=False, auxs=None, rowsum=False, tile=0,
                 splitk=0, scatter_hw=0, Cs=None, bf16=False):
    """n independent problems of one shape in a single launch.  Returns (list of C, list of rowsum or None).
    scatter_hw > 0: C_i is a caller-provided zero-padded [M][32][hw+4][hw+4] gradient buffer (pass Cs)."""
    n = len(As)
    dev = As[0].device
    if Cs is None:
        Cs = [_alloc((M, N), torch.float32, dev) for _ in range(n)]
    rs = [_alloc((M,), torch.float32, dev) for _ in range(n)] if rowsum else None
    ws = _alloc((16 * 1024 * 1024,), torch.float32, dev, "ws")
    if bf16:
        launch("drq_gemm_batched_bf16", n, _ptr_array(As), lda, int(a_kc), _ptr_array(Bs), ldb, int(b_kc),
               _ptr_array(Cs), N, M, N, K, _ptr_array(biases) if biases else None, int(relu),
               _ptr_array(auxs) if auxs else None, (auxs[0].shape[-1] if auxs else 0), _ptr_array(rs) if rs else None,
               scatter_hw, splitk, ptr(ws), ws.numel() * 4)
        return Cs, rs
    launch("drq_gemm_batched_f32", n, _ptr_array(As), lda, int(a_kc), _ptr_array(Bs), ldb, int(b_kc), _ptr_array(Cs), N,
           M, N, K, _ptr_array(biases) if biases else None, int(relu), _ptr_array(auxs) if auxs else None,
           (auxs[0].shape[-1] if auxs else 0), _ptr_array(rs) if rs else None, scatter_hw, tile, splitk, ptr(ws),
           ws.numel() * 4)
    return Cs, rs


def gemm_batched_partial(As, Bs, M, N, K, lda, ldb):
    """Forward form (both operands k-contiguous) through the internal entry the update uses for the trunk:
    returns (sum of the split-K partial records per problem [n][M][N], split count).  Test / tool helper."""
    import ctypes
    n = len(As)
    dev = As[0].device
    Cs = [_alloc((M, N), torch.float32, dev, "zero") for _ in range(n)]
    ws = _alloc((16 * 1024 * 1024,), torch.float32, dev, "zero")
    sk = ctypes.c_int(0)
    launch("drq_gemm_batched_partial", n, _ptr_array(As), lda, 1, _ptr_array(Bs), ldb, 1, _ptr_array(Cs), N, M, N, K,
           None, ptr(ws), ws.numel() * 4, ctypes.byref(sk))
    k = sk.value
    if k <= 1:
        return torch.stack(Cs), k
    return ws[: n * k * M * N].view(n, k, M, N).sum(dim=1), k


def qout_fwd(hs, ws_, bs):
    B, H = hs[0].shape
    qs = [_alloc((B,), torch.float32, hs[0].device) for _ in hs]
    launch("drq_qout_fwd", len(hs), _ptr_array(hs), _ptr_array(ws_), _ptr_array(bs), _ptr_array(qs), B, H)
    return qs


def qout_bwd(dqs, hs, ws_, want_wgrad=True):
    B, H = hs[0].shape
    dev = hs[0].device
    dhs = [_alloc((B, H), torch.float32, dev) for _ in hs]
    dws = [_alloc((H,), torch.float32, dev) for _ in hs] if want_wgrad else None
    dbs = [_alloc((1,), torch.float32, dev) for _ in hs] if want_wgrad else None
    launch("drq_qout_bwd", len(hs), _ptr_array(dqs), _ptr_array(hs), _ptr_array(ws_), _ptr_array(dhs),
           _ptr_array(dws) if dws else None, _ptr_array(dbs) if dbs else None, B, H)
    return dhs, dws, dbs


def mlp_fwd(xs, ws_, bs, relu=True, qws=None, ys=None, ldy=None):
    """hidden-layer forward on the LDS-DMA ring kernel; qws: weight rows of a following Linear(N,1) -> partial dots.
    Returns (list of y, list of qpart [M][nq] or None).  xs / ws_ may be row-strided views (their stride(0) is the
    leading dimension); ys / ldy: caller-provided [M][ldy] output buffers (tests: rows longer than N)."""
    import ctypes
    M, K = xs[0].shape
    N = ws_[0].shape[0]
    dev = xs[0].device
    ldy = N if ldy is None else ldy
    if ys is None:
        ys = [_alloc((M, ldy), torch.float32, dev) for _ in xs]
    qps = [_alloc((M, N // 32), torch.float32, dev, "zero") for _ in xs] if qws else None
    nq = ctypes.c_int(0)
    launch("drq_mlp_fwd", len(xs), _ptr_array(xs), xs[0].stride(0), _ptr_array(ws_), ws_[0].stride(0), _ptr_array(ys),
           ldy, M, N, K, _ptr_array(bs) if bs else None, int(relu), _ptr_array(qws) if qws else None,
           _ptr_array(qps) if qps else None, ctypes.byref(nq))
    if qps:
        qps = [q.view(-1)[: M * nq.value].view(M, nq.value) for q in qps]
    return ys, qps


def mlp_dgrad(dys, ws_, masks=None, dxs=None, lddx=None):
    """dxs / lddx: caller-provided [M][lddx] output buffers; dys / ws_ / masks may be row-strided views."""
    M, K = dys[0].shape
    N = ws_[0].shape[1]
    lddx = N if lddx is None else lddx
    if dxs is None:
        dxs = [_alloc((M, lddx), torch.float32, dys[0].device) for _ in dys]
    launch("drq_mlp_dgrad", len(dys), _ptr_array(dys), dys[0].stride(0), _ptr_array(ws_), ws_[0].stride(0),
           _ptr_array(dxs), lddx, M, N, K, _ptr_array(masks) if masks else None, (masks[0].stride(0) if masks else 0))
    return dxs


def mlp_wgrad_dgrad(dys, xs, ws_, masks=None, dws=None, dxs=None, lddx=None):
    """both gradients of one hidden layer in one launch: returns (dws, dbs, dxs).  dws (dense [Nout][Kin]) and dxs
    ([Brows][lddx]) may be caller-provided buffers; dys / xs / ws_ / masks may be row-strided views."""
    Brows, Nout = dys[0].shape
    Kin = xs[0].shape[1]
    dev = dys[0].device
    lddx = Kin if lddx is None else lddx
    if dws is None:
        dws = [_alloc((Nout, Kin), torch.float32, dev) for _ in dys]
    dbs = [_alloc((Nout,), torch.float32, dev) for _ in dys]
    if dxs is None:
        dxs = [_alloc((Brows, lddx), torch.float32, dev) for _ in dys]
    launch("drq_mlp_wgrad_dgrad", len(dys), _ptr_array(dys), dys[0].stride(0), _ptr_array(xs), xs[0].stride(0),
           _ptr_array(dws), _ptr_array(dbs), _ptr_array(ws_), ws_[0].stride(0), _ptr_array(dxs), lddx,
           _ptr_array(masks) if masks else None, (masks[0].stride(0) if masks else 0), Brows, Nout, Kin)
    return dws, dbs, dxs


def _int_array(vals):
    import ctypes
    return (ctypes.c_int * len(vals))(*vals)


def ln_l1_fwd(jobs, F, H, splitk=0, slab=0):
    """jobs: list of dicts with keys z or part (+bias), gamma, beta, rows, optional tail [rows][A], save (bool),
    heads: list of (w [H][K], b [H]).  Returns per job dict(out [rows][F+tail_n], xhat, rstd, ys=[...])."""
    dev = jobs[0]["gamma"].device
    res, part, z, bias, gamma, beta, out, ldo, xhat, rstd, tail, tld, tn, rows, nh, w, b, y = ([] for _ in range(18))
    for j in jobs:
        r = j["rows"]
        t = j.get("tail")
        n_t = t.shape[1] if t is not None else 0
        o = _alloc((r, F + n_t), torch.float32, dev, "zero")
        xh = _alloc((r, F), torch.float32, dev) if j.get("save", True) else None
        rs = _alloc((r,), torch.float32, dev) if j.get("save", True) else None
        heads = j.get("heads", [])
        ys = [_alloc((r, H), torch.float32, dev) for _ in heads]
        res.append(dict(out=o, xhat=xh, rstd=rs, ys=ys))
        part.append(j.get("part")); z.append(j.get("z")); bias.append(j.get("bias"))
        gamma.append(j["gamma"]); beta.append(j["beta"]); out.append(o); ldo.append(F + n_t)
        xhat.append(xh); rstd.append(rs); tail.append(t); tld.append(t.stride(0) if t is not None else 0); tn.append(n_t)
        rows.append(r); nh.append(len(heads))
        for h in range(2):
            w.append(heads[h][0] if h < len(heads) else None)
            b.append(heads[h][1] if h < len(heads) else None)
            y.append(ys[h] if h < len(heads) else None)
    launch("drq_ln_l1_fwd", len(jobs), _ptr_array(part) if splitk else None, _ptr_array(z) if not splitk else None,
           _ptr_array(bias), _ptr_array(gamma), _ptr_array(beta), _ptr_array(out), _int_array(ldo), _ptr_array(xhat),
           _ptr_array(rstd), _ptr_array(tail), _int_array(tld), _int_array(tn), _int_array(rows), _int_array(nh),
           _ptr_array(w), _ptr_array(b), _ptr_array(y), F, H, splitk, slab)
    return res


def policy_out_l1_fwd(p2, w3, b3, srow0, F, std, clip, noise_hi, ha_hi, noise_lo=None, ha_lo=None, heads=None):
    """policy output layer + sample (+ first layers on the hi rows).  ha_hi [rows-srow0][F+A] holds h in its first F
    columns; returns dict(p3, mu_hi, mu_lo, ys)."""
    rows, H = p2.shape
    A = w3.shape[0]
    dev = p2.device
    p3 = _alloc((rows, A), torch.float32, dev)
    mu_hi = _alloc((rows - srow0, A), torch.float32, dev)
    mu_lo = _alloc((srow0, A), torch.float32, dev) if noise_lo is not None else None
    ys = [_alloc((rows - srow0, H), torch.float32, dev) for _ in (heads or [])]
    launch("drq_policy_out_l1_fwd", ptr(p2), ptr(w3), ptr(b3), ptr(p3), rows, srow0, H, A, F, float(std),
           float(clip if clip is not None else 0.0), int(clip is not None), ptr(noise_hi), ptr(mu_hi), ptr(ha_hi),
           ha_hi.stride(0), ptr(noise_lo), ptr(mu_lo), ptr(ha_lo), (ha_lo.stride(0) if ha_lo is not None else 0),
           len(heads or []), _ptr_array([h[0] for h in heads]) if heads else None,
           _ptr_array([h[1] for h in heads]) if heads else None, _ptr_array(ys) if heads else None)
    return dict(p3=p3, mu_hi=mu_hi, mu_lo=mu_lo, ys=ys)
