"""torch.autograd Functions over the HIP kernels: the module forwards of drqv2.py (Encoder, the Actor / Critic trunks and
MLPs, RandomShiftsAug) as differentiable ops, so that a loss of the user's own reaches the agent's parameters.

Each forward issues exactly the launches the module forward issued before (same values, bit for bit); what it saves
for the backward is kept only when a gradient is needed: ctx.needs_input_grad, and grad mode on where the module was
called (`keep`: under torch.no_grad() ctx.needs_input_grad still reports the inputs' requires_grad, and the forward
itself always runs with grad mode off, so the wrappers below pass the caller's mode in).
The backwards run on the library's kernels -- the conv and nn.Linear gradients of the fused update(), plus the
input-gradient kernels of csrc/autograd.hip -- and none of them is differentiable again (once_differentiable).
fp32 throughout (the bf16 mode belongs to update() alone).  GPU tensors only, like drqv2_amd.ops."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import check, launch, ptr

_WS = {}


def _workspace(device):
    """One fp32 workspace per (device, stream), reused by every GEMM and conv weight gradient of the backwards (all
    of them run in order on that stream): ops.gemm would otherwise allocate 64 MB per call."""
    stream = torch.cuda.current_stream(device)
    key = (device.index, stream.cuda_stream)
    ws = _WS.get(key)
    if ws is None:
        n = max(16 * 1024 * 1024, _lib.load().drq_conv3x3_wgrad_ws_bytes() // 4)
        ws = _WS[key] = torch.empty((n,), device=device, dtype=torch.float32)
    return ws


def _interior(t):
    """[n,c,h+4,h+4] zero-padded gradient buffer -> its [n,c,h,h] interior (a strided view)."""
    return t[:, :, 2:-2, 2:-2]


class EncoderFn(torch.autograd.Function):
    """x [B,C,84,84] fp32 (already /255 - 0.5), the four Conv2d weights / biases -> features [B, 39200] (drqv2.py:63-67)."""

    @staticmethod
    def forward(ctx, keep, x, w1, b1, w2, b2, w3, b3, w4, b4):
        ws, bs = (w1, w2, w3, w4), (b1, b2, b3, b4)
        acts = [x]
        for li in range(4):
            acts.append(ops.conv3x3_fwd(acts[-1], ws[li], bs[li], 2 if li == 0 else 1, relu=True))
        if keep and any(ctx.needs_input_grad):
            ctx.save_for_backward(*acts, *ws)
        feat = acts[-1]
        return feat.view(feat.shape[0], -1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        acts, ws = saved[:5], saved[5:]
        need = ctx.needs_input_grad[1:]     # x, (w, b) of conv1 .. conv4
        wsb = _workspace(g.device)
        grads = [None] * 9
        # conv4's pre-activation gradient: the incoming one where the features are > 0, zero-padded by 2
        dy = ops.relu_mask_pad(g.reshape(acts[4].shape).contiguous(), acts[4])
        for li in (3, 2, 1):                # conv4 .. conv2: Winograd forms, as update() runs them
            if need[1 + 2 * li] or need[2 + 2 * li]:
                grads[1 + 2 * li], grads[2 + 2 * li] = ops.conv3x3_wgrad(acts[li], _interior(dy), 1, wino=True, ws=wsb)
            if not any(need[:1 + 2 * li]):
                return (None, *grads)
            # the gradient of this layer's input = the previous layer's pre-activation gradient (masked by its ReLU)
            dy = ops.conv3x3_dgrad(dy, ws[li], acts[li], wino=True, pad_out=True)
        if need[1] or need[2]:
            grads[1], grads[2] = ops.conv3x3_wgrad(acts[0], _interior(dy), 2, ws=wsb)
        if need[0]:
            grads[0] = ops.conv1_dgrad(dy, ws[0])
        return (None, *grads)


class TrunkFn(torch.autograd.Function):
    """nn.Linear(R, F) -> nn.LayerNorm(F) -> tanh (drqv2.py:74-75, 100-101)."""

    @staticmethod
    def forward(ctx, keep, x, w, b, gamma, beta):
        z = ops.linear_fwd(x, w, b)
        save = keep and any(ctx.needs_input_grad)
        h, xhat, rstd = ops.ln_tanh_fwd(z, gamma, beta, save=save)
        if save:
            ctx.save_for_backward(x, w, gamma, h, xhat, rstd)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        x, w, gamma, h, xhat, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad[1:]
        rows, F = h.shape
        if dh.stride(1) != 1:               # the critic's slice of the [h, action] gradient is a row-strided view
            dh = dh.contiguous()
        dz, dln = torch.empty_like(h), torch.empty_like(h)
        dg, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        launch("drq_ln_tanh_bwd", ptr(dh), dh.stride(0), None, 0, ptr(h), F, ptr(xhat), ptr(rstd), ptr(gamma), ptr(dz),
               ptr(dln), ptr(dg), ptr(dbeta), rows, F)
        wsb = _workspace(dh.device)
        dx = dw = db = None
        if need[1] or need[2]:
            dw, db = ops.linear_wgrad(dz, x, ws=wsb)
        if need[0]:
            dx = ops.linear_dgrad(dz, w, ws=wsb)
        return None, dx, dw, db, dg, dbeta


def _hidden_wgrad_dgrad(dz, h, w, wsb):
    """Both gradients of a hidden Linear+ReLU whose input h is also its mask (drqv2.py:78-79,104-105): the one-launch
    kernel of the update where the shape allows it (multiples of 64), else a masked dgrad GEMM + wgrad GEMM."""
    B, Nout = dz.shape
    Kin = h.shape[1]
    if B % 64 == 0 and Nout % 64 == 0 and Kin % 64 == 0:
        dw = torch.empty((Nout, Kin), device=dz.device, dtype=torch.float32)
        db = torch.empty((Nout,), device=dz.device, dtype=torch.float32)
        dx = torch.empty((B, Kin), device=dz.device, dtype=torch.float32)
        pa = ops._ptr_array
        rc = _lib.load().drq_mlp_wgrad_dgrad(1, pa([dz]), Nout, pa([h]), Kin, pa([dw]), pa([db]), pa([w]), Kin, pa([dx]),
                                             Kin, pa([h]), Kin, B, Nout, Kin, _lib.current_stream())
        if rc == 0:
            return dw, db, dx
        if rc != -1:                        # -1: operands not eligible for that kernel, the GEMMs below take them
            check(rc, "drq_mlp_wgrad_dgrad")
    dw, db = ops.linear_wgrad(dz, h, ws=wsb)
    return dw, db, ops.linear_dgrad(dz, w, mask=h, ws=wsb)


class MLP3Fn(torch.autograd.Function):
    """Linear-ReLU-Linear-ReLU-Linear (drqv2.py:77-81, 103-111), with the policy's tanh (drqv2.py:89) if tanh_out."""

    @staticmethod
    def forward(ctx, keep, tanh_out, x, w0, b0, w1, b1, w2, b2):
        h1 = ops.linear_fwd(x, w0, b0, relu=True)
        h2 = ops.linear_fwd(h1, w1, b1, relu=True)
        y = ops.linear_fwd(h2, w2, b2)
        if tanh_out:
            y = ops.tanh(y)
        ctx.tanh_out = bool(tanh_out)
        if keep and any(ctx.needs_input_grad):
            ctx.save_for_backward(x, w0, w1, w2, h1, h2, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w0, w1, w2, h1, h2, y = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        wsb = _workspace(g.device)
        g = g.contiguous()
        if ctx.tanh_out:
            g = ops.tanh_bwd(y, g)
        B, H = h2.shape
        grads = [None] * 7
        # output layer; its input gradient is masked by the second ReLU
        if w2.shape[0] == 1 and (B + 1088) * 4 <= 60 * 1024:      # the Q heads' Linear(H, 1): drq_qout_bwd
            dh, dws, dbs = ops.qout_bwd([g.view(-1)], [h2], [w2.view(-1)], want_wgrad=True)
            dz2, grads[5], grads[6] = dh[0], dws[0].view(1, H), dbs[0]
        else:
            grads[5], grads[6] = ops.linear_wgrad(g, h2, ws=wsb)
            dz2 = ops.linear_dgrad(g, w2, mask=h2, ws=wsb)
        # hidden layer (its input gradient masked by the first ReLU)
        grads[3], grads[4], dz1 = _hidden_wgrad_dgrad(dz2, h1, w1, wsb)
        # first layer
        if need[1] or need[2]:
            grads[1], grads[2] = ops.linear_wgrad(dz1, x, ws=wsb)
        if need[0]:
            grads[0] = ops.linear_dgrad(dz1, w0, ws=wsb)
        return (None, None, *grads)


class RandomShiftsAugFn(torch.autograd.Function):
    """drq_aug_fwd_f32 / drq_aug_fwd (drqv2.py:19-45) with the given shift draw; differentiable in the float frame."""

    @staticmethod
    def forward(ctx, keep, x, shift, pad):
        out = ops.random_shifts_aug(x, shift, pad)
        ctx.pad = pad
        if keep and ctx.needs_input_grad[1]:
            ctx.save_for_backward(shift)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (shift,) = ctx.saved_tensors
        return None, ops.aug_bwd_f32(g.contiguous(), shift, ctx.pad), None, None


def encoder(enc, x):
    """Encoder.forward's layers on the normalised input x."""
    c = enc.convnet
    return EncoderFn.apply(torch.is_grad_enabled(), x, c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[4].weight, c[4].bias, c[6].weight,
                           c[6].bias)


def trunk(seq, x):
    return TrunkFn.apply(torch.is_grad_enabled(), x, seq[0].weight, seq[0].bias, seq[1].weight, seq[1].bias)


def mlp3(seq, x, tanh_out=False):
    return MLP3Fn.apply(torch.is_grad_enabled(), tanh_out, x, seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias,
                        seq[4].weight, seq[4].bias)


def random_shifts_aug(x, shift, pad):
    return RandomShiftsAugFn.apply(torch.is_grad_enabled(), x, shift, pad)
