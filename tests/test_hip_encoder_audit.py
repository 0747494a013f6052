"""Per-launch audit of the encoder inside the fused update.

Several convolution code paths run only from step.hip (the three-layer Winograd weight gradient, the four-job reduce,
the Winograd forward / input gradient on the U images a rider of the aug+conv1 launch prepared, conv1's deferred
weight gradient, the bf16 update's *_bf16_lay entries); the whole-update tests hold them to end-to-end bounds only.
Here ONE update() runs, its own buffers are read back through ws_view, and every encoder launch is compared with an
fp64 evaluation of that launch alone on the operands the launch actually read (the weights snapshotted before the
update, the activations and gradients the update left), at the op-level bounds of test_hip_ops.py / test_hip_bf16.py:

  fp32   forward, input gradient 2e-6 normwise; weight and bias gradient 3e-6
  bf16   (step_flags 12: activations and gradients between the layers stay fp32 NCHW) 1e-5 against fp64 on the operands
         rounded to bf16; conv1's weight gradient and every bias gradient 3e-6 on the unrounded values they sum

The batch sizes come from tests/conv_variants.py (AUDIT_ROWS, with the reason for each);
tests/test_cpu_conv_variants.py keeps them on both sides of every launch decision.  Every stage prints one line:
batch, dtype, update, stage, measured normwise error, bound."""
import pytest
import torch
import torch.nn.functional as Fn

from tests import conv_variants as cv
from tests.test_hip_step import make_agent, run_hip

pytestmark = pytest.mark.gpu

FWD, DGRAD, WGRAD, BF16 = 2e-6, 2e-6, 3e-6, 1e-5
H = cv.ENC_H                                    # 84, 41, 39, 37, 35
ACT = ("AUG", "ACT1", "ACT2", "ACT3", "FEAT")   # ACT[l] = input of layer l+1 = output of layer l
DY = (None, "DY1", "DY2", "DY3", "DY4")         # DY[l] = gradient of layer l's pre-activation, zero-padded by 2


def cfg_for(B):
    return dict(C=9, A=6, F=50, H=1024, B=B, lr=1e-4, sched="linear(1.0,0.1,500000)", wseed=20 + B % 7, bseed=200 + B,
                updates=2, step0=0, smooth=True)


def enc_slices(ag):
    """[(name, offset, shape)] of the encoder segment in parameters() order: convnet.{0,2,4,6}.{weight,bias}"""
    eng = ag._engine
    out = [(n, off, tuple(p.shape)) for (n, p), off in zip(ag.encoder.named_parameters(), eng.layout["enc"])]
    assert [n for n, _, _ in out] == ["convnet.%d.%s" % (i, k) for i in (0, 2, 4, 6) for k in ("weight", "bias")]
    return out


def read_segment(ag, arena):
    """{layer 1..4: (weight-shaped, bias-shaped)} copies out of a flat arena (eng.params or eng.grads)"""
    t = []
    for _, off, shape in enc_slices(ag):
        n = 1
        for s in shape:
            n *= s
        t.append(arena[off:off + n].view(shape).clone())
    return {l: (t[2 * l - 2], t[2 * l - 1]) for l in (1, 2, 3, 4)}


def read_buffers(ag, B):
    eng = ag._engine
    buf = {"AUG": eng.ws_view("AUG", B, (2 * B, 9, 84, 84)).clone()}
    for l in (1, 2, 3, 4):
        buf[ACT[l]] = eng.ws_view(ACT[l], B, (2 * B, 32, H[l], H[l])).clone()
        buf[DY[l]] = eng.ws_view(DY[l], B, (B, 32, H[l] + 4, H[l] + 4)).clone()
    return buf


def r16(t):
    return t.to(torch.bfloat16).double()


def stage_pairs(w, buf, grads, B, dtype, only=None):
    """yields (stage, got, fp64 reference, bound) for every encoder launch of one update: w = {layer: (weight, bias)}
    as the update read them, buf = the update's buffers, grads = {layer: (dW, db)} it left"""
    bf = dtype == "bf16"
    rd = r16 if bf else (lambda t: t.double())
    want = lambda s: only is None or s in only
    # forward, both views
    for l in (1, 2, 3, 4):
        if want(ACT[l]):
            ref = torch.relu(Fn.conv2d(rd(buf[ACT[l - 1]]), rd(w[l][0]), w[l][1].double(), stride=2 if l == 1 else 1))
            yield ACT[l], buf[ACT[l]], ref, BF16 if bf else FWD
    for l in (4, 3, 2, 1):
        dy = buf[DY[l]][:, :, 2:-2, 2:-2]
        x = buf[ACT[l - 1]][:B]
        stride = 2 if l == 1 else 1
        # input gradient of layer l -> DY[l-1], masked by the ReLU of the layer below (obs view)
        if l > 1 and want(DY[l - 1]):
            xd = torch.zeros_like(x, dtype=torch.float64).requires_grad_(True)
            (gx,) = torch.autograd.grad(Fn.conv2d(xd, rd(w[l][0])), xd, rd(dy))
            yield DY[l - 1], buf[DY[l - 1]][:, :, 2:-2, 2:-2], gx * (x > 0), BF16 if bf else DGRAD
        # weight and bias gradient of layer l (conv1's weight gradient is an fp32 kernel in the bf16 update too, and
        # every bias gradient sums the unrounded gradient)
        if want("dW%d" % l):
            rounded = bf and l > 1
            rw = r16 if rounded else (lambda t: t.double())
            wd = w[l][0].double().requires_grad_(True)
            (gw,) = torch.autograd.grad(Fn.conv2d(rw(x), wd, stride=stride), wd, rw(dy))
            yield "dW%d" % l, grads[l][0], gw, BF16 if rounded else WGRAD
        if want("db%d" % l):
            yield "db%d" % l, grads[l][1], dy.double().sum((0, 2, 3)), WGRAD


STAGES = ["ACT1", "ACT2", "ACT3", "FEAT", "DY3", "dW4", "db4", "DY2", "dW3", "db3", "DY1", "dW2", "db2", "dW1", "db1"]


def nerr(got, ref):
    """normwise error; NaN or Inf anywhere -> inf"""
    e = float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))
    return e if e == e else float("inf")


def verdicts(w, buf, grads, B, dtype, only=None):
    """{stage: (error, bound, ok)}"""
    return {s: (nerr(g, r), b, nerr(g, r) <= b) for s, g, r, b in stage_pairs(w, buf, grads, B, dtype, only)}


_cache = {}


def audited(row):
    """run the row's update(s) once: [(weights before the update, buffers after it, encoder gradients after it)]"""
    key = (row.B, row.dtype)
    if key not in _cache:
        cfg = cfg_for(row.B)
        ag = make_agent(cfg)
        if row.dtype == "bf16":
            ag = ag.set_compute_dtype("bf16")
            ag._engine.step_flags = 12
        eng = ag._engine
        out = []
        for u in range(row.updates):
            torch.cuda.synchronize()
            w = read_segment(ag, eng.params)
            run_hip(ag, cfg, u)
            torch.cuda.synchronize()
            out.append((w, read_buffers(ag, row.B), read_segment(ag, eng.grads)))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("row", cv.AUDIT_ROWS, ids=lambda r: "b%d-%s" % (r.B, r.dtype))
def test_every_encoder_launch_of_the_update_meets_its_op_bound(row):
    """B = 1 is accepted by every entry of the update.  Measured on the MI355X, worst over all rows and updates:
    fp32  ACT1..3, FEAT 1.3-1.6e-7 (bound 2e-6); DY3..1 1.7-1.8e-7 (2e-6); dW1..4 1.6-1.9e-7, db1..4 1.5-1.8e-7 (3e-6)
    bf16  ACT1..3, FEAT 5.4-8.3e-8 (1e-5); DY3..1 6.9-7.2e-8 (1e-5); dW2..4 1.2-1.4e-7 (1e-5); dW1 1.5e-7, db1..4
          1.5-2.1e-7 (3e-6); every border exactly zero"""
    bad = []
    for u, (w, buf, grads) in enumerate(audited(row)):
        v = verdicts(w, buf, grads, row.B, row.dtype)
        assert list(v) == STAGES
        for s, (e, b, ok) in v.items():
            print("audit B=%d dtype=%s update=%d stage=%s err=%.3e bound=%.0e%s"
                  % (row.B, row.dtype, u, s, e, b, "" if ok else "  MISS"))
            if not ok:
                bad.append((u, s, e, b))
        # the two-wide border of every gradient buffer is exactly zero: the Winograd weight gradient reads it as the
        # empty half of the last tile, the input gradients as the padding of the transposed convolution
        for l in (1, 2, 3, 4):
            border = buf[DY[l]].clone()
            border[:, :, 2:-2, 2:-2] = 0
            nz = int((border != 0).sum()) + int(torch.isnan(border).sum())
            print("audit B=%d dtype=%s update=%d stage=%s-border nonzero=%d" % (row.B, row.dtype, u, DY[l], nz))
            if nz:
                bad.append((u, DY[l] + "-border", nz, 0))
        # the update did something: no stage compares zeros with zeros
        assert all(float(buf[k].abs().max()) > 0 for k in buf), [k for k in buf if float(buf[k].abs().max()) == 0]
    assert not bad, bad


def test_the_comparison_rejects_one_changed_filter_tap():
    """positive control, host side only: the reference computed from a weight snapshot with ONE tap of ONE conv3 filter
    changed by 1e-3 relative must miss the bound at the stages that read conv3's weights (its forward ACT3, its input
    gradient DY2) and at no other; nothing on the GPU is perturbed"""
    row = next(r for r in cv.AUDIT_ROWS if (r.B, r.dtype) == (2, "fp32"))
    w, buf, grads = audited(row)[0]
    w3 = w[3][0].clone()
    idx = int(w3.abs().argmax())
    w3.view(-1)[idx] *= 1.0 + 1e-3
    wp = dict(w)
    wp[3] = (w3, w[3][1])
    only = ("ACT2", "ACT3", "FEAT", "DY3", "DY2", "DY1")
    good = verdicts(w, buf, grads, row.B, "fp32", only)
    pert = verdicts(wp, buf, grads, row.B, "fp32", only)
    for s in only:
        print("control stage=%s err=%.3e perturbed=%.3e bound=%.0e" % (s, good[s][0], pert[s][0], good[s][1]))
    assert all(ok for _, _, ok in good.values()), good
    assert not pert["ACT3"][2] and not pert["DY2"][2], pert
    assert pert["ACT2"][2] and pert["FEAT"][2] and pert["DY3"][2] and pert["DY1"][2], pert
