"""Every kernel family once more with its INPUTS between guard bands of NaN (tests/poison.py: put) and its outputs
poisoned, at one ragged and one training-size shape each.  Same fp64 references and the same bounds as the tests of
the same kernels in test_hip_ops.py / test_hip_bf16.py / test_hip_mlp.py / test_hip_rowblock.py.

What this adds: a load past the end (or before the start) of an operand reads NaN here, not the allocator's rounding
slack or a finite neighbour.  If the value is USED -- even multiplied by a zero weight instead of being masked -- the
result is NaN and the comparison fails; a value that is loaded and discarded changes nothing.  Operands whose border
a kernel reads by contract (the zero-padded gradient buffers, include/drqv2_hip.h) are guarded as the whole padded
buffer.  Every case stays inside its own allocation, guards included."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from drqv2_amd import ops as o, _lib
    _lib.load()
    assert torch.cuda.is_available()
    return o


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def G(t):
    """the tensor on the GPU between two guard bands"""
    return poison.put(t, "cuda")


def err(a, b):
    """normwise error against an fp64 reference (on either device)"""
    a = a.detach().double()
    b = b.detach().double().to(a.device)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def r16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def positive_control_inputs(hin, nb):
    return rnd(nb, 32, hin, hin, seed=1), rnd(32, 32, 3, 3, seed=2, scale=0.2), rnd(32, seed=3, scale=0.1)


def test_positive_control_a_short_write_is_reported_exactly(ops):
    """The harness on the GPU: drq_conv3x3_fwd asked for nb - 1 frames into a poisoned nb-frame output, right after a
    full, correct call of the same shape (whose freed result is what torch.empty would hand out next).  check() must
    report the last frame's 32*hout^2 elements as unwritten, and nothing else."""
    hin, nb = 39, 4
    hout = hin - 2
    x, w, b = (G(t) for t in positive_control_inputs(hin, nb))
    y_full = ops.conv3x3_fwd(x, w, b, 1)
    poison.check()
    ref = y_full.clone()
    poison.forget(y_full)
    del y_full
    y = poison.alloc((nb, 32, hout, hout), torch.float32, "cuda", name="y (short call)")
    lib = ops._lib.load()
    rc = lib.drq_conv3x3_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), nb - 1, 32, hin, 1, 1, 32 * hout * hout,
                             hout * hout, hout, 0, None)
    assert rc == 0
    (f,) = poison.report()
    assert f.name.startswith("y (short call)") and "never written" in f.what
    assert f.count == 32 * hout * hout
    assert f.first[0] == ((nb - 1) * 32 * hout * hout, (nb - 1, 0, 0, 0)) and f.last == (nb * 32 * hout * hout - 1, (nb - 1, 31, hout - 1, hout - 1))
    with pytest.raises(AssertionError, match="never written"):
        poison.check()
    assert torch.equal(y[:nb - 1], ref[:nb - 1])
    poison.forget(y)


# ------------------------------------------------------------------------------------------------ convolutions
CONV = [(37, 3), (41, 1), (39, 256)]          # ragged tiles / ragged last unit; a training batch


@pytest.mark.parametrize("form", ["direct", "wino", "bf16"])
@pytest.mark.parametrize("hin,nb", CONV)
def test_conv_fwd_dgrad_wgrad_guarded(ops, form, hin, nb):
    kw = dict(wino=form == "wino", bf16=form == "bf16")
    rd = r16 if form == "bf16" else (lambda t: t.double())
    big = nb >= 64            # test_conv_kernels_at_training_batch_sizes holds the direct weight gradient to 3e-6 there
    tol, tol_w = (1e-5, 1e-5) if form == "bf16" else (2e-6, 2e-6 if form == "direct" and not big else 3e-6)
    hout = hin - 2
    x, w, b = rnd(nb, 32, hin, hin, seed=1), rnd(32, 32, 3, 3, seed=2, scale=0.2), rnd(32, seed=3, scale=0.1)
    dy = rnd(nb, 32, hout, hout, seed=4)
    mask = rnd(nb, 32, hin, hin, seed=6).clamp_min(0)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()                    # for the fp64 references, on the GPU
    # forward
    y = ops.conv3x3_fwd(G(x), G(w), G(b), 1, relu=True, **kw)
    assert err(y, torch.relu(F.conv2d(rd(xg), rd(wg), bg.double()))) <= tol
    y0 = ops.conv3x3_fwd(G(x), G(w), G(b), 1, relu=False, **kw)
    assert err(y0, F.conv2d(rd(xg), rd(wg), bg.double())) <= tol
    # input gradient: the padded gradient buffer and the mask between guards
    dy_pad = G(F.pad(dy, (2, 2, 2, 2)).contiguous())
    dx = ops.conv3x3_dgrad(dy_pad, G(w), G(mask), **kw)
    gx = F.conv_transpose2d(rd(dy.cuda()), rd(wg))
    assert err(dx, gx * (mask.cuda() > 0)) <= tol
    if form != "bf16":                                           # the bf16 entry takes no NULL mask
        assert err(ops.conv3x3_dgrad(dy_pad, G(w), None, **kw), gx) <= tol
    if form == "wino":                                           # the padded destination of the update
        dxp = ops.conv3x3_dgrad(dy_pad, G(w), G(mask), wino=True, pad_out=True)
        assert torch.equal(dxp[:, :, 2:-2, 2:-2], dx)
        brd = dxp.clone()
        brd[:, :, 2:-2, 2:-2] = 0
        assert not bool(brd.any())
    # weight gradient: dy is the interior of the padded buffer (the Winograd and bf16 forms read its zero border by contract)
    dw, db = ops.conv3x3_wgrad(G(x), dy_pad[:, :, 2:-2, 2:-2], 1, **kw)
    wd = wg.double().requires_grad_(True)
    (gw,) = torch.autograd.grad(F.conv2d(rd(xg), wd), wd, rd(dy.cuda()))
    assert err(dw, gw) <= tol_w
    assert err(db, dy.double().sum((0, 2, 3))) <= (2e-6 if form == "direct" and not big else 3e-6)


@pytest.mark.parametrize("nb", [3, 256])
def test_conv1_direct_guarded(ops, nb):
    x, w, b = rnd(nb, 9, 84, 84, seed=1), rnd(32, 9, 3, 3, seed=2, scale=0.2), rnd(32, seed=3, scale=0.1)
    dy = rnd(nb, 32, 41, 41, seed=8)
    y = ops.conv3x3_fwd(G(x), G(w), G(b), 2)
    assert err(y, torch.relu(F.conv2d(x.cuda().double(), w.cuda().double(), b.cuda().double(), stride=2))) <= 2e-6
    dy_pad = G(F.pad(dy, (2, 2, 2, 2)).contiguous())
    dw, db = ops.conv3x3_wgrad(G(x), dy_pad[:, :, 2:-2, 2:-2], 2)
    wd = w.cuda().double().requires_grad_(True)
    (gw,) = torch.autograd.grad(F.conv2d(x.cuda().double(), wd, stride=2), wd, dy.cuda().double())
    tol = 2e-6 if nb < 64 else 3e-6      # test_conv_wgrad / test_conv_kernels_at_training_batch_sizes
    assert err(dw, gw) <= tol and err(db, dy.double().sum((0, 2, 3))) <= tol


@pytest.mark.parametrize("hin,nb", [(37, 3), (41, 130)])
def test_conv_bf16_channel_contiguous_guarded(ops, hin, nb):
    """the bf16 [frame][y][x][32] layout: operands in that layout between guards (2-byte NaN), bit for bit the
    fp32-storage kernels"""
    hout = hin - 2
    x, w, b = rnd(nb, 32, hin, hin, seed=1).cuda(), rnd(32, 32, 3, 3, seed=2, scale=0.1).cuda(), rnd(32, seed=3, scale=0.1).cuda()
    xn = poison.put(ops.to_nhwc_bf16(x))
    y = ops.conv3x3_fwd(x, w, b, 1, bf16=True)
    assert torch.equal(ops.conv3x3_fwd_bf16_nhwc(xn, G(w.cpu()), G(b.cpu()), y_nhwc=False), y)
    assert torch.equal(ops.from_nhwc_bf16(ops.conv3x3_fwd_bf16_nhwc(xn, G(w.cpu()), G(b.cpu()))), y.to(torch.bfloat16).float())
    dy_pad = F.pad(rnd(nb, 32, hout, hout, seed=4), (2, 2, 2, 2)).contiguous().cuda()
    mask = torch.relu(rnd(nb, 32, hin, hin, seed=5)).cuda()
    dx = ops.conv3x3_dgrad(dy_pad, w, mask, bf16=True)
    dyn, maskn = poison.put(ops.to_nhwc_bf16(dy_pad)), poison.put(ops.to_nhwc_bf16(mask))
    assert torch.equal(ops.conv3x3_dgrad_bf16_nhwc(dyn, w, maskn), dx)
    buf = ops.conv3x3_dgrad_bf16_nhwc(dyn, w, maskn, dx_nhwc=True)
    full = ops.from_nhwc_bf16(buf)
    assert torch.equal(full[:, :, 2:-2, 2:-2], dx.to(torch.bfloat16).float())
    full[:, :, 2:-2, 2:-2] = 0
    assert not bool(full.any())
    dw, _ = ops.conv3x3_wgrad(x, dy_pad[:, :, 2:-2, 2:-2], 1, bf16=True)
    dwp, dbp = ops.conv3x3_wgrad_bf16_nhwc(xn, dyn)
    assert torch.equal(dwp, dw)
    assert err(dbp, r16(dy_pad).sum((0, 2, 3))) <= 3e-6


# ------------------------------------------------------------------------------------------------ augmentation, fused conv1
def edge_shifts(n):
    sh = torch.from_numpy(np.random.RandomState(n).randint(0, 9, (n, 2)).astype(np.float32))
    corners = torch.tensor([[0, 0], [8, 8], [0, 8], [8, 0]], dtype=torch.float32)
    sh[:min(n, 4)] = corners[:min(n, 4)]
    return sh


@pytest.mark.parametrize("n,c", [(4, 9), (5, 2), (64, 9)])
def test_random_shifts_aug_guarded(ops, n, c):
    """shifts 0 and 8 on both axes: the clamped taps at the frame edges; uint8 and float frames; the input gradient"""
    from oracle import drq_oracle as O
    obs = torch.from_numpy(np.random.RandomState(c).randint(0, 256, (n, c, 84, 84)).astype(np.uint8))
    sh = edge_shifts(n)
    out = ops.random_shifts_aug(G(obs), G(sh), 4)
    ora = O.random_shifts_aug(obs.float(), sh.int(), 4)
    assert torch.equal(out.cpu(), ora)
    assert torch.equal(ops.random_shifts_aug(G(obs.float()), G(sh), 4).cpu(), ora)
    assert torch.equal(ops.random_shifts_aug(G(obs), G(sh), 4, fuse_norm=True).cpu(), ora / 255.0 - 0.5)
    assert torch.equal(out.cpu().round(), O.aug_integer_crop(obs.float(), sh.int()))
    # the adjoint of the same taps "with the forward's own fp32 weights" (include/drqv2_hip.h).  Reference: autograd
    # through the oracle in fp32, whose forward is the kernel's bit for bit (above), so whose weights are those weights:
    # 2e-6, the suite's fp32 floor (either side adds at most a few dozen fp32 products per element).  Against the fp64
    # adjoint the distance is that of the weights themselves: the fp32 grid coordinate (values up to 92) leaves each
    # weight a few 1e-6 off 0 / 1, which test_aug_vs_oracle_and_reference allows the forward as 4e-3 on the 0..255
    # scale; the same fraction of full scale, 4e-3 / 255, here.
    dy = rnd(n, c, 84, 84, seed=7)
    dx = ops.aug_bwd_f32(G(dy), G(sh), 4)
    x32 = obs.float().requires_grad_(True)
    (O.random_shifts_aug(x32, sh.int(), 4) * dy).sum().backward()
    xd = obs.double().requires_grad_(True)
    (O.random_shifts_aug(xd, sh.int(), 4) * dy.double()).sum().backward()
    print(f"aug_bwd n={n} c={c}: vs fp32-weight adjoint {err(dx, x32.grad):.3e}, vs fp64 adjoint {err(dx, xd.grad):.3e}")
    assert err(dx, x32.grad) <= 2e-6
    assert err(dx, xd.grad) <= 4e-3 / 255


@pytest.mark.parametrize("n", [3, 200])
def test_fused_aug_conv1_guarded(ops, n):
    g = torch.Generator().manual_seed(n)
    obs = torch.randint(0, 256, (n, 9, 84, 84), generator=g, dtype=torch.uint8)
    obs1 = torch.randint(0, 256, (n, 9, 84, 84), generator=g, dtype=torch.uint8)
    sh, sh1 = edge_shifts(n), edge_shifts(n).flip(0).contiguous()
    w, b = rnd(32, 9, 3, 3, seed=5, scale=0.2), rnd(32, seed=6, scale=0.1)
    y, xaug = ops.conv1_aug_fwd(G(obs), G(sh), G(obs1), G(sh1), G(w), G(b), n_store=2 * n)
    x0 = ops.random_shifts_aug(obs.cuda(), sh.cuda(), 4, fuse_norm=True)
    x1 = ops.random_shifts_aug(obs1.cuda(), sh1.cuda(), 4, fuse_norm=True)
    assert torch.equal(xaug[:n], x0) and torch.equal(xaug[n:], x1)
    assert torch.equal(y[:n], ops.conv3x3_fwd(x0, w.cuda(), b.cuda(), 2)) and torch.equal(y[n:], ops.conv3x3_fwd(x1, w.cuda(), b.cuda(), 2))
    ref = torch.relu(F.conv2d(torch.cat([x0, x1]).double(), w.cuda().double(), b.cuda().double(), stride=2))
    assert err(y, ref) <= 2e-6
    yb, xb = ops.conv1_aug_fwd(G(obs), G(sh), G(obs1), G(sh1), G(w), G(b), n_store=2 * n, bf16=True)
    assert torch.equal(xb, xaug)
    assert err(yb, torch.relu(F.conv2d(r16(xaug), r16(w.cuda()), b.cuda().double(), stride=2))) <= 1e-5
    yn, _ = ops.conv1_aug_fwd(G(obs), G(sh), G(obs1), G(sh1), G(w), G(b), n_store=2 * n, bf16=True, y_nhwc=True)
    assert torch.equal(ops.from_nhwc_bf16(yn), yb.to(torch.bfloat16).float())


@pytest.mark.parametrize("slots,n", [(5, 7), (300, 200)])
def test_fused_aug_conv1_indexed_guarded(ops, slots, n):
    """the frame store between guards; the indices touch slot 0 and the last slot"""
    r = np.random.RandomState(slots)
    frames = torch.from_numpy(r.randint(0, 256, (slots, 9 * 84 * 84)).astype(np.uint8))
    idx, idx1 = (torch.from_numpy(r.randint(0, slots, n).astype(np.int64)) for _ in range(2))
    idx[0], idx[1], idx1[0], idx1[-1] = 0, slots - 1, slots - 1, 0
    sh, sh1 = edge_shifts(n), edge_shifts(n).flip(0).contiguous()
    w, b = rnd(32, 9, 3, 3, seed=5, scale=0.2), rnd(32, seed=6, scale=0.1)
    store = G(frames)
    y1, x1 = ops.conv1_aug_fwd_indexed(store, G(idx), G(sh), store, G(idx1), G(sh1), G(w), G(b), n_store=2 * n)
    obs, obs1 = (frames[i].view(n, 9, 84, 84).contiguous().cuda() for i in (idx, idx1))
    y0, x0 = ops.conv1_aug_fwd(obs, sh.cuda(), obs1, sh1.cuda(), w.cuda(), b.cuda(), n_store=2 * n)
    assert torch.equal(y0, y1) and torch.equal(x0, x1)
    assert err(y1, torch.relu(F.conv2d(x0.double(), w.cuda().double(), b.cuda().double(), stride=2))) <= 2e-6


# ------------------------------------------------------------------------------------------------ GEMMs
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M,N,K,n", [(33, 21, 130, 3), (70, 100, 56, 2), (256, 1024, 1024, 2)])
def test_gemm_batched_three_layouts_guarded(ops, M, N, K, n, bf16):
    rd = r16 if bf16 else (lambda t: t.double())
    tol = 1e-5 if bf16 else 3e-6
    xs = [rnd(M, K, seed=1 + i) for i in range(n)]
    ws = [rnd(N, K, seed=11 + i, scale=K ** -0.5) for i in range(n)]
    bs = [rnd(N, seed=21 + i) for i in range(n)]
    dys = [rnd(M, N, seed=31 + i) for i in range(n)]
    mks = [rnd(M, K, seed=41 + i) for i in range(n)]
    Gs = lambda ts: [G(t) for t in ts]
    ys, _ = ops.gemm_batched(Gs(xs), True, Gs(ws), True, M, N, K, K, K, biases=Gs(bs), relu=True, bf16=bf16)
    dxs, _ = ops.gemm_batched(Gs(dys), True, Gs(ws), False, M, K, N, N, K, auxs=Gs(mks), bf16=bf16)
    dws, dbs = ops.gemm_batched(Gs(dys), False, Gs(xs), False, N, K, M, N, K, rowsum=True, bf16=bf16)
    for i in range(n):
        assert err(ys[i], torch.relu(rd(xs[i]) @ rd(ws[i]).T + bs[i].double())) <= tol
        assert err(dxs[i], (rd(dys[i]) @ rd(ws[i])) * (mks[i].double() > 0)) <= tol
        assert err(dws[i], rd(dys[i]).T @ rd(xs[i])) <= tol
        assert err(dbs[i], dys[i].double().sum(0)) <= 3e-6


@pytest.mark.parametrize("M,K,hw", [(33, 21, 16), (256, 50, 35)])
def test_skinny_trunk_dgrad_and_scatter_guarded(ops, M, K, hw):
    N = 32 * hw * hw
    dz, w, mask = rnd(M, K, seed=1), rnd(K, N, seed=2, scale=K ** -0.5), rnd(M, N, seed=3)
    ref = (dz.cuda().double() @ w.cuda().double()) * (mask.cuda().double() > 0)
    args = lambda: ([G(dz)], True, [G(w)], False, M, N, K, K, N)
    (c_fast,), _ = ops.gemm_batched(*args(), auxs=[G(mask)])
    (c_gen,), _ = ops.gemm_batched(*args(), auxs=[G(mask)], tile=2, splitk=1)
    assert err(c_fast, ref) <= 3e-6 and err(c_gen, ref) <= 3e-6
    hp = hw + 4
    for kw in (dict(), dict(tile=2, splitk=1)) + ((dict(bf16=True),) if hw == 35 else ()):
        pad = poison.alloc((M, 32, hp, hp), torch.float32, "cuda", name=f"scatter {kw}", kind="zero")
        ops.gemm_batched(*args(), auxs=[G(mask)], scatter_hw=hw, Cs=[pad], **kw)
        want = (r16(dz.cuda()) @ r16(w.cuda())) * (mask.cuda().double() > 0) if kw.get("bf16") else ref
        assert err(pad[:, :, 2:-2, 2:-2].reshape(M, N), want) <= (1e-5 if kw.get("bf16") else 3e-6)
        border = pad.clone()
        border[:, :, 2:-2, 2:-2] = 0
        assert not bool(border.any())


@pytest.mark.parametrize("M,N,K,n", [(96, 7, 8192, 3), (64, 65, 4096, 2), (32, 100, 39200, 1), (256, 50, 39200, 4)])
def test_trunk_forward_partials_guarded(ops, M, N, K, n):
    """weight rows past N read as zero: with NaN behind the last weight row, "read and multiplied by zero" fails"""
    xs = [rnd(M, K, seed=i) for i in range(n)]
    wts = [rnd(N, K, seed=5 + i, scale=K ** -0.5) for i in range(n)]
    got, sk = ops.gemm_batched_partial([G(x) for x in xs], [G(w) for w in wts], M, N, K, K, K)
    assert sk > 1
    for i in range(n):
        assert err(got[i], xs[i].cuda().double() @ wts[i].cuda().double().t()) <= 3e-6


@pytest.mark.parametrize("n,M,N,K", [(3, 128, 192, 128), (2, 256, 1024, 1024)])
def test_mlp_kernels_guarded(ops, n, M, N, K):
    xs = [rnd(M, K, seed=10 + i) for i in range(n)]
    ws = [rnd(N, K, seed=20 + i, scale=K ** -0.5) for i in range(n)]
    bs = [rnd(N, seed=30 + i) for i in range(n)]
    qw = [rnd(N, seed=40 + i, scale=N ** -0.5) for i in range(n)]
    Gs = lambda ts: [G(t) for t in ts]
    ys, qps = ops.mlp_fwd(Gs(xs), Gs(ws), Gs(bs), relu=True, qws=Gs(qw))
    for i in range(n):
        ref = torch.relu(xs[i].double() @ ws[i].double().t() + bs[i].double())
        assert err(ys[i], ref) <= 3e-6
        nq = qps[i].shape[1]
        part_ref = (ref * qw[i].double()).view(M, nq, N // nq).sum(2)
        assert float((qps[i].double().cpu() - part_ref).abs().max() / part_ref.abs().max()) <= 3e-6
    # dgrad: dx [M][K] = dy [M][N] w [N][K], masked
    dys, mk = [rnd(M, N, seed=50 + i) for i in range(n)], [rnd(M, K, seed=60 + i) for i in range(n)]
    dxs = ops.mlp_dgrad(Gs(dys), Gs(ws), Gs(mk))
    for i in range(n):
        assert err(dxs[i], (dys[i].double() @ ws[i].double()) * (mk[i] > 0).double()) <= 3e-6
    # both gradients of the layer in one launch; the mask is the layer's (post-ReLU) input
    xr = [x.clamp_min(0) for x in xs]
    xg = Gs(xr)
    dws, dbs, dx2 = ops.mlp_wgrad_dgrad(Gs(dys), xg, Gs(ws), xg)
    for i in range(n):
        assert err(dws[i], dys[i].double().t() @ xr[i].double()) <= 3e-6
        assert err(dbs[i], dys[i].double().sum(0)) <= 3e-6
        assert err(dx2[i], (dys[i].double() @ ws[i].double()) * (xr[i] > 0).double()) <= 3e-6


@pytest.mark.parametrize("B,H,n", [(7, 100, 2), (1030, 100, 1), (7, 1024, 1), (1030, 1024, 2)])
def test_qout_guarded(ops, B, H, n):
    hs = [rnd(B, H, seed=i).clamp_min(0) for i in range(n)]
    ws_ = [rnd(H, seed=10 + i, scale=H ** -0.5) for i in range(n)]
    bs = [rnd(1, seed=20 + i) for i in range(n)]
    dqs = [rnd(B, seed=30 + i) for i in range(n)]
    Gs = lambda ts: [G(t) for t in ts]
    qs = ops.qout_fwd(Gs(hs), Gs(ws_), Gs(bs))
    dhs, dws, dbs = ops.qout_bwd(Gs(dqs), Gs(hs), Gs(ws_))
    for i in range(n):
        assert err(qs[i], hs[i].double() @ ws_[i].double() + bs[i].double()) <= 2e-6
        assert err(dhs[i], torch.outer(dqs[i].double(), ws_[i].double()) * (hs[i] > 0).double()) <= 2e-6
        assert err(dws[i], dqs[i].double() @ hs[i].double()) <= 3e-6
        assert err(dbs[i], dqs[i].double().sum().view(1)) <= 3e-6


# ------------------------------------------------------------------------------------------------ row-local stages
def ln64(z, g, b):
    return torch.tanh(F.layer_norm(z.double(), (z.shape[1],), g.double(), b.double(), 1e-5))


@pytest.mark.parametrize("rows,Fd", [(7, 100), (5, 256), (256, 50)])
def test_ln_tanh_guarded(ops, rows, Fd):
    z, g, b, dh = rnd(rows, Fd, seed=1, scale=2.0), 1 + 0.1 * rnd(Fd, seed=2), 0.1 * rnd(Fd, seed=3), rnd(rows, Fd, seed=4)
    h, xhat, rstd = ops.ln_tanh_fwd(G(z), G(g), G(b))
    zd, gd, bd = (t.double().requires_grad_(True) for t in (z, g, b))
    ref = ln64(zd, gd, bd)
    assert err(h, ref) <= 2e-6
    (ref * dh.double()).sum().backward()
    dz, dg, dbeta = ops.ln_tanh_bwd(G(dh), poison.put(h), poison.put(xhat), poison.put(rstd), G(g))
    assert err(dz, zd.grad) <= 1e-5 and err(dg, gd.grad) <= 1e-5 and err(dbeta, bd.grad) <= 1e-5


@pytest.mark.parametrize("rows,Fd,splitk", [(7, 50, 3), (32, 50, 37), (256, 100, 16)])
def test_ln_l1_from_split_k_records_guarded(ops, rows, Fd, splitk):
    """the 16-slab batches of sum_partials load slab min(k, splitk - 1) for k >= splitk and must not add it"""
    H = 256
    parts = rnd(2, splitk, rows, Fd, seed=5)
    bias = [rnd(Fd, seed=6), rnd(Fd, seed=7)]
    g, bt = 1 + 0.1 * rnd(Fd, seed=8), 0.1 * rnd(Fd, seed=9)
    w, b = rnd(H, Fd, seed=11, scale=Fd ** -0.5), rnd(H, seed=12)
    pc = G(parts)
    jobs = [dict(part=pc[0], bias=G(bias[0]), gamma=G(g), beta=G(bt), rows=rows, heads=[(G(w), G(b))]),
            dict(part=pc[1], bias=G(bias[1]), gamma=G(g), beta=G(bt), rows=rows)]
    res = ops.ln_l1_fwd(jobs, Fd, H, splitk=splitk, slab=rows * Fd)
    for j in range(2):
        assert err(res[j]["out"], ln64(parts[j].double().sum(0) + bias[j].double(), g, bt)) <= 2e-6
    assert err(res[0]["ys"][0], torch.relu(res[0]["out"].double().cpu() @ w.double().t() + b.double())) <= 3e-6


@pytest.mark.parametrize("rows,Fd,A,H", [(19, 50, 1, 256), (5, 64, 3, 64), (256, 50, 6, 1024)])
def test_ln_l1_guarded(ops, rows, Fd, A, H):
    z = [rnd(rows, Fd, seed=s, scale=3.0) for s in (1, 2)]
    g = [1 + 0.1 * rnd(Fd, seed=10 + s) for s in range(2)]
    bt = [0.1 * rnd(Fd, seed=20 + s) for s in range(2)]
    act = rnd(rows, A, seed=4)
    wq = [rnd(H, Fd + A, seed=30 + h, scale=(Fd + A) ** -0.5) for h in range(2)]
    bq = [rnd(H, seed=40 + h) for h in range(2)]
    wp, bp = rnd(H, Fd, seed=50, scale=Fd ** -0.5), rnd(H, seed=51)
    jobs = [dict(z=G(z[0]), gamma=G(g[0]), beta=G(bt[0]), rows=rows, tail=G(act), heads=[(G(wq[0]), G(bq[0])), (G(wq[1]), G(bq[1]))]),
            dict(z=G(z[1]), gamma=G(g[1]), beta=G(bt[1]), rows=rows, heads=[(G(wp), G(bp))])]
    res = ops.ln_l1_fwd(jobs, Fd, H)
    for j in range(2):
        h, xh, rs = ops.ln_tanh_fwd(z[j].cuda(), g[j].cuda(), bt[j].cuda())
        assert torch.equal(res[j]["out"][:, :Fd], h) and torch.equal(res[j]["xhat"], xh) and torch.equal(res[j]["rstd"], rs)
        assert err(h, ln64(z[j], g[j], bt[j])) <= 1e-6
    assert torch.equal(res[0]["out"][:, Fd:], act.cuda())
    x0 = torch.cat([res[0]["out"][:, :Fd].double().cpu(), act.double()], 1)
    for hd in range(2):
        assert err(res[0]["ys"][hd], torch.relu(x0 @ wq[hd].double().t() + bq[hd].double())) <= 3e-6
    assert err(res[1]["ys"][0], torch.relu(res[1]["out"].double().cpu() @ wp.double().t() + bp.double())) <= 3e-6


@pytest.mark.parametrize("B,Fd,A,H", [(19, 50, 1, 256), (256, 50, 6, 1024)])
def test_policy_out_l1_guarded(ops, B, Fd, A, H):
    p2 = torch.relu(rnd(2 * B, H, seed=1))
    w3, b3 = rnd(A, H, seed=2, scale=H ** -0.5), rnd(A, seed=3)
    nz_hi, nz_lo = rnd(B, A, seed=4), rnd(B, A, seed=5)
    h_t = torch.tanh(rnd(B, Fd, seed=6))
    wq = [rnd(H, Fd + A, seed=30 + h, scale=(Fd + A) ** -0.5) for h in range(2)]
    bq = [rnd(H, seed=40 + h) for h in range(2)]
    ha_hi = G(torch.cat([h_t, torch.zeros(B, A)], 1))
    ha_lo = G(torch.zeros(B, Fd + A))
    std, clip = 0.7, 0.3
    r = ops.policy_out_l1_fwd(G(p2), G(w3), G(b3), B, Fd, std, clip, G(nz_hi), ha_hi, G(nz_lo), ha_lo,
                              heads=[(G(wq[0]), G(bq[0])), (G(wq[1]), G(bq[1]))])
    assert err(r["p3"], p2.double() @ w3.double().t() + b3.double()) <= 3e-6
    mu_hi, a_hi = ops.trunc_normal_sample(r["p3"][B:].contiguous(), nz_hi.cuda(), std, clip)
    mu_lo, a_lo = ops.trunc_normal_sample(r["p3"][:B].contiguous(), nz_lo.cuda(), std, clip)
    assert torch.equal(r["mu_hi"], mu_hi) and torch.equal(ha_hi[:, Fd:], a_hi)
    assert torch.equal(r["mu_lo"], mu_lo) and torch.equal(ha_lo[:, Fd:], a_lo)
    assert torch.equal(ha_hi[:, :Fd], h_t.cuda())
    x = ha_hi.double().cpu()
    for hd in range(2):
        assert err(r["ys"][hd], torch.relu(x @ wq[hd].double().t() + bq[hd].double())) <= 3e-6
