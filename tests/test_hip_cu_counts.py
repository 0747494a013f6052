"""The kernels at the CU counts of a partitioned device (2 .. 128), on a whole one: drq_set_num_cus (include/drqv2_hip.h)
makes every planner of the library see a smaller count, and the rows of tests/cu_rows.py take the launch decisions that
no batch takes at 256 CUs -- the XCD remaps of the Winograd weight gradients on grids in eights, the overshoot loop and
the share walk of the three-layer weight gradient, its per-layer fallback, the sixteens remap of the Winograd forward on
small grids, the full shift table of the fused aug+conv1 launch, the second, ragged pass of the flat kernels' grid-stride
loop on a tiny tensor.  Ops run as in tests/test_hip_guarded.py: outputs poisoned, inputs between guard bands, so a
workgroup the remap skips leaves sentinels, and one that is mapped twice or reads past an operand shows as well.

Bounds are the project's: 2e-6 forward and input gradient, 3e-6 weight and bias gradient, 1e-5 bf16 on bf16-rounded
operands, all normwise against fp64.

Bit-identity across grids, decided from the kernels:
  same bits at any CU count   conv3x3_kernel (direct forward / input gradient: a wave owns whole 32-pixel tiles, the grid
                              only says which), conv3x3_wino_kernel (units and half-units have one owner whatever the grid,
                              csrc/conv_plan.h wino_deal), conv3x3_bf16_kernel (a workgroup owns whole (sample, rows)
                              units), conv1_aug_kernel (whole (frame, band) units), the flat elementwise kernels
  fp64 bound only             every weight gradient (conv3x3_wgrad_kernel, conv3x3_wgrad3_kernel,
                              conv3x3_wgrad_wino_kernel, conv3x3_wgrad_wino3_kernel, conv3x3_wgrad_bf16_kernel): one
                              partial record per workgroup, so the grid sets the length of the partial sums and the
                              number of records the reduce adds

The override is restored by the fixture's finaliser, and an autouse check holds drq_num_cus_in_effect() to the hardware
count before and after every test.  The calls under test -- agents and their workspaces included -- are made inside the
override; what they are compared with bit for bit (the same call, or the two-kernel path) runs at the hardware count.

Measured on the MI355X: the figures stand in the docstrings of the tests; no test found a defect."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_variants as cv
from tests import cu_rows
from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse)
from tests.test_hip_guarded import G, edge_shifts, err, r16, rnd

pytestmark = pytest.mark.gpu
INT_MAX = 2 ** 31 - 1
FWD, WGRAD, BF16 = 2e-6, 3e-6, 1e-5


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope="module")
def ops(lib):
    from drqv2_amd import ops as o
    return o


def hardware_cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(autouse=True)
def no_override_is_left_behind(lib):
    assert lib.drq_num_cus_in_effect() == hardware_cus()
    yield
    assert lib.drq_num_cus_in_effect() == hardware_cus()


@pytest.fixture
def cus(lib):
    """cus(n): plan with n CUs from here on (0: the hardware's again); restored when the test ends, whatever happens"""
    def set_(n):
        assert lib.drq_set_num_cus(n) == 0, n
        assert lib.drq_num_cus_in_effect() == (n or hardware_cus())
    yield set_
    lib.drq_set_num_cus(0)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ (a) the two entries
def test_entries_refuse_and_restore(lib):
    hw = hardware_cus()
    ws0 = lib.drq_conv3x3_wgrad_ws_bytes()
    sizes = lambda: (lib.drq_conv3x3_wgrad_ws_bytes(), lib.drq_step_ws_bytes(8, 9, 6, 50, 1024),
                     lib.drq_explore_knn_ws_bytes(64, 1000, 1), lib.drq_act_ws_bytes(16, 9, 6, 50, 1024))
    at_hw = sizes()
    assert all(s > 0 for s in at_hw)
    try:
        for bad in (-1, hw + 1, INT_MAX):
            assert lib.drq_set_num_cus(bad) == -1 and lib.drq_num_cus_in_effect() == hw, bad
        assert lib.drq_set_num_cus(hw) == 0 and lib.drq_num_cus_in_effect() == hw
        for n in (8, 1, 32):
            assert lib.drq_set_num_cus(n) == 0 and lib.drq_num_cus_in_effect() == n
            assert lib.drq_conv3x3_wgrad_ws_bytes() <= ws0                  # never grows
            assert sizes() == at_hw                                       # sized alike: serves launches at either count
            for bad in (-1, hw + 1, INT_MAX):                             # a refusal changes nothing
                assert lib.drq_set_num_cus(bad) == -1 and lib.drq_num_cus_in_effect() == n
        assert lib.drq_set_num_cus(0) == 0 and lib.drq_num_cus_in_effect() == hw
    finally:
        lib.drq_set_num_cus(0)


# ------------------------------------------------------------------------------------------------ (b) convolution ops
def conv_operands(cin, hin, stride, nb):
    hout = (hin - 3) // stride + 1
    return (rnd(nb, cin, hin, hin, seed=1), rnd(32, cin, 3, 3, seed=2, scale=0.2), rnd(32, seed=3, scale=0.1),
            rnd(nb, 32, hout, hout, seed=4), rnd(nb, cin, hin, hin, seed=6).clamp_min(0))


def fwd_dgrad(ops, cus, n_cus, nb, hin, stride, kw, rd, tol):
    """forward (and, for the 32->32 layers, the masked input gradient) under the override: the fp64 bound, and the bits
    of the same call at the hardware count"""
    cin = 9 if hin == 84 else 32
    x, w, b, dy, mask = conv_operands(cin, hin, stride, nb)
    xg, wg, bg = x.cuda(), w.cuda(), b.cuda()
    run = lambda: ops.conv3x3_fwd(G(x), G(w), G(b), stride, relu=True, **kw)
    cus(n_cus)
    y = run()
    cus(0)
    e = err(y, torch.relu(F.conv2d(rd(xg), rd(wg), bg.double(), stride=stride)))
    print("cus=%d nb=%d hin=%d %s fwd err=%.3e bound=%.0e" % (n_cus, nb, hin, kw, e, tol))
    assert e <= tol and same(y, run())
    if cin == 32:
        dy_pad = F.pad(dy, (2, 2, 2, 2)).contiguous()
        run = lambda: ops.conv3x3_dgrad(G(dy_pad), G(w), G(mask), **kw)
        cus(n_cus)
        dx = run()
        cus(0)
        e = err(dx, F.conv_transpose2d(rd(dy.cuda()), rd(wg)) * (mask.cuda() > 0))
        print("cus=%d nb=%d hin=%d %s dgrad err=%.3e bound=%.0e" % (n_cus, nb, hin, kw, e, tol))
        assert e <= tol and same(dx, run())


@pytest.mark.parametrize("n_cus,nb", [(8, 3), (32, 11)])
def test_direct_forward_and_input_gradient(ops, cus, n_cus, nb):
    """conv_v.rounds>1 and the capped grid at 3 and 11 frames.  Measured: forward 1.6-3.1e-7, input gradient 3.0e-7 of 2e-6; same bits as at 256 CUs"""
    for hin, stride in cu_rows.DIRECT_HIN:
        fwd_dgrad(ops, cus, n_cus, nb, hin, stride, {}, lambda t: t.double(), FWD)


@pytest.mark.parametrize("n_cus,nb", [(8, 2), (8, 3), (32, 8)])
def test_winograd_forward_and_input_gradient(ops, cus, n_cus, nb):
    """grids of 16 with the sixteens remap (8 CUs), full rounds at 3 frames; 32 CUs: 41..56 workgroups.  Measured:
    forward and input gradient 2.0e-7 of 2e-6; same bits as at 256 CUs"""
    for hin in cu_rows.WINO_HIN:
        fwd_dgrad(ops, cus, n_cus, nb, hin, 1, dict(wino=True), lambda t: t.double(), FWD)


def wgrad_case(ops, cus, n_cus, nb, cin, hin, stride, kw, rd, tol):
    x, w, _, dy, _ = conv_operands(cin, hin, stride, nb)
    dy_pad = G(F.pad(dy, (2, 2, 2, 2)).contiguous())
    cus(n_cus)
    dw, db = ops.conv3x3_wgrad(G(x), dy_pad[:, :, 2:-2, 2:-2], stride, **kw)
    cus(0)
    wd = w.cuda().double().requires_grad_(True)
    (gw,) = torch.autograd.grad(F.conv2d(rd(x.cuda()), wd, stride=stride), wd, rd(dy.cuda()))
    ew, eb = err(dw, gw), err(db, dy.double().sum((0, 2, 3)))
    print("cus=%d nb=%d cin=%d hin=%d %s dW err=%.3e bound=%.0e db err=%.3e bound=%.0e" % (n_cus, nb, cin, hin, kw, ew, tol, eb, WGRAD))
    assert ew <= tol and eb <= WGRAD


@pytest.mark.parametrize("nb", [1, 5])
@pytest.mark.parametrize("n_cus", [8, 16, 64])
def test_single_layer_winograd_weight_gradient(ops, cus, n_cus, nb):
    """grids of 8, 16 and 64 workgroups: the (G & 7) == 0 remap of conv3x3_wgrad_wino_kernel (64 CUs, 1 frame: 21..25
    workgroups, no remap).  Measured: dW 1.5-2.6e-7, db 0.8-1.4e-7 of 3e-6"""
    for hin in cu_rows.WINO_HIN:
        assert cv.launch_ww(nb, hin, n_cus).decisions["ww.xcd_remap"] == (not (n_cus == 64 and nb == 1))
        wgrad_case(ops, cus, n_cus, nb, 32, hin, 1, dict(wino=True), lambda t: t.double(), WGRAD)


@pytest.mark.parametrize("nb", [1, 3])
def test_direct_weight_gradient_with_fewer_than_16_records(ops, cus, nb):
    """8 CUs: 8 records per 32->32 layer, 11 / 16 for conv1; some of the reduce's sixteen groups never enter its loop.
    Measured: dW 1.3-2.3e-7, db 1.1-2.1e-7 of 3e-6"""
    for cin, hin, stride in ((9, 84, 2), (32, 41, 1), (32, 39, 1), (32, 37, 1)):
        wgrad_case(ops, cus, 8, nb, cin, hin, stride, {}, lambda t: t.double(), WGRAD)


@pytest.mark.parametrize("hin", [41, 37])
def test_bf16_ops_past_their_grid_cap(ops, cus, hin):
    """8 CUs, 9 frames: 27 units on grids of 16 (fp32 storage) and 24 (bf16 channel-contiguous storage), both in eights,
    so the kernel's remap is on and its unit loop runs a second, ragged round.  Measured: fwd / dgrad 8.9-9.1e-8, dW
    1.2-1.3e-7 of 1e-5, db 1.1-1.4e-7 of 3e-6; same bits as at 256 CUs"""
    nb = 9
    fwd_dgrad(ops, cus, 8, nb, hin, 1, dict(bf16=True), r16, BF16)
    wgrad_case(ops, cus, 8, nb, 32, hin, 1, dict(bf16=True), r16, BF16)
    # the channel-contiguous layout: bit for bit the fp32-storage kernels (tests/test_hip_guarded.py), under the override
    x, w, b, dy, mask = (t.cuda() for t in conv_operands(32, hin, 1, nb))
    dy_pad = F.pad(dy, (2, 2, 2, 2)).contiguous()
    y, dx = ops.conv3x3_fwd(x, w, b, 1, bf16=True), ops.conv3x3_dgrad(dy_pad, w, mask, bf16=True)
    xn, dyn, maskn = (poison.put(ops.to_nhwc_bf16(t)) for t in (x, dy_pad, mask))
    cus(8)
    yn = ops.conv3x3_fwd_bf16_nhwc(xn, G(w.cpu()), G(b.cpu()))
    y32 = ops.conv3x3_fwd_bf16_nhwc(xn, G(w.cpu()), G(b.cpu()), y_nhwc=False)
    dx32 = ops.conv3x3_dgrad_bf16_nhwc(dyn, w, maskn)
    buf = ops.conv3x3_dgrad_bf16_nhwc(dyn, w, maskn, dx_nhwc=True)
    dwp, dbp = ops.conv3x3_wgrad_bf16_nhwc(xn, dyn)
    cus(0)
    assert same(y32, y) and same(ops.from_nhwc_bf16(yn), y.to(torch.bfloat16).float()) and same(dx32, dx)
    full = ops.from_nhwc_bf16(buf)
    assert same(full[:, :, 2:-2, 2:-2], dx.to(torch.bfloat16).float())
    full[:, :, 2:-2, 2:-2] = 0
    assert not bool(full.any())
    wd = w.double().requires_grad_(True)
    (gw,) = torch.autograd.grad(F.conv2d(r16(x), wd), wd, r16(dy))
    assert err(dwp, gw) <= BF16 and err(dbp, r16(dy).sum((0, 2, 3))) <= WGRAD


# ------------------------------------------------------------------------------------------------ (c) fused aug + conv1
@pytest.mark.parametrize("n", [103, 110, 3])
def test_fused_aug_conv1_with_a_full_shift_table(ops, cus, n):
    """8 CUs: the grid outgrows its cap of 16 at 103 frames because a workgroup's shift table holds 64 units (17 and 18
    workgroups at 103 and 110 frames); 3 frames stay on the capped side.  Bit for bit the two-kernel path, as
    test_fused_aug_conv1_is_bit_identical_to_the_two_kernel_path holds at 256 CUs; the _indexed, _frames and bf16 forms
    share the launcher.  No public entry passes riders: the update's six ride in test_the_update_under_an_override."""
    la = cv.launch_conv1_aug(n, 0, 8)
    assert la.decisions["conv1_aug.table_full"] == (n >= 103) and la.grid == (-(-10 * n // 64) if n >= 103 else 16)
    g = torch.Generator().manual_seed(n)
    slots = 37
    frames = torch.randint(0, 256, (slots, 9 * 84 * 84), generator=g, dtype=torch.uint8)
    idx, idx1 = (torch.randint(0, slots, (n,), generator=g) for _ in range(2))
    idx[0], idx[1], idx1[0], idx1[-1] = 0, slots - 1, slots - 1, 0
    obs, obs1 = (frames[i].view(n, 9, 84, 84).contiguous() for i in (idx, idx1))
    sh, sh1 = edge_shifts(n), edge_shifts(n).flip(0).contiguous()
    w, b = rnd(32, 9, 3, 3, seed=5, scale=0.2), rnd(32, seed=6, scale=0.1)
    # the two-kernel path and the bf16 form at the hardware count
    x0 = ops.random_shifts_aug(obs.cuda(), sh.cuda(), 4, fuse_norm=True)
    x1 = ops.random_shifts_aug(obs1.cuda(), sh1.cuda(), 4, fuse_norm=True)
    y01 = torch.cat([ops.conv3x3_fwd(x0, w.cuda(), b.cuda(), 2), ops.conv3x3_fwd(x1, w.cuda(), b.cuda(), 2)])
    yb_hw, _ = ops.conv1_aug_fwd(obs.cuda(), sh.cuda(), obs1.cuda(), sh1.cuda(), w.cuda(), b.cuda(), n_store=2 * n, bf16=True)
    x01 = torch.cat([x0, x1])
    del x0, x1
    cus(8)
    y, xaug = ops.conv1_aug_fwd(G(obs), G(sh), G(obs1), G(sh1), G(w), G(b), n_store=2 * n)
    assert same(xaug, x01) and same(y, y01)
    del xaug
    store = G(frames)
    yi, xi = ops.conv1_aug_fwd_indexed(store, G(idx), G(sh), store, G(idx1), G(sh1), G(w), G(b), n_store=2 * n)
    assert same(yi, y01) and same(xi, x01)
    del xi
    yb, xb = ops.conv1_aug_fwd(G(obs), G(sh), G(obs1), G(sh1), G(w), G(b), n_store=2 * n, bf16=True)
    assert same(xb, x01) and same(yb, yb_hw)
    del xb
    yn, _ = ops.conv1_aug_fwd(G(obs), G(sh), G(obs1), G(sh1), G(w), G(b), n_store=2 * n, bf16=True, y_nhwc=True)
    assert same(ops.from_nhwc_bf16(yn), yb_hw.to(torch.bfloat16).float())
    # a ring of single frames: the stacks drq_vec_stack_gather finds are the reference's operands
    R, N = 8, 4
    ring = torch.randint(0, 256, (R * N, 3 * 84 * 84), generator=g, dtype=torch.uint8)
    first = (torch.rand(R * N, generator=g) < 0.2).to(torch.uint8)
    ridx, ridx1 = (torch.randint(0, R * N, (n,), generator=g) for _ in range(2))
    d_ring, d_first, d_idx, d_idx1 = G(ring), G(first), G(ridx), G(ridx1)
    for bf in (False, True):
        yf, xf = ops.conv1_aug_fwd_frames(d_ring, d_first, R, N, d_idx, G(sh), d_idx1, G(sh1), G(w), G(b), n_store=n, bf16=bf)
        cus(0)
        so, so1 = (ops.vec_stack_gather(d_ring, d_first, R, N, ix).view(n, 9, 84, 84) for ix in (d_idx, d_idx1))
        yw, xw = ops.conv1_aug_fwd(so, sh.cuda(), so1, sh1.cuda(), w.cuda(), b.cuda(), n_store=n, bf16=bf)
        cus(8)
        assert same(yf, yw) and same(xf, xw), bf
        del xf, xw
    cus(0)
    assert err(y, torch.relu(F.conv2d(x01.double(), w.cuda().double(), b.cuda().double(), stride=2))) <= FWD


# ------------------------------------------------------------------------------------------------ (d) the whole update
@pytest.mark.parametrize("row", cu_rows.CU_ROWS, ids=lambda r: "cus%d-b%d-%s" % (r.cus, r.B, r.dtype))
def test_the_update_under_an_override(cus, row):
    """The per-launch audit of tests/test_hip_encoder_audit.py with the CU count of the row: every encoder stage to its
    op bound, every gradient border exactly zero; the two-update row also to the whole-update oracle bounds of
    tests/test_hip_step.py (metrics 1e-5, features 2e-6, gradients within twice the fp32 oracle's own error).  What each
    row newly exercises is printed from cu_rows.describe(); the update's fused aug+conv1 launch carries its six riders.
    Measured on the MI355X, worst over all rows and updates:
    fp32  ACT1..3, FEAT 1.2-1.6e-7 (bound 2e-6); DY3..1 1.6-1.8e-7 (2e-6); dW1..4 1.1-1.8e-7, db1..4 0.5-1.8e-7 (3e-6)
    bf16  ACT1..3, FEAT 5.4-7.3e-8, DY3..1 6.0-7.2e-8, dW2..4 8.3-8.7e-8 (1e-5); dW1 1.1e-7, db1..4 1.3-1.6e-7 (3e-6)
    whole update (32 CUs, B = 2, two updates): every gradient within 1.9 times the fp32 oracle's own error against fp64
    (bound 2; worst 1.4e-6 normwise); every border zero; no row needed a bound of its own"""
    from tests import test_hip_encoder_audit as A
    from tests import test_hip_step as S
    print("row: " + cu_rows.describe(row))
    cfg = A.cfg_for(row.B)
    cus(row.cus)
    ag = S.make_agent(cfg)
    if row.dtype == "bf16":
        ag = ag.set_compute_dtype("bf16")
        ag._engine.step_flags = 12
    eng = ag._engine
    whole = row.updates == 2 and row.dtype == "fp32"
    o32, o64 = (S.make_oracle(cfg, dt) for dt in (torch.float32, torch.float64)) if whole else (None, None)
    bad = []
    for u in range(row.updates):
        torch.cuda.synchronize()
        w = A.read_segment(ag, eng.params)
        if whole and u > 0:
            S.sync_oracle_state(o32, ag)
            S.sync_oracle_state(o64, ag)
        m, batch, (sh_o, sh_n, n_c, n_a) = S.run_hip(ag, cfg, u)
        torch.cuda.synchronize()
        buf, grads = A.read_buffers(ag, row.B), A.read_segment(ag, eng.grads)
        v = A.verdicts(w, buf, grads, row.B, row.dtype)
        assert list(v) == A.STAGES
        for s, (e, b, ok) in v.items():
            print("audit cus=%d B=%d dtype=%s update=%d stage=%s err=%.3e bound=%.0e%s"
                  % (row.cus, row.B, row.dtype, u, s, e, b, "" if ok else "  MISS"))
            if not ok:
                bad.append((u, s, e, b))
        for l in (1, 2, 3, 4):
            border = buf[A.DY[l]].clone()
            border[:, :, 2:-2, 2:-2] = 0
            nz = int((border != 0).sum()) + int(torch.isnan(border).sum())
            if nz:
                bad.append((u, A.DY[l] + "-border", nz, 0))
        assert all(float(buf[k].abs().max()) > 0 for k in buf)
        assert all(np.isfinite(x) for x in m.values()), m
        if whole:
            B = row.B
            xin = S.check_encoder_inputs_bitwise(ag, cfg, batch, sh_o, sh_n)
            S.check_relu_decisions(ag, cfg, o64, xin[:B])
            acts, crit_masks = S.hip_masks(ag, cfg)
            critic_before = {k: t.clone() for k, t in o64.critic.items()}
            kw = dict(enc_in_override=(xin[:B], xin[B:]), keep=True, relu_masks=acts, critic_relu_masks=crit_masks)
            step = cfg["step0"] + 2 * u
            o32.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
            m64 = o64.update(batch, step, sh_o, sh_n, n_c, n_a, **kw)
            S.check_critic_decisions(o64, critic_before, crit_masks)
            for k in m64:
                assert m[k] == pytest.approx(m64[k], rel=1e-5, abs=1e-5), (u, k, m[k], m64[k])
            feat = eng.ws_view("FEAT", B, (2 * B, 39200))
            assert S.nerr(feat[:B], o64.last["feat"]) <= 2e-6 and S.nerr(feat[B:], o64.last["feat_next"]) <= 2e-6
            for nm, mod, key in (("enc", ag.encoder, "g_enc"), ("critic", ag.critic, "g_critic"), ("actor", ag.actor, "g_actor")):
                for (pn, p), g64, g32 in zip(mod.named_parameters(), o64.last[key].values(), o32.last[key].values()):
                    e_hip, e_o32 = S.nerr(p.grad, g64), S.nerr(g32, g64)
                    print("oracle cus=%d B=%d update=%d %s.%s err=%.3e fp32-oracle=%.3e" % (row.cus, B, u, nm, pn, e_hip, e_o32))
                    assert e_hip <= max(2.0 * e_o32, 2e-5 if nm != "actor" else 2e-3), (u, nm, pn, e_hip, e_o32)
    cus(0)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (e) GEMM and head families
def _smallest_gemm_rows():
    from tests import gemm_variants as gv
    small = {}
    for r in gv.TABLE:
        k, size = gv.base(r.expect), r.n * r.M * r.N * r.K
        if k not in small or size < small[k][0]:
            small[k] = (size, r)
    return [r for _, r in small.values()]


def _gemm_ids():
    from tests import gemm_variants as gv
    return [gv.row_id(r) for r in _smallest_gemm_rows()]


@pytest.mark.parametrize("n_cus", [32, 8])
@pytest.mark.parametrize("row", _smallest_gemm_rows(), ids=_gemm_ids())
def test_gemm_family_under_an_override(ops, cus, monkeypatch, row, n_cus):
    """The smallest row of each of the 28 variant families of tests/gemm_variants.py at 32 and 8 CUs, through the bodies
    of tests/test_hip_gemm_variants.py (same inputs, same poisoned buffers, same bound: gemm_variants.compare, 3e-6
    normwise and the componentwise any-order summation bound), with the prediction those bodies assert taken from
    gv.select(row, cus) instead of the 256-CU table -- so *splitk_out and *nq_out are held to the restated planner at
    the overridden count.  A family's smallest row keeps its variant at both counts except the three trunk-forward
    rows: n8-64x64x4096 leaves 4 records at 32 CUs and falls to the LDS-staged kernel without records at 8 (the only
    no-record result drq_gemm_batched_partial returns in the suite); n1-32x64x4128 and n1-32x100x4128 keep their
    kernel with 8 records for 32.  The trunk weight gradient runs on grids of 32 and 8 workgroups for 1024 / 256 at
    the hardware count.  Measured, largest error / componentwise bound over both counts: mlp_fwd 0.022, mlp_dgrad
    0.022, mlp_pair 0.024, batched 0.046 (the skinny kernel), gemm_f32 0.012, partial 5e-4; normwise at most 2.8e-7
    of 3e-6, except the trunk forward on 4 records at 32 CUs (8.2e-7: one pass over K / 4 = 1024 per record)."""
    from tests import gemm_variants as gv
    from tests import test_hip_gemm_variants as TG
    at_hw, here = gv.label(gv.select(row)), gv.label(gv.select(row, cus=n_cus))
    assert at_hw == row.expect and gv.select(row, cus=n_cus).name != gv.EARG
    print("gemm cus=%d %s: %s%s" % (n_cus, gv.row_id(row), here, "" if here == at_hw else "  (at 256 CUs: %s)" % at_hw))
    monkeypatch.setattr(TG, "predicted", lambda r: gv.select(r, cus=n_cus))
    body = {"mlp_fwd": TG.test_ring_forward, "mlp_dgrad": TG.test_ring_input_gradient, "mlp_pair": TG.test_ring_gradient_pair,
            "batched": TG.test_batched_entry, "gemm_f32": TG.test_lds_kernel_forward_misaligned,
            "partial": TG.test_trunk_forward_split_count}[row.entry]
    cus(n_cus)
    body(ops, row)
    cus(0)


@pytest.mark.parametrize("n_cus", [32, 8])
@pytest.mark.parametrize("row", cu_rows.head_rows(), ids=lambda r: "%s" % getattr(r, "mode", r))
def test_head_family_under_an_override(cus, row, n_cus):
    """The smallest row of each mode of tests/head_variants.py (fp32, bf16, bc, per) at 32 and 8 CUs through the per-launch
    head audit of tests/test_hip_head_audit.py: every stage to the bound that audit holds it to, the phased update bit
    for bit the plain one.  The ten decisions of a row are the same at both counts (tests/test_cpu_head_audit.py holds
    that to the planner); what changes is how many split-K records the trunk products leave (64 at 256 CUs; 8 / 32 at
    32 CUs, 2 / 8 at 8 CUs for the 32-row fp32 shapes), and the grids of every GEMM behind them.  Measured, largest
    error / bound over the rows and both counts (each row prints its own as head-audit-worst): trunk+LayerNorm+tanh on
    the records 0.59-0.69 of 2e-6 (0.06-0.30 at 256 CUs: fewer, longer records), everything else below 0.11, the exact
    stages 0."""
    from tests import head_variants as hv
    from tests import test_hip_head_audit as HA
    key = hv.row_id(row)
    kept = HA._cache.pop(key, None)                  # the audit's cache is keyed by the row alone: never share an entry
    cus(n_cus)
    try:
        bad = []
        for rec, _, _, _, _ in HA.audited(row):
            print("head-audit-worst cus=%d %s %s" % (n_cus, rec.tag, " ".join("%s=%.2f" % kv for kv in sorted(rec.worst.items()))))
            bad += [(rec.tag,) + b for b in rec.bad]
    finally:
        cus(0)
        HA._cache.pop(key, None)
        if kept is not None:
            HA._cache[key] = kept
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ (f) the overlapped update
def test_overlapped_update_equals_the_serial_one_at_32_cus(cus):
    """wino_overlap_budget scales with the CU count: 2 * 32 * 224 / 512 = 28 slots at 32 CUs, which plan_wino counts in
    sixteens as 16 (csrc/conv_plan.h; tests/conv_variants.py does not restate the budget), against grids of 46, 50 and
    56 workgroups at 8 rows -- the first run on a budget other than the 256-CU one.  Bit for bit the serial
    update under the same override, three updates in a row (tests/test_hip_overlap.py's feed at 8 rows)"""
    from drqv2_amd import synth
    from tests import test_hip_overlap as OV
    cfg = dict(OV.CASES["cheetah_run_b32"], B=8)
    assert [cv.launch_wino(8, h + 4, 32).grid for h in (39, 37, 35)] == [56, 50, 46]

    def run(overlap):
        ag = OV.make_agent(cfg, overlap)
        metrics = []
        for u in range(OV.UPDATES):
            batch = tuple(x.numpy() for x in synth.make_batch(cfg["B"], cfg["A"], cfg["C"], seed=cfg["bseed"] + u, smooth=cfg["smooth"]))
            draws = tuple(t.float().cuda() for t in synth.make_draws(cfg["B"], cfg["A"], seed=cfg["bseed"] + u))
            ag._draw_hook = lambda n, A, draws=draws: draws
            metrics.append(ag.update(iter([batch]), cfg["step0"] + 2 * u))
        torch.cuda.synchronize()
        e = ag._engine
        assert (e._side_handle is not None) == overlap
        return metrics, {"params": e.params.clone(), "adam_m": e.adam_m.clone(), "adam_v": e.adam_v.clone(), "grads": e.grads.clone()}

    cus(32)
    serial, overlapped, serial_2 = run(False), run(True), run(False)
    cus(0)
    assert all(np.isfinite(x) for m in serial[0] for x in m.values())
    OV.assert_same(serial, overlapped, "serial, then overlapped, at 32 CUs")
    OV.assert_same(serial, serial_2, "serial after overlapped, at 32 CUs")


# ------------------------------------------------------------------------------------------------ (g) flat kernels
def test_flat_kernels_on_a_second_ragged_pass_at_2_cus(lib, ops, cus):
    """2 CUs: one pass of the grid covers 8 * 2 * 256 = 4096 elements, so 4096 + 257 elements take a second pass with a
    ragged end on a tiny tensor.  drq_lerp_flat walks aligned operands as 16-byte vectors: its aligned case has
    4096 + 257 vectors and 3 scalars, its misaligned one 4096 + 257 scalars.  Bit for bit the references of
    tests/test_hip_entries.py / test_hip_dormant.py"""
    from oracle import drq_oracle as O
    from tests.test_hip_dormant import lerp_case
    from tests.test_hip_entries import dev, is_sent, out, p, same_bits
    n, lr, tau, step = 4096 + 257, 1e-4, 0.01, 10
    cus(2)
    p0, g = rnd(n, seed=1), rnd(n, seed=2, scale=1e-3)
    m0, v0, t0 = rnd(n, seed=3, scale=1e-3), rnd(n, seed=4, scale=1e-3) ** 2, rnd(n, seed=5)
    g[::7] = 0.0
    pk, mk, vk, tk = dev(p0, "p"), dev(m0, "m"), dev(v0, "v"), dev(t0, "target")
    assert lib.drq_adam_flat(p(pk), p(dev(g, "g")), p(mk), p(vk), n, lr, step, 1.0, None, 0.0, None) == 0
    pr, mr, vr, tr = p0.clone(), m0.clone(), v0.clone(), t0.clone()
    O.adam_step(pr, g, mr, vr, step, lr)
    assert same_bits(mk, mr) and same_bits(vk, vr) and same_bits(pk, pr)
    assert lib.drq_ema_flat(p(pk), p(tk), n, tau, None) == 0
    O.polyak(pr, tr, tau)
    assert same_bits(tk, tr) and same_bits(pk, pr)
    lerp_case(lib, 4 * n + 3, 0.9, 0, 0, special=True)               # 4096 + 257 vectors: the vector loop's second pass
    lerp_case(lib, n, 0.9, 1, 0)                                     # misaligned against each other: scalar throughout
    i = torch.arange(n)
    x = ((i + i // 256) % 256).to(torch.uint8)
    assert same_bits(ops.u8_normalize(dev(x)), x.float() / 255.0 - 0.5)
    buf = poison.partial(out(n + 7, name="fill"))
    assert lib.drq_fill(buf[3:].data_ptr(), n, 1.5, None) == 0
    assert same_bits(buf[3:3 + n], torch.full((n,), 1.5)) and bool(is_sent(buf[:3]).all()) and bool(is_sent(buf[3 + n:]).all())
    cus(0)
