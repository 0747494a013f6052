"""Direct tests of the exported entries that were reached only through whole-update tests (or only on two ranks):
each is called through the C ABI with every input between guard bands and every output poisoned (tests/poison.py),
and compared with an fp64 reference on the CPU, or bit for bit where the entry promises that.

Bounds.  Normwise 2e-6 / 3e-6 / 1e-5 are the ones the op suite already holds the same kernels to.
The metric sums of drq_td_mse / drq_actor_loss are fixed-order fp32 sums of n terms -- per thread ceil(n/256) serial
adds, then an 8-level tree -- and are held to the standard bound of that summation order with 4 roundings allowed for
forming a term:  |s_hip - s_fp64| <= (ceil(n/256) + 8 + 4) * 2**-24 * sum|term_fp64|.  Derived, not measured.

Where each export of include/drqv2_hip.h (the list of tests/test_cpu_interface.py) meets an fp64 or bit-exact reference:
  here            td_mse, actor_loss, actor_dmu, colsum, copy_cols, fill, u8_normalize, tanh, tanh_bwd, relu_mask_pad,
                  trunc_normal_sample, ln_tanh_fwd / fwd2 / fwd_multi / bwd, sum_slices, adam_reduce_flat, adam_flat,
                  ema_flat, gemm_f32 (nbatch > 1), publish_sums
  test_hip_guarded   aug_fwd, aug_fwd_f32, aug_bwd_f32, conv1_aug_fwd (+ _bf16, _bf16_nhwc, _indexed), conv3x3_fwd / dgrad /
  (and test_hip_ops, wgrad (+ _wino, _bf16, _bf16_nhwc), conv3x3_wgrad_ws_bytes, gemm_batched_f32 / _bf16 / _partial, mlp_fwd /
  _bf16, _mlp,       dgrad / wgrad_dgrad, qout_fwd / bwd, ln_l1_fwd, policy_out_l1_fwd
  _rowblock)
  test_hip_autograd  conv1_dgrad;  test_hip_replay  nstep_gather;  test_hip_act_batch  act_batch, act_ws_bytes
  test_hip_step      update_phase, act_forward, rng_draws, param_layout, step_ws_bytes, step_ws_offset (whole updates
                     against the oracle);  abi_version: checked at every load (drqv2_amd/_lib.py)"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse: drqv2_amd.ops allocates poisoned memory; check() after every test)

pytestmark = pytest.mark.gpu
EARG = -1
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope="module")
def ops():
    from drqv2_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cap():
    """elements one launch of the flat elementwise kernels covers before its grid-stride loop starts"""
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256


def rs_(seed):
    return np.random.RandomState(seed)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def rnd(*shape, seed=0, scale=1.0, mean=0.0):
    return f32(rs_(seed).standard_normal(shape) * scale + mean)


def nerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def dev(t, name=None):
    return poison.put(t, "cuda", name=name)


def out(*shape, dtype=torch.float32, name=None):
    return poison.alloc(shape, dtype, "cuda", name=name)


def wide(rows, ld, name=None, kind="in"):
    """a [rows][ld] buffer full of the sentinel: the caller fills the columns an entry may touch, the rest is gap"""
    return poison.alloc((rows, ld), torch.float32, "cuda", name=name, kind=kind)


def is_sent(t):
    return t.contiguous().view(torch.int32) == poison.SENTINEL


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def p(t):
    return None if t is None else t.data_ptr()


def sum_bound(n, terms64):
    return (math.ceil(n / 256) + 8 + 4) * U * float(terms64.abs().sum())


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("centre", [5.0, -5.0, 0.0])
@pytest.mark.parametrize("dp", [1, 2])
@pytest.mark.parametrize("B", [1, 7, 255, 256, 257, 2048])
def test_td_mse(lib, B, dp, centre):
    """drq_td_mse (drqv2.py:185-189): rewards in [0, 1], Q values around `centre` (0: the zero-mean case), a third of
    the rows with tq1 == tq2; inv_global_B = 1/B and 1/(2B), the data-parallel value.  The two heads' estimates lie 6
    above and below the target values, so that q - y is not a difference of nearly equal numbers: dq is held to a
    bound relative to its own norm, which at B = 1 is one element."""
    r = rs_(1000 * B + dp)
    reward, disc = f32(r.uniform(0, 1, B)), f32(np.where(r.uniform(size=B) < 0.1, 0.0, 0.99))
    tq1, tq2 = f32(centre + r.standard_normal(B)), f32(centre + r.standard_normal(B))
    tq2[::3] = tq1[::3]
    q1, q2 = f32(centre + 6 + 0.3 * r.standard_normal(B)), f32(centre - 6 + 0.3 * r.standard_normal(B))
    inv = float(np.float32(1.0 / (dp * B)))
    dq1, dq2 = out(B, name="dq1"), out(B, name="dq2")
    marker = torch.arange(10.0, 18.0)
    sums = dev(marker, "sums")
    rc = lib.drq_td_mse(p(dev(tq1)), p(dev(tq2)), p(dev(q1)), p(dev(q2)), p(dev(reward)), p(dev(disc)), p(dq1), p(dq2),
                        p(sums), B, inv, None)
    assert rc == 0
    d = lambda t: t.double()
    y = d(reward) + d(disc) * torch.minimum(d(tq1), d(tq2))
    e1, e2 = d(q1) - y, d(q2) - y
    assert nerr(dq1, 2 * e1 * inv) <= 2e-6 and nerr(dq2, 2 * e2 * inv) <= 2e-6
    s = sums.cpu().double()
    for i, term in enumerate((d(reward), y, d(q1), d(q2), e1 * e1 + e2 * e2)):
        err, bound = abs(float(s[i] - term.sum())), sum_bound(B, term)
        print(f"td_mse B={B} sums[{i}]: |hip - fp64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (i, float(s[i]), float(term.sum()), err, bound)
    assert same_bits(sums[5:], marker[5:])                       # sums[5..7] belong to the actor loss


@pytest.mark.parametrize("centre", [5.0, 0.0])
@pytest.mark.parametrize("B,A", [(1, 1), (37, 6), (256, 6), (256, 21), (2048, 21), (100, 7)])
def test_actor_loss(lib, B, A, centre):
    """drq_actor_loss (drqv2.py:212-216,225).  B*A below (1, 222, 700), equal to a multiple of (1536, 43008) and ragged
    against (5376 = 5*1024 + 256) the 1024-element batch of the log-prob loop; the action read as columns [F, F+A) of a
    wider buffer whose other columns are poison; exact ties q1 == q2 on every third row."""
    Fd, std = 50, 0.37
    r = rs_(77 * B + A)
    q1, q2 = f32(centre + r.standard_normal(B)), f32(centre + r.standard_normal(B))
    q2[::3] = q1[::3]
    mu = torch.tanh(f32(r.standard_normal((B, A))))
    a = (mu + f32(r.standard_normal((B, A))) * std).clamp(-1 + 1e-6, 1 - 1e-6)
    ha = wide(B, Fd + A, "ha")
    ha[:, Fd:] = a.cuda()
    inv = float(np.float32(1.0 / B))
    dq1, dq2 = out(B, name="dq1"), out(B, name="dq2")
    marker = torch.arange(10.0, 18.0)
    sums = dev(marker, "sums")
    rc = lib.drq_actor_loss(p(dev(q1)), p(dev(q2)), ha[:, Fd:].data_ptr(), Fd + A, p(dev(mu)), std, p(dq1), p(dq2),
                            p(sums), B, A, inv, None)
    assert rc == 0
    g = torch.tensor(-inv, dtype=torch.float32)
    zero, half = torch.zeros(()), g * 0.5
    assert same_bits(dq1, torch.where(q1 < q2, g, torch.where(q1 == q2, half, zero)))
    assert same_bits(dq2, torch.where(q2 < q1, g, torch.where(q1 == q2, half, zero)))
    assert int((q1 == q2).sum()) == (B + 2) // 3
    s = sums.cpu().double()
    t5 = -torch.minimum(q1.double(), q2.double())
    lp = torch.distributions.Normal(mu.double(), float(np.float32(std))).log_prob(a.double())
    for i, term, n in ((5, t5, B), (6, lp, B * A)):
        err, bound = abs(float(s[i] - term.sum())), sum_bound(n, term)
        print(f"actor_loss B={B} A={A} sums[{i}]: |hip - fp64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (i, float(s[i]), float(term.sum()), err, bound)
    assert same_bits(sums[:5], marker[:5]) and same_bits(sums[7:], marker[7:])
    assert bool(is_sent(ha[:, :Fd]).all())


@pytest.mark.parametrize("B,A", [(1, 1), (37, 6), (256, 21), (2048, 21), (100, 1)])
def test_actor_dmu(lib, B, A):
    col0, ld = 50, 50 + A + 3
    d1, d2 = wide(B, ld, "dha1"), wide(B, ld, "dha2")
    a1, a2 = rnd(B, A, seed=1), rnd(B, A, seed=2)
    d1[:, col0:col0 + A], d2[:, col0:col0 + A] = a1.cuda(), a2.cuda()
    mu = torch.tanh(rnd(B, A, seed=3))
    dpre = out(B, A, name="dpre")
    assert lib.drq_actor_dmu(p(d1), p(d2), ld, col0, p(dev(mu)), p(dpre), B, A, None) == 0
    assert nerr(dpre, (a1.double() + a2.double()) * (1 - mu.double() ** 2)) <= 2e-6
    assert lib.drq_actor_dmu(None, p(d2), ld, col0, p(dev(mu)), p(dpre), B, A, None) == EARG
    assert lib.drq_actor_dmu(p(d1), p(d2), ld, col0, p(dev(mu)), p(dpre), 0, A, None) == EARG


# ------------------------------------------------------------------------------------------------ column sums, copies
@pytest.mark.parametrize("M", [1, 15, 16, 17, 63, 1023, 1024, 1025, 2051])
def test_colsum_batched_and_strided(lib, M):
    """drq_colsum, both workgroup shapes (64 columns below 1,024 rows, 16 from there on), ld > N, three problems whose
    inputs and outputs lie further apart than they must: every gap is poison before and after.  The inputs have mean
    0.5 so that a column sum is not a small difference of large terms (the bound is relative to the sums' norm)."""
    for N in (1, 15, 16, 17, 63, 64, 65, 1000):
        ld, nb = N + 3, 3
        dy_bs, out_bs = M * ld + 5, N + 2
        x = rnd(nb, M, N, seed=M + N, mean=0.5)
        src = poison.alloc((nb * dy_bs,), torch.float32, "cuda", name=f"dy N={N}", kind="in")
        dst = poison.partial(out(nb * out_bs, name=f"colsum N={N}"))
        for b in range(nb):
            src[b * dy_bs:b * dy_bs + M * ld].view(M, ld)[:, :N] = x[b].cuda()
        assert lib.drq_colsum(p(src), ld, dy_bs, p(dst), out_bs, M, N, nb, None) == 0
        got = torch.stack([dst[b * out_bs:b * out_bs + N] for b in range(nb)])
        assert nerr(got, x.double().sum(1)) <= 3e-6, (M, N, nerr(got, x.double().sum(1)))
        gaps = torch.cat([dst[b * out_bs + N:(b + 1) * out_bs] for b in range(nb)])
        assert bool(is_sent(gaps).all()), (M, N)
        one = out(N, name=f"colsum1 N={N}")                       # nbatch = 1, tight output
        assert lib.drq_colsum(p(src), ld, 0, p(one), 0, M, N, 1, None) == 0
        assert same_bits(one, got[0])
    assert lib.drq_colsum(None, 4, 0, p(one), 0, M, 1, 1, None) == EARG
    assert lib.drq_colsum(p(src), 4, 0, p(one), 0, 0, 1, 1, None) == EARG


def _sizes(cap):
    return [(1, 1), (5, 51), (257, 1), (-(-(cap + 13) // 7), 7)]      # B*A = 1, 255, 257 and just above the grid cap


def test_copy_cols(lib, cap):
    for B, A in _sizes(cap):
        lds, ldd = A + 2, A + 5
        x = rnd(B, A, seed=B)
        src, dst = wide(B, lds, f"src {B}x{A}"), wide(B, ldd, f"dst {B}x{A}", kind="zero")
        dst.view(torch.int32).fill_(poison.SENTINEL)
        src[:, :A] = x.cuda()
        assert lib.drq_copy_cols(p(src), lds, p(dst), ldd, B, A, None) == 0
        assert same_bits(dst[:, :A], x) and bool(is_sent(dst[:, A:]).all()), (B, A)
    assert lib.drq_copy_cols(None, 1, p(dst), 1, 1, 1, None) == EARG and lib.drq_copy_cols(p(src), 1, p(dst), 1, 1, 0, None) == EARG


def test_fill(lib, cap):
    for n in (1, 255, 257, cap + 13):
        for v in (1.5, -0.0):
            buf = poison.partial(out(n + 7, name=f"fill n={n}"))
            assert lib.drq_fill(buf[3:].data_ptr(), n, v, None) == 0
            assert same_bits(buf[3:3 + n], torch.full((n,), v)), (n, v)
            assert bool(is_sent(buf[:3]).all()) and bool(is_sent(buf[3 + n:]).all()), (n, v)
    assert lib.drq_fill(None, 4, 0.0, None) == EARG and lib.drq_fill(p(buf), 0, 0.0, None) == EARG


def test_u8_normalize_every_byte_at_every_position(ops, lib, cap):
    """obs/255 - 0.5 (drqv2.py:64): all 256 byte values at every position mod 256 of a ragged-length array, bit for bit
    the division torch does on the CPU; and past the grid cap."""
    for n in (256 * 256 + 17, cap + 13):
        i = torch.arange(n)
        x = ((i + i // 256) % 256).to(torch.uint8)
        y = ops.u8_normalize(dev(x))
        assert same_bits(y, x.float() / 255.0 - 0.5)
    assert lib.drq_u8_normalize(None, p(y), 4, None) == EARG and lib.drq_u8_normalize(p(dev(x)), p(y), 0, None) == EARG


def _tanh_inputs(extra=0):
    mag = torch.logspace(-8, math.log10(20.0), 200, dtype=torch.float64).float()
    x = torch.cat([mag, -mag, torch.tensor([0.0, -0.0, 20.0, -20.0, 1.0, -1.0, 0.5])])
    if extra:
        x = torch.cat([x, rnd(extra, seed=3, scale=2.0)])
    return x


def test_tanh_and_tanh_bwd(ops, lib, cap):
    for extra in (0, cap + 13 - 407):
        x = _tanh_inputs(extra)
        assert x.numel() % 4 != 0
        y = ops.tanh(dev(x))
        assert float((y.cpu().double() - torch.tanh(x.double())).abs().max()) <= 2e-7
        dy = rnd(x.numel(), seed=5)
        dx = ops.tanh_bwd(poison.put(y), dev(dy))
        assert nerr(dx, dy.double() * (1 - y.cpu().double() ** 2)) <= 2e-6
    assert lib.drq_tanh(None, p(y), 4, None) == EARG and lib.drq_tanh(p(y), p(y), 0, None) == EARG
    assert lib.drq_tanh_bwd(p(y), None, p(dx), 4, None) == EARG and lib.drq_tanh_bwd(p(y), p(y), p(dx), 0, None) == EARG


@pytest.mark.parametrize("pad", [2, 1])
def test_relu_mask_pad_with_a_mask(ops, pad):
    n, c, h = 2, 3, 7
    dy = rnd(n, c, h, h, seed=1)
    mask = rnd(n, c, h, h, seed=2)
    mask.view(-1)[::5] = 0.0
    mask.view(-1)[1::7] = -0.0
    o = ops.relu_mask_pad(dev(dy), dev(mask), pad)
    want = torch.zeros(n, c, h + 2 * pad, h + 2 * pad)
    want[:, :, pad:pad + h, pad:pad + h] = torch.where(mask > 0, dy, torch.zeros(()))
    assert torch.equal(o.cpu(), want)
    border = o.clone()
    border[:, :, pad:pad + h, pad:pad + h] = 0
    assert same_bits(border.abs(), torch.zeros_like(want))       # the border is exactly zero
    o2 = ops.relu_mask_pad(dev(dy), None, pad)
    assert torch.equal(o2[:, :, pad:pad + h, pad:pad + h].cpu(), dy)


@pytest.mark.parametrize("use_clip,with_mu", [(1, False), (0, True), (0, False)])
def test_trunc_normal_sample_strided_no_mu_no_clip(ops, lib, use_clip, with_mu):
    from oracle import drq_oracle as O
    B, A, std, clip = 37, 6, 0.37, 0.3
    pre, noise = rnd(B, A, seed=1, scale=1.5), rnd(B, A, seed=2)
    mu_k, _ = ops.trunc_normal_sample(dev(pre), dev(noise), std, clip)      # the kernel's own mu (tanhf)
    lda = A + 3
    dst = wide(B, lda, "a_out", kind="zero")
    dst.view(torch.int32).fill_(poison.SENTINEL)
    mu = out(B, A, name="mu") if with_mu else None
    rc = lib.drq_trunc_normal_sample(p(dev(pre)), p(dev(noise)), std, clip, use_clip, p(mu), p(dst), lda, B, A, None)
    assert rc == 0
    a_ref = O.trunc_normal_sample(mu_k.cpu(), noise, std, clip if use_clip else None)
    assert same_bits(dst[:, :A], a_ref) and bool(is_sent(dst[:, A:]).all())
    if with_mu:
        assert same_bits(mu, mu_k)
    if not use_clip:
        assert not torch.equal(a_ref, O.trunc_normal_sample(mu_k.cpu(), noise, std, clip))      # the clip would have bitten
    assert lib.drq_trunc_normal_sample(p(dev(pre)), p(dev(noise)), std, clip, 1, None, None, lda, B, A, None) == EARG


# ------------------------------------------------------------------------------------------------ LayerNorm + tanh
def ln64(z, g, b):
    return torch.tanh(torch.nn.functional.layer_norm(z, (z.shape[1],), g, b, 1e-5))


@pytest.mark.parametrize("Fd", [1, 63, 64, 65, 128, 129, 255, 256])
def test_ln_tanh_fwd_bwd_shapes(ops, Fd):
    """drq_ln_tanh_fwd / _bwd around the 64-lane and 4-rows-per-workgroup edges, bounds of test_ln_tanh"""
    for rows in (1, 3, 4, 5, 258):
        z = rnd(rows, Fd, seed=rows + Fd, scale=2.0)
        g, b, dh = 1 + 0.1 * rnd(Fd, seed=2), 0.1 * rnd(Fd, seed=3), rnd(rows, Fd, seed=4)
        h, xhat, rstd = ops.ln_tanh_fwd(dev(z), dev(g), dev(b))
        zd, gd, bd = (t.double().requires_grad_(True) for t in (z, g, b))
        ref = ln64(zd, gd, bd)
        assert nerr(h, ref) <= 2e-6, (rows, Fd)
        (ref * dh.double()).sum().backward()
        dz, dg, dbeta = ops.ln_tanh_bwd(dev(dh), h, xhat, rstd, dev(g))
        assert nerr(dbeta, bd.grad) <= 1e-5, (rows, Fd)
        if Fd == 1:       # LayerNorm of one element is the constant beta: both gradients are exactly 0 (fp64 autograd
            assert not bool(dz.any()) and not bool(dg.any())       # leaves rounding dust of 1e-17 there, not a reference)
        else:
            assert nerr(dz, zd.grad) <= 1e-5 and nerr(dg, gd.grad) <= 1e-5, (rows, Fd)
        h2, _, _ = ops.ln_tanh_fwd(dev(z), dev(g), dev(b), save=False)
        assert same_bits(h2, h)


def test_ln_tanh_constant_row_and_large_row(ops):
    """a row of variance 0 (the eps decides) and a row 1e4 times larger than the others (LayerNorm is scale-free)"""
    rows, Fd = 6, 100
    z = rnd(rows, Fd, seed=1, scale=2.0)
    z[0] = 0.1
    z[1] *= 1e4
    g, b = 1 + 0.1 * rnd(Fd, seed=2), 0.1 * rnd(Fd, seed=3)
    h, xhat, rstd = ops.ln_tanh_fwd(dev(z), dev(g), dev(b))
    assert nerr(h, ln64(z.double(), g.double(), b.double())) <= 2e-6
    assert nerr(h[0], torch.tanh(b.double())) <= 2e-6 and nerr(h[1], ln64(z[1:2].double(), g.double(), b.double())[0]) <= 2e-6
    assert bool(torch.isfinite(xhat).all()) and bool(torch.isfinite(rstd).all())


def test_ln_tanh_refuses_bad_arguments(lib):
    z, g = dev(rnd(4, 257)), dev(rnd(257))
    o = poison.partial(out(4, 257))
    a = (p(z), 257, p(g), p(g), p(o), 257, None, None, 4)
    assert lib.drq_ln_tanh_fwd(*a, 257, None) == EARG                      # F > 256
    assert lib.drq_ln_tanh_fwd(*a, 0, None) == EARG
    assert lib.drq_ln_tanh_fwd(None, 256, p(g), p(g), p(o), 256, None, None, 4, 256, None) == EARG
    assert lib.drq_ln_tanh_fwd(p(z), 256, p(g), p(g), p(o), 256, None, None, 0, 256, None) == EARG
    ptrs = (ctypes.c_void_p * 5)(*[p(z)] * 5)
    ldo = (ctypes.c_int * 5)(*[257] * 5)
    assert lib.drq_ln_tanh_fwd_multi(5, ptrs, 257, ptrs, ptrs, ptrs, ldo, None, None, 4, 50, None) == EARG       # n > 4
    assert lib.drq_ln_tanh_fwd_multi(2, ptrs, 257, ptrs, ptrs, ptrs, ldo, None, None, 4, 257, None) == EARG
    assert bool(is_sent(o).all())                                               # nothing was launched


@pytest.mark.parametrize("rows,Fd", [(37, 50), (258, 256), (5, 65)])
def test_ln_tanh_fwd2_and_multi_equal_the_single_launch(ops, lib, rows, Fd):
    """drq_ln_tanh_fwd2 / _multi (n = 1..4): out, xhat, rstd bit-identical to drq_ln_tanh_fwd per problem, with ldz > F,
    a different ldo > F per problem (gap untouched) and xhat / rstd left out for some problems."""
    ldz = Fd + 3
    zs, gs, bs, single = [], [], [], []
    for i in range(4):
        zt = rnd(rows, Fd, seed=10 + i, scale=2.0)
        zw = wide(rows, ldz, f"z{i}")
        zw[:, :Fd] = zt.cuda()
        zs.append(zw)
        gs.append(dev(1 + 0.1 * rnd(Fd, seed=20 + i)))
        bs.append(dev(0.1 * rnd(Fd, seed=30 + i)))
        o, xh, r = out(rows, Fd), out(rows, Fd), out(rows)
        assert lib.drq_ln_tanh_fwd(p(zw), ldz, p(gs[i]), p(bs[i]), p(o), Fd, p(xh), p(r), rows, Fd, None) == 0
        single.append((o, xh, r))
        assert nerr(o, ln64(zt.double(), gs[i].cpu().double(), bs[i].cpu().double())) <= 2e-6

    def fresh(n, saved):
        outs, xhs, rss = [], [], []
        for i in range(n):
            o = wide(rows, Fd + 1 + i, f"out{i}", kind="zero")
            o.view(torch.int32).fill_(poison.SENTINEL)
            outs.append(o)
            xhs.append(out(rows, Fd, name=f"xhat{i}") if saved[i] else None)
            rss.append(out(rows, name=f"rstd{i}") if saved[i] else None)
        return outs, xhs, rss

    def compare(n, outs, xhs, rss):
        for i in range(n):
            assert same_bits(outs[i][:, :Fd], single[i][0]) and bool(is_sent(outs[i][:, Fd:]).all()), (n, i)
            if xhs[i] is not None:
                assert same_bits(xhs[i], single[i][1]) and same_bits(rss[i], single[i][2]), (n, i)

    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[p(t) for t in ts])
    for n in (1, 2, 3, 4):
        saved = [(i + n) % 2 == 0 for i in range(n)]
        outs, xhs, rss = fresh(n, saved)
        ldo = (ctypes.c_int * n)(*[Fd + 1 + i for i in range(n)])
        rc = lib.drq_ln_tanh_fwd_multi(n, arr(zs[:n]), ldz, arr(gs[:n]), arr(bs[:n]), arr(outs), ldo, arr(xhs), arr(rss),
                                       rows, Fd, None)
        assert rc == 0
        compare(n, outs, xhs, rss)
    for saved in ((True, False), (False, True)):
        outs, xhs, rss = fresh(2, saved)
        rc = lib.drq_ln_tanh_fwd2(p(zs[0]), p(zs[1]), ldz, p(gs[0]), p(bs[0]), p(gs[1]), p(bs[1]), p(outs[0]), Fd + 1,
                                  p(outs[1]), Fd + 2, p(xhs[0]), p(rss[0]), p(xhs[1]), p(rss[1]), rows, Fd, None)
        assert rc == 0
        compare(2, outs, xhs, rss)


@pytest.mark.parametrize("rows,Fd", [(37, 50), (258, 256), (3, 65)])
def test_ln_tanh_bwd_two_sources_strides_and_optional_param_grads(ops, lib, rows, Fd):
    z = rnd(rows, Fd, seed=1, scale=2.0)
    g, b = 1 + 0.1 * rnd(Fd, seed=2), 0.1 * rnd(Fd, seed=3)
    d0, d1 = rnd(rows, Fd, seed=4), rnd(rows, Fd, seed=5)
    h, xhat, rstd = ops.ln_tanh_fwd(dev(z), dev(g), dev(b))
    ld0, ld1, ldh = Fd + 1, Fd + 2, Fd + 3
    w0, w1, wh = wide(rows, ld0, "dh0"), wide(rows, ld1, "dh1"), wide(rows, ldh, "h")
    w0[:, :Fd], w1[:, :Fd], wh[:, :Fd] = d0.cuda(), d1.cuda(), h
    xh, rsd, gc = poison.put(xhat), poison.put(rstd), dev(g)
    zd, gd, bd = (t.double().requires_grad_(True) for t in (z, g, b))
    (ln64(zd, gd, bd) * (d0.double() + d1.double())).sum().backward()
    dz, dln, dg, db = out(rows, Fd, name="dz"), out(rows, Fd, name="dln"), out(Fd, name="dgamma"), out(Fd, name="dbeta")
    rc = lib.drq_ln_tanh_bwd(p(w0), ld0, p(w1), ld1, p(wh), ldh, p(xh), p(rsd), p(gc), p(dz), p(dln), p(dg), p(db), rows, Fd,
                             None)
    assert rc == 0
    assert nerr(dz, zd.grad) <= 1e-5 and nerr(dg, gd.grad) <= 1e-5 and nerr(db, bd.grad) <= 1e-5
    # the one-source call on dh0 + dh1 (summed in fp32 beforehand, as the kernel does): the same against fp64
    dz1, dg1, db1 = ops.ln_tanh_bwd(dev(d0 + d1), h, xhat, rstd, gc)
    assert nerr(dz1, zd.grad) <= 1e-5 and nerr(dg1, gd.grad) <= 1e-5 and nerr(db1, bd.grad) <= 1e-5
    assert same_bits(dz1, dz)
    # without parameter gradients: dz and dln are still written in full (check() sees to it) and are the same
    dz2, dln2 = out(rows, Fd, name="dz (no param grads)"), out(rows, Fd, name="dln (no param grads)")
    rc = lib.drq_ln_tanh_bwd(p(w0), ld0, p(w1), ld1, p(wh), ldh, p(xh), p(rsd), p(gc), p(dz2), p(dln2), None, None, rows, Fd,
                             None)
    assert rc == 0 and same_bits(dz2, dz) and same_bits(dln2, dln)
    hd = h.cpu().double()
    assert nerr(dln, (d0.double() + d1.double()) * (1 - hd * hd)) <= 2e-6
    # only one of them: refused, nothing launched
    dz3 = poison.partial(out(rows, Fd, name="dz (refused)"))
    for a, c in ((p(dg), None), (None, p(db))):
        assert lib.drq_ln_tanh_bwd(p(w0), ld0, p(w1), ld1, p(wh), ldh, p(xh), p(rsd), p(gc), p(dz3), p(dln2), a, c, rows, Fd,
                                   None) == EARG
    assert lib.drq_ln_tanh_bwd(p(w0), ld0, None, 0, p(wh), ldh, p(xh), p(rsd), p(gc), p(dz3), p(dln2), None, None, rows, 257,
                               None) == EARG
    assert bool(is_sent(dz3).all())


# ------------------------------------------------------------------------------------------------ ZeRO-1 pair, Adam, Polyak
def _slices(world, n, stride, seed):
    """the `world` ranks' copies of a gradient slice, copy r at [r*stride, r*stride + n), poison in between"""
    g = rnd(world, n, seed=seed, scale=1e-3)
    g[:, ::11] = 0.0
    buf = poison.alloc((world * stride,), torch.float32, "cuda", name=f"recv world={world} n={n}", kind="in")
    for r in range(world):
        buf[r * stride:r * stride + n] = g[r].cuda()
    return g, buf


def _rank_ordered_sum(g):
    s = g[0].clone()
    for r in range(1, g.shape[0]):
        s = s + g[r]                                               # fp32, ((r0 + r1) + r2) + ...
    return s


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_sum_slices(lib, cap, world):
    for n in (1, 257, cap + 13):
        stride = n + 5
        g, buf = _slices(world, n, stride, seed=world + n % 97)
        o = out(n, name=f"sum n={n}")
        assert lib.drq_sum_slices(p(buf), stride, world, p(o), n, None) == 0
        assert same_bits(o, _rank_ordered_sum(g)), (world, n)
    assert lib.drq_sum_slices(p(buf), n - 1, world, p(o), n, None) == EARG
    assert lib.drq_sum_slices(p(buf), stride, 0, p(o), n, None) == EARG
    assert lib.drq_sum_slices(None, stride, world, p(o), n, None) == EARG


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_adam_reduce_flat_equals_sum_slices_then_adam_flat(lib, cap, world):
    """The ZeRO-1 promise of include/drqv2_hip.h: p, m, v after drq_adam_reduce_flat are bit-identical to drq_sum_slices
    followed by drq_adam_flat from the same state, over three consecutive steps."""
    lr = 1e-4
    for n, combos in ((257, [(s, gs) for s in (1, 2, 1000, 10 ** 6) for gs in (1.0, 0.25)]), (cap + 13, [(1000, 0.25)])):
        stride = n + 5
        for step0, gscale in combos:
            p0, m0 = rnd(n, seed=1), rnd(n, seed=2, scale=1e-3)
            v0 = rnd(n, seed=3, scale=1e-3) ** 2
            pa, ma, va = dev(p0), dev(m0), dev(v0)
            pb, mb, vb = dev(p0), dev(m0), dev(v0)
            for k in range(3):
                g, buf = _slices(world, n, stride, seed=10 * world + k)
                gsum = out(n, name="gsum")
                assert lib.drq_sum_slices(p(buf), stride, world, p(gsum), n, None) == 0
                assert lib.drq_adam_flat(p(pa), p(gsum), p(ma), p(va), n, lr, step0 + k, gscale, None, 0.0, None) == 0
                assert lib.drq_adam_reduce_flat(p(pb), p(buf), stride, world, p(mb), p(vb), n, lr, step0 + k, gscale, None) == 0
                assert same_bits(pa, pb) and same_bits(ma, mb) and same_bits(va, vb), (world, n, step0, gscale, k)
            assert not same_bits(pa, p0)
    a = (p(mb), p(vb), n, lr)
    assert lib.drq_adam_reduce_flat(p(pb), p(buf), n - 1, world, *a, 1, 1.0, None) == EARG        # stride < n
    assert lib.drq_adam_reduce_flat(p(pb), p(buf), stride, 0, *a, 1, 1.0, None) == EARG           # world < 1
    assert lib.drq_adam_reduce_flat(p(pb), p(buf), stride, world, *a, 0, 1.0, None) == EARG       # step < 1
    assert same_bits(pa, pb)


@pytest.mark.parametrize("fused_target", [False, True])
@pytest.mark.parametrize("step", [1, 10, 1000, 10 ** 6])
def test_adam_flat_and_ema_flat_bitwise_beyond_the_grid_cap(lib, cap, step, fused_target):
    """drq_adam_flat / drq_ema_flat against oracle.adam_step / oracle.polyak (pinned to torch by
    tests/golden/elementwise.npz), n above the point where the grid stops growing and the grid-stride loop starts;
    moments carried in; gradients with exact zeros and values near 1e-20 on elements whose v is zero or tiny, so that v
    is zero or subnormal and eps decides the step."""
    from oracle import drq_oracle as O
    n, lr, tau = cap + 13, 1e-4, 0.01
    p0, g = rnd(n, seed=1), rnd(n, seed=2, scale=1e-3)
    m0, v0 = rnd(n, seed=3, scale=1e-3), rnd(n, seed=4, scale=1e-3) ** 2
    g[::7] = 0.0
    g[1::13] = 1e-20
    g[2::13] = -3e-21
    g[3::13] = 1e-22
    v0[1::13], v0[2::13], v0[3::13] = 0.0, 1e-42, 0.0
    m0[1::13], m0[3::13] = 0.0, 1e-21
    t0 = rnd(n, seed=5)
    pk, mk, vk = dev(p0, "p"), dev(m0, "m"), dev(v0, "v")
    tk = dev(t0, "target") if fused_target else None
    assert lib.drq_adam_flat(p(pk), p(dev(g, "g")), p(mk), p(vk), n, lr, step, 1.0, p(tk), tau, None) == 0
    pr, mr, vr, tr = p0.clone(), m0.clone(), v0.clone(), t0.clone()
    O.adam_step(pr, g, mr, vr, step, lr)
    assert same_bits(mk, mr) and same_bits(vk, vr) and same_bits(pk, pr)
    assert int(((vr > 0) & (vr < 1.1754944e-38)).sum()) > 1000 and int((vr == 0).sum()) > 1000       # the cases are there
    if fused_target:
        O.polyak(pr, tr, tau)
        assert same_bits(tk, tr)
    else:
        tk = dev(t0, "target")
        assert lib.drq_ema_flat(p(pk), p(tk), n, tau, None) == 0
        O.polyak(pr, tr, tau)
        assert same_bits(tk, tr)
    assert lib.drq_adam_flat(p(pk), None, p(mk), p(vk), n, lr, step, 1.0, None, tau, None) == EARG
    assert lib.drq_adam_flat(p(pk), p(pk), p(mk), p(vk), 0, lr, step, 1.0, None, tau, None) == EARG
    assert lib.drq_adam_flat(p(pk), p(pk), p(mk), p(vk), n, lr, 0, 1.0, None, tau, None) == EARG
    assert lib.drq_ema_flat(None, p(tk), n, tau, None) == EARG and lib.drq_ema_flat(p(pk), p(tk), 0, tau, None) == EARG
    assert same_bits(pk, pr)


# ------------------------------------------------------------------------------------------------ strided batched GEMM
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("M,N,K", [(37, 50, 130), (256, 256, 256)])
@pytest.mark.parametrize("layout", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("nbatch", [2, 4])
def test_gemm_f32_batched_strides(ops, nbatch, layout, M, N, K, shared):
    """drq_gemm_f32 with nbatch > 1: shared (a_bs = bias_bs = aux_bs = 0) or per-problem A / bias / mask, C rows longer
    than N and problems further apart than M*ldc (gaps stay poison), every tile x split-K choice, against fp64."""
    a_kc, b_kc = layout != "wgrad", layout == "fwd"
    na = 1 if shared else nbatch
    A = rnd(na, M, K, seed=1) if a_kc else rnd(na, K, M, seed=1)
    Bm = rnd(nbatch, N, K, seed=2, scale=K ** -0.5) if b_kc else rnd(nbatch, K, N, seed=2, scale=K ** -0.5)
    bias = rnd(na, N, seed=3) if layout == "fwd" else None
    mask = rnd(na, M, N, seed=4) if layout == "dgrad" else None
    Ad, Bd = A.double() if a_kc else A.double().transpose(1, 2), Bm.double().transpose(1, 2) if b_kc else Bm.double()
    ref = Ad.expand(nbatch, M, K) @ Bd
    if bias is not None:
        ref = torch.relu(ref + bias.double()[:, None, :])
    if mask is not None:
        ref = ref * (mask.double() > 0)
    Ac, Bc, bc, mc = dev(A, "A"), dev(Bm, "B"), (dev(bias, "bias") if bias is not None else None), (dev(mask, "mask") if mask is not None else None)
    ws = poison.alloc((4 * 1024 * 1024,), torch.float32, "cuda", name="split-K workspace", kind="ws")
    ldc = N + 3
    c_bs = M * ldc + 7
    for tile in (0, 1, 2, 3, 4, 5, 6):
        for splitk in (0, 1, 3):
            C = poison.partial(out(nbatch * c_bs, name=f"C tile={tile} splitk={splitk}"))
            ops.gemm(Ac, a_kc, Bc, b_kc, M, N, K, bias=bc, relu=layout == "fwd", aux=mc, nbatch=nbatch,
                     a_bs=0 if shared else M * K, b_bs=N * K, c_bs=c_bs, bias_bs=0 if shared else N,
                     aux_bs=0 if shared else M * N, tile=tile, splitk=splitk, out=C, ldc=ldc, ws=ws)
            for b in range(nbatch):
                blk = C[b * c_bs:(b + 1) * c_bs]
                rows = blk[:M * ldc].view(M, ldc)
                assert nerr(rows[:, :N], ref[b]) <= 3e-6, (tile, splitk, b, nerr(rows[:, :N], ref[b]))
                assert bool(is_sent(rows[:, N:]).all()) and bool(is_sent(blk[M * ldc:]).all()), (tile, splitk, b)


# ------------------------------------------------------------------------------------------------ metrics mirror
@pytest.mark.parametrize("seq", [1, 2 ** 32 - 1])
def test_publish_sums(lib, seq):
    marker = -123.25
    host = torch.full((16,), marker).pin_memory()
    vals = rnd(8, seed=seq % 7, scale=10.0)
    sums = dev(vals, "sums")
    assert lib.drq_publish_sums(p(sums), host.data_ptr(), seq, None) == 0
    torch.cuda.synchronize()
    assert same_bits(host[:8], vals)
    assert int(host[8:9].view(torch.int32)) == (seq if seq < 2 ** 31 else seq - 2 ** 32)
    assert same_bits(host[9:], torch.full((7,), marker))
    assert same_bits(sums, vals)
