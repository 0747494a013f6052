"""Every kernel variant of the fp32 GEMM family (csrc/gemm.hip, gemm2.hip, gemm3.hip, skinny.hip) at its smallest shape,
through the C ABI against fp64 on the CPU.  The rows, the variant each is meant to reach and the edge it sits at are the
table of tests/gemm_variants.py (tests/test_cpu_gemm_variants.py checks that the table covers the dispatch); here each
row runs, and the two dispatch decisions the ABI shows (*nq_out, *splitk_out) are asserted against the prediction.

Bounds (gemm_variants.compare): the project's normwise 3e-6 and the componentwise any-order summation bound
|C - C_ref| <= 2 (K+2) 2^-24 (|A| |B| + |bias|), evaluated in fp64; masked-out elements exactly +0.0f; leading-dimension
gaps and refused outputs still poison.  Inputs: weights randn K^-1/2, post-ReLU activations, gradients with real zeros,
masks with +0.0, -0.0 and NaN planted in every 32x32 tile; every problem of a batch has its own data.

For the record (not a tolerance): the largest error / componentwise bound seen on an MI355X was 0.022 for drq_mlp_fwd,
0.022 for drq_mlp_dgrad, 0.024 for drq_mlp_wgrad_dgrad, 0.046 for drq_gemm_batched_f32 (the skinny dgrad kernel), 0.012
for drq_gemm_f32 and 6e-5 for drq_gemm_batched_partial (K >= 4064).  Run with -s for the figure of every row."""
import ctypes
import json

import pytest
import torch

from tests import gemm_variants as gv
from tests import poison
from tests.poison import poisoned_ops  # noqa: F401  (autouse: drqv2_amd.ops allocates poisoned memory; check() after every test)

pytestmark = pytest.mark.gpu
EARG = -1
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from drqv2_amd import ops as o, _lib
    _lib.load()
    assert torch.cuda.is_available()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == gv.CUS, (f"the GEMM variant table is built for the {gv.CUS} CUs of the MI355X, the only target; this "
                           f"device has {cus}: the rows would not reach the variants they name")
    return o


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nGEMM-VARIANTS largest error / componentwise bound per entry: " + json.dumps(RATIOS, sort_keys=True))


def rows(entry):
    sel = [r for r in gv.TABLE if r.entry == entry]
    return pytest.mark.parametrize("row", sel, ids=[gv.row_id(r) for r in sel])


def G(t, name=None):
    """an input between two poisoned guard bands"""
    return poison.put(t, "cuda", name=name)


def wide_in(t, ld, name):
    """t as the first columns of a poisoned [rows][ld] buffer: a read of the gap reads the sentinel NaN"""
    buf = poison.alloc((t.shape[0], ld), torch.float32, "cuda", name=name, kind="in")
    v = buf[:, :t.shape[1]]
    v.copy_(t)
    return v


def wide_out(nrows, ld, name):
    """a poisoned [rows][ld] output: the test checks itself that the logical columns were written and the gap was not"""
    return poison.alloc((nrows, ld), torch.float32, "cuda", name=name, kind="ws")


def is_sent(t):
    return t.contiguous().view(torch.int32) == poison.SENTINEL


def logical(buf, cols, what):
    """the first `cols` columns of an output buffer; gap columns must still be poison, logical ones must not"""
    assert bool(is_sent(buf[:, cols:]).all()), f"{what}: a leading-dimension gap was written"
    assert not bool(is_sent(buf[:, :cols]).any()), f"{what}: elements never written"
    return buf[:, :cols]


def hold(got, ref, mag, K, what, row, mask=None):
    ok, nerr, ratio = gv.compare(got, ref, mag, K)
    print(f"{gv.row_id(row)} {what}: normwise {nerr:.3g}, error/bound {ratio:.3g}")
    if ratio > RATIOS.get(what, (0.0, ""))[0]:
        RATIOS[what] = (ratio, gv.row_id(row))
    assert ok, (gv.row_id(row), row.expect, what, "normwise", nerr, "error/bound", ratio)
    if mask is not None:
        out = got.detach().cpu().contiguous().view(torch.int32)[~(mask > 0)]
        assert bool((out == 0).all()), (gv.row_id(row), what, "a masked-out element is not +0.0f")


def predicted(row):
    sel = gv.select(row)
    assert gv.label(sel) == row.expect, (gv.row_id(row), gv.label(sel))
    return sel


def seeds(row, b, k):
    return (k, b, row.M, row.N, row.K, row.n)


# ------------------------------------------------------------------------------------------------ ring kernel
@rows("mlp_fwd")
def test_ring_forward(ops, row):
    n, M, N, K = row.n, row.M, row.N, row.K
    sel = predicted(row)
    ld = row.opts.get("ld")
    xs = [gv.make_act(M, K, seeds(row, b, 1)) for b in range(n)]
    ws = [gv.make_weight(N, K, K, seeds(row, b, 2)) for b in range(n)]
    bs = [gv.randn(N, seed=seeds(row, b, 3)) for b in range(n)]
    qw = [gv.randn(N, seed=seeds(row, b, 4), scale=N ** -0.5) for b in range(n)]
    if ld:
        xc = [wide_in(t, K + 4, f"x{b}") for b, t in enumerate(xs)]
        wc = [wide_in(t, K + 8, f"w{b}") for b, t in enumerate(ws)]
        yb = [wide_out(M, N + 4, f"y{b}") for b in range(n)]
    else:
        xc, wc, yb = [G(t, f"x{b}") for b, t in enumerate(xs)], [G(t, f"w{b}") for b, t in enumerate(ws)], None
    ys, qps = ops.mlp_fwd(xc, wc, [G(t) for t in bs], relu=True, qws=[G(t) for t in qw], ys=yb,
                          ldy=N + 4 if ld else None)
    assert qps[0].shape[1] == sel.nq, (qps[0].shape, sel)
    for b in range(n):
        ref, mag = gv.reference(xs[b].double(), ws[b].double().t(), bs[b].double(), relu=True)
        y = logical(ys[b], N, f"y{b}") if ld else ys[b]
        hold(y, ref, mag, K, "mlp_fwd", row)
        # every partial is the dot over its own column tile (as tests/test_hip_mlp.py holds it)
        part_ref = (ref * qw[b].double()).view(M, sel.nq, N // sel.nq).sum(2)
        perr = float((qps[b].double().cpu() - part_ref).abs().max() / part_ref.abs().max())
        assert perr <= 3e-6, (gv.row_id(row), b, perr)


@rows("mlp_dgrad")
def test_ring_input_gradient(ops, row):
    n, M, N, K = row.n, row.M, row.N, row.K
    predicted(row)
    ld = row.opts.get("ld")
    dys = [gv.make_grad(M, K, seeds(row, b, 1)) for b in range(n)]
    ws = [gv.make_weight(K, N, K, seeds(row, b, 2)) for b in range(n)]
    mk = [gv.make_mask(M, N, seeds(row, b, 3)) for b in range(n)]
    if ld:
        dc = [wide_in(t, K + 4, f"dy{b}") for b, t in enumerate(dys)]
        wc = [wide_in(t, N + 8, f"w{b}") for b, t in enumerate(ws)]
        mc = [wide_in(t, N + 12, f"mask{b}") for b, t in enumerate(mk)]
        xb = [wide_out(M, N + 4, f"dx{b}") for b in range(n)]
    else:
        dc, wc, mc, xb = [G(t) for t in dys], [G(t) for t in ws], [G(t) for t in mk], None
    dxs = ops.mlp_dgrad(dc, wc, mc, dxs=xb, lddx=N + 4 if ld else None)
    for b in range(n):
        ref, mag = gv.reference(dys[b].double(), ws[b].double(), mask=mk[b])
        dx = logical(dxs[b], N, f"dx{b}") if ld else dxs[b]
        hold(dx, ref, mag, K, "mlp_dgrad", row, mask=mk[b])


@rows("mlp_pair")
def test_ring_gradient_pair(ops, row):
    n, B, Kin, Nout = row.n, row.M, row.N, row.K
    predicted(row)
    ld = row.opts.get("ld")
    dys = [gv.make_grad(B, Nout, seeds(row, b, 1)) for b in range(n)]
    xs = [gv.make_act(B, Kin, seeds(row, b, 2)) for b in range(n)]
    ws = [gv.make_weight(Nout, Kin, Nout, seeds(row, b, 3)) for b in range(n)]
    mk = [gv.make_mask(B, Kin, seeds(row, b, 4)) for b in range(n)]
    if ld:
        dc = [wide_in(t, Nout + 4, f"dy{b}") for b, t in enumerate(dys)]
        xc = [wide_in(t, Kin + 4, f"x{b}") for b, t in enumerate(xs)]
        wc = [wide_in(t, Kin + 8, f"w{b}") for b, t in enumerate(ws)]
        mc = [wide_in(t, Kin + 12, f"mask{b}") for b, t in enumerate(mk)]
        xb = [wide_out(B, Kin + 4, f"dx{b}") for b in range(n)]
        wb = [poison.alloc((Nout, Kin), torch.float32, "cuda", name=f"dw{b}") for b in range(n)]
    else:
        dc, xc, wc, mc = ([G(t) for t in ts] for ts in (dys, xs, ws, mk))
        xb = wb = None
    dws, dbs, dxs = ops.mlp_wgrad_dgrad(dc, xc, wc, mc, dws=wb, dxs=xb, lddx=Kin + 4 if ld else None)
    for b in range(n):
        d64 = dys[b].double()
        ref, mag = gv.reference(d64.t(), xs[b].double())
        hold(dws[b], ref, mag, B, "mlp_pair.dw", row)
        hold(dbs[b], d64.sum(0), d64.abs().sum(0), B, "mlp_pair.db", row)
        ref, mag = gv.reference(d64, ws[b].double(), mask=mk[b])
        dx = logical(dxs[b], Kin, f"dx{b}") if ld else dxs[b]
        hold(dx, ref, mag, Nout, "mlp_pair.dx", row, mask=mk[b])


def _refusal_ids():
    return [f"{c[0]}-{c[6].replace(' ', '_')}" for c in gv.REFUSALS]


@pytest.mark.parametrize("case", gv.REFUSALS, ids=_refusal_ids())
def test_ring_refusals_write_nothing(ops, lib, case):
    """DRQ_EARG and every output (and *nq_out) untouched: the poison check holds `refused` buffers to that"""
    entry, n, M, N, K, o, why = case
    assert gv.select(gv.Row(entry, None, n, M, N, K, o, gv.EARG, why)).name == gv.EARG
    ldx, off = o.get("ldx", K), 1 if o.get("misalign") else 0

    def inp(nrows, cols, ld=None, off=0, name=None):
        ld = ld or cols
        buf = poison.alloc((nrows * ld + 4,), torch.float32, "cuda", name=name, kind="in")
        buf.fill_(0.25)
        return buf[off:off + nrows * ld].view(nrows, ld)[:, :cols]

    def refused(*shape, name=None):
        return poison.alloc(shape, torch.float32, "cuda", name=name, kind="refused")

    PA = lambda t: ops._ptr_array([t] * n)
    st = ops._stream()
    a = inp(M, K, ldx, off, "x / dy")                      # x [M][K] or dy [M][K] (pair: dy [Brows][Nout])
    if entry == "mlp_fwd":
        w, bias, qw = inp(N, K, name="w"), inp(1, N, name="bias"), inp(1, N, name="qw")
        y, qp = refused(M, N, name="y"), refused(M, max(N // 32, 1), name="qpart")
        nq = ctypes.c_int(-7)
        rc = lib.drq_mlp_fwd(n, PA(a), ldx, PA(w), K, PA(y), N, M, N, K, PA(bias), 1, PA(qw),
                             None if o.get("qw_only") else PA(qp), ctypes.byref(nq), st)
        assert nq.value == -7, why
    elif entry == "mlp_dgrad":
        w, mask, dx = inp(K, N, name="w"), inp(M, N, name="mask"), refused(M, N, name="dx")
        rc = lib.drq_mlp_dgrad(n, PA(a), ldx, PA(w), N, PA(dx), N, M, N, K, PA(mask), N, st)
    else:
        x, w, mask = inp(M, N, name="x"), inp(K, N, name="w"), inp(M, N, name="mask")
        dw, db, dx = refused(K, N, name="dw"), refused(K, name="db"), refused(M, N, name="dx")
        rc = lib.drq_mlp_wgrad_dgrad(n, PA(a), ldx, PA(x), N, PA(dw), PA(db), PA(w), N, PA(dx), N, PA(mask), N, M, K, N, st)
    assert rc == EARG, (why, rc)


# ------------------------------------------------------- drq_gemm_batched_f32: LDS-free, skinny, trunk wgrad, LDS kernel
@rows("batched")
def test_batched_entry(ops, row):
    n, M, N, K, lay = row.n, row.M, row.N, row.K, row.layout
    predicted(row)
    bias = mask = None
    if lay == "fwd":
        A = [gv.make_act(M, K, seeds(row, b, 1)) for b in range(n)]
        Bm = [gv.make_weight(N, K, K, seeds(row, b, 2)) for b in range(n)]
        bias = [gv.randn(N, seed=seeds(row, b, 3)) for b in range(n)]
        A64, B64, lda, ldb = [t.double() for t in A], [t.double().t() for t in Bm], K, K
    elif lay == "dgrad":
        A = [gv.make_grad(M, K, seeds(row, b, 1)) for b in range(n)]
        Bm = [gv.make_weight(K, N, K, seeds(row, b, 2)) for b in range(n)]
        mask = [gv.make_mask(M, N, seeds(row, b, 3)) for b in range(n)]
        A64, B64, lda, ldb = [t.double() for t in A], [t.double() for t in Bm], K, N
    else:                                                   # dW [M][N] = dy [K][M]^T x [K][N]
        A = [gv.make_grad(K, M, seeds(row, b, 1)) for b in range(n)]
        Bm = [gv.make_act(K, N, seeds(row, b, 2)) for b in range(n)]
        A64, B64, lda, ldb = [t.double().t() for t in A], [t.double() for t in Bm], M, N
    Cs, rs = ops.gemm_batched([G(t, f"A{b}") for b, t in enumerate(A)], lay != "wgrad",
                              [G(t, f"B{b}") for b, t in enumerate(Bm)], lay == "fwd", M, N, K, lda, ldb,
                              biases=[G(t) for t in bias] if bias else None, relu=lay == "fwd",
                              auxs=[G(t) for t in mask] if mask else None, rowsum=lay == "wgrad",
                              tile=row.opts.get("tile", 0), splitk=row.opts.get("splitk", 0))
    for b in range(n):
        ref, mag = gv.reference(A64[b], B64[b], bias[b].double() if bias else None, relu=lay == "fwd",
                                mask=mask[b] if mask else None)
        hold(Cs[b], ref, mag, K, "batched." + gv.base(row.expect), row, mask=mask[b] if mask else None)
        if rs:
            hold(rs[b], A64[b].sum(1), A64[b].abs().sum(1), K, "batched.rowsum." + gv.base(row.expect), row)


@rows("gemm_f32")
def test_lds_kernel_forward_misaligned(ops, row):
    """drq_gemm_f32, forward layout, A one float off a 16-byte boundary: the scalar loaders under every block tile;
    C rows longer than N and problems further apart than M*ldc (gaps stay poison)"""
    n, M, N, K = row.n, row.M, row.N, row.K
    predicted(row)
    A = torch.stack([gv.make_act(M, K, seeds(row, b, 1)) for b in range(n)])
    Bm = torch.stack([gv.make_weight(N, K, K, seeds(row, b, 2)) for b in range(n)])
    bias = torch.stack([gv.randn(N, seed=seeds(row, b, 3)) for b in range(n)])
    abuf = poison.alloc((n * M * K + 1,), torch.float32, "cuda", name="A (off by one float)", kind="in")
    Ac = abuf[1:].view(n, M, K)
    Ac.copy_(A)
    assert Ac.data_ptr() % 16 == 4
    ws = poison.alloc((1024 * 1024,), torch.float32, "cuda", name="split-K workspace", kind="ws")
    ldc = N + 3
    c_bs = M * ldc + 7
    C = poison.alloc((n * c_bs,), torch.float32, "cuda", name="C", kind="ws")
    ops.gemm(Ac, True, G(Bm, "B"), True, M, N, K, bias=G(bias, "bias"), relu=True, nbatch=n, a_bs=M * K, b_bs=N * K,
             c_bs=c_bs, bias_bs=N, tile=row.opts["tile"], splitk=0, out=C, ldc=ldc, ws=ws)
    for b in range(n):
        blk = C[b * c_bs:(b + 1) * c_bs]
        assert bool(is_sent(blk[M * ldc:]).all()), "the gap between two problems was written"
        ref, mag = gv.reference(A[b].double(), Bm[b].double().t(), bias[b].double(), relu=True)
        hold(logical(blk[:M * ldc].view(M, ldc), N, f"C{b}"), ref, mag, K, "gemm_f32." + gv.base(row.expect), row)


# ------------------------------------------------------------------------------------------------ trunk forward
@rows("partial")
def test_trunk_forward_split_count(ops, row):
    """*splitk_out is the predicted one and the sum of the records is the GEMM (long-K rows: on a sample of the output
    rows that touches every 32-row tile, to keep the fp64 reference small)"""
    n, M, N, K = row.n, row.M, row.N, row.K
    sel = predicted(row)
    xs = [gv.make_act(M, K, seeds(row, b, 1)) for b in range(n)]
    ws = [gv.make_weight(N, K, K, seeds(row, b, 2)) for b in range(n)]
    got, sk = ops.gemm_batched_partial([G(t, f"x{b}") for b, t in enumerate(xs)], [G(t, f"w{b}") for b, t in enumerate(ws)],
                                       M, N, K, K, K)
    assert sk == sel.split, (gv.row_id(row), sk, sel)
    idx = torch.arange(M)
    if n * M * N * K > 2e8:
        idx = torch.unique(torch.cat([torch.arange(0, M, max(1, M // 37)), torch.tensor([M - 1])]))
    for b in range(n):
        ref, mag = gv.reference(xs[b][idx].double(), ws[b].double().t())
        hold(got[b].cpu()[idx], ref, mag, K, "partial." + gv.base(row.expect), row)
