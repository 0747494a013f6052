"""The host-side dispatch of the fp32 GEMM family, restated in plain Python, and the table of op-test cases built on it
(a helper module: not collected, needs no GPU).

One public call can land on many kernels depending on shape, alignment and the CU count.  The library decides that in
one place, the planners of drqv2_amd/csrc/gemm_plan.h (plan_ring, plan_batched, plan_partial); the functions below
restate their fp32 rules (the 2 GiB operand-size refusals are left out: no test shape comes near them) and also record
each threshold decision on the way, which the planner does not.  tests/test_cpu_gemm_variants.py compiles the planner
for the host and holds this restatement to it, variant, split count and nq, over the table and a sweep across every
threshold; it also says which variant lost its test row or which threshold is no longer tested on both sides.
tests/test_hip_gemm_variants.py asserts the two decisions the ABI shows (*nq_out of drq_mlp_fwd, *splitk_out of
drq_gemm_batched_partial).

Every function returns a Sel: the variant name (EARG = the entry refuses), the split count where there is one, the
number of partial-dot columns of the forward, and the threshold decisions it took on the way (name -> bool).
compare() is the bound every GPU row is held to; make_*() are the inputs.
"""
from collections import namedtuple

import numpy as np
import torch

CUS = 256                       # drq_num_cus() on the MI355X: the table is built for it
U = 2.0 ** -24                  # unit roundoff of fp32
NORMWISE = 3e-6
EARG = "EARG"

Sel = namedtuple("Sel", "name split nq decisions")


def _cdiv(a, b):
    return -(-a // b)


class _D(dict):
    def __call__(self, key, value):
        self[key] = bool(value)
        return bool(value)


def _sel(name, d, split=None, nq=None):
    return Sel(name, split, nq, dict(d))


# ---------------------------------------------------------------------------------------------- plan_ring
def _g3_fill(n, M, N, K, lda, ldb, aligned):
    if n <= 0 or n > 8 or M % 64 or N % 32 or K % 32 or M < 64 or N < 32 or K < 64:
        return False
    if lda % 4 or ldb % 4:
        return False
    return bool(aligned)


def ring_fwd(n, M, N, K, ldx=None, ldw=None, aligned=True, qw=False, qpart=None, cus=CUS):
    """drq_mlp_fwd -> drq_gemm3_fwd"""
    d = _D()
    ldx, ldw = K if ldx is None else ldx, K if ldw is None else ldw
    qpart = qw if qpart is None else qpart
    if not _g3_fill(n, M, N, K, ldx, ldw, aligned) or N % 64 or bool(qw) != bool(qpart):
        return _sel(EARG, d)
    if d("g3_fwd.t64>=cus", (M // 64) * (N // 64) * n >= cus):
        d("xcd.remap", ((M // 64) * (N // 64) * n) % 8 == 0)
        return _sel("g3_fwd_64x64", d, nq=N // 64)
    d("xcd.remap", ((M // 64) * (N // 32) * n) % 8 == 0)
    return _sel("g3_fwd_64x32", d, nq=N // 32)


def ring_dgrad(n, M, N, K, lddy=None, ldw=None, aligned=True, cus=CUS):
    """drq_mlp_dgrad -> drq_gemm3_dgrad: dx [M][N] = dy [M][K] w [K][N]"""
    d = _D()
    lddy, ldw = K if lddy is None else lddy, N if ldw is None else ldw
    if not _g3_fill(n, M, N, K, lddy, ldw, aligned) or N % 64:
        return _sel(EARG, d)
    if d("g3_dgrad.t64>=cus", (M // 64) * (N // 64) * n >= cus):
        d("xcd.remap", ((M // 64) * (N // 64) * n) % 8 == 0)
        return _sel("g3_dgrad_64x64", d)
    d("xcd.remap", ((M // 64) * (N // 32) * n) % 8 == 0)
    return _sel("g3_dgrad_64x32", d)


def ring_pair(n, Brows, Nout, Kin, lddy=None, ldx=None, ldw=None, aligned=True, cus=CUS):
    """drq_mlp_wgrad_dgrad -> drq_gemm3_wgrad_dgrad"""
    d = _D()
    lddy, ldx, ldw = Nout if lddy is None else lddy, Kin if ldx is None else ldx, Kin if ldw is None else ldw
    if not _g3_fill(n, Nout, Kin, Brows, lddy, ldx, aligned) or not _g3_fill(n, Brows, Kin, Nout, lddy, ldw, aligned):
        return _sel(EARG, d)
    if Kin % 64 or Nout % 64 or Brows % 64:
        return _sel(EARG, d)
    nxw = (Nout // 64) * (Kin // 64)
    big = d("g3_pair.td64>=cus", (Brows // 64) * (Kin // 64) * n >= cus)
    nxd = (Brows // 64) * (Kin // (64 if big else 32))
    # xcd_decode is applied to the two halves of the grid separately
    rw, rd = (nxw * n) % 8 == 0, (nxd * n) % 8 == 0
    d("xcd.remap_w", rw), d("xcd.remap_d", rd), d("xcd.remap_mixed", rw != rd)
    return _sel("g3_pair_d64" if big else "g3_pair_d32", d)


# ------------------------------------------------------------------- plan_batched, plan_partial (fp32)
def batched(layout, n, M, N, K, lda=None, ldb=None, a_al=True, b_al=True, tile=0, splitk=0, bias=False, relu=False,
            aux=False, rowsum=False, scatter_hw=0, cus=CUS, _d=None):
    """drq_gemm_batched_f32 / drq_gemm_f32 -> drq_gemm_batched_any(bf16 = 0)"""
    d = _D() if _d is None else _d
    a_kc, b_kc = layout != "wgrad", layout == "fwd"
    lda = (K if a_kc else M) if lda is None else lda
    ldb = (K if b_kc else N) if ldb is None else ldb
    if M <= 0 or N <= 0 or K <= 0 or n <= 0 or n > 8 or (rowsum and a_kc):
        return _sel(EARG, d)
    plain = n == 1 and tile == 0 and splitk == 0 and not bias and not relu
    # the skinny dgrad kernel
    if plain and layout == "dgrad" and not rowsum and N % 32 == 0:
        if d("skinny.N>=4096", N >= 4096) and d("skinny.K<=128", K <= 128):
            return _sel("skinny_dgrad", d)
    # the trunk weight gradient
    if plain and scatter_hw == 0 and layout == "wgrad" and not aux:
        if d("trunk_wgrad.M<=128", M <= 128) and d("trunk_wgrad.N>=4096", N >= 4096) and N % 32 == 0:
            if d("trunk_wgrad.K in {128,256,512}", K in (128, 256, 512)):
                return _sel("trunk_wgrad_%d" % (K // 32), d)
    # the LDS-free kernel (not the forward layout)
    if tile == 0 and splitk == 0 and scatter_hw == 0:
        ok = M % 32 == 0 and N % 32 == 0 and K % 32 == 0 and K >= 64 and M >= 32 and N >= 32 and not b_kc
        if a_kc:
            ok = ok and lda % 4 == 0 and a_al
        if d("g2.eligible", ok):
            tiles = (M // 32) * (N // 32)
            split = (d("g2.tiles*n<8cus", tiles * n < 4 * cus * 2) and d("g2.K%128==0", K % 128 == 0)
                     and d("g2.K>=512", K >= 512))
            return _sel("g2_ks4" if split else "g2_ks1", d)
    # the LDS-staged kernel
    t_big = _cdiv(M, 64) * _cdiv(N, 64) * n
    t_small = _cdiv(M, 32) * _cdiv(N, 32) * n
    if tile == 0:
        tile = 2 if d("lds.auto.t_big>=2cus", t_big >= 2 * cus) else 1
    tiles = t_big if tile == 2 else ((t_big + t_small) // 2 if tile >= 3 else t_small)
    if rowsum:
        splitk = 1
    if splitk == 0:
        splitk = 1
        if d("lds.autosplit.tiles<2cus", tiles < 2 * cus) and d("lds.autosplit.K>=256", K >= 256):
            splitk = max(1, min(_cdiv(3 * cus, tiles), K // 128))
    kchunk = _cdiv(_cdiv(K, splitk), 64) * 64
    splitk = _cdiv(K, kchunk)
    v4 = K % 4 == 0 and (a_kc or b_kc)
    if a_kc:
        v4 = v4 and lda % 4 == 0 and a_al
    if b_kc:
        v4 = v4 and ldb % 4 == 0 and b_al
    if layout == "wgrad":
        v4 = False                                   # both operands row-contiguous -> the scalar loaders
    else:
        d("lds.v4", v4)
    if tile not in (2, 3, 4, 5, 6):
        tile = 1
    name = "lds_tile%d_%s" % (tile, "v4" if v4 else "scalar")
    if tile == 1 and layout == "fwd" and v4 and d("lds.full", M % 32 == 0 and N % 32 == 0 and K % 32 == 0):
        name += "_full"
    return _sel(name, d, split=splitk)


def partial(n, M, N, K, lda=None, ldb=None, ldc=None, aligned=True, cus=CUS):
    """drq_gemm_batched_partial (fp32, forward layout) -> drq_trunk_fwd_partial or the LDS kernel with tile = 1"""
    d = _D()
    lda, ldb, ldc = K if lda is None else lda, K if ldb is None else ldb, N if ldc is None else ldc
    if N <= 128 and d("trunk_fwd.K>=4096", K >= 4096) and ldc == N:
        ok = 0 < n <= 8 and M % 32 == 0 and M >= 32 and N >= 1 and K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0
        if ok and aligned:
            steps = K // 32
            wide = d("trunk_fwd.N>64", N > 64)
            tm2 = (not wide and d("trunk_fwd.M%64==0", M % 64 == 0)
                   and d("trunk_fwd.n*(M/32)*4>=64", n * (M // 32) * 4 >= 64))
            rows = M // 64 if tm2 else M // 32
            bk = _cdiv(cus, n * rows)
            if d("trunk_fwd.4*blocks_k>steps", bk * 4 > steps):
                bk = steps // 4
            if d("trunk_fwd.blocks_k>64", bk > 64):
                bk = 64
            if bk >= 2:
                return _sel("trunk_fwd_wide" if wide else "trunk_fwd_tm2" if tm2 else "trunk_fwd_tm1", d, split=bk)
    return batched("fwd", n, M, N, K, lda, ldb, aligned, aligned, tile=1, cus=cus, _d=d)


VARIANTS = (
    ["g3_fwd_64x64", "g3_fwd_64x32", "g3_dgrad_64x64", "g3_dgrad_64x32", "g3_pair_d64", "g3_pair_d32", "g2_ks1", "g2_ks4",
     "skinny_dgrad", "trunk_wgrad_4", "trunk_wgrad_8", "trunk_wgrad_16", "trunk_fwd_tm1", "trunk_fwd_tm2",
     "trunk_fwd_wide", "lds_tile1_v4_full"]
    + ["lds_tile%d_%s" % (t, v) for t in range(1, 7) for v in ("v4", "scalar")])

THRESHOLDS = (
    "g3_fwd.t64>=cus", "g3_dgrad.t64>=cus", "g3_pair.td64>=cus", "xcd.remap", "xcd.remap_w", "xcd.remap_d",
    "xcd.remap_mixed", "skinny.N>=4096", "skinny.K<=128", "trunk_wgrad.M<=128", "trunk_wgrad.N>=4096",
    "trunk_wgrad.K in {128,256,512}", "g2.eligible", "g2.tiles*n<8cus", "g2.K%128==0", "g2.K>=512",
    "lds.auto.t_big>=2cus", "lds.autosplit.tiles<2cus", "lds.autosplit.K>=256", "lds.v4", "lds.full",
    "trunk_fwd.K>=4096", "trunk_fwd.N>64", "trunk_fwd.M%64==0", "trunk_fwd.n*(M/32)*4>=64",
    "trunk_fwd.4*blocks_k>steps", "trunk_fwd.blocks_k>64")


# ------------------------------------------------------------------------------------------------ the table
# entry: mlp_fwd / mlp_dgrad / mlp_pair (the ring kernel; the pair's M, N, K are Brows, Kin, Nout: those of its input-
# gradient half), batched (drq_gemm_batched_f32 through ops.gemm_batched: dgrad rows carry a mask, wgrad rows the fused
# row sum, fwd rows bias + ReLU), gemm_f32 (drq_gemm_f32, forward layout, A one float off a 16-byte boundary),
# partial (drq_gemm_batched_partial).  expect: variant, "/s<split count>" where the call has one.
Row = namedtuple("Row", "entry layout n M N K opts expect edge")


def _r(entry, layout, n, M, N, K, expect, edge, **opts):
    return Row(entry, layout, n, M, N, K, opts, expect, edge)


def _build_table():
    T = []
    for e, lay, big, small in (("mlp_fwd", "fwd", "g3_fwd_64x64", "g3_fwd_64x32"),
                               ("mlp_dgrad", "dgrad", "g3_dgrad_64x64", "g3_dgrad_64x32"),
                               ("mlp_pair", "pair", "g3_pair_d64", "g3_pair_d32")):
        T.append(_r(e, lay, 8, 128, 1024, 64, big, "exactly 256 64x64 tiles (>=), 2 k-tiles in a 6-stage ring"))
        T.append(_r(e, lay, 8, 128, 960, 64, small, "240 64x64 tiles: just below the threshold"))
        if e != "mlp_pair":
            for K in range(64, 449, 32):
                T.append(_r(e, lay, 1, 64, 64, K, small, "%d k-tiles: residue %d mod 6 stages, %d mod 2 wave groups"
                            % (K // 32, (K // 32) % 6, (K // 32) % 2)))
            for K in (96, 160, 192, 224, 416):
                T.append(_r(e, lay, 8, 128, 1024, K, big, "%d k-tiles in the 64x64 variant" % (K // 32)))
            for n in (3, 4, 5, 7, 8):
                T.append(_r(e, lay, n, 64, 64, 96, small, "%d problems, %d workgroups (%s multiple of 8)"
                            % (n, 2 * n, "a" if (2 * n) % 8 == 0 else "no")))
            T.append(_r(e, lay, 2, 128, 192, 96, small, "every leading dimension longer than its row", ld=True))
        else:
            for B in (64, 128, 192, 320):
                T.append(_r(e, lay, 1, B, 64, 64, small, "%d k-tiles in the 4-stage weight-gradient half" % (B // 32)))
            for n in (3, 4, 5, 7, 8):
                T.append(_r(e, lay, n, 64, 64, 64, small, "%d problems: %d + %d workgroups in the two halves"
                            % (n, n, 2 * n)))
            T.append(_r(e, lay, 2, 128, 192, 128, small, "every leading dimension longer than its row", ld=True))
    # ---- LDS-free kernel
    for lay in ("dgrad", "wgrad"):
        for n in (1, 3):
            T.append(_r("batched", lay, n, 96, 96, 64, "g2_ks1", "9 tiles: the last packed workgroup has one live wave"))
        T.append(_r("batched", lay, 1, 32, 32, 384, "g2_ks1", "K below the k-split"))
        T.append(_r("batched", lay, 1, 32, 32, 512, "g2_ks4", "K at the k-split: 4 k-steps per wave"))
        T.append(_r("batched", lay, 1, 32, 32, 576, "g2_ks1", "K >= 512 but no multiple of 128"))
        T.append(_r("batched", lay, 1, 32, 32, 640, "g2_ks4", "5 k-steps per wave (odd)"))
        T.append(_r("batched", lay, 1, 32, 64, 512, "g2_ks4", "k-split with mask / fused row sum"))
        T.append(_r("batched", lay, 8, 64, 64, 128, "g2_ks1", "8 problems, packed form"))
        T.append(_r("batched", lay, 8, 32, 32, 512, "g2_ks4", "8 problems, k-split form"))
        T.append(_r("batched", lay, 2, 37, 50, 130, "lds_tile1_scalar/s1", "ragged: not the LDS-free kernel's"))
    T.append(_r("batched", "dgrad", 8, 512, 512, 512, "g2_ks1", "2048 tiles: the chip is full without the k-split"))
    # ---- skinny dgrad and its neighbours
    T.append(_r("batched", "dgrad", 1, 33, 4096, 50, "skinny_dgrad", "smallest N of the skinny kernel, ragged M"))
    T.append(_r("batched", "dgrad", 1, 32, 4096, 128, "skinny_dgrad", "largest K of the skinny kernel"))
    T.append(_r("batched", "dgrad", 1, 32, 4096, 160, "g2_ks1", "K past the skinny kernel"))
    T.append(_r("batched", "dgrad", 1, 32, 4064, 64, "g2_ks1", "N below the skinny kernel"))
    T.append(_r("batched", "dgrad", 1, 33, 4096, 160, "lds_tile1_v4/s1", "neither skinny nor LDS-free"))
    # ---- trunk weight gradient
    for M in (1, 32, 33, 128):
        for K in (128, 256, 512):
            for N in (4096, 4128):
                T.append(_r("batched", "wgrad", 1, M, N, K, "trunk_wgrad_%d" % (K // 32),
                            "%d column tiles for %d wave groups" % (N // 32, 1024 // _cdiv(M, 32))))
    T.append(_r("batched", "wgrad", 1, 33, 4096, 384, "lds_tile1_scalar/s1", "K without a register depth: generic kernel"))
    T.append(_r("batched", "wgrad", 1, 160, 4096, 128, "g2_ks1", "M past the trunk weight gradient"))
    T.append(_r("batched", "wgrad", 1, 32, 4064, 128, "g2_ks1", "N below the trunk weight gradient"))
    # ---- LDS kernel, forward layout, aligned
    for tile in range(1, 7):
        T.append(_r("batched", "fwd", 2, 37, 50, 132, "lds_tile%d_v4/s1" % tile, "ragged in every tile", tile=tile))
    T.append(_r("batched", "fwd", 2, 37, 50, 132, "lds_tile5_v4/s3", "explicit split, k-tile 64", tile=5, splitk=3))
    T.append(_r("batched", "fwd", 1, 64, 64, 64, "lds_tile1_v4_full/s1", "the variant without range masks", tile=1))
    T.append(_r("batched", "fwd", 2, 256, 256, 256, "lds_tile1_v4_full/s2", "auto tile 1, auto split at K = 256"))
    T.append(_r("batched", "fwd", 8, 512, 512, 64, "lds_tile2_v4/s1", "512 64x64 tiles: auto tile 2 (>=), no split"))
    # ---- LDS kernel, forward layout, A off a 16-byte boundary: the scalar loaders under every tile
    for M, N, K, s in ((37, 50, 130, 1), (256, 256, 256, 2)):
        for tile in range(0, 7):
            T.append(_r("gemm_f32", "fwd", 2, M, N, K, "lds_tile%d_scalar/s%d" % (max(tile, 1), s),
                        "A 4 bytes off a 16-byte boundary", tile=tile))
    # ---- trunk forward (split-K records)
    for M, N, K, n, exp, edge in (
            (256, 50, 39200, 4, "trunk_fwd_tm2/s16", "the critic update's four trunks"),
            (256, 50, 39200, 1, "trunk_fwd_tm1/s32", "one problem: too few row tiles for two per wave"),
            (64, 50, 4096, 2, "trunk_fwd_tm1/s32", "split limited by 4 k-steps per workgroup"),
            (32, 64, 4128, 1, "trunk_fwd_tm1/s32", "N = 64: the widest two-tile form, slices of unequal length"),
            (96, 7, 8192, 3, "trunk_fwd_tm1/s29", "M no multiple of 64"),
            (512, 50, 39200, 1, "trunk_fwd_tm2/s32", "16 row tiles: at the two-row-tile threshold"),
            (256, 100, 39200, 4, "trunk_fwd_wide/s8", "feature_dim 100"),
            (32, 100, 39200, 1, "trunk_fwd_wide/s64", "split capped at 64 records"),
            (64, 65, 4096, 2, "trunk_fwd_wide/s32", "N = 65: first wide shape"),
            (32, 128, 4096, 1, "trunk_fwd_wide/s32", "N = 128: last wide shape"),
            (32, 100, 4128, 1, "trunk_fwd_wide/s32", "wide, slices of unequal length"),
            (64, 64, 4096, 8, "trunk_fwd_tm2/s32", "8 problems, at the two-row-tile threshold"),
            (64, 50, 4096, 7, "trunk_fwd_tm1/s19", "7 problems: just below the two-row-tile threshold"),
            (96, 7, 4096, 6, "trunk_fwd_tm1/s15", "enough row tiles, but M no multiple of 64"),
            (64, 50, 4064, 2, "lds_tile1_v4/s22", "K below the trunk kernel: LDS kernel, records kept")):
        T.append(_r("partial", "fwd", n, M, N, K, exp, edge))
    return T


TABLE = _build_table()

# calls the ring entries must refuse without writing anything: (entry, n, M, N, K, options, why)
REFUSALS = [
    ("mlp_fwd", 9, 64, 64, 64, {}, "nbatch = 9"),
    ("mlp_fwd", 1, 64, 64, 64, {"ldx": 66}, "ldx % 4 != 0"),
    ("mlp_fwd", 1, 64, 64, 64, {"misalign": True}, "x 4 bytes off a 16-byte boundary"),
    ("mlp_fwd", 1, 64, 64, 32, {}, "K = 32"),
    ("mlp_fwd", 1, 64, 32, 64, {}, "N = 32 (the forward needs N % 64 == 0)"),
    ("mlp_fwd", 1, 64, 64, 64, {"qw_only": True}, "qw without qpart"),
    ("mlp_dgrad", 9, 64, 64, 64, {}, "nbatch = 9"),
    ("mlp_dgrad", 1, 64, 64, 64, {"ldx": 66}, "lddy % 4 != 0"),
    ("mlp_dgrad", 1, 64, 64, 64, {"misalign": True}, "dy 4 bytes off a 16-byte boundary"),
    ("mlp_dgrad", 1, 64, 64, 32, {}, "K = 32"),
    ("mlp_pair", 9, 64, 64, 64, {}, "nbatch = 9"),
    ("mlp_pair", 1, 64, 64, 64, {"ldx": 66}, "lddy % 4 != 0"),
    ("mlp_pair", 1, 64, 64, 64, {"misalign": True}, "dy 4 bytes off a 16-byte boundary"),
    ("mlp_pair", 1, 64, 64, 32, {}, "Nout = 32"),
]


def select(row, cus=CUS):
    """the Sel the helper predicts for a table row (or a REFUSALS tuple turned into a Row)"""
    n, M, N, K, o = row.n, row.M, row.N, row.K, row.opts
    pad = 4 if o.get("ld") else 0
    if row.entry == "mlp_fwd":
        return ring_fwd(n, M, N, K, o.get("ldx", K + pad), K + 2 * pad, not o.get("misalign"), qw=True,
                        qpart=not o.get("qw_only"), cus=cus)
    if row.entry == "mlp_dgrad":
        return ring_dgrad(n, M, N, K, o.get("ldx", K + pad), N + 2 * pad, not o.get("misalign"), cus=cus)
    if row.entry == "mlp_pair":
        return ring_pair(n, M, K, N, o.get("ldx", K + pad), N + pad, N + 2 * pad, not o.get("misalign"), cus=cus)
    if row.entry == "batched":
        return batched(row.layout, n, M, N, K, tile=o.get("tile", 0), splitk=o.get("splitk", 0),
                       bias=row.layout == "fwd", relu=row.layout == "fwd", aux=row.layout == "dgrad",
                       rowsum=row.layout == "wgrad", cus=cus)
    if row.entry == "gemm_f32":
        return batched("fwd", n, M, N, K, a_al=False, tile=o.get("tile", 0), bias=True, relu=True, cus=cus)
    if row.entry == "partial":
        return partial(n, M, N, K, cus=cus)
    raise ValueError(row.entry)


def label(sel):
    return sel.name if sel.split is None or sel.name == EARG else "%s/s%d" % (sel.name, sel.split)


def base(name):
    return name.split("/")[0]


def row_id(row):
    o = "".join("-%s%s" % (k, "" if v is True else v) for k, v in sorted(row.opts.items()))
    return "%s-%s-n%d-%dx%dx%d%s" % (row.entry, row.layout, row.n, row.M, row.N, row.K, o)


# ------------------------------------------------------------------------------------------------ inputs
def _rs(*key):
    return np.random.RandomState([abs(int(k)) % (2 ** 31) for k in key])


def randn(*shape, seed, scale=1.0):
    return torch.from_numpy((_rs(*seed).standard_normal(shape) * scale).astype(np.float32))


def make_weight(rows, cols, K, seed):
    """randn * K^-1/2"""
    return randn(rows, cols, seed=seed, scale=K ** -0.5)


def make_act(rows, cols, seed):
    """post-ReLU activations: about half the elements are exactly 0.0f"""
    return torch.relu(randn(rows, cols, seed=seed))


def make_grad(rows, cols, seed):
    """a gradient that came through a ReLU mask: both signs, about half the elements exactly 0.0f"""
    return randn(rows, cols, seed=seed) * (randn(rows, cols, seed=tuple(seed) + (1,)) > 0).float()


# planted in every 32x32 tile of a mask (row, column, value): first and last row and column included
PLANTED = ((0, 0, float("nan")), (0, 31, -0.0), (31, 0, 0.0), (31, 31, float("nan")), (0, 5, 0.0), (5, 0, -0.0),
           (31, 7, -0.0), (7, 31, 0.0), (13, 17, float("nan")), (14, 17, 1.0), (0, 1, 1.0), (31, 30, 1.0))


def make_mask(rows, cols, seed):
    """relu(randn) with +0.0, -0.0 and NaN (and a few certain positives) planted in every 32x32 tile; the kernels'
    contract is `mask > 0`, which is false for all three"""
    m = torch.relu(randn(rows, cols, seed=seed))
    for r0 in range(0, rows, 32):
        for c0 in range(0, cols, 32):
            for r, c, v in PLANTED:
                if r0 + r < rows and c0 + c < cols:
                    m[r0 + r, c0 + c] = v
    return m


# ------------------------------------------------------------------------------------------------ the comparison
def reference(A64, B64, bias64=None, relu=False, mask=None):
    """fp64 C = epi(A B + bias) and the componentwise magnitude (|A| |B| + |bias|), zero where the mask is not > 0"""
    ref = A64 @ B64
    mag = A64.abs() @ B64.abs()
    if bias64 is not None:
        ref = ref + bias64
        mag = mag + bias64.abs()
    if relu:
        ref = torch.relu(ref)                        # 1-Lipschitz: the bound carries over
    if mask is not None:
        keep = (mask > 0).to(ref.dtype)              # false for +0.0, -0.0 and NaN
        ref, mag = ref * keep, mag * keep
    return ref, mag


def compare(got, ref, mag, K):
    """(ok, normwise error, largest componentwise error / bound).  Normwise: the project's 3e-6.  Componentwise:
    |got - ref| <= 2 (K+2) 2^-24 mag, the any-order summation bound (K products, K-1 additions, the bias addition, the
    final rounding; the factor 2 for re-added split-K records and the MFMA's internal order).  Where mag is 0 (masked
    out, or an all-zero dot) the result must be exactly zero; a NaN never passes."""
    g = got.detach().double().cpu()
    err = (g - ref).abs()
    bound = 2.0 * (K + 2) * U * mag
    bad = ~(err <= bound)                            # NaN -> bad
    nerr = float(err.norm() / ref.norm().clamp_min(1e-30)) if not bool(torch.isnan(err).any()) else float("nan")
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    if bool(bad.any()) and not ratio > 1.0:
        ratio = float("inf")                         # a nonzero (or NaN) where the bound is exactly zero
    return (not bool(bad.any())) and nerr <= NORMWISE, nerr, ratio
