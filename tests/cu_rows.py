"""The rows tests/test_hip_cu_counts.py runs under an override of the CU count (drq_set_num_cus, include/drqv2_hip.h): a
whole device made to plan like a partition of itself (a helper module: not collected, needs no GPU).

Every launch of the library sizes its grid from the CU count, and the kernels decide from their grid how to walk it.  At
256 CUs several of those decisions have one side only (tests/conv_variants.py: UNREACHABLE_AT_256); the rows below take
the other side at 2..128 CUs, at batches of 1 to 11 frames.  What a row
exercises -- its grids, its shares and the sides it adds to the 256-CU rows -- is computed from the restated planners of
conv_variants (describe(), new_sides()), and tests/test_cpu_conv_variants.py holds that restatement to the planners of
csrc/conv_plan.h on exactly these rows, and the 256-CU baseline to the lines of tests/test_hip_guarded.py it is read from."""
from collections import namedtuple

from tests import conv_variants as cv

# ---- whole updates: (CU count, batch, compute dtype, updates audited).  The fp32 rows are the audit of
# tests/test_hip_encoder_audit.py under an override; the bf16 row is its step_flags 12 update.
CuRow = namedtuple("CuRow", "cus B dtype updates")
CU_ROWS = [
    CuRow(32, 1, "fp32", 1),     # one XCD's worth of CUs (CPX): what a CPX user runs first
    CuRow(32, 2, "fp32", 2),     # ... and a second update on rebuilt U images
    CuRow(32, 8, "fp32", 1),
    CuRow(8, 2, "fp32", 1),
    CuRow(8, 3, "fp32", 1),
    CuRow(64, 2, "fp32", 1),     # QPX
    CuRow(128, 2, "fp32", 1),    # DPX
    CuRow(2, 1, "fp32", 1),      # fewer CUs than layers: the three-layer weight gradient refuses
    CuRow(3, 1, "fp32", 1),      # the smallest merged grid
    CuRow(32, 2, "bf16", 1),
]

# ---- single ops: (CU count, the launcher of conv_variants, its arguments without the CU count)
OpRow = namedtuple("OpRow", "cus fn args")
DIRECT_HIN = ((84, 2), (41, 1), (39, 1), (37, 1))       # (hin, stride) of the direct forward
WINO_HIN = (41, 39, 37)                                  # forward inputs; the input gradient's kernel side is hout + 4
OP_ROWS = (
    [OpRow(c, "launch_conv_v", (nb, hin, s)) for c, nb in ((8, 3), (32, 11)) for hin, s in DIRECT_HIN]
    + [OpRow(c, "launch_conv_v", (nb, hin + 2, 1)) for c, nb in ((8, 3), (32, 11)) for hin in WINO_HIN]       # dgrad
    + [OpRow(c, "launch_wino", (nb, hin + d)) for c, nb in ((8, 2), (8, 3), (32, 8)) for hin in WINO_HIN for d in (0, 2)]
    + [OpRow(c, "launch_ww", (nb, hin)) for c in (8, 16, 64) for nb in (1, 5) for hin in WINO_HIN]
    + [OpRow(8, "launch_wgrad", (nb, cin, hin, s)) for nb in (1, 3) for cin, hin, s in ((9, 84, 2), (32, 41, 1), (32, 39, 1), (32, 37, 1))]
    + [OpRow(8, "launch_conv_bf16", (9, hin + d, lay)) for hin in (41, 37) for d in (0, 2) for lay in (0, 1)]
    + [OpRow(8, "launch_wgrad_bf16", (9, hin)) for hin in (41, 37)]
    + [OpRow(8, "launch_conv1_aug", (n, 0)) for n in (103, 110, 3)]
)

# ---- the convolution launches the GPU suite already makes at 256 CUs, beside the audit rows and cv.op_test_launches():
# the fused aug+conv1 launches (tests/test_hip_guarded.py, test_hip_ops.py: n up to 200) and the bf16 forward / input
# gradient (test_hip_guarded.py CONV and its channel-contiguous rows)
# -- as (test of tests/test_hip_guarded.py, the source line that holds its shapes), in the manner of cv.OP_TEST_ROWS:
# tests/test_cpu_conv_variants.py asserts that each line still stands in front of its test, so a changed shape there
# fails here instead of leaving this baseline behind
GUARDED_ROWS = {
    "conv": ("test_conv_fwd_dgrad_wgrad_guarded", 'CONV = [(37, 3), (41, 1), (39, 256)]'),
    "aug": ("test_fused_aug_conv1_guarded", '@pytest.mark.parametrize("n", [3, 200])'),
    "aug_indexed": ("test_fused_aug_conv1_indexed_guarded", '@pytest.mark.parametrize("slots,n", [(5, 7), (300, 200)])'),
    "bf16_nhwc": ("test_conv_bf16_channel_contiguous_guarded", '@pytest.mark.parametrize("hin,nb", [(37, 3), (41, 130)])'),
}


def _shapes(key):
    return eval(GUARDED_ROWS[key][1][GUARDED_ROWS[key][1].index("["):].rstrip(")"))


AUG_N_AT_256 = tuple(_shapes("aug")) + tuple(n for _, n in _shapes("aug_indexed"))
BF16_AT_256 = [(nb, hin + d, 0) for hin, nb in _shapes("conv") for d in (0, 2)] + \
              [(nb, hin + d, 1) for hin, nb in _shapes("bf16_nhwc") for d in (0, 2)]
AUG_DECISIONS = ("conv1_aug.blocks>cap", "conv1_aug.table_full")
BF16_DECISIONS = ("conv_bf16.blocks>cap",)


def launches_at_256():
    """(stage, Launch) of every convolution launch named above, at the hardware count"""
    out = []
    for r in cv.AUDIT_ROWS:
        out += cv.update_launches(r.B, r.dtype)
        out.append(("conv1_aug", cv.launch_conv1_aug(r.B, 6 if r.dtype == "fp32" else 0)))
    out += cv.op_test_launches()
    out += [("conv1_aug", cv.launch_conv1_aug(n, 0)) for n in AUG_N_AT_256]
    out += [("conv_bf16", cv.launch_conv_bf16(nb, hin, lay)) for nb, hin, lay in BF16_AT_256]
    return out


def row_launches(row):
    """(stage, Launch) of one row of CU_ROWS (the update's launches and its fused aug+conv1) or of OP_ROWS"""
    if isinstance(row, CuRow):
        riders = 6 if row.dtype == "fp32" else 0
        return cv.update_launches(row.B, row.dtype, row.cus) + [("conv1_aug", cv.launch_conv1_aug(row.B, riders, row.cus))]
    return [(row.fn, getattr(cv, row.fn)(*row.args, cus=row.cus))]


def override_launches():
    return [la for row in list(CU_ROWS) + list(OP_ROWS) for la in row_launches(row)]


def new_sides(row, seen=None):
    """{decision: sides} this row takes that no launch at 256 CUs does"""
    seen = cv.decisions_of(launches_at_256()) if seen is None else seen
    return {k: sorted(v - seen.get(k, set())) for k, v in cv.decisions_of(row_launches(row)).items() if v - seen.get(k, set())}


def describe(row):
    """one line on what an update row launches, read off the restated planners"""
    la = dict(row_launches(row))
    w3 = la.get("dW2-4")
    parts = ["%d CUs B=%d %s" % (row.cus, row.B, row.dtype)]
    if row.dtype == "fp32":
        parts.append("wino fwd %s igrad %s" % ([la[s].grid for s in ("ACT2", "ACT3", "FEAT")], [la[s].grid for s in ("DY3", "DY2", "DY1")]))
        parts.append("ww3 refused, per layer %s" % [la["dW%d" % l].grid for l in (2, 3, 4)] if w3.kernel == cv.EARG
                     else "ww3 grid %d shares %s" % (w3.grid, w3.records))
    parts.append("dW1 %d records, conv1_aug %d" % (la["dW1"].grid, la["conv1_aug"].grid))
    new = new_sides(row)
    parts.append("new: " + (", ".join("%s=%s" % (k, "/".join(str(s) for s in v)) for k, v in sorted(new.items())) or "none"))
    return "; ".join(parts)


# Far sides of UNREACHABLE_AT_256 that stay unreachable: no CU count up to 256 takes them at any batch 1..4096
# (tests/test_cpu_conv_variants.py sweeps SWEEP_CUS and asserts each entry).
STILL_UNREACHABLE = {
    "ww3.share<1": "a share rounds to zero only where steps[l] * cus < tot / 2; the three layers' steps are within 25 % "
                   "of each other (th = 20, 19, 18: 400 : 361 : 324), so every share is at least 0.29 cus, which is "
                   "above one half for every cus >= 3 the merged launch accepts",
}


# ---- the head section and the GEMM family (tests/head_variants.py, tests/gemm_variants.py) at 32 and 8 CUs
FAMILY_CUS = (32, 8)


def head_rows():
    """the smallest row (B A F H) of each mode of the head audit"""
    from tests import head_variants as hv
    small = {}
    for r in hv.AUDIT_ROWS:
        if r.mode not in small or r.B * r.A * r.F * r.H < small[r.mode].B * small[r.mode].A * small[r.mode].F * small[r.mode].H:
            small[r.mode] = r
    return list(small.values())
