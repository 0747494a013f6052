"""The host-side launch arithmetic of the convolution family, restated in plain Python, and the list of batch sizes the
per-launch audit of the fused update runs (a helper module: not collected, needs no GPU).

The grid of a convolution launch, the number of partial records it leaves and the way a workgroup walks its share all
depend on the batch and on the CU count.  The functions below mirror, rule for rule,

  csrc/conv.hip             launch_conv_v(), launch_wgrad(), conv3x3_wgrad_reduce_multi_kernel (its record loop)
  csrc/conv_wino.hip        launch_wino() and the work split at the top of conv3x3_wino_kernel
  csrc/conv_wino_wgrad.hip  launch_ww(), drq_conv3x3_wgrad_partial_wino3(), the XCD remap of both kernels
  csrc/conv_bf16.hip        launch_conv_bf16() (the grid), launch_wgrad_bf16() (the records it feeds the same reduce kernel)
  csrc/conv1aug.hip         drq_conv1_aug_fwd_any() (the grid)
  csrc/step.hip             phase_encode() / phase_conv_backward(): which of these one update issues, with which batch

(the 2 GiB operand-size refusals are left out: no test shape comes near them).  The host side of those functions now
lives in csrc/conv_plan.h, and tests/test_cpu_conv_variants.py holds this module against it through
tests/conv_plan_dump.cpp: the grid, the records and the merged-or-fallback choice of every function below, for batches
1..4096, every instantiated geometry and eight CU counts.  A change to a planner that is not repeated here fails that
sweep; the test then also says which decision is no longer taken on both sides by the rows of
tests/test_hip_encoder_audit.py.  What a kernel decides for itself from its grid cannot be read from the host and stays
restated here only: the Winograd kernel's unit split (wino.full_rounds, wino.left_over*), the XCD remaps (*.xcd_remap),
conv_v.rounds>1, the ragged ends and the record loop of the reduce (reduce.*).

Every function takes the CU count (default 256, drq_num_cus() on the MI355X) and returns a Launch: the kernel, its grid,
the partial records it leaves for the reduce (None where there are none) and the decisions taken on the way
(name -> bool).
"""
from collections import namedtuple

CUS = 256
EARG = "EARG"
ENC_H = (84, 41, 39, 37, 35)            # kEncH: the side of the encoder input and of the four layer outputs

Launch = namedtuple("Launch", "kernel grid records decisions")


def _cdiv(a, b):
    return -(-a // b)


class _D(dict):
    def __call__(self, key, value):
        self[key] = bool(value)
        return bool(value)


# ------------------------------------------------------------------------------------------------- csrc/conv.hip
def launch_conv_v(nb, hin, stride, blk=2, tpw=1, cus=CUS):
    """launch_conv_v<CIN, HIN, STRIDE, BLK, TPW>: the direct forward / input-gradient kernel (512 threads = 8 waves, a
    contiguous run of `per` 32-pixel tiles per workgroup, one tile per wave and round)"""
    d = _D()
    hout = (hin - 3) // stride + 1
    ntiles = (nb * hout * hout + 31) // 32
    blocks = (ntiles + 8 * tpw - 1) // (8 * tpw)
    if d("conv_v.blocks>cap", blocks > blk * cus):
        blocks = blk * cus
    blocks = max(blocks, 1)
    per = _cdiv(ntiles, blocks)
    d("conv_v.rounds>1", per > 8)
    d("conv_v.ragged_last_tile", (nb * hout * hout) % 32 != 0)
    return Launch("conv3x3_kernel", blocks, None, dict(d))


def launch_wgrad(nb, cin, hin, stride, cus=CUS):
    """launch_wgrad<CIN, HIN, STRIDE>: the direct weight gradient; one partial record per workgroup.  SMALL (conv1:
    3 cin <= 32) runs two workgroups per CU."""
    d = _D()
    hout = (hin - 3) // stride + 1
    small = cin * 3 <= 32
    units = (nb * hout + 3) // 4
    blocks = (2 if small else 1) * cus
    if d("wgrad.blocks>units", blocks > units):
        blocks = units
    blocks = max(blocks, 1)
    d("wgrad.units_ragged", (nb * hout) % 4 != 0)
    return Launch("conv3x3_wgrad_kernel" if small else "conv3x3_wgrad3_kernel", blocks, [blocks], dict(d))


def reduce_records(nblocks):
    """the record loop of conv3x3_wgrad_reduce_multi_kernel for one job: 16 groups of threads take records grp, grp+16,
    ..., sixteen in flight per pass (loads past the end are clamped to the last record and not added)"""
    d = _D()
    d("reduce.records<16", nblocks < 16)            # some of the 16 groups never enter the loop
    d("reduce.records<256", nblocks < 256)          # no group has sixteen live records in flight
    d("reduce.second_pass", nblocks > 256)          # k0 += 256 runs again
    d("reduce.clamped_loads", nblocks % 256 != 0)   # min(k0 + 16 u, nblocks - 1) clamps in the last pass
    return dict(d)


def reduce_multi(records, cins):
    """drq_conv3x3_wgrad_reduce_multi: grid (largest record / 64, jobs); the decisions of every job, in job order"""
    assert 0 < len(records) <= 4 and len(records) == len(cins)
    part = [(3 if c * 3 <= 32 else 9) * 1024 + 64 for c in cins]
    return Launch("conv3x3_wgrad_reduce_multi_kernel", (max(part) // 64, len(records)), None,
                  [reduce_records(n) for n in records])


# -------------------------------------------------------------------------------------------- csrc/conv_wino.hip
def launch_wino(nb, hin, cus=CUS):
    """launch_wino<HIN> and the work split of conv3x3_wino_kernel.  hin is the kernel's input side: the layer input in
    the forward, the zero-padded gradient (hout + 4) in the input gradient.  A unit is 16 tiles of 2x2 outputs; a wave
    takes whole units round-robin and the left-over units are cut in halves where that evens the load."""
    d = _D()
    hout = hin - 2
    th = (hout + 1) // 2
    ntile = nb * th * th
    nunit = (ntile + 15) // 16
    blocks = (nunit + 3) // 4
    if d("wino.blocks>cap", blocks > 2 * cus):
        blocks = 2 * cus
    blocks = max(blocks, 1)
    d("wino.xcd_remap", blocks & 15 == 0)
    nwave = blocks * 4
    q, r = nunit // nwave, nunit % nwave
    nf = 2 * r - nwave if 2 * r > nwave else 0
    d("wino.full_rounds", q > 0)
    d("wino.left_over", r > 0)
    d("wino.left_over_whole", nf > 0)               # 2r > nwave: the first nf waves take a whole left-over unit
    d("wino.left_over_halves", r - nf > 0)          # waves that take a half-unit
    d("wino.ragged_last_unit", ntile % 16 != 0)
    return Launch("conv3x3_wino_kernel", blocks, None, dict(d))


# -------------------------------------------------------------------------------------- csrc/conv_wino_wgrad.hip
def _ww_steps(nb, hin):
    th = (hin - 1) // 2
    return (nb * th * th + 3) // 4


def launch_ww(nb, hin, cus=CUS):
    """launch_ww<HIN>: the Winograd weight gradient of one 32->32 layer"""
    d = _D()
    blocks = cus
    steps = _ww_steps(nb, hin)
    if d("ww.blocks*4>steps", blocks * 4 > steps):
        blocks = (steps + 3) // 4
    blocks = max(blocks, 1)
    d("ww.xcd_remap", blocks & 7 == 0)
    return Launch("conv3x3_wgrad_wino_kernel", blocks, [blocks], dict(d))


def wgrad_partial_wino3(nb, cus=CUS):
    """drq_conv3x3_wgrad_partial_wino3: conv2..4 in one launch, the grid shared out in proportion to the layers' steps.
    kernel == EARG: the entry refuses and step.hip launches the layers one by one (launch_ww)."""
    d = _D()
    steps = [_ww_steps(nb, h) for h in ENC_H[1:4]]
    tot = sum(steps)
    if d("ww3.fallback", cus < 3 or tot < 3 * 4):
        return Launch(EARG, 0, None, dict(d))
    share, under, cap = [], False, False
    for s in steps:
        n = (s * cus + tot // 2) // tot
        if n < 1:
            n, under = 1, True
        if n * 4 > s:
            n, cap = (s + 3) // 4, True
        share.append(n)
    d("ww3.share<1", under)
    d("ww3.cap", cap)
    used = sum(share)
    d("ww3.overshoot", used > cus)
    while used > cus:
        m = 0
        for l in (1, 2):
            if share[l] > share[m]:
                m = l
        share[m] -= 1
        used -= 1
    d("ww3.xcd_remap", used & 7 == 0)
    return Launch("conv3x3_wgrad_wino3_kernel", used, share, dict(d))


# -------------------------------------------------------------------------------------------- csrc/conv_bf16.hip
def launch_wgrad_bf16(nb, hin, cus=CUS):
    """launch_wgrad_bf16<HIN>: the record count it hands to the reduce"""
    d = _D()
    units = nb * (hin - 2)
    blocks = cus
    if d("wgrad_bf16.blocks*4>units", blocks * 4 > units):
        blocks = (units + 3) // 4
    blocks = max(blocks, 1)
    return Launch("conv3x3_wgrad_bf16_kernel", blocks, [blocks], dict(d))


def launch_conv_bf16(nb, hin, lay=0, cus=CUS):
    """launch_conv_bf16<HIN, MASK, LAY>: (sample, part of the output rows) units, three workgroups per CU with bf16
    input (lay & 1), else two; hin is the kernel's input side as for launch_wino"""
    d = _D()
    wgs = 3 if lay & 1 else 2
    blocks = nb * (4 if wgs == 3 and hin >= 43 else 3)
    if d("conv_bf16.blocks>cap", blocks > wgs * cus):
        blocks = wgs * cus
    return Launch("conv3x3_bf16_kernel", max(blocks, 1), None, dict(d))


# --------------------------------------------------------------------------------------------- csrc/conv1aug.hip
def launch_conv1_aug(n, riders=0, cus=CUS):
    """drq_conv1_aug_fwd_any: both views' (frame, band of output rows) units over two workgroups per CU; a workgroup's
    shift table holds 64 units, so the grid grows beyond the cap instead; `riders` workgroups lead the grid"""
    d = _D()
    units = 2 * n * 5
    blocks = units
    if d("conv1_aug.blocks>cap", blocks > 2 * cus):
        blocks = 2 * cus
    if d("conv1_aug.table_full", blocks * 64 < units):
        blocks = _cdiv(units, 64)
    return Launch("conv1_aug_kernel", blocks + riders, None, dict(d))


# ------------------------------------------------------------------------------------------------ csrc/step.hip
def update_launches(B, dtype="fp32", cus=CUS):
    """The convolution launches of one update() at batch B that this module restates, as (stage, Launch) in issue order.
    fp32: the Winograd forward of conv2..4 on both views (2B frames), the Winograd input gradients of conv4..2 (B
    frames), the three-layer Winograd weight gradient (or its per-layer fallback), conv1's deferred direct weight
    gradient, one reduce.  bf16: the forward and input-gradient kernels of conv_bf16.hip are not restated; the weight
    gradients are, for the records they hand to the reduce."""
    out = []
    if dtype == "fp32":
        for l in (1, 2, 3):
            out.append(("ACT%d" % (l + 1) if l < 3 else "FEAT", launch_wino(2 * B, ENC_H[l], cus)))
        for l in (3, 2, 1):
            out.append(("DY%d" % l, launch_wino(B, ENC_H[l + 1] + 4, cus)))
        w3 = wgrad_partial_wino3(B, cus)
        out.append(("dW2-4", w3))
        if w3.kernel == EARG:
            per_layer = [launch_ww(B, ENC_H[l], cus) for l in (1, 2, 3)]
            out.extend(("dW%d" % (l + 1), la) for l, la in zip((1, 2, 3), per_layer))
            rec234 = [la.records[0] for la in per_layer]
        else:
            rec234 = list(w3.records)
    else:
        per_layer = [launch_wgrad_bf16(B, ENC_H[l], cus) for l in (1, 2, 3)]
        out.extend(("dW%d" % (l + 1), la) for l, la in zip((1, 2, 3), per_layer))
        rec234 = [la.records[0] for la in per_layer]
    w1 = launch_wgrad(B, 9, 84, 2, cus)
    out.append(("dW1", w1))
    out.append(("reduce", reduce_multi(w1.records + rec234, [9, 32, 32, 32])))
    return out


def decisions_of(launches):
    """name -> set of the sides taken, over a list of (stage, Launch)"""
    seen = {}
    for _, la in launches:
        for dd in (la.decisions if isinstance(la.decisions, list) else [la.decisions]):
            for k, v in dd.items():
                seen.setdefault(k, set()).add(v)
    return seen


# the rows of tests/test_hip_encoder_audit.py: (B, compute dtype, updates audited) and why the row is there
Row = namedtuple("Row", "B dtype updates edge")
AUDIT_ROWS = [
    Row(1, "fp32", 1, "capped wino3 shares [25, 23, 21]; 11 conv1 records (< 16) in the reduce; grids of 7..50 workgroups"),
    Row(2, "fp32", 2, "capped shares; a second update on rebuilt U images"),
    Row(3, "fp32", 1, "the last batch on the capped side of n*4 > steps"),
    Row(5, "fp32", 1, "the first odd batch on the uncapped split [94, 85, 76]"),
    Row(32, "fp32", 2, "328 conv1 records: the reduce takes a second pass; a second update"),
    Row(96, "fp32", 1, "every Winograd forward / input-gradient grid capped at 2 per CU (full rounds and left-over "
                       "halves), conv1's weight gradient at its full 512 workgroups"),
    Row(2, "bf16", 1, "bf16 update, fp32 storage (step_flags 12): 21 conv1 records"),
    Row(32, "bf16", 1, "bf16 update, fp32 storage: full 256-record jobs next to conv1's 328"),
]
AUDIT_BATCHES = {"fp32": [r.B for r in AUDIT_ROWS if r.dtype == "fp32"], "bf16": [r.B for r in AUDIT_ROWS if r.dtype == "bf16"]}

# every decision of the launches one fp32 update issues (and of the reduce, which the bf16 update shares)
DECISIONS = (
    "wino.blocks>cap", "wino.xcd_remap", "wino.full_rounds", "wino.left_over", "wino.left_over_whole",
    "wino.left_over_halves", "wino.ragged_last_unit",
    "ww3.fallback", "ww3.share<1", "ww3.cap", "ww3.overshoot", "ww3.xcd_remap",
    "wgrad.blocks>units", "wgrad.units_ragged", "wgrad_bf16.blocks*4>units",
    "reduce.records<16", "reduce.records<256", "reduce.second_pass", "reduce.clamped_loads")

# decision -> the side no batch 1..4096 takes on a 256-CU device.  The branches stay in the code: other CU counts (a
# partitioned device) take the overshoot loop (32 CUs) and the remap (8, 16, 64, 128 CUs); the other two guard the
# arithmetic (fewer than 3 CUs; a share that rounds to zero).  tests/test_cpu_conv_variants.py asserts that each entry is still true, and that
# nothing else is one-sided over the audit rows.  The far sides run on the device all the same: tests/cu_rows.py lists the
# rows tests/test_hip_cu_counts.py runs under an override of the CU count (32 CUs: overshoot and remap; 8, 64, 128: the
# remap; 2: the fallback), and which far side no count reaches (STILL_UNREACHABLE: ww3.share<1).
UNREACHABLE_AT_256 = {
    "ww3.fallback": True,       # tot = 273 steps at B = 1 already
    "ww3.share<1": True,        # the three layers' steps are within 25 % of each other: every share is about cus / 3
    "ww3.overshoot": True,      # the three rounded shares sum to 255 for every B >= 4, the capped ones to less
    "ww3.xcd_remap": True,      # grids of 69, 137, 204 (B = 1, 2, 3) and 255 (B >= 4): none a multiple of 8
}

# The launchers the update does not reach (the direct forward / input gradient, the single-layer Winograd weight
# gradient, the 32->32 direct weight gradient) are public ops; their decisions are taken on both sides by these rows of
# tests/test_hip_ops.py: (test, parametrize line) and the launches each row makes.
OP_TEST_ROWS = {
    "conv_v": ("test_conv_fwd", '[(9, 84, 2, 5), (32, 41, 1, 3), (32, 39, 1, 4), (32, 37, 1, 2)]',
               "test_conv_kernels_at_training_batch_sizes",
               '[(9, 84, 2, 256), (32, 41, 1, 512), (32, 39, 1, 256), (32, 37, 1, 96)]'),
    "ww": ("test_conv_wgrad_winograd", '[(41, 5), (39, 2), (37, 7), (41, 1), (37, 64), (39, 256)]'),
    # the public direct weight gradient ends in the multi-job reduce: conv1 at 11, 31, 52 and 328 records
    "wgrad": ("test_conv_wgrad", '[(9, 84, 2, 3), (32, 41, 1, 5), (32, 39, 1, 2), (32, 37, 1, 7), (9, 84, 2, 1), '
                                 '(9, 84, 2, 5), (9, 84, 2, 32)]'),
}
OP_DECISIONS = ("conv_v.blocks>cap", "conv_v.rounds>1", "conv_v.ragged_last_tile", "ww.blocks*4>steps", "ww.xcd_remap")


def op_test_launches(cus=CUS):
    out = []
    for spec in (OP_TEST_ROWS["conv_v"][1], OP_TEST_ROWS["conv_v"][3]):
        for cin, hin, stride, nb in eval(spec):
            out.append(("fwd", launch_conv_v(nb, hin, stride, cus=cus)))
    for hin, nb in eval(OP_TEST_ROWS["ww"][1]):
        out.append(("dW", launch_ww(nb, hin, cus)))
    return out
