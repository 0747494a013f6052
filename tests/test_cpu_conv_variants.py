"""The batch sizes of the per-launch encoder audit (tests/test_hip_encoder_audit.py) take every decision of the
convolution launch arithmetic restated in tests/conv_variants.py on both sides, except the sides no batch can reach on a
256-CU device, which are listed and checked as such.  No GPU needed."""
import os

from tests import conv_variants as cv

ISSUE_BATCHES = {"fp32": [1, 2, 3, 5, 32], "bf16": [2, 32]}      # the audit may add rows, never lose one of these
SECOND_UPDATE = [2, 32]


def audit_launches(cus=cv.CUS):
    out = []
    for r in cv.AUDIT_ROWS:
        out += cv.update_launches(r.B, r.dtype, cus)
    return out


def test_the_audit_keeps_its_batch_sizes():
    for dt, want in ISSUE_BATCHES.items():
        assert set(want) <= set(cv.AUDIT_BATCHES[dt]), (dt, cv.AUDIT_BATCHES[dt])
    assert [r.B for r in cv.AUDIT_ROWS if r.dtype == "fp32" and r.updates == 2] == SECOND_UPDATE
    assert len({(r.B, r.dtype) for r in cv.AUDIT_ROWS}) == len(cv.AUDIT_ROWS)


def test_every_decision_is_taken_on_both_sides_by_an_audit_row():
    seen = cv.decisions_of(audit_launches())
    assert set(seen) - set(cv.DECISIONS) == set(), "decisions the list does not name"
    assert set(cv.UNREACHABLE_AT_256) <= set(cv.DECISIONS)
    one_sided = {}
    for k in cv.DECISIONS:
        missing = {True, False} - seen.get(k, set())
        if k in cv.UNREACHABLE_AT_256:
            missing -= {cv.UNREACHABLE_AT_256[k]}
        if missing:
            one_sided[k] = sorted(missing)
    assert not one_sided, "sides no audit row takes: %r" % one_sided


def test_the_unreachable_table_is_accurate():
    """no batch 1..4096 takes the listed side at 256 CUs, in either compute dtype, and every other decision is
    reachable on both sides in that range (so nothing hides behind the table)"""
    seen = {}
    for B in range(1, 4097):
        for dt in ("fp32", "bf16"):
            for k, v in cv.decisions_of(cv.update_launches(B, dt)).items():
                seen.setdefault(k, set()).update(v)
    for k, side in cv.UNREACHABLE_AT_256.items():
        assert side not in seen[k], "%s is %s for some batch: it needs an audit row, not a table entry" % (k, side)
    for k in cv.DECISIONS:
        if k not in cv.UNREACHABLE_AT_256:
            assert seen[k] == {True, False}, (k, seen[k])


def test_the_dead_branches_are_live_at_other_cu_counts():
    """why they stay in the code: a device (or partition) of 32 CUs runs the overshoot loop, one of 64 the remap"""
    assert cv.wgrad_partial_wino3(8, cus=32).decisions["ww3.overshoot"]
    w = cv.wgrad_partial_wino3(8, cus=64)
    assert w.decisions["ww3.xcd_remap"] and w.grid == 64 and sum(w.records) == 64
    assert cv.wgrad_partial_wino3(8, cus=2).kernel == cv.EARG


def test_the_split_is_the_one_the_kernel_comments_describe():
    """figures read off the mirror at 256 CUs: one split for every B >= 4, capped shares below, conv1's records"""
    assert {tuple(cv.wgrad_partial_wino3(B).records) for B in range(4, 600)} == {(94, 85, 76)}
    assert cv.wgrad_partial_wino3(1).records == [25, 23, 21]
    assert [cv.wgrad_partial_wino3(B).grid for B in (1, 2, 3, 4)] == [69, 137, 204, 255]
    assert [cv.launch_wgrad(B, 9, 84, 2).records[0] for B in (1, 2, 3, 5, 32, 96)] == [11, 21, 31, 52, 328, 512]
    for B in range(1, 4097):
        w = cv.wgrad_partial_wino3(B)
        assert all(n >= 1 for n in w.records) and sum(w.records) == w.grid <= cv.CUS
        steps = [cv._ww_steps(B, h) for h in cv.ENC_H[1:4]]
        assert all(4 * n <= s + 3 for n, s in zip(w.records, steps))       # no workgroup without a step


def test_the_grids_of_the_audit_rows_and_the_first_batch_past_each_threshold():
    """pinned figures: a threshold changed in the mirror (or in the code it restates, once repeated here) moves one"""
    Bs = [1, 2, 3, 5, 32, 96]
    assert [cv.launch_wino(2 * B, 41).grid for B in Bs] == [13, 25, 38, 63, 400, 512]        # conv2 forward, 2B frames
    assert [cv.launch_wino(B, 43).grid for B in Bs] == [7, 14, 21, 35, 221, 512]             # conv2 input gradient
    first = lambda f: next(n for n in range(1, 4097) if f(n))
    assert first(lambda n: cv.launch_wino(n, 41).decisions["wino.blocks>cap"]) == 82
    assert first(lambda n: cv.launch_wino(n, 39).decisions["wino.blocks>cap"]) == 91
    assert first(lambda n: not cv.launch_wgrad(n, 9, 84, 2).decisions["wgrad.blocks>units"]) == 50
    assert first(lambda n: not cv.wgrad_partial_wino3(n).decisions["ww3.cap"]) == 4
    assert first(lambda n: not cv.launch_ww(n, 41).decisions["ww.blocks*4>steps"]) == 11
    assert first(lambda n: cv.launch_conv_v(n, 84, 2).decisions["conv_v.blocks>cap"]) == 78
    assert first(lambda n: not cv.launch_wgrad_bf16(n, 41).decisions["wgrad_bf16.blocks*4>units"]) == 27
    assert [k for k, v in cv.reduce_records(16).items() if v] == ["reduce.records<256", "reduce.clamped_loads"]
    assert [k for k, v in cv.reduce_records(256).items() if v] == []
    assert [k for k, v in cv.reduce_records(257).items() if v] == ["reduce.second_pass", "reduce.clamped_loads"]


def test_a_moved_threshold_is_noticed():
    """the same rows on a device with another CU count no longer sit on both sides of the Winograd grid cap, and the
    reduce no longer sees a second pass for conv1: the coverage check is sensitive to the thresholds it restates"""
    seen = cv.decisions_of(audit_launches(cus=1024))
    assert seen["wino.blocks>cap"] == {False}
    seen = cv.decisions_of(audit_launches(cus=128))
    assert seen["reduce.second_pass"] == {False}


def test_the_other_launchers_are_covered_by_the_op_tests():
    """launch_conv_v and launch_ww are not reached from the update; the rows of tests/test_hip_ops.py named in
    OP_TEST_ROWS take their decisions on both sides, and those rows are still there"""
    with open(os.path.join(os.path.dirname(__file__), "test_hip_ops.py")) as f:
        src = f.read()
    for spec in cv.OP_TEST_ROWS.values():
        for test, params in zip(spec[0::2], spec[1::2]):
            at = src.index("def %s(" % test)
            assert params in src[src.rindex("@pytest.mark.parametrize", 0, at):at], test
    seen = cv.decisions_of(cv.op_test_launches())
    assert set(seen) == set(cv.OP_DECISIONS)
    assert all(v == {True, False} for v in seen.values()), seen
