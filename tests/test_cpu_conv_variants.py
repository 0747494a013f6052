"""The batch sizes of the per-launch encoder audit (tests/test_hip_encoder_audit.py) take every decision of the
convolution launch arithmetic restated in tests/conv_variants.py on both sides, except the sides no batch can reach on a
256-CU device, which are listed and checked as such; and that restatement agrees with the planner the library launches
from (csrc/conv_plan.h, through tests/conv_plan_dump.cpp).  No GPU needed."""
import os
import subprocess

import pytest

from tests import conv_variants as cv
from tests import cu_rows

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


# ------------------------------------------------------------------------- the mirror against csrc/conv_plan.h
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """tests/conv_plan_dump.cpp compiled for the host: lines of launches in; rc, grid, grid_y, three record counts, the
    merged flag and the workspace bytes out"""
    from drqv2_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_dump")
    subprocess.check_call([build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(here, "conv_plan_dump.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True).stdout
        return [[int(v) for v in ln.split()] for ln in out.splitlines()]
    return run


def _line(kind, cus, nb, hin=0, stride=1, cin=32, lay=0, ws=-1):
    return "%s %d %d %d %d %d %d %d\n" % (kind, cus, nb, hin, stride, cin, lay, ws)


SWEEP_CUS = (2, 3, 8, 32, 64, 128, 256, 304)
DIRECT_GEOMS = [(9, 84, 2), (32, 41, 1), (32, 39, 1), (32, 37, 1)]   # (cin, hin, stride) of the direct kernels
PART = {9: (3 * 1024 + 64) * 4, 32: (9 * 1024 + 64) * 4}             # bytes of a partial record by cin


def sweep_cases(cus, batches):
    """(input line, the mirror's Launch) for every host-side function of the mirror at every geometry its launcher is
    instantiated for.  hin 43 is the padded gradient of conv2's input gradient."""
    for nb in batches:
        for cin, hin, stride in DIRECT_GEOMS + [(32, 43, 1)]:
            yield _line("conv_v", cus, nb, hin, stride, cin), cv.launch_conv_v(nb, hin, stride, cus=cus)
        for cin, hin, stride in DIRECT_GEOMS:
            yield _line("wgrad", cus, nb, hin, stride, cin), cv.launch_wgrad(nb, cin, hin, stride, cus)
        for hin in (41, 39, 37, 43):
            yield _line("wino", cus, nb, hin), cv.launch_wino(nb, hin, cus)
            for lay in (0, 1):
                yield _line("conv_bf16", cus, nb, hin, lay=lay), cv.launch_conv_bf16(nb, hin, lay, cus)
        for hin in (41, 39, 37):
            yield _line("ww", cus, nb, hin), cv.launch_ww(nb, hin, cus)
            yield _line("wgrad_bf16", cus, nb, hin), cv.launch_wgrad_bf16(nb, hin, cus)
        yield _line("ww3", cus, nb), cv.wgrad_partial_wino3(nb, cus)
        for riders in (0, 6):
            yield _line("conv1_aug", cus, nb, lay=riders), cv.launch_conv1_aug(nb, riders, cus)
    for cins in ([9], [32], [9, 32], [32, 32, 32], [9, 32, 32, 32]):
        yield (_line("reduce", cus, len(cins), cin=cins[0]), cv.reduce_multi([1] * len(cins), cins))


def test_the_mirror_agrees_with_the_planner(plan_dump):
    """per launch: the grid, the records left per layer and the merged-or-fallback choice, for batches 1..4096 at eight
    CU counts (2: the three-layer launch never merges; 32: its overshoot loop; 8..128: its remap).  The C++ is the
    behaviour: a disagreement is a bug of the mirror."""
    cases = [c for cus in SWEEP_CUS for c in sweep_cases(cus, range(1, 4097))]
    got = plan_dump([c[0] for c in cases])
    assert len(got) == len(cases) > 900000
    wrong = []
    for (line, la), (rc, grid, grid_y, r0, r1, r2, merged, _) in zip(cases, got):
        if la.kernel == cv.EARG:
            ok = rc == -1 and not merged
        else:
            want_grid = la.grid if isinstance(la.grid, tuple) else (la.grid, 1)
            ok = rc == 0 and merged and (grid, grid_y) == want_grid and [r0, r1, r2] == (list(la.records or []) + [0] * 3)[:3]
        if not ok:
            wrong.append((line.strip(), la.kernel, la.grid, la.records, (rc, grid, grid_y, r0, r1, r2, merged)))
    assert not wrong, (len(wrong), wrong[:10])


def test_the_planner_sizes_and_refuses_workspaces(plan_dump):
    """the mirror has no workspace, so these are direct: a weight gradient needs one record per workgroup and layer, the
    single-layer Winograd one a record per CU whatever its grid (and a padded dy); one byte less is DRQ_EWS (-2); a
    geometry without a kernel is DRQ_EARG (-1) before the workspace is looked at"""
    rc = lambda lines: [(g[0], g[-1]) for g in plan_dump(lines)]
    assert rc([_line("wgrad", 256, 5, 84, 2, 9, ws=52 * PART[9]), _line("wgrad", 256, 5, 84, 2, 9, ws=52 * PART[9] - 1),
               _line("wgrad", 256, 5, 41, 1, 32, ws=49 * PART[32] - 1), _line("wgrad", 256, 5, 43, 1, 32, ws=0),
               _line("wgrad", 256, 5, 84, 1, 9, ws=0)]) == [(0, 52 * PART[9]), (-2, 52 * PART[9]), (-2, 49 * PART[32]),
                                                          (-1, 0), (-1, 0)]
    assert cv.launch_ww(1, 41).grid == 25
    assert rc([_line("ww", 256, 1, 41, ws=256 * PART[32]), _line("ww", 256, 1, 41, ws=256 * PART[32] - 1),
               _line("ww_flat", 256, 1, 41)]) == [(0, 256 * PART[32]), (-2, 256 * PART[32]), (-1, 0)]
    assert rc([_line("ww3", 256, 8, ws=94 * PART[32]), _line("ww3", 256, 8, ws=94 * PART[32] - 1),
               _line("ww3", 2, 8, ws=0)]) == [(0, 94 * PART[32]), (-2, 94 * PART[32]), (-1, 0)]
    assert rc([_line("wgrad_bf16", 256, 2, 41, ws=20 * PART[32]), _line("wgrad_bf16", 256, 2, 41, ws=20 * PART[32] - 1),
               _line("wgrad_bf16", 256, 2, 43, ws=0)]) == [(0, 20 * PART[32]), (-2, 20 * PART[32]), (-1, 0)]


# ------------------------------------------------------- the rows run under an override of the CU count (tests/cu_rows.py)
def test_the_override_rows_hold_the_rows_asked_for():
    rows = {(r.cus, r.B, r.dtype) for r in cu_rows.CU_ROWS}
    assert {(32, 1, "fp32"), (32, 2, "fp32"), (32, 8, "fp32"), (8, 2, "fp32"), (8, 3, "fp32"), (64, 2, "fp32"),
            (128, 2, "fp32"), (2, 1, "fp32"), (3, 1, "fp32"), (32, 2, "bf16")} <= rows
    assert len(rows) == len(cu_rows.CU_ROWS) and all(1 <= r.cus <= cv.CUS for r in cu_rows.CU_ROWS + cu_rows.OP_ROWS)
    at = lambda cus, B: dict(cu_rows.row_launches(cu_rows.CuRow(cus, B, "fp32", 1)))
    for B in (1, 2, 8):                             # 32 CUs: the overshoot and the remap, a grid of exactly 32
        w = at(32, B)["dW2-4"]
        assert w.decisions["ww3.overshoot"] and w.decisions["ww3.xcd_remap"] and w.grid == 32 == sum(w.records)
    f = at(32, 8)["ACT2"]
    assert f.grid == 64 and f.decisions["wino.blocks>cap"] and f.decisions["wino.xcd_remap"]
    for B in (2, 3):                                # 8 CUs: forward grids of 16 (remap on), a weight-gradient grid of 8
        la = at(8, B)
        assert [la[s].grid for s in ("ACT2", "ACT3", "FEAT")] == [16] * 3 and la["ACT2"].decisions["wino.xcd_remap"]
        assert la["dW2-4"].grid == 8 and la["dW2-4"].decisions["ww3.xcd_remap"]
    assert at(8, 3)["ACT2"].decisions["wino.full_rounds"] and [at(8, 3)[s].grid for s in ("DY3", "DY2", "DY1")] == [16] * 3
    for cus in (64, 128):
        w = at(cus, 2)["dW2-4"]
        assert w.decisions["ww3.xcd_remap"] and w.grid == cus
    assert at(2, 1)["dW2-4"].kernel == cv.EARG and [at(2, 1)["dW%d" % l].grid for l in (2, 3, 4)] == [2, 2, 2]
    assert at(3, 1)["dW2-4"].records == [1, 1, 1]
    # the fused aug+conv1 rows at 8 CUs: the shift table is full at 103 and 110 frames (grid = ceil(10 n / 64)), not at 3
    aug = {r.args[0]: cu_rows.row_launches(r)[0][1] for r in cu_rows.OP_ROWS if r.fn == "launch_conv1_aug"}
    assert {n: (la.grid, la.decisions["conv1_aug.table_full"]) for n, la in aug.items()} == \
        {103: (17, True), 110: (18, True), 3: (16, False)}
    first = lambda f: next(n for n in range(1, 4097) if f(n))
    assert first(lambda n: cv.launch_conv1_aug(n, 0, 8).decisions["conv1_aug.table_full"]) == 103
    assert first(lambda n: cv.launch_conv1_aug(n, 0, 256).decisions["conv1_aug.table_full"]) == 3277
    assert all(cu_rows.describe(r) for r in cu_rows.CU_ROWS)


def test_every_far_side_of_the_unreachable_table_is_taken_under_an_override():
    """... by a row of cu_rows, unless no CU count of the sweep takes it at any batch 1..4096: those are listed in
    STILL_UNREACHABLE with the reason, and the list is held true"""
    seen = cv.decisions_of(cu_rows.override_launches())
    swept = {}
    for cus in SWEEP_CUS:
        if cus <= cv.CUS:
            for B in range(1, 4097):
                for k, v in cv.wgrad_partial_wino3(B, cus).decisions.items():
                    swept.setdefault(k, set()).add(v)
    assert set(cu_rows.STILL_UNREACHABLE) <= set(cv.UNREACHABLE_AT_256)
    for k, side in cv.UNREACHABLE_AT_256.items():
        if k in cu_rows.STILL_UNREACHABLE:
            assert side not in swept[k] and side not in seen[k], "%s is reachable: it needs a row" % k
        else:
            assert side in seen[k], "no override row takes %s = %s" % (k, side)


def test_what_is_one_sided_at_256_is_two_sided_with_the_override_rows():
    names = cv.DECISIONS + cv.OP_DECISIONS + cu_rows.AUG_DECISIONS + cu_rows.BF16_DECISIONS
    old = cv.decisions_of(cu_rows.launches_at_256())
    both = cv.decisions_of(cu_rows.launches_at_256() + cu_rows.override_launches())
    assert set(both) == set(names)
    one_sided = sorted(k for k in names if old.get(k, set()) != {True, False})
    assert one_sided == sorted(list(cv.UNREACHABLE_AT_256) + ["conv1_aug.table_full"])
    left = {k: sorted(both[k]) for k in one_sided if both[k] != {True, False}}
    assert set(left) == set(cu_rows.STILL_UNREACHABLE), left
    # every fp32 update row but the 3-CU one (the same sides at the smallest merged grid) adds a side of its own
    assert [r.cus for r in cu_rows.CU_ROWS if r.dtype == "fp32" and not cu_rows.new_sides(r, old)] == [3]


def test_the_planner_agrees_with_the_mirror_on_the_override_rows(plan_dump):
    """the sweep covers them; this guards the table: every launch of every row, through the library's own planner"""
    kinds = {"launch_conv_v": lambda nb, hin, s: _line("conv_v", 0, nb, hin, s, 9 if hin == 84 else 32),
             "launch_wino": lambda nb, hin: _line("wino", 0, nb, hin),
             "launch_ww": lambda nb, hin: _line("ww", 0, nb, hin),
             "launch_wgrad": lambda nb, cin, hin, s: _line("wgrad", 0, nb, hin, s, cin),
             "launch_conv_bf16": lambda nb, hin, lay: _line("conv_bf16", 0, nb, hin, lay=lay),
             "launch_wgrad_bf16": lambda nb, hin: _line("wgrad_bf16", 0, nb, hin),
             "launch_conv1_aug": lambda n, riders: _line("conv1_aug", 0, n, lay=riders)}
    cases = []
    for r in cu_rows.OP_ROWS:
        kind, rest = kinds[r.fn](*r.args).split(" ", 1)
        cases.append(("%s %d %s" % (kind, r.cus, rest.split(" ", 1)[1]), cu_rows.row_launches(r)[0][1]))
    for r in cu_rows.CU_ROWS:
        cases.append((_line("ww3", r.cus, r.B), cv.wgrad_partial_wino3(r.B, r.cus)))
        cases.append((_line("wgrad", r.cus, r.B, 84, 2, 9), cv.launch_wgrad(r.B, 9, 84, 2, r.cus)))
        for l in (1, 2, 3):
            cases.append((_line("wino", r.cus, 2 * r.B, cv.ENC_H[l]), cv.launch_wino(2 * r.B, cv.ENC_H[l], r.cus)))
            cases.append((_line("wino", r.cus, r.B, cv.ENC_H[l + 1] + 4), cv.launch_wino(r.B, cv.ENC_H[l + 1] + 4, r.cus)))
            cases.append((_line("ww", r.cus, r.B, cv.ENC_H[l]), cv.launch_ww(r.B, cv.ENC_H[l], r.cus)))
            cases.append((_line("wgrad_bf16", r.cus, r.B, cv.ENC_H[l]), cv.launch_wgrad_bf16(r.B, cv.ENC_H[l], r.cus)))
        for riders in (0, 6):
            cases.append((_line("conv1_aug", r.cus, r.B, lay=riders), cv.launch_conv1_aug(r.B, riders, r.cus)))
    got = plan_dump([c[0] for c in cases])
    assert len(got) == len(cases) > 200
    for (line, la), (rc, grid, grid_y, r0, r1, r2, merged, _) in zip(cases, got):
        if la.kernel == cv.EARG:
            assert rc == -1 and not merged, line
        else:
            assert rc == 0 and (grid, grid_y) == (la.grid, 1) and [r0, r1, r2] == (list(la.records or []) + [0] * 3)[:3], (line, la)


def test_the_baseline_at_256_is_the_shapes_the_guarded_tests_run():
    """cu_rows reads the 256-CU launches of the fused aug+conv1 and bf16 kernels off these lines of
    tests/test_hip_guarded.py: each still stands there, the parametrize lines right in front of their tests"""
    with open(os.path.join(os.path.dirname(__file__), "test_hip_guarded.py")) as f:
        src = f.read()
    for test, line in cu_rows.GUARDED_ROWS.values():
        at = src.index("def %s(" % test)
        if line.startswith("@"):
            assert line in src[src.rindex("\n\n", 0, at):at], test
        else:
            assert src.count(line) == 1 and line.split(" = ")[0] in src[src.rindex("\n\n", 0, at):at], test
    assert cu_rows.AUG_N_AT_256 == (3, 200, 7, 200) and len(cu_rows.BF16_AT_256) == 10
