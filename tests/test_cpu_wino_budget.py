"""The Winograd input gradients on a budget of workgroup slots (plan_wino's budget, the overlapped update's launches):
a host walk of the decode the kernel itself uses (wino_deal of csrc/conv_plan.h, through tests/wino_budget_walk.cpp).
Whatever the grid, every unit of 16 tiles and every half-unit must have exactly one owner -- that, and the fact that a
unit's arithmetic does not depend on its owner, is why a budgeted launch writes the same bits.  No GPU needed."""
import os
import subprocess

import pytest

HINS = (39, 41, 43)                       # kernel inputs of the three input gradients: dY4, dY3, dY2 zero-padded by 2
SWEEP = (512, 480, 448, 416, 384, 320, 256, 224, 192)   # the budgets of profiles/overlap_budget_sweep.txt (512 = the whole chip)
SMALL = (16, 32, 48, 128, 256)            # budgets that bind at small batches too
BATCHES = (1, 2, 3, 256)
CUS = 256


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    from drqv2_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path_factory.mktemp("wino_budget") / "wino_budget_walk")
    subprocess.check_call([build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(here, "wino_budget_walk.cpp"), "-o", exe])

    def run(rows):
        text = "".join("%d %d %d %d\n" % r for r in rows)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
        assert len(got) == len(rows)
        return got
    return run


def units(nb, hin):
    th = (hin - 1) // 2
    return (nb * th * th + 15) // 16


def grid_of(cus, nb, hin, budget):
    """the planner's rule, restated: a budget counts in sixteens, is at least 16 and never enlarges a grid"""
    cap = 2 * cus
    if 0 < budget < cap:
        cap = max(16, budget // 16 * 16)
    return max(1, min((units(nb, hin) + 3) // 4, cap))


def test_every_unit_and_half_unit_has_one_owner_on_every_budget(walk):
    rows = [(CUS, nb, hin, b) for hin in HINS for nb in BATCHES for b in SWEEP + SMALL + (0,)]
    for row, (grid, grid0, nunit, once, other, stray, most, least) in zip(rows, walk(rows)):
        cus, nb, hin, budget = row
        assert nunit == units(nb, hin), row
        assert grid == grid_of(cus, nb, hin, budget), row
        assert grid0 == grid_of(cus, nb, hin, 0), row
        assert (once, other, stray) == (2 * nunit, 0, 0), row
        # the deal is level: in half-units, the busiest wave carries the mean rounded up and the idlest the mean rounded
        # down (left-over units go out as halves wherever that keeps the busiest wave one half-unit lower)
        assert most == -(-2 * nunit // (4 * grid)) and least == 2 * nunit // (4 * grid), row


def test_the_budget_binds_at_the_headline_batch_and_nowhere_else_changes_a_plan(walk):
    rows = [(CUS, 256, hin, b) for hin in HINS for b in SWEEP]
    for (cus, nb, hin, budget), got in zip(rows, walk(rows)):
        assert got[0] == budget and got[1] == 512
    # no budget, a budget of the whole chip or more, and a batch too small to fill the budget: today's grid
    rows = [(cus, nb, hin, b) for cus in (256, 304, 64) for nb in (1, 3, 32, 256) for hin in HINS + (37,)
            for b in (0, 2 * cus, 2 * cus + 16, 4096)]
    for row, got in zip(rows, walk(rows)):
        assert got[0] == got[1], row
    rows = [(CUS, 3, hin, b) for hin in HINS for b in (512, 384)]
    for row, got in zip(rows, walk(rows)):
        assert got[0] == got[1] == (units(3, row[2]) + 3) // 4, row


def test_budgets_are_taken_in_sixteens(walk):
    rows = [(CUS, 256, 41, b) for b in (1, 15, 16, 17, 31, 383, 385, 400, 511)]
    want = [16, 16, 16, 16, 16, 368, 384, 400, 496]
    assert [g[0] for g in walk(rows)] == want
    for (grid, _, nunit, once, other, stray, _, _) in walk(rows):
        assert grid % 16 == 0 and (once, other, stray) == (2 * nunit, 0, 0)


def test_the_overlapped_updates_default_is_one_of_the_swept_budgets():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "drqv2_amd", "csrc", "conv_plan.h")) as f:
        text = f.read()
    import re
    m = re.search(r"constexpr int kWinoOverlapBudget512 = (\d+);", text)
    assert m and int(m.group(1)) in SWEEP
