"""The GEMM op-test table (tests/gemm_variants.py) covers the dispatch it restates, and the bound the GPU rows are held
to is both tight enough to see a subtly wrong kernel and valid for a correct fp32 one.  No GPU needed."""
import pytest
import torch

from tests import gemm_variants as gv


def test_every_row_reaches_the_variant_it_is_meant_for():
    wrong = [(gv.row_id(r), r.expect, gv.label(gv.select(r))) for r in gv.TABLE if gv.label(gv.select(r)) != r.expect]
    assert not wrong, wrong
    ids = [gv.row_id(r) for r in gv.TABLE]
    assert len(set(ids)) == len(ids)


def test_every_variant_has_a_row():
    reached = {gv.base(r.expect) for r in gv.TABLE}
    assert set(gv.VARIANTS) - reached == set(), "variants without a table row"
    assert reached - set(gv.VARIANTS) == set(), "table rows with a name the list does not know"


def test_every_threshold_has_a_row_on_each_side():
    seen = {}
    for r in gv.TABLE:
        for k, v in gv.select(r).decisions.items():
            seen.setdefault(k, set()).add(v)
    assert set(seen) - set(gv.THRESHOLDS) == set(), "decisions the threshold list does not name"
    one_sided = {k: sorted(seen.get(k, ())) for k in gv.THRESHOLDS if seen.get(k) != {True, False}}
    assert not one_sided, one_sided


def test_the_coverage_check_notices_a_moved_threshold():
    """with another CU count the same table no longer sits on both sides of the ring kernel's tile threshold"""
    seen = set()
    for r in gv.TABLE:
        if r.entry == "mlp_fwd":
            seen.add(gv.select(r, cus=304).decisions.get("g3_fwd.t64>=cus"))
    assert seen == {False}


def test_refusals_are_predicted():
    for entry, n, M, N, K, opts, why in gv.REFUSALS:
        row = gv.Row(entry, None, n, M, N, K, opts, gv.EARG, why)
        assert gv.select(row).name == gv.EARG, why


# ---------------------------------------------------------------------------------------- the comparison function
M_, N_, K_ = 64, 64, 96          # the table row mlp_fwd / mlp_dgrad n=1 64x64x96 (3 k-tiles), with bias and mask at once


@pytest.fixture(scope="module")
def case():
    assert any(r.M == M_ and r.N == N_ and r.K == K_ for r in gv.TABLE)
    x = gv.make_act(M_, K_, seed=(1,))
    w = gv.make_weight(N_, K_, K_, seed=(2,))
    b = gv.randn(N_, seed=(3,))
    mask = gv.make_mask(M_, N_, seed=(4,))
    ref, mag = gv.reference(x.double(), w.double().t(), b.double(), relu=False, mask=mask)
    return x, w, b, mask, ref, mag


def epi64(acc, b, mask, ge=False):
    keep = (mask >= 0) if ge else (mask > 0)
    return (acc + b.double()) * keep.double()


def test_compare_accepts_an_fp32_matmul(case):
    x, w, b, mask, ref, mag = case
    got = (torch.matmul(x, w.t()) + b) * (mask > 0).float()
    ok, nerr, ratio = gv.compare(got, ref, mag, K_)
    assert ok and ratio < 1.0, (nerr, ratio)
    # and the reference itself, rounded once
    assert gv.compare(ref.float(), ref, mag, K_)[0]


def test_compare_rejects_a_dropped_k_term(case):
    x, w, b, mask, ref, mag = case
    keep = torch.nonzero(mask > 0)                           # an element the mask lets through
    i, j = (int(v) for v in keep[len(keep) // 2])
    terms = x[i].double() * w[j].double()
    k = int(terms.abs().argmax())
    bad = ref.clone()
    bad[i, j] -= terms[k]
    ok, nerr, ratio = gv.compare(bad.float(), ref, mag, K_)
    assert not ok and ratio > 1.0, (nerr, ratio)


def test_compare_rejects_one_tile_with_bf16_operands(case):
    x, w, b, mask, ref, mag = case
    acc = x.double() @ w.double().t()
    xb, wb = x[32:64].bfloat16().double(), w[0:32].bfloat16().double()
    acc[32:64, 0:32] = xb @ wb.t()
    ok, nerr, ratio = gv.compare(epi64(acc, b, mask).float(), ref, mag, K_)
    assert not ok and ratio > 1.0, (nerr, ratio)


def test_compare_rejects_a_mask_tested_with_greater_or_equal(case):
    x, w, b, mask, ref, mag = case
    acc = x.double() @ w.double().t()
    ok, nerr, ratio = gv.compare(epi64(acc, b, mask, ge=True).float(), ref, mag, K_)
    assert not ok and ratio == float("inf"), (nerr, ratio)
    # the sign-bit test (mask is not negative) fails the same way: it lets +0.0 and NaN through
    sign = (~torch.signbit(mask)).double()
    assert not gv.compare(((acc + b.double()) * sign).float(), ref, mag, K_)[0]


def test_compare_rejects_a_bias_moved_by_one(case):
    x, w, b, mask, ref, mag = case
    acc = x.double() @ w.double().t()
    ok, nerr, ratio = gv.compare(epi64(acc, torch.roll(b, 1), mask).float(), ref, mag, K_)
    assert not ok and ratio > 1.0, (nerr, ratio)


def test_masks_hold_the_planted_values_in_every_tile():
    m = gv.make_mask(128, 192, seed=(9,))
    bits = m.view(torch.int32)
    for r0 in range(0, 128, 32):
        for c0 in range(0, 192, 32):
            t, tb = m[r0:r0 + 32, c0:c0 + 32], bits[r0:r0 + 32, c0:c0 + 32]
            assert torch.isnan(t[0, 0]) and torch.isnan(t[31, 31]) and torch.isnan(t[13, 17])
            assert int(tb[0, 31]) == -2 ** 31 and int(tb[31, 0]) == 0 and int(tb[5, 0]) == -2 ** 31 and int(tb[0, 5]) == 0
    frac = float((m > 0).float().mean())
    assert 0.3 < frac < 0.6
