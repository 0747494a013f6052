"""The GEMM op-test table (tests/gemm_variants.py) covers the dispatch it restates, and the bound the GPU rows are held
to is both tight enough to see a subtly wrong kernel and valid for a correct fp32 one.  No GPU needed."""
import itertools
import os
import subprocess

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


# ------------------------------------------------------------------------- the mirror against csrc/gemm_plan.h
@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """tests/gemm_plan_dump.cpp compiled for the host: lines of shapes in, the planner's variant names out"""
    from drqv2_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    subprocess.check_call([build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(here, "gemm_plan_dump.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


def _line(kind, cus, n, M, N, K, lda, ldb, ldc=None, a_al=True, b_al=True, tile=0, splitk=0, bias=False, relu=False,
          aux=False, rowsum=False, qw=False, qpart=False, ldx=0, scatter_hw=0, ws_bytes=1 << 40):
    f = (cus, n, M, N, K, lda, ldb, N if ldc is None else ldc, a_al, b_al, tile, splitk, bias, relu, aux, rowsum, qw,
         qpart, ldx, scatter_hw, ws_bytes)
    return kind + "".join(" %d" % int(v) for v in f) + "\n"


def _batched(layout, cus, n, M, N, K, a_al=True, b_al=True, tile=0, splitk=0, scatter_hw=0):
    """gv.select's conventions for a drq_gemm_batched_f32 row: (input line, the mirror's Sel)"""
    fl = dict(bias=layout == "fwd", relu=layout == "fwd", aux=layout == "dgrad", rowsum=layout == "wgrad",
              scatter_hw=scatter_hw)
    lda, ldb = (M if layout == "wgrad" else K), (K if layout == "fwd" else N)
    return (_line(layout, cus, n, M, N, K, lda, ldb, a_al=a_al, b_al=b_al, tile=tile, splitk=splitk, **fl),
            gv.batched(layout, n, M, N, K, a_al=a_al, b_al=b_al, tile=tile, splitk=splitk, cus=cus, **fl))


def _ring(entry, cus, n, M, N, K, lda=None, pad=0, aligned=True, qpart=True):
    """the three ring entries as gv.select calls them; the pair's (M, N, K) are (Brows, Kin, Nout)"""
    lda = K + pad if lda is None else lda
    if entry == "mlp_fwd":
        return (_line(entry, cus, n, M, N, K, lda, K + 2 * pad, a_al=aligned, qw=True, qpart=qpart),
                gv.ring_fwd(n, M, N, K, lda, K + 2 * pad, aligned, qw=True, qpart=qpart, cus=cus))
    if entry == "mlp_dgrad":
        return (_line(entry, cus, n, M, N, K, lda, N + 2 * pad, a_al=aligned, aux=True),
                gv.ring_dgrad(n, M, N, K, lda, N + 2 * pad, aligned, cus=cus))
    return (_line(entry, cus, n, M, N, K, lda, N + 2 * pad, a_al=aligned, aux=True, ldx=N + pad),
            gv.ring_pair(n, M, K, N, lda, N + pad, N + 2 * pad, aligned, cus=cus))


def _row_case(row, cus):
    o = row.opts
    if row.entry.startswith("mlp_"):
        return _ring(row.entry, cus, row.n, row.M, row.N, row.K, o.get("ldx"), 4 if o.get("ld") else 0,
                     not o.get("misalign"), not o.get("qw_only"))
    if row.entry == "partial":
        return _line("partial", cus, row.n, row.M, row.N, row.K, row.K, row.K), gv.partial(row.n, row.M, row.N, row.K, cus=cus)
    if row.entry == "gemm_f32":
        return _batched("fwd", cus, row.n, row.M, row.N, row.K, a_al=False, tile=o.get("tile", 0))
    return _batched(row.layout, cus, row.n, row.M, row.N, row.K, tile=o.get("tile", 0), splitk=o.get("splitk", 0))


def test_the_mirror_agrees_with_the_planner(plan_dump):
    """every table row, every refusal and a sweep across every threshold, at two CU counts: the planner the library
    launches from and the Python restatement the table is built on name the same variant, split count and nq"""
    cases = []                                                       # (input line, the mirror's Sel, a name)
    for cus in (256, 304):
        rows = gv.TABLE + [gv.Row(e, None, n, M, N, K, o, gv.EARG, why) for e, n, M, N, K, o, why in gv.REFUSALS]
        for row in rows:
            line, sel = _row_case(row, cus)
            assert sel == gv.select(row, cus), gv.row_id(row)          # _row_case follows gv.select
            cases.append((line, sel, "%s cus=%d" % (gv.row_id(row), cus)))
        Ms, Ns = (1, 32, 33, 64, 128, 160), (32, 50, 64, 100, 128, 4064, 4096)
        Ks = (32, 64, 128, 130, 256, 384, 512, 4064, 4096)
        for n, M, N, K, al in itertools.product((1, 2, 8, 9), Ms, Ns, Ks, (True, False)):
            sweep = [_batched(layout, cus, n, M, N, K, a_al=al, b_al=al, tile=tile, splitk=splitk)
                     for layout, tile, splitk in itertools.product(("fwd", "dgrad", "wgrad"), range(7), (0, 3))]
            sweep.extend(_batched(layout, cus, n, M, N, K, a_al=al, b_al=al, scatter_hw=35)
                         for layout in ("fwd", "dgrad", "wgrad"))      # the padded scatter keeps the generic kernels
            sweep.append((_line("partial", cus, n, M, N, K, K, K, a_al=al, b_al=al),
                          gv.partial(n, M, N, K, aligned=al, cus=cus)))
            sweep.extend(_ring(e, cus, n, M, N, K, aligned=al) for e in ("mlp_fwd", "mlp_dgrad", "mlp_pair"))
            cases.extend((line, sel, line.strip()) for line, sel in sweep)
    got = plan_dump([c[0] for c in cases])
    assert len(got) == len(cases) > 250000
    wrong = [(name, gv.label(sel), sel.nq, g) for (_, sel, name), g in zip(cases, got)
             if g[0] != gv.label(sel) or (sel.nq is not None and int(g[1]) != sel.nq)]
    assert not wrong, (len(wrong), wrong[:10])


def test_the_planner_refuses_a_workspace_that_is_too_small(plan_dump):
    """the mirror has no workspace, so these are direct: the split-K records of a call are nbatch * splitk * M * N floats
    (the split counts are those of the table rows with the same shapes); one byte less, or no workspace at all, is EWS"""
    trunk, lds = 4 * 16 * 256 * 50 * 4, 2 * 2 * 256 * 256 * 4
    got = plan_dump([_line("partial", 256, 4, 256, 50, 39200, 39200, 39200, ws_bytes=trunk),
                     _line("partial", 256, 4, 256, 50, 39200, 39200, 39200, ws_bytes=trunk - 1),
                     _line("partial", 256, 4, 256, 50, 39200, 39200, 39200, ws_bytes=0),
                     _line("fwd", 256, 2, 256, 256, 256, 256, 256, ws_bytes=lds),
                     _line("fwd", 256, 2, 256, 256, 256, 256, 256, ws_bytes=lds - 1),
                     _line("fwd", 256, 2, 256, 256, 256, 256, 256, ws_bytes=0),
                     _line("fwd", 256, 2, 256, 256, 128, 128, 128, ws_bytes=0)])
    assert [g[0] for g in got] == ["trunk_fwd_tm2/s16", "EWS", "EWS", "lds_tile1_v4_full/s2", "EWS", "EWS",
                                   "lds_tile1_v4_full/s1"]


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
