"""The rows of the per-launch head audit (tests/head_variants.py) against the planner the library launches from
(csrc/step_plan.h and csrc/gemm_plan.h through tests/step_plan_dump.cpp): every decision of the head section is taken on
both sides by a row, except the sides no batch can reach, listed with their reason; and the stage references of
tests/head_audit.py, chained on the CPU in fp64, are the reference update (OracleAgent, its BC and PER forms, torch autograd).  No GPU needed."""
import os
import subprocess
from collections import OrderedDict

import pytest
import torch

from tests import gemm_variants as gv
from tests import head_audit as ha
from tests import head_variants as hv

# (B, A, F, H, mode) the audit may add rows to, never lose one of
ISSUE_ROWS = [(8, 6, 50, 256, "fp32"), (32, 6, 50, 256, "fp32"), (128, 6, 50, 1024, "fp32"), (32, 21, 100, 256, "fp32"),
              (32, 1, 50, 256, "fp32"), (8, 33, 50, 64, "fp32"), (8, 65, 20, 64, "fp32"), (1024, 12, 50, 256, "fp32"),
              (32, 6, 50, 1024, "bf16"), (32, 6, 50, 256, "bc"), (8, 33, 50, 64, "bc"), (32, 6, 50, 256, "per")]


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """tests/step_plan_dump.cpp compiled for the host: lines of shapes in, the ten decisions out"""
    from drqv2_amd import build
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan_dump")
    subprocess.check_call([build._hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Werror",
                           os.path.join(here, "step_plan_dump.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, check=True).stdout
        return [[int(v) for v in ln.split()] for ln in out.splitlines()]
    return run


def test_the_audit_keeps_its_rows():
    have = [(r.B, r.A, r.F, r.H, r.mode) for r in hv.AUDIT_ROWS]
    assert len(set(have)) == len(have)
    assert set(ISSUE_ROWS) <= set(have), set(ISSUE_ROWS) - set(have)
    assert [r.B for r in hv.AUDIT_ROWS if r.updates == 2] == [32]
    assert not hasattr(hv, "NOT_AUDITED")               # one exemption only: the sides no batch reaches
    assert all(r.B <= hv.MAX_BATCH and r.reaches for r in hv.AUDIT_ROWS)


def test_each_rows_expected_decisions_are_the_planners(plan_dump):
    got = plan_dump([hv.dump_line(r) for r in hv.AUDIT_ROWS])
    assert len(got) == len(hv.AUDIT_ROWS)
    for r, values in zip(hv.AUDIT_ROWS, got):
        assert min(values) >= 0, (hv.row_id(r), values)                 # -1: the planner refuses a product
        assert hv.decisions_of(values) == hv.expected(r), (hv.row_id(r), values)
        assert r.expect <= set(hv.DECISIONS)


def test_the_rows_run_under_a_cu_override_keep_their_decisions(plan_dump):
    """tests/test_hip_cu_counts.py runs the smallest row of each mode at 32 and 8 CUs with the row's own `expect`: the
    planner takes the same ten decisions there, and leaves fewer split-K records per trunk product than at 256 CUs"""
    from tests import cu_rows
    rows = cu_rows.head_rows()
    assert sorted(r.mode for r in rows) == ["bc", "bf16", "fp32", "per"]
    at_hw = plan_dump([hv.dump_line(r) for r in rows])
    for cus in cu_rows.FAMILY_CUS:
        for r, values, hw in zip(rows, plan_dump([hv.dump_line(r, cus=cus) for r in rows]), at_hw):
            assert min(values) >= 0 and hv.decisions_of(values) == hv.expected(r), (cus, hv.row_id(r), values)
            assert 1 < values[5] < hw[5] and 1 < values[6] < hw[6], (cus, hv.row_id(r), values, hw)


def test_the_trunk_records_are_the_ones_the_gemm_mirror_predicts(plan_dump):
    """"trunk forward leaves records" read from tests/gemm_variants.py (held to the planner by its own CPU test) agrees
    with the dump, split count included, for the fp32 rows (the mirror restates the fp32 rules only)"""
    rows = [r for r in hv.AUDIT_ROWS if r.mode != "bf16"]
    for r, values in zip(rows, plan_dump([hv.dump_line(r) for r in rows])):
        for n, col in ((4, 5), (1, 6)):
            sel = gv.partial(n, r.B, r.F, ha.R)
            assert sel.name != gv.EARG and (sel.split or 1) == values[col], (hv.row_id(r), n, sel.name, sel.split, values)


def one_sided(decisions):
    """{decision: the sides none of the given {decision: bool} dicts takes}, the UNREACHABLE sides left out"""
    seen = {k: set() for k in hv.DECISIONS}
    for dec in decisions:
        for k, v in dec.items():
            seen[k].add(v)
    out = {}
    for k in hv.DECISIONS:
        missing = {True, False} - seen[k]
        if k in hv.UNREACHABLE:
            assert hv.UNREACHABLE[k][0] not in seen[k] and hv.UNREACHABLE[k][1], "%s: a row takes the listed side" % k
            missing -= {hv.UNREACHABLE[k][0]}
        if missing:
            out[k] = sorted(missing)
    return out


def test_every_decision_is_taken_on_both_sides_by_a_row():
    assert set(hv.UNREACHABLE) <= set(hv.DECISIONS)
    assert one_sided(hv.expected(r) for r in hv.AUDIT_ROWS) == {}, "sides no audit row takes"


def test_the_table_of_unreachable_sides_is_accurate(plan_dump):
    """no batch 1..MAX_BATCH takes a listed side, at the action and feature widths of the rows and at the largest ones,
    in either compute dtype; every other decision is reachable on both sides in that range (nothing hides behind the
    table); and the rows that take the two no-record sides of the trunk products are the smallest batches that do"""
    shapes = sorted({(r.A, r.F, r.H) for r in hv.AUDIT_ROWS} | {(32, 256, 1024), (256, 256, 1024)})
    cases = [(B, A, F, H, bf) for (A, F, H) in shapes for bf in (0, 1) for B in range(1, hv.MAX_BATCH + 1)]
    got = plan_dump(["%d %d %d %d %d %d 0\n" % (hv.CUS, B, A, F, H, bf) for B, A, F, H, bf in cases])
    assert len(got) == len(cases)
    seen = {k: set() for k in hv.DECISIONS}
    first = {}
    for case, values in zip(cases, got):
        for k, v in hv.decisions_of(values).items():
            seen[k].add(v)
            first.setdefault((k, v, case[2], case[4]), case[0])
    for k, (side, _) in hv.UNREACHABLE.items():
        assert side not in seen[k], "%s is %s for some batch: it needs an audit row, not a table entry" % (k, side)
    for k in hv.DECISIONS:
        if k not in hv.UNREACHABLE:
            assert seen[k] == {True, False}, (k, seen[k])
    assert first[("sk.trunk1", False, 256, 0)] == 2017 and first[("sk.trunk1", False, 100, 0)] == 4065
    assert first[("sk.trunk4", False, 256, 0)] == 481
    # the limit of the LDS of the loss-carrying Q output backward
    assert [v[2] for v in plan_dump(["256 10224 6 50 256 0 0\n", "256 10225 6 50 256 0 0\n"])] == [1, 0]


def test_a_moved_threshold_is_noticed(plan_dump):
    """the coverage check is sensitive to the decisions it is fed: with the planner's answers for the same rows under
    DRQ_STEP_NO_ROW_FUSION (fuse_rows false everywhere) it reports fuse_rows as one-sided, and with a row removed the
    side only that row takes"""
    got = plan_dump([hv.dump_line(r, flags=1) for r in hv.AUDIT_ROWS])
    assert one_sided(hv.decisions_of(v) for v in got) == {"fuse_rows": [True]}
    without = [hv.expected(r) for r in hv.AUDIT_ROWS if r.B != 2017]
    assert one_sided(without) == {"sk.trunk1": [False]}
    without = [hv.expected(r) for r in hv.AUDIT_ROWS if r.A != 65]
    assert one_sided(without) == {"out_layer_kernel": [False]}


# ------------------------------------------------------------------------ the stage references compose to the update
B, A, F, H = 4, 3, 20, 64
LR, TAU, STD, CLIP = 1e-3, 0.01, 0.2, 0.3


def nerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _setup():
    from drqv2_amd import synth
    enc, actor, critic = synth.make_weights(9, A, F, H, 3)
    batch = synth.make_batch(B, A, 9, seed=30, smooth=True)
    sh_o, sh_n, n_c, n_a = synth.make_draws(B, A, seed=30)
    return enc, actor, critic, batch, (sh_o, sh_n, n_c.double(), n_a.double())


def _chain(o, batch, draws, alpha=None, weights=None):
    """tests/head_audit.py's update on the oracle's own features, from the oracle's state BEFORE its update"""
    from oracle import drq_oracle as O
    dd = lambda d: OrderedDict((k, v.clone()) for k, v in d.items())
    actor, critic, target = dd(o.actor), dd(o.critic), dd(o.critic_target)
    obs_a = O.random_shifts_aug(batch[0].double(), draws[0], 4)
    next_a = O.random_shifts_aug(batch[4].double(), draws[1], 4)
    feat = O.encoder_forward(o.enc, obs_a).detach()
    feat_next = O.encoder_forward(o.enc, next_a).detach()
    r = ha.head_update(actor, critic, target, feat, feat_next, batch[1].double(), batch[2].double().reshape(-1),
                       batch[3].double().reshape(-1), draws[2], draws[3], STD, CLIP, LR, TAU, alpha=alpha, weights=weights)
    return r, actor, critic, target, feat


@pytest.mark.parametrize("mode", ["plain", "bc", "per"])
def test_the_stage_references_chain_to_the_oracles_update(mode):
    """gradients, sums and stepped parameters of the chained stages against OracleAgent (BCOracleAgent, PEROracleAgent)
    in fp64, 1e-12 normwise; the oracle differentiates with autograd, the stages with the formulas the kernels
    implement"""
    from oracle import drq_oracle as O
    from tests.bc_oracle import BCOracleAgent
    from tests.per_oracle import PEROracleAgent
    enc, actor, critic, batch, draws = _setup()
    kw = dict(stddev_schedule=str(STD), stddev_clip=CLIP, critic_target_tau=TAU, dtype=torch.float64)
    w = None
    if mode == "bc":
        o = BCOracleAgent(enc, actor, critic, LR, alpha=2.5, **kw)
    elif mode == "per":
        o = PEROracleAgent(enc, actor, critic, LR, **kw)
        w = torch.linspace(0.2, 1.0, B, dtype=torch.float64)
    else:
        o = O.OracleAgent(enc, actor, critic, LR, **kw)
    r, actor1, critic1, target1, feat = _chain(o, batch, draws, alpha=2.5 if mode == "bc" else None, weights=w)
    extra = {"weights": w} if mode == "per" else {}
    m = o.update(batch, 0, draws[0], draws[1], draws[2], draws[3], keep=True, **extra)
    for k, g in o.last["g_critic"].items():
        assert nerr(r["g_critic"][k], g) <= 1e-12, (k, nerr(r["g_critic"][k], g))
    for k, g in o.last["g_actor"].items():
        assert nerr(r["g_actor"][k], g) <= 1e-12, (k, nerr(r["g_actor"][k], g))
    for name, mine, theirs in (("critic", critic1, o.critic), ("actor", actor1, o.actor), ("target", target1, o.critic_target)):
        for k in theirs:
            assert nerr(mine[k], theirs[k]) <= 1e-12, (name, k)
    assert nerr(r["a"], o.last["a"]) <= 1e-12 and nerr(r["mu"], o.last["mu"]) <= 1e-12
    s = r["sums"]
    means = {"batch_reward": s[0] / B, "critic_target_q": s[1] / B, "critic_q1": s[2] / B, "critic_q2": s[3] / B,
             "critic_loss": s[4] / B, "actor_logprob": s[6] / B}
    if mode == "bc":
        means["actor_bc_loss"] = s[9] / (B * A)
        means["actor_bc_lambda"] = r["lam"]
        means["actor_loss"] = r["lam"] * s[5] / B + s[9] / (B * A)
        assert float(s[10]) == pytest.approx(float(o.last["bc"]["qmin"].abs().sum()), rel=1e-12)
    else:
        means["actor_loss"] = s[5] / B
    for k, v in means.items():
        assert float(v) == pytest.approx(m[k], rel=1e-12, abs=1e-14), (k, float(v), m[k])
    if mode == "per":
        assert nerr(r["td_abs"], o.last["td_abs"]) <= 1e-12


def test_the_stage_references_agree_with_autograd_on_the_features():
    """the critic loss's gradient of the encoder output (what DY4 holds): the chain's masked product against autograd
    through oracle.critic_q"""
    from oracle import drq_oracle as O
    enc, actor, critic, batch, draws = _setup()
    o = O.OracleAgent(enc, actor, critic, LR, stddev_schedule=str(STD), stddev_clip=CLIP, critic_target_tau=TAU,
                      dtype=torch.float64)
    r, _, _, _, feat = _chain(o, batch, draws)
    fr = feat.clone().requires_grad_(True)
    next_a = O.random_shifts_aug(batch[4].double(), draws[1], 4)
    with torch.no_grad():
        fn = O.encoder_forward(o.enc, next_a)
        a_next = O.trunc_normal_sample(O.actor_mu(o.actor, fn), draws[2], STD, CLIP)
        tq1, tq2 = O.critic_q(o.critic_target, fn, a_next)
        y = batch[2].double() + batch[3].double() * torch.minimum(tq1, tq2)
    q1, q2 = O.critic_q(o.critic, fr, batch[1].double())
    loss = ((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean()
    (g,) = torch.autograd.grad(loss, fr)
    assert nerr(r["dfeat"], g * (feat > 0)) <= 1e-12
