"""Per-launch audit of the head section inside the fused update, phase by phase.

After the encoder forward update() runs about forty launches (trunks, LayerNorm+tanh, policy MLP and both draws, four Q
networks, two losses with their backward passes, three optimiser steps), many of them reachable only from step.hip; the
whole-update tests hold them to end-to-end bounds (2e-3 normwise for the actor's gradients).  Here the update is issued
as its three composite phases (DRQ_PHASE_CRITIC, _ACTOR, _OPT: the launches of DRQ_PHASE_ALL, which a twin agent running
the plain update proves bit for bit), its buffers are read back after each, and every stage is compared with the fp64
evaluation of that stage alone (tests/head_audit.py) on the operands the launch read: the weights snapshotted before
the phase and the update's own upstream buffers, its own ReLU decisions, xhat, rstd and mu included.  Bounds, all the
project's own:

  GEMM-like stages   tests/gemm_variants.compare: 3e-6 normwise and 2 (K+2) 2^-24 (|A||B| + |bias|) componentwise.  Two
                     stages chain what the update never stores: the loss gradient dq (a few fp32 operations on q, r, d
                     tq: K = 4 on |q| + |r| + |d tq|) into the Q output backward, and dpre into the fused policy output
                     backward (K = the sum of both reductions)
  LayerNorm+tanh     forward (with the trunk product in front of it, whose records are never stored) 2e-6; backward,
                     parameter gradients and the two composites that end in it 1e-5 (test_ln_tanh)
  loss sums, td_abs  rel 1e-5, abs 1e-5 against fp64 (test_hip_step)
  bf16               products on the MFMA: 1e-5 normwise on operands rounded to bf16, bias gradients 3e-6 on the
                     unrounded values they sum (test_hip_bf16); everything else in the bf16 update is an fp32 kernel
  optimiser, Polyak, draws of the obs rows, copied action columns   bit for bit

What the audit cannot see: where the rows are fused (fuse_rows) and drq_lnl1_fwd refuses a shape with DRQ_EARG, step.hip
falls back to drq_ln_tanh_fwd_multi_part and separate first-layer launches, which write the same buffers: the NaN map
cannot tell the two apart, so the rows that name the rowblock kernels are not proof that those kernels ran (their
values are held to the same bounds either way).

Before phase 0 every head buffer is filled with NaN: no audited output may hold one, and the buffers the taken path does
not write must still be all NaN afterwards, which is how the test sees which path ran (tests/head_variants.py says
which, tests/test_cpu_head_audit.py holds that to the planner).  One line per stage: row, update, phase, stage,
measured error, bound (GEMM-like: normwise error, then the largest componentwise error / bound)."""
from collections import OrderedDict

import pytest
import torch

import utils
from drqv2_amd import _lib, synth
from oracle import drq_oracle as O
from tests import gemm_variants as gv
from tests import head_audit as ha
from tests import head_variants as hv
from tests.test_hip_step import make_agent

pytestmark = pytest.mark.gpu

LN_FWD, LN_BWD, BF16, BIAS16 = 2e-6, 1e-5, 1e-5, 3e-6
R = ha.R
NAN = float("nan")


def shapes(B, A, F, H):
    FA, hid = F + A, (2, B, H)
    return {"Z_NEXT": (B, 2 * F), "Z_OBS": (B, 2 * F), "HA_T": (B, FA), "HA_C": (B, FA), "H_AN": (B, F), "H_AO": (B, F),
            "Q": (2, B), "TQ": (2, B), "DQ": (2, B), "MU_O": (B, A), "DZ_C": (B, F), "DZ_A": (B, F), "HA_C2": (B, FA),
            "XHAT_C": (B, F), "RSTD_C": (B,), "XHAT_A": (B, F), "RSTD_A": (B,), "Z_C2": (B, F), "HROWS": (2 * B, F),
            "P1": (2 * B, H), "P2": (2 * B, H), "P3": (2 * B, A), "Z4": (4, B, F), "T1": hid, "T2": hid, "C1": hid,
            "C2": hid, "DC2": hid, "DC1": hid, "DHA": (2, B, FA), "DLN": (B, F), "DPRE": (B, A), "DP2": (B, H),
            "DP1": (B, H), "DH_A": (B, F), "DA": (2, B, A)}


def cfg_for(row):
    return dict(C=9, A=row.A, F=row.F, H=row.H, B=row.B, lr=1e-4, sched="linear(1.0,0.1,500000)", wseed=30 + row.B % 11,
                bseed=300 + row.B + row.A, updates=row.updates, step0=0, smooth=row.B < 2000)


def r16(t):
    return t.to(torch.bfloat16).double()


def net_tensors(ag, arena, net):
    """{parameter name: view} of one network's tensors inside a flat arena (eng.params, eng.grads or a clone)"""
    mod = ag._engine.modules[net]
    return OrderedDict((n, arena[off:off + p.numel()].view(p.shape))
                       for (n, p), off in zip(mod.named_parameters(), ag._engine.layout[net]))


def snapshot(ag, row, big=False):
    eng = ag._engine
    torch.cuda.synchronize()
    s = dict(params=eng.params.clone(), grads=eng.grads.clone(), m=eng.adam_m.clone(), v=eng.adam_v.clone(),
             sums=eng._sums_all.clone())
    s["ws"] = {k: eng.ws_view(k, row.B, shp).clone() for k, shp in shapes(row.B, row.A, row.F, row.H).items()}
    if big:
        s["ws"]["FEAT"] = eng.ws_view("FEAT", row.B, (2 * row.B, R)).clone()
        s["ws"]["DY4"] = eng.ws_view("DY4", row.B, (row.B, 32, 39, 39)).clone()
    return s


def inputs(cfg, u):
    B, A = cfg["B"], cfg["A"]
    obs, action, reward, discount, next_obs = synth.make_batch(B, A, cfg["C"], seed=cfg["bseed"] + u, smooth=cfg["smooth"])
    sh_o, sh_n, n_c, n_a = synth.make_draws(B, A, seed=cfg["bseed"] + u)
    f = lambda t, *shp: t.float().reshape(*shp).contiguous().cuda()
    return dict(obs=obs.contiguous().cuda(), next_obs=next_obs.contiguous().cuda(), action=f(action, B, A),
                reward=f(reward, B), discount=f(discount, B), sh_o=f(sh_o, B, 2), sh_n=f(sh_n, B, 2), n_c=f(n_c, B, A),
                n_a=f(n_a, B, A), w=torch.linspace(0.2, 1.0, B).cuda().contiguous())


def prepare(row, cfg):
    ag = make_agent(cfg)
    if row.mode == "bf16":
        ag = ag.set_compute_dtype("bf16")
    if row.mode == "bc":
        ag.set_behavior_cloning(hv.BC_ALPHA)
    if row.updates > 1:
        ag._engine.encoder_opt.t = 3          # step_enc != step_actor: the per-segment scalars of drq_adam_flat2
    return ag


def phased_update(ag, row, cfg, u, x):
    """one update as DRQ_PHASE_CRITIC, _ACTOR, _OPT with the descriptor StepEngine.update's single-GPU branch fills;
    returns the four snapshots (before, after each phase) and the scalars of the step"""
    eng, B = ag._engine, row.B
    std = utils.schedule(ag.stddev_schedule, cfg["step0"] + 2 * u)
    per = eng._loss_weights(x["w"], B) if row.mode == "per" else None
    steps = (eng.critic_opt.begin_step(), eng.encoder_opt.begin_step(), eng.actor_opt.begin_step())
    d = eng.make_desc(B, B, std, ag.stddev_clip, ag.critic_target_tau, steps)
    d.obs, d.next_obs = _lib.ptr(x["obs"]), _lib.ptr(x["next_obs"])
    d.obs_index, d.next_obs_index = None, None
    d.action, d.reward, d.discount = _lib.ptr(x["action"]), _lib.ptr(x["reward"]), _lib.ptr(x["discount"])
    d.shift_obs, d.shift_next = _lib.ptr(x["sh_o"]), _lib.ptr(x["sh_n"])
    d.noise_critic, d.noise_actor = _lib.ptr(x["n_c"]), _lib.ptr(x["n_a"])
    eng._throttle(steps[2] & 0xFFFFFFFF)
    for k, shp in shapes(B, row.A, row.F, row.H).items():
        eng.ws_view(k, B, shp).fill_(NAN)
    snaps = [snapshot(ag, row)]
    for phase in (_lib.PHASE_CRITIC, _lib.PHASE_ACTOR, _lib.PHASE_OPT):
        eng._phase(d, phase, per)
        snaps.append(snapshot(ag, row, big=phase == _lib.PHASE_CRITIC))
    eng.last_td_abs = per[1] if per is not None else None
    eng._last_seq = steps[2] & 0xFFFFFFFF
    return snaps, dict(std=float(std), clip=float(ag.stddev_clip), tau=float(ag.critic_target_tau), steps=steps,
                       lr=float(eng.critic_opt.lr), td_abs=None if per is None else per[1].clone())


def plain_update(ag, cfg, u, x, row):
    eng = ag._engine
    std = utils.schedule(ag.stddev_schedule, cfg["step0"] + 2 * u)
    kw = {"loss_weights": x["w"]} if row.mode == "per" else {}
    eng.update(x["obs"], x["action"], x["reward"], x["discount"], x["next_obs"], x["sh_o"], x["sh_n"], x["n_c"], x["n_a"],
               std, ag.stddev_clip, ag.critic_target_tau, **kw)
    torch.cuda.synchronize()


class Rec:
    def __init__(self, row, u):
        self.tag, self.bad, self.worst = "%s update=%d" % (hv.row_id(row), u), [], {}
        self.bf16 = row.mode == "bf16"

    def add(self, phase, stage, err, bound, ok, extra=""):
        err = err if err == err else float("inf")
        print("head-audit %s phase=%d stage=%s err=%.3e bound=%.0e%s%s" % (self.tag, phase, stage, err, bound, extra,
                                                                        "" if ok else "  MISS"))
        self.worst[stage] = max(self.worst.get(stage, 0.0), err / bound if bound else (0.0 if ok else float("inf")))
        if not ok:
            self.bad.append((phase, stage, err, bound))

    def norm(self, phase, stage, got, ref, bound):
        e = float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))
        self.add(phase, stage, e, bound, e <= bound and float(ref.abs().max()) > 0)

    def comp(self, phase, stage, got, ref, mag, K):
        ok, ne, ratio = gv.compare(got.reshape(ref.shape), ref.cpu(), mag.cpu(), K)
        # (a reference that is zero throughout is legitimate here: a Q head that never holds the minimum gets no gradient)
        self.add(phase, stage, ne, gv.NORMWISE, ok, " componentwise=%.3f" % ratio)

    def gemm(self, phase, stage, got, A, Bm, K, bias=None, relu=False, mask=None, mfma=False):
        """got against A [M][K] Bm [K][N] (+ bias, ReLU, mask); mfma: the launch runs on the bf16 MFMA in a bf16 update"""
        if mfma and self.bf16:
            ref, _ = gv.reference(r16(A), r16(Bm), None if bias is None else bias.double(), relu, mask)
            return self.norm(phase, stage, got.reshape(ref.shape), ref, BF16)
        ref, mag = gv.reference(A.double(), Bm.double(), None if bias is None else bias.double(), relu, mask)
        self.comp(phase, stage, got, ref, mag, K)

    def colsum(self, phase, stage, got, dy):
        """a bias gradient: the column sums of dy (bf16 update: of the unrounded values, 3e-6)"""
        if self.bf16:
            return self.norm(phase, stage, got, dy.double().sum(0), BIAS16)
        self.comp(phase, stage, got, dy.double().sum(0), dy.double().abs().sum(0), dy.shape[0])

    def close(self, phase, stage, got, ref):
        """rel 1e-5, abs 1e-5 against fp64, elementwise"""
        got, ref = got.double().reshape(-1), ref.double().reshape(-1)
        e = float(((got - ref).abs() / (1e-5 + 1e-5 * ref.abs())).max())
        self.add(phase, stage, e, 1.0, e <= 1.0)

    def absolute(self, phase, stage, got, ref, bound):
        e = float((got.double() - ref.double()).abs().max())
        self.add(phase, stage, e, bound, e <= bound)

    def exact(self, phase, stage, got, want):
        n = int((got != want).sum()) + int(torch.isnan(got).sum())
        self.add(phase, stage, float(n), 0.0, n == 0 and got.shape == want.shape, " (elements that differ)")

    def all_nan(self, phase, name, t, want):
        """want: the buffer was not written (every element still NaN); else: no element is NaN"""
        n = int(torch.isnan(t).sum())
        ok = n == t.numel() if want else n == 0
        self.add(phase, name + (".untouched" if want else ".written"), float(t.numel() - n if want else n), 0.0, ok,
                 " (elements that are not)")


TRUNK = ("trunk.0.weight", "trunk.0.bias", "trunk.1.weight", "trunk.1.bias")


def trunk_stage(rec, ph, tag, feat, p, h_got, xh_got=None, rs_got=None, z_got=None):
    rd = r16 if rec.bf16 else (lambda t: t.double())
    w, b, g, bt = (p[k] for k in TRUNK)
    h, xh, rs, _ = ha.trunk_ln(rd(feat), rd(w), b.double(), g.double(), bt.double())
    fwd = BF16 if rec.bf16 else LN_FWD
    if z_got is None:
        # records: the product is never stored, the stage is the composite product + LayerNorm + tanh
        rec.norm(ph, tag, h_got, h, fwd)
    else:
        # no records: the product is stored, and it is the operand the LayerNorm launch read.  Each launch is judged on
        # its own and the composite is not: through the unsplit 39200-long product h measures 1.9e-6 and xhat 2.5e-6 at
        # F = 256 (the product's own error, inside its 3e-6, grows by |z| / sigma in (z - mean) rstd), which says
        # nothing about either launch that the two lines below do not
        rec.gemm(ph, tag + ".z", z_got, feat, w.t(), R, bias=b, mfma=True)
        h, xh, rs = ha.ln_tanh(z_got.double(), g.double(), bt.double())
        fwd = LN_FWD
        rec.norm(ph, tag + ".ln_of_z", h_got, h, fwd)
    if xh_got is not None:
        rec.norm(ph, tag + ".xhat", xh_got, xh, fwd)
        rec.norm(ph, tag + ".rstd", rs_got, rs, fwd)


def q_forward_stage(rec, ph, tag, p, x, h1, h2, q):
    for i, k in enumerate(("Q1", "Q2")):
        rec.gemm(ph, "%s1.%s" % (tag, k), h1[i], x, p[k + ".0.weight"].t(), x.shape[1], p[k + ".0.bias"], True, mfma=True)
        rec.gemm(ph, "%s2.%s" % (tag, k), h2[i], h1[i], p[k + ".2.weight"].t(), h1.shape[2], p[k + ".2.bias"], True, mfma=True)
        rec.gemm(ph, "%sQ.%s" % (tag, k), q[i].reshape(-1, 1), h2[i], p[k + ".4.weight"].t(), h2.shape[2], p[k + ".4.bias"])


def ln_backward_stage(rec, ph, tag, d, h, xhat, rstd, p, dz_got, dln_got, g_gamma, g_beta, g_w, g_b, feat):
    """the composite that ends in the LayerNorm+tanh backward, the parameter gradients and the trunk's gradients"""
    dz, dln = ha.ln_tanh_bwd(d, h.double(), xhat.double(), rstd.double(), p["trunk.1.weight"].double())
    rec.norm(ph, tag + ".DLN", dln_got, dln, LN_BWD)
    rec.norm(ph, tag + ".DZ", dz_got, dz, LN_BWD)
    gg, gb = ha.ln_param_grads(dln_got.double(), xhat.double())
    rec.norm(ph, tag + ".dgamma", g_gamma, gg, LN_BWD)
    rec.norm(ph, tag + ".dbeta", g_beta, gb, LN_BWD)
    # the trunk's weight gradient is an fp32 kernel below 512 rows in the bf16 update too (Ctx::wgrad_call)
    rec.gemm(ph, tag + ".trunk_dW", g_w, dz_got.t(), feat, feat.shape[0], mfma=feat.shape[0] >= 512)
    rec.colsum(ph, tag + ".trunk_db", g_b, dz_got)


def audit_phase0(rec, ag, row, s0, s1, x, sc):
    B, F, H = row.B, row.F, row.H
    dec = hv.expected(row)
    b = s1["ws"]
    cr, ac, tg = (net_tensors(ag, s0["params"], n) for n in ("critic", "actor", "target"))
    gc = net_tensors(ag, s1["grads"], "critic")
    fo, fn = b["FEAT"][:B], b["FEAT"][B:]
    z4 = None if dec["sk.trunk4"] else b["Z4"]
    # ---- which path ran
    for k in ("Z_NEXT", "Z_OBS", "H_AN", "H_AO", "Z_C2", "DZ_A", "DP2", "DP1", "DH_A", "DA", "DPRE"):
        rec.all_nan(0, k, b[k], True)
    rec.all_nan(0, "HA_C2[:, :F]", b["HA_C2"][:, :F], True)
    rec.all_nan(0, "Z4", b["Z4"], dec["sk.trunk4"])
    rec.all_nan(0, "DQ", b["DQ"], dec["qout_loss_fits_lds"])
    rec.all_nan(0, "DHA", b["DHA"], dec["sk.dha"])
    # ---- trunks + LayerNorm + tanh
    trunk_stage(rec, 0, "HA_C", fo, cr, b["HA_C"][:, :F], b["XHAT_C"], b["RSTD_C"], None if z4 is None else z4[0])
    trunk_stage(rec, 0, "HROWS.obs", fo, ac, b["HROWS"][:B], b["XHAT_A"], b["RSTD_A"], None if z4 is None else z4[1])
    trunk_stage(rec, 0, "HROWS.next", fn, ac, b["HROWS"][B:], None, None, None if z4 is None else z4[2])
    trunk_stage(rec, 0, "HA_T", fn, tg, b["HA_T"][:, :F], None, None, None if z4 is None else z4[3])
    rec.exact(0, "HA_C.action", b["HA_C"][:, F:], x["action"])
    # ---- policy MLP on the 2B rows; the output layer is an fp32 kernel up to 64 actions
    rec.gemm(0, "P1", b["P1"], b["HROWS"], ac["policy.0.weight"].t(), F, ac["policy.0.bias"], True, mfma=True)
    rec.gemm(0, "P2", b["P2"], b["P1"], ac["policy.2.weight"].t(), H, ac["policy.2.bias"], True, mfma=True)
    rec.gemm(0, "P3", b["P3"], b["P2"], ac["policy.4.weight"].t(), H, ac["policy.4.bias"], mfma=not dec["out_layer_kernel"])
    rec.absolute(0, "MU_O", b["MU_O"], torch.tanh(b["P3"][:B].double()), 2e-7)
    # ---- both draws through the oracle's clamp chain (test_trunc_normal_sample_bitwise's method)
    a_obs = O.trunc_normal_sample(b["MU_O"].cpu(), x["n_a"].cpu(), sc["std"], sc["clip"])
    rec.exact(0, "HA_C2.action", b["HA_C2"][:, F:].cpu(), a_obs)
    mu_next = torch.tanh(b["P3"][B:].double()).float().cpu()
    a_next = O.trunc_normal_sample(mu_next, x["n_c"].cpu(), sc["std"], sc["clip"])
    rec.absolute(0, "HA_T.action", b["HA_T"][:, F:].cpu(), a_next, 2e-7)
    # ---- the four Q networks
    q_forward_stage(rec, 0, "T", tg, b["HA_T"], b["T1"], b["T2"], b["TQ"])
    q_forward_stage(rec, 0, "C", cr, b["HA_C"], b["C1"], b["C2"], b["Q"])
    # ---- TD loss
    w = x["w"].double() if row.mode == "per" else None
    tq, q, r, dsc = b["TQ"].double(), b["Q"].double(), x["reward"].double(), x["discount"].double()
    y, dq, sums, td_abs = ha.td_loss(tq, q, r, dsc, B, w)
    rec.close(0, "sums[0..4]", s1["sums"][:5], sums)
    if row.mode == "per":
        rec.close(0, "td_abs", sc["td_abs"], td_abs)
    # what the fp32 evaluation of dq can be off by: four operations on these magnitudes
    mag_dq = 2.0 / B * (q.abs() + r.abs() + (dsc * torch.minimum(tq[0], tq[1])).abs()) * (1.0 if w is None else w)
    if not dec["qout_loss_fits_lds"]:
        rec.comp(0, "DQ", b["DQ"], dq, mag_dq, 4)
    for i, k in enumerate(("Q1", "Q2")):
        w2 = cr[k + ".4.weight"].double().reshape(1, -1)
        keep = (b["C2"][i] > 0).double()
        rec.comp(0, "DC2." + k, b["DC2"][i], dq[i][:, None] * w2 * keep, mag_dq[i][:, None] * w2.abs() * keep, 4)
        rec.comp(0, "dW3." + k, gc[k + ".4.weight"], (dq[i] @ b["C2"][i].double()).reshape(1, -1),
                 (mag_dq[i] @ b["C2"][i].double().abs()).reshape(1, -1), B + 4)
        rec.comp(0, "db3." + k, gc[k + ".4.bias"], dq[i].sum().reshape(1), mag_dq[i].sum().reshape(1), B + 4)
        # layer 2
        rec.gemm(0, "DC1." + k, b["DC1"][i], b["DC2"][i], cr[k + ".2.weight"], H, mask=b["C1"][i].double(), mfma=True)
        rec.gemm(0, "dW2." + k, gc[k + ".2.weight"], b["DC2"][i].t(), b["C1"][i], B, mfma=True)
        rec.colsum(0, "db2." + k, gc[k + ".2.bias"], b["DC2"][i])
        # layer 1
        rec.gemm(0, "dW1." + k, gc[k + ".0.weight"], b["DC1"][i].t(), b["HA_C"], B, mfma=True)
        rec.colsum(0, "db1." + k, gc[k + ".0.bias"], b["DC1"][i])
        if not dec["sk.dha"]:
            rec.gemm(0, "DHA." + k, b["DHA"][i], b["DC1"][i], cr[k + ".0.weight"], H, mfma=True)
    rd = r16 if rec.bf16 else (lambda t: t.double())
    d = sum(rd(b["DC1"][i]) @ rd(cr[k + ".0.weight"][:, :F]) for i, k in enumerate(("Q1", "Q2")))
    ln_backward_stage(rec, 0, "critic", d, b["HA_C"][:, :F], b["XHAT_C"], b["RSTD_C"], cr, b["DZ_C"], b["DLN"],
                      gc["trunk.1.weight"], gc["trunk.1.bias"], gc["trunk.0.weight"], gc["trunk.0.bias"], fo)
    # ---- d feat, masked by relu(conv4), scattered into the gradient buffer padded by 2 (an fp32 kernel in both dtypes)
    dy4 = b["DY4"]
    ref, mag = gv.reference(b["DZ_C"].double(), cr["trunk.0.weight"].double(), mask=fo.double())
    rec.comp(0, "DY4", dy4[:, :, 2:-2, 2:-2].reshape(B, R), ref, mag, F)
    border = dy4.clone()
    border[:, :, 2:-2, 2:-2] = 0
    rec.exact(0, "DY4.border", border, torch.zeros_like(border))


def flat_adam(seg, p0, g, m0, v0, t, lr):
    """O.adam_step on a copy of one segment; returns (p, m, v) on the CPU"""
    b, e = seg
    p, gg, m, v = (a[b:e].detach().cpu().clone() for a in (p0, g, m0, v0))
    O.adam_step(p, gg, m, v, t, lr)
    return p, m, v


def audit_phase1(rec, ag, row, s1, s2, x, sc, pull_factor=1.0):
    """pull_factor: the positive control's wrong scale of the BC pull in the REFERENCE (1 = the definition)"""
    B, A, F, H = row.B, row.A, row.F, row.H
    dec = hv.expected(row)
    eng = ag._engine
    b, feat = s2["ws"], s1["ws"]["FEAT"][:B]
    seg = eng.layout["seg"]
    # ---- critic_opt.step() and Polyak, bit for bit
    p, m, v = flat_adam(seg["critic"], s1["params"], s1["grads"], s1["m"], s1["v"], sc["steps"][0], sc["lr"])
    c0, c1 = seg["critic"]
    rec.exact(1, "adam.critic.p", s2["params"][c0:c1].cpu(), p)
    rec.exact(1, "adam.critic.m", s2["m"][c0:c1].cpu(), m)
    rec.exact(1, "adam.critic.v", s2["v"][c0:c1].cpu(), v)
    t0, t1 = seg["target"]
    tgt = s1["params"][t0:t1].cpu().clone()
    O.polyak(p, tgt, sc["tau"])
    rec.exact(1, "polyak", s2["params"][t0:t1].cpu(), tgt)
    rec.exact(1, "critic.grads.untouched", s2["grads"][c0:c1], s1["grads"][c0:c1])
    # ---- which path ran
    rec.all_nan(1, "Z_C2", b["Z_C2"], dec["sk.trunk1"])
    rec.all_nan(1, "DQ", b["DQ"], dec["qout_loss_fits_lds"])
    rec.all_nan(1, "DPRE", b["DPRE"], dec["fused_head"])
    rec.all_nan(1, "DA", b["DA"], dec["fused_head"] and dec["sk.da"])
    rec.all_nan(1, "DH_A", b["DH_A"], dec["sk.dh"])
    rec.all_nan(1, "DHA", b["DHA"], dec["sk.dha"])
    for k in ("Z_NEXT", "Z_OBS", "H_AN", "H_AO"):
        rec.all_nan(1, k, b[k], True)
    # ---- the stepped critic on (obs, a)
    cr, ac = net_tensors(ag, s2["params"], "critic"), net_tensors(ag, s2["params"], "actor")
    ga = net_tensors(ag, s2["grads"], "actor")
    trunk_stage(rec, 1, "HA_C2", feat, cr, b["HA_C2"][:, :F], None, None, None if dec["sk.trunk1"] else b["Z_C2"])
    rec.exact(1, "HA_C2.action.kept", b["HA_C2"][:, F:], s1["ws"]["HA_C2"][:, F:])
    rec.exact(1, "MU_O.kept", b["MU_O"], s1["ws"]["MU_O"])
    q_forward_stage(rec, 1, "T", cr, b["HA_C2"], b["T1"], b["T2"], b["TQ"])
    # ---- actor loss
    bc = row.mode == "bc"
    a, mu, a_beh = b["HA_C2"][:, F:].double(), b["MU_O"].double(), x["action"].double()
    std32 = float(torch.tensor(sc["std"], dtype=torch.float32))
    q = b["TQ"].double()
    dq, s5, s6, s9, s10, lam = ha.actor_loss(q, a, mu, std32, B, a_beh if bc else None, hv.BC_ALPHA if bc else None)
    rec.close(1, "sums[5..6]", s2["sums"][5:7], torch.stack([s5, s6]))
    if bc:
        rec.close(1, "sums[9..10]", s2["sums"][9:11], torch.stack([s9, s10]))
    mag_dq = dq.abs()
    if not dec["qout_loss_fits_lds"]:
        rec.comp(1, "DQ", b["DQ"], dq, mag_dq, B + 2 if bc else 1)
    kq = B + 4 if bc else 2         # BC: lambda carries the fixed-order sum of |Qmin| over the batch
    da_ref, da_mag = 0, 0
    for i, k in enumerate(("Q1", "Q2")):
        w2 = cr[k + ".4.weight"].double().reshape(1, -1)
        keep = (b["T2"][i] > 0).double()
        rec.comp(1, "DC2." + k, b["DC2"][i], dq[i][:, None] * w2 * keep, mag_dq[i][:, None] * w2.abs() * keep, kq)
        rec.gemm(1, "DC1." + k, b["DC1"][i], b["DC2"][i], cr[k + ".2.weight"], H, mask=b["T1"][i].double(), mfma=True)
        w0a = cr[k + ".0.weight"][:, F:]
        if not (dec["fused_head"] and dec["sk.da"]):
            rec.gemm(1, "DA." + k, b["DA"][i], b["DC1"][i], w0a, H, mfma=True)
        rd = r16 if rec.bf16 else (lambda t: t.double())
        da_ref = da_ref + rd(b["DC1"][i]) @ rd(w0a)
        da_mag = da_mag + rd(b["DC1"][i]).abs() @ rd(w0a).abs()
    # ---- dpre: (da_1 + da_2 [+ the BC pull]) (1 - mu^2)
    bc_scale = 2.0 / (B * A) * pull_factor
    dpre = ha.dpre_of(da_ref, mu, a, a_beh if bc else None, bc_scale)
    dpre_mag = (da_mag + (bc_scale * ((a - a_beh).abs() if bc else 0.0))) * (1.0 - mu * mu)
    kd = H + 6                      # the reduction over H, the sum of the heads, the pull, 1 - mu^2 and the product
    tol16 = rec.bf16                # bf16 update: da comes from MFMA products, held to 1e-5 normwise
    p2, p1, hr = b["P2"][:B], b["P1"][:B], b["HROWS"][:B]
    w3 = ac["policy.4.weight"].double()
    keep2 = (p2 > 0).double()
    if not dec["fused_head"]:
        if tol16:
            rec.norm(1, "DPRE", b["DPRE"], dpre, BF16)
        else:
            rec.comp(1, "DPRE", b["DPRE"], dpre, dpre_mag, kd)
        rec.gemm(1, "policy.dW3", ga["policy.4.weight"], b["DPRE"].t(), p2, B, mfma=True)
        rec.colsum(1, "policy.db3", ga["policy.4.bias"], b["DPRE"])
        rec.gemm(1, "DP2", b["DP2"], b["DPRE"], ac["policy.4.weight"], A, mask=p2.double(), mfma=True)
    else:
        # one fp32 kernel computes dpre in LDS and all three outputs from it: the chain's bound is the sum of its links'
        outs = (("policy.dW3", ga["policy.4.weight"], dpre.t() @ p2.double(), dpre_mag.t() @ p2.double().abs(), kd + B),
                ("policy.db3", ga["policy.4.bias"], dpre.sum(0), dpre_mag.sum(0), kd + B),
                ("DP2", b["DP2"], (dpre @ w3) * keep2, (dpre_mag @ w3.abs()) * keep2, kd + A))
        for name, got, ref, mag, K in outs:
            if tol16:
                rec.norm(1, name, got.reshape(ref.shape), ref, BF16)
            else:
                rec.comp(1, name, got, ref, mag, K)
    # ---- policy MLP backward
    rec.gemm(1, "DP1", b["DP1"], b["DP2"], ac["policy.2.weight"], H, mask=p1.double(), mfma=True)
    rec.gemm(1, "policy.dW2", ga["policy.2.weight"], b["DP2"].t(), p1, B, mfma=True)
    rec.colsum(1, "policy.db2", ga["policy.2.bias"], b["DP2"])
    rec.gemm(1, "policy.dW1", ga["policy.0.weight"], b["DP1"].t(), hr, B, mfma=True)
    rec.colsum(1, "policy.db1", ga["policy.0.bias"], b["DP1"])
    if not dec["sk.dh"]:
        rec.gemm(1, "DH_A", b["DH_A"], b["DP1"], ac["policy.0.weight"], H, mfma=True)
    rd = r16 if rec.bf16 else (lambda t: t.double())
    d = rd(b["DP1"]) @ rd(ac["policy.0.weight"])
    ln_backward_stage(rec, 1, "actor", d, hr, b["XHAT_A"], b["RSTD_A"], ac, b["DZ_A"], b["DLN"], ga["trunk.1.weight"],
                      ga["trunk.1.bias"], ga["trunk.0.weight"], ga["trunk.0.bias"], feat)


def audit_phase2(rec, ag, s2, s3, sc):
    seg = ag._engine.layout["seg"]
    for net, t in (("enc", sc["steps"][1]), ("actor", sc["steps"][2])):
        p, m, v = flat_adam(seg[net], s2["params"], s2["grads"], s2["m"], s2["v"], t, sc["lr"])
        b, e = seg[net]
        rec.exact(2, "adam.%s.p" % net, s3["params"][b:e].cpu(), p)
        rec.exact(2, "adam.%s.m" % net, s3["m"][b:e].cpu(), m)
        rec.exact(2, "adam.%s.v" % net, s3["v"][b:e].cpu(), v)
    for net in ("critic", "target"):
        b, e = seg[net]
        rec.exact(2, "%s.kept" % net, s3["params"][b:e], s2["params"][b:e])
    rec.exact(2, "grads.kept", s3["grads"], s2["grads"])


_cache = {}
# the rows the positive controls read again: only their agents and snapshots outlive the row's own test
KEPT = ("b32-a6-f50-h256-fp32", "b32-a6-f50-h256-bc")


def audited(row):
    """run the row once: [(Rec with every verdict, and for the KEPT rows the snapshots, inputs, scalars, agent)] per
    update"""
    key = hv.row_id(row)
    if key not in _cache:
        cfg = cfg_for(row)
        ag, twin = prepare(row, cfg), prepare(row, cfg)
        out = []
        for u in range(row.updates):
            x = inputs(cfg, u)
            snaps, sc = phased_update(ag, row, cfg, u, x)
            plain_update(twin, cfg, u, x, row)
            rec = Rec(row, u)
            for name, mine, theirs in (("params", ag._engine.params, twin._engine.params),
                                       ("grads", ag._engine.grads, twin._engine.grads),
                                       ("adam_m", ag._engine.adam_m, twin._engine.adam_m),
                                       ("adam_v", ag._engine.adam_v, twin._engine.adam_v),
                                       ("sums", ag._engine._sums_all, twin._engine._sums_all)):
                rec.exact(3, "phases==update()." + name, mine, theirs)
            audit_phase0(rec, ag, row, snaps[0], snaps[1], x, sc)
            audit_phase1(rec, ag, row, snaps[1], snaps[2], x, sc)
            audit_phase2(rec, ag, snaps[2], snaps[3], sc)
            out.append((rec, snaps, x, sc, ag) if key in KEPT else (rec, None, None, None, None))
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize("row", hv.AUDIT_ROWS, ids=hv.row_id)
def test_every_head_launch_of_the_update_meets_its_op_bound(row):
    """For the record, measured on the MI355X, the largest error / bound over all rows and updates (each row prints its
    own as "head-audit-worst"; a row takes 0.2-1.5 s, the 8-row one 3 s, the 481-, 1024- and 2017-row ones 4-5 s):
    trunk product where it is stored (B = 481 and 2017, F = 256: one pass over K = 39200, no split) 0.83 and 0.88 of
    3e-6, every componentwise ratio below 0.01: the thinnest margin of the audit, and the line expected to move first
    if that sum is reordered; trunk+LayerNorm+tanh where the product is left in records 0.06-0.30 of 2e-6; LayerNorm on the stored z 0.02, xhat 0.37, rstd 0.06; P1..P3, T1, T2, C1, C2, TQ, Q 0.05-0.14; MU_O
    0.34 of 2e-7, the next rows' draw 0.60 of 2e-7, the obs rows' draw exact; DC2 0.02, DC1 0.08, DHA / DA / DH_A /
    DPRE 0.03-0.05, DP2, DP1 0.07; weight gradients of the MLPs 0.09-0.18, bias gradients 0.03-0.18; both composites
    into the LayerNorm backward, DLN, DZ and the LayerNorm parameter gradients 0.01-0.02 of 1e-5; trunk weight /
    bias gradients 0.16 / 0.05; DY4 0.10, its border exactly zero; loss sums 0.03, td_abs 0.00; bf16 row: every MFMA
    product 4e-8..1.4e-7 against 1e-5; Adam, Polyak, copied columns, untouched buffers and phases == update(): 0
    elements differ.
    Three arithmetic mutations of a scratch copy of the library, run once each and not kept: the second dgrad
    problem's records skipped in ln_tanh_bwd_kernel missed at critic.DLN and critic.DZ (0.7-0.9 against 1e-5) in every
    row that leaves those records; the bias dropped on the records path of ln_tanh_fwd_kernel at HA_C, HA_C.xhat,
    HA_C.rstd, HROWS.obs, HROWS.next, HA_T and phase 1's HA_C2 (6e-2 against 2e-6) in every row whose rows are not
    fused; bc_scale A in drq_policy_out_bwd at policy.dW3, policy.db3 and DP2 of the b32 BC row, and nowhere else."""
    bad = []
    for rec, _, _, _, _ in audited(row):
        print("head-audit-worst %s %s" % (rec.tag, " ".join("%s=%.2f" % kv for kv in sorted(rec.worst.items()))))
        bad += [(rec.tag,) + b for b in rec.bad]
    assert not bad, bad


def test_the_comparison_rejects_a_dropped_bias_and_a_dropped_head():
    """positive control, host side only: the critic trunk's reference without its bias must miss the LayerNorm forward
    bound, and the composite into the LayerNorm backward with one head's records left out must miss 1e-5; nothing on the
    GPU is perturbed"""
    row = next(r for r in hv.AUDIT_ROWS if (r.B, r.A, r.mode) == (32, 6, "fp32"))
    _, snaps, x, sc, ag = audited(row)[0]
    b, B, F = snaps[1]["ws"], row.B, row.F
    cr = net_tensors(ag, snaps[0]["params"], "critic")
    w, bias, g, bt = (cr[k].double() for k in TRUNK)
    h, _, _, _ = ha.trunk_ln(b["FEAT"][:B].double(), w, torch.zeros_like(bias), g, bt)
    ctl = Rec(row, 0)
    ctl.norm(0, "control.no_bias", b["HA_C"][:, :F], h, LN_FWD)
    d = b["DC1"][0].double() @ cr["Q1.0.weight"][:, :F].double()
    dz, _ = ha.ln_tanh_bwd(d, b["HA_C"][:, :F].double(), b["XHAT_C"].double(), b["RSTD_C"].double(), g)
    ctl.norm(0, "control.one_head", b["DZ_C"], dz, LN_BWD)
    assert [s for _, s, _, _ in ctl.bad] == ["control.no_bias", "control.one_head"], ctl.bad


def test_the_comparison_rejects_a_bc_pull_scaled_by_one_over_b():
    """positive control, host side only: phase 1 of the BC row judged against a reference whose pull is 2 / B where
    2 / (B A) is right must miss at the three outputs of the fused policy output backward, and nowhere else"""
    row = next(r for r in hv.AUDIT_ROWS if (r.B, r.A, r.mode) == (32, 6, "bc"))
    _, snaps, x, sc, ag = audited(row)[0]
    ctl = Rec(row, 0)
    ctl.tag = "control " + ctl.tag
    audit_phase1(ctl, ag, row, snaps[1], snaps[2], x, sc, pull_factor=float(row.A))
    assert sorted(s for _, s, _, _ in ctl.bad) == ["DP2", "policy.dW3", "policy.db3"], ctl.bad
