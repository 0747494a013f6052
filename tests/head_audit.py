"""fp64 references of the head section's stages, one plain function per launch (or per pair of launches whose hand-over
stays in the GEMM workspace), shared by tests/test_hip_head_audit.py, which holds every launch of update() to them on
the operands the launch read, and tests/test_cpu_head_audit.py, which chains them into a whole update on the CPU and
holds that to oracle.drq_oracle.OracleAgent and to autograd: the formulas are known to compose to the reference update
before they judge a kernel.  A helper module: not collected, needs no GPU.  Every function takes and returns tensors of
one dtype on one device; nothing here knows about the workspace."""
import math
from collections import OrderedDict

import torch

from oracle import drq_oracle as O

R = 32 * 35 * 35


# ------------------------------------------------------------------------------------------------ forward stages
def trunk_ln(feat, w, b, gamma, beta):
    """Linear(39200 -> F) + LayerNorm + tanh (drqv2.py:74-75): (h, xhat, rstd, z)"""
    z = feat @ w.t() + b
    return ln_tanh(z, gamma, beta) + (z,)


def ln_tanh(z, gamma, beta):
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + O.LN_EPS)
    xhat = (z - mean) * rstd
    return torch.tanh(xhat * gamma + beta), xhat, rstd.reshape(-1)


def linear(x, w, b=None, relu=False):
    y = x @ w.t()
    if b is not None:
        y = y + b
    return torch.relu(y) if relu else y


def td_loss(tq, q, reward, discount, B_global, weights=None):
    """drqv2.py:185-189 with an optional weight per row (include/drqv2_hip.h, drq_td_mse_w).  tq, q [2][B];
    returns y [B], dq [2][B], sums [5] (sum r, sum y, sum q1, sum q2, sum w ((q1-y)^2 + (q2-y)^2)), td_abs [B]"""
    y = reward + discount * torch.minimum(tq[0], tq[1])
    e = q - y
    w = torch.ones_like(y) if weights is None else weights
    dq = 2.0 * e / B_global * w
    sums = torch.stack([reward.sum(), y.sum(), q[0].sum(), q[1].sum(), (w * (e[0] ** 2 + e[1] ** 2)).sum()])
    return y, dq, sums, 0.5 * (e[0].abs() + e[1].abs())


def actor_loss(q, a, mu, std, B_global, a_beh=None, alpha=None):
    """drqv2.py:212-216, or the DrQ+BC loss with alpha: dq [2][B] = -lambda / B_global on the head that holds the
    minimum (a tie gives each head half), lambda = alpha / mean |Qmin| (1 without BC);
    s5 = sum -Qmin, s6 = sum log N(a | mu, std), s9 = sum (a - a_beh)^2, s10 = sum |Qmin| (BC only, else None)"""
    qmin = torch.minimum(q[0], q[1])
    lam = 1.0 if alpha is None else alpha / (qmin.abs().sum() / q.shape[1])
    g = -lam / B_global
    one, half, zero = torch.ones_like(qmin), torch.full_like(qmin, 0.5), torch.zeros_like(qmin)
    share = torch.stack([torch.where(q[0] < q[1], one, torch.where(q[0] == q[1], half, zero)),
                         torch.where(q[1] < q[0], one, torch.where(q[0] == q[1], half, zero))])
    logp = -((a - mu) ** 2) / (2 * std * std) - math.log(std) - math.log(math.sqrt(2 * math.pi))
    s9 = None if alpha is None else ((a - a_beh) ** 2).sum()
    s10 = None if alpha is None else qmin.abs().sum()
    return share * g, (-qmin).sum(), logp.sum(), s9, s10, lam


# ------------------------------------------------------------------------------------------------ backward stages
def qout_bwd(dq, h2, w2):
    """Linear(H, 1) backward for one head: dh2 = (dq w2) * (h2 > 0), dw [1][H], db [1]"""
    return dq[:, None] * w2.reshape(1, -1) * (h2 > 0).to(dq.dtype), (dq @ h2).reshape(1, -1), dq.sum().reshape(1)


def dgrad(dy, w, mask=None):
    dx = dy @ w
    return dx if mask is None else dx * (mask > 0).to(dx.dtype)


def wgrad(dy, x):
    return dy.t() @ x, dy.sum(0)


def ln_tanh_bwd(d, h, xhat, rstd, gamma):
    """gradient d of tanh(LN(z))'s output -> (dz, dln): dln the gradient of LayerNorm's output"""
    dln = d * (1.0 - h * h)
    dxh = dln * gamma
    m1 = dxh.mean(-1, keepdim=True)
    m2 = (dxh * xhat).mean(-1, keepdim=True)
    return rstd.reshape(-1, 1) * (dxh - m1 - xhat * m2), dln


def ln_param_grads(dln, xhat):
    return (dln * xhat).sum(0), dln.sum(0)


def dpre_of(da, mu, a=None, a_beh=None, bc_scale=0.0):
    """d(policy output before the tanh) = (da_1 + da_2 [+ bc_scale (a - a_beh)]) (1 - mu^2): the clamp of the sample is
    straight-through (utils.py:112-115)"""
    dmu = da if a_beh is None else da + bc_scale * (a - a_beh)
    return dmu * (1.0 - mu * mu)


# ------------------------------------------------------------------------------------------------ the chain
def mlp_forward(p, prefix, x):
    h1 = linear(x, p[prefix + ".0.weight"], p[prefix + ".0.bias"], True)
    h2 = linear(h1, p[prefix + ".2.weight"], p[prefix + ".2.bias"], True)
    return h1, h2, linear(h2, p[prefix + ".4.weight"], p[prefix + ".4.bias"])


def mlp_backward(p, prefix, x, h1, h2, dout, need_w=True):
    """backward of mlp_forward from dout [rows][out]: (gradient dict, dx)"""
    g = OrderedDict()
    if dout.shape[1] == 1:
        d2, g[prefix + ".4.weight"], g[prefix + ".4.bias"] = qout_bwd(dout[:, 0], h2, p[prefix + ".4.weight"])
    else:
        g[prefix + ".4.weight"], g[prefix + ".4.bias"] = wgrad(dout, h2)
        d2 = dgrad(dout, p[prefix + ".4.weight"], h2)
    g[prefix + ".2.weight"], g[prefix + ".2.bias"] = wgrad(d2, h1)
    d1 = dgrad(d2, p[prefix + ".2.weight"], h1)
    g[prefix + ".0.weight"], g[prefix + ".0.bias"] = wgrad(d1, x)
    dx = dgrad(d1, p[prefix + ".0.weight"])
    order = [prefix + ".%d.%s" % (i, k) for i in (0, 2, 4) for k in ("weight", "bias")]
    return OrderedDict((k, g[k]) for k in order), dx


def trunk_backward(p, feat, h, xhat, rstd, d):
    dz, dln = ln_tanh_bwd(d, h, xhat, rstd, p["trunk.1.weight"])
    g = OrderedDict()
    g["trunk.0.weight"], g["trunk.0.bias"] = wgrad(dz, feat)
    g["trunk.1.weight"], g["trunk.1.bias"] = ln_param_grads(dln, xhat)
    return g, dgrad(dz, p["trunk.0.weight"], feat)      # d feat, masked by the ReLU of conv4


def head_update(actor, critic, target, feat, feat_next, action, reward, discount, noise_c, noise_a, std, clip, lr, tau,
                steps=(1, 1), alpha=None, weights=None, moments=None):
    """The head half of one update composed from the stages above, in update()'s order.  actor / critic / target:
    parameter dicts (the reference's state_dict keys), changed in place like OracleAgent's; feat / feat_next [B][39200];
    reward, discount [B]; steps = (critic, actor) Adam step counts; moments: {"critic": (m, v), "actor": (m, v)} dicts
    of dicts, zeros when None.  Returns g_critic, g_actor, dfeat (the critic loss's gradient of feat), sums (dict by
    slot) and td_abs."""
    B = feat.shape[0]
    cat = lambda h, a: torch.cat([h, a], -1)
    # ---- phase 4
    hc, xc, rc, _ = trunk_ln(feat, *(critic["trunk.%s" % k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")))
    ha, xa, ra, _ = trunk_ln(feat, *(actor["trunk.%s" % k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")))
    hn, _, _, _ = trunk_ln(feat_next, *(actor["trunk.%s" % k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")))
    ht, _, _, _ = trunk_ln(feat_next, *(target["trunk.%s" % k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")))
    p1, p2, p3 = mlp_forward(actor, "policy", torch.cat([ha, hn]))
    mu, mu_next = torch.tanh(p3[:B]), torch.tanh(p3[B:])
    a = O.trunc_normal_sample(mu, noise_a, std, clip).detach()
    a_next = O.trunc_normal_sample(mu_next, noise_c, std, clip).detach()
    tq = torch.stack([mlp_forward(target, q, cat(ht, a_next))[2][:, 0] for q in ("Q1", "Q2")])
    fw = {q: mlp_forward(critic, q, cat(hc, action)) for q in ("Q1", "Q2")}
    q = torch.stack([fw[k][2][:, 0] for k in ("Q1", "Q2")])
    _, dq, s04, td_abs = td_loss(tq, q, reward, discount, B, weights)
    g_critic, dha = OrderedDict(), 0
    for i, k in enumerate(("Q1", "Q2")):
        g, dx = mlp_backward(critic, k, cat(hc, action), fw[k][0], fw[k][1], dq[i][:, None])
        g_critic.update(g)
        dha = dha + dx
    gt, dfeat = trunk_backward(critic, feat, hc, xc, rc, dha[:, :hc.shape[1]])
    g_critic = OrderedDict(list(gt.items()) + list(g_critic.items()))
    # ---- phase 6: critic_opt.step(), Polyak, the actor loss through the stepped critic
    zeros = lambda d: OrderedDict((k, torch.zeros_like(v)) for k, v in d.items())
    mom = moments or {"critic": (zeros(critic), zeros(critic)), "actor": (zeros(actor), zeros(actor))}
    for k in critic:
        O.adam_step(critic[k], g_critic[k], mom["critic"][0][k], mom["critic"][1][k], steps[0], lr)
        O.polyak(critic[k], target[k], tau)
    hc2, _, _, _ = trunk_ln(feat, *(critic["trunk.%s" % k] for k in ("0.weight", "0.bias", "1.weight", "1.bias")))
    fw = {k: mlp_forward(critic, k, cat(hc2, a)) for k in ("Q1", "Q2")}
    aq = torch.stack([fw[k][2][:, 0] for k in ("Q1", "Q2")])
    dq, s5, s6, s9, s10, lam = actor_loss(aq, a, mu, std, B, action if alpha is not None else None, alpha)
    # ---- phase 7
    F = hc.shape[1]
    da = sum(mlp_backward(critic, k, cat(hc2, a), fw[k][0], fw[k][1], dq[i][:, None])[1][:, F:]
             for i, k in enumerate(("Q1", "Q2")))
    dpre = dpre_of(da, mu, a, action if alpha is not None else None, 2.0 / (B * a.shape[1]))
    g_pol, dh = mlp_backward(actor, "policy", ha, p1[:B], p2[:B], dpre)
    gt, _ = trunk_backward(actor, feat, ha, xa, ra, dh)
    g_actor = OrderedDict(list(gt.items()) + list(g_pol.items()))
    for k in actor:
        O.adam_step(actor[k], g_actor[k], mom["actor"][0][k], mom["actor"][1][k], steps[1], lr)
    sums = {0: s04[0], 1: s04[1], 2: s04[2], 3: s04[3], 4: s04[4], 5: s5, 6: s6, 9: s9, 10: s10}
    return dict(g_critic=g_critic, g_actor=g_actor, dfeat=dfeat, sums=sums, td_abs=td_abs, lam=lam, a=a, mu=mu)
