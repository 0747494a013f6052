"""fp32 / fp64 restatement of the DrQ+BC actor step (a helper module: not collected), composed from the public functions
of oracle/drq_oracle.py.  DrQ+BC is not in the reference; the definitions of DrQV2Agent.set_behavior_cloning are the
contract and this file states them once more in plain torch, with autograd doing the differentiation:

    a      = TruncatedNormal(mu, std).sample(clip)          fourth draw, gradient straight through to mu
    Qmin_i = min(Q1, Q2)(feat_i.detach(), a_i)              through the already stepped critic
    lambda = alpha / mean_i |Qmin_i|                        detached, no epsilon
    bc     = mean over all B*A elements of (a - a_beh)^2
    loss   = -lambda * mean_i Qmin_i + bc

bc_actor_step() evaluates that; closed_form() gives the gradients the kernels implement (dq into the critic heads, dmu
into the policy output) for comparison with autograd; BCOracleAgent runs OracleAgent.update for the critic side and
replaces its actor step.
"""
from collections import OrderedDict

import torch

from oracle import drq_oracle as O


def bc_actor_step(actor, critic, feat, a_beh, noise, std, clip, alpha):
    """actor / critic: parameter dicts (the critic already stepped), feat [B, 39200] detached, all of one dtype.
    Returns a dict: loss, lam, bc (0-d tensors), g_actor (OrderedDict), and the intermediates mu, a, q1, q2 with the
    autograd gradients of the loss with respect to them (dmu is the TOTAL gradient into mu, through the critic and the
    BC term)."""
    req = OrderedDict((k, v.detach().requires_grad_(True)) for k, v in actor.items())
    mu = O.actor_mu(req, feat)
    a = O.trunc_normal_sample(mu, noise, std, clip)
    q1, q2 = O.critic_q(critic, feat, a)
    qmin = torch.minimum(q1, q2)
    lam = (alpha / qmin.abs().mean()).detach()
    bc = ((a - a_beh) ** 2).mean()
    loss = -lam * qmin.mean() + bc
    grads = torch.autograd.grad(loss, list(req.values()) + [mu, q1, q2])
    n = len(req)
    return dict(loss=loss.detach(), lam=lam, bc=bc.detach(), g_actor=OrderedDict(zip(req, grads[:n])),
                mu=mu.detach(), a=a.detach(), q1=q1.detach(), q2=q2.detach(), qmin=qmin.detach(),
                logp=O.normal_log_prob(a, mu, std).sum(-1, keepdim=True).detach(),
                dmu=grads[n], dq1=grads[n + 1], dq2=grads[n + 2])


def closed_form(critic, feat, a, a_beh, q1, q2, alpha, B_global=None):
    """The formulas the kernels implement.  dq_k[i] = -lambda / B_global on the head that holds the minimum (a tie
    gives each head half); dmu = da_1 + da_2 + 2 (a - a_beh) / (B_global A), da_k the gradient that dq_k sends back
    through head k to the action."""
    B, A = a.shape
    Bg = B if B_global is None else B_global
    qmin = torch.minimum(q1, q2)
    lam = alpha / qmin.abs().mean()
    g = -lam / Bg
    zero = torch.zeros_like(q1)
    dq1 = torch.where(q1 < q2, g, torch.where(q1 == q2, 0.5 * g, zero))
    dq2 = torch.where(q2 < q1, g, torch.where(q1 == q2, 0.5 * g, zero))
    ar = a.detach().requires_grad_(True)
    r1, r2 = O.critic_q(critic, feat, ar)
    da = torch.autograd.grad([r1, r2], ar, [dq1, dq2])[0]          # da_1 + da_2
    dmu = da + 2.0 * (a - a_beh) / (Bg * A)
    return dict(lam=lam, dq1=dq1, dq2=dq2, dmu=dmu)


class BCOracleAgent(O.OracleAgent):
    """OracleAgent whose actor step minimises the DrQ+BC loss.  The critic side is OracleAgent.update's, untouched: that
    call runs first (keep=True), then the actor -- parameters, Adam moments and step count as they were BEFORE the call --
    is stepped again with the BC gradients through the critic that call stepped."""

    def __init__(self, *args, alpha, **kw):
        super().__init__(*args, **kw)
        self.alpha = float(alpha)

    def update(self, batch, step, shifts_obs, shifts_next, noise_critic, noise_actor, **kw):
        clone = lambda d: OrderedDict((k, v.clone()) for k, v in d.items())
        before = clone(self.actor), clone(self.m["actor"]), clone(self.v["actor"]), self.t["actor"]
        kw["keep"] = True
        metrics = super().update(batch, step, shifts_obs, shifts_next, noise_critic, noise_actor, **kw)
        if not metrics:
            return metrics
        self.actor, self.m["actor"], self.v["actor"], self.t["actor"] = before
        dt = self.dtype
        std = O.schedule(self.stddev_schedule, step)
        r = bc_actor_step(self.actor, self.critic, self.last["feat"], batch[1].to(dt), noise_actor.to(dt), std,
                          self.stddev_clip, self.alpha)
        self._adam("actor", self.actor, r["g_actor"])
        metrics["actor_loss"] = r["loss"].item()
        metrics["actor_logprob"] = r["logp"].mean().item()
        metrics["actor_bc_loss"] = r["bc"].item()
        metrics["actor_bc_lambda"] = r["lam"].item()
        self.last.update(g_actor=r["g_actor"], mu=r["mu"], a=r["a"], aq1=r["q1"], aq2=r["q2"], bc=r)
        return metrics
