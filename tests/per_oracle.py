"""float64 restatement of prioritized replay (a helper module: not collected).  Proportional prioritization is not in the
reference; the contract is the comment of include/drqv2_hip.h, stated here once more in numpy:

  tree      double [2L]: node 1 the root, children of k are 2k and 2k+1, the leaf of slot s is tree[L+s], every inner
            node exactly tree[2k] + tree[2k+1]; tree[0] the largest leaf a priority update ever wrote
  fill      leaves [lo, hi) <- 0 or tree[0], ancestors recomputed
  descend   row i aims at (i + u_i) / B * tree[1]; at node k: left if (m < left and left > 0) or right == 0, else
            m -= left and right
  weights   (n_valid leaf / tree[1])^-beta, divided by the batch's largest
  update    leaf[pos_i] <- (td_i + eps)^alpha, the highest row of a repeated position wins; ancestors; tree[0] <- max

and the critic step with the weighted loss (PEROracleAgent): OracleAgent.update's statements, composed from the public
functions of oracle/drq_oracle.py, with  critic_loss = mean_i w_i (Q1 - y)_i^2 + mean_i w_i (Q2 - y)_i^2.
"""
from collections import OrderedDict

import numpy as np
import torch

from oracle import drq_oracle as O


# ------------------------------------------------------------------------------------------------ the tree
def leaves_of(capacity):
    L = 1
    while L < capacity:
        L *= 2
    return L


def new_tree(capacity):
    t = np.zeros(2 * leaves_of(capacity), np.float64)
    t[0] = 1.0
    return t


def rebuild(tree, nodes):
    """recompute the ancestors of the given leaf NODES (indices into tree), level by level"""
    nodes = np.unique(np.asarray(nodes, np.int64))
    while nodes.size and nodes[0] > 1:
        nodes = np.unique(nodes >> 1)
        tree[nodes] = tree[2 * nodes] + tree[2 * nodes + 1]


def build(leaves):
    """the tree of a full list of leaf values (length a power of two)"""
    leaves = np.asarray(leaves, np.float64)
    L = leaves.size
    t = np.zeros(2 * L, np.float64)
    t[0] = 1.0
    t[L:] = leaves
    n = L // 2
    while n >= 1:
        t[n:2 * n] = t[2 * n:4 * n:2] + t[2 * n + 1:4 * n:2]
        n //= 2
    return t


def fill(tree, lo, hi, mode):
    L = tree.size // 2
    if lo == hi:
        return
    tree[L + lo:L + hi] = tree[0] if mode else 0.0
    rebuild(tree, np.arange(L + lo, L + hi))


def descend(tree, u):
    """positions (slots) of the B stratified draws u"""
    L = tree.size // 2
    B = len(u)
    out = np.empty(B, np.int64)
    for i in range(B):
        m = (i + np.float64(u[i])) / B * tree[1]
        k = 1
        while k < L:
            left, right = tree[2 * k], tree[2 * k + 1]
            if (m < left and left > 0) or right == 0:
                k = 2 * k
            else:
                m -= left
                k = 2 * k + 1
        out[i] = k - L
    return out


def weights(tree, pos, n_valid, beta):
    L = tree.size // 2
    w = (n_valid * tree[L + np.asarray(pos)] / tree[1]) ** (-np.float64(beta))
    return w / w.max()


def update(tree, pos, td_abs, alpha, eps):
    """td_abs float32; rows in order, so the highest row of a repeated position is the one that stays"""
    L = tree.size // 2
    v = np.power(np.asarray(td_abs, np.float32).astype(np.float64) + eps, alpha)
    written = {}
    for p, x in zip(np.asarray(pos).tolist(), v.tolist()):
        written[p] = x
    for p, x in written.items():
        tree[L + p] = x
    rebuild(tree, L + np.array(list(written), np.int64))
    tree[0] = max(tree[0], max(written.values()))
    return written


def drawable(episodes, nstep):
    """the slots DeviceReplay.draw_positions can return for a list of [start, steps]"""
    s = set()
    for start, n in episodes:
        if n - 1 >= nstep:
            s.update(range(start + 1, start + n - nstep + 1))
    return s


# ------------------------------------------------------------------------------------------------ the weighted update
def weighted_td(q1, q2, target_q, w):
    """(critic_loss, td_abs) of the definition; q1, q2, target_q [B,1], w [B]"""
    w = w.reshape(-1, 1)
    loss = (w * (q1 - target_q) ** 2).mean() + (w * (q2 - target_q) ** 2).mean()
    td = 0.5 * ((q1 - target_q).abs() + (q2 - target_q).abs())
    return loss, td.detach().reshape(-1)


def closed_form_dq(q1, q2, target_q, w, B_global=None):
    """what the kernels implement: dq_k[i] = 2 w_i (Q_k,i - y_i) / B_global"""
    Bg = q1.shape[0] if B_global is None else B_global
    w = w.reshape(-1, 1)
    return 2.0 * w * (q1 - target_q) / Bg, 2.0 * w * (q2 - target_q) / Bg


class PEROracleAgent(O.OracleAgent):
    """OracleAgent whose critic loss carries a weight per sample.  update() takes `weights` ([B], None = all ones) and
    restates OracleAgent.update statement by statement with that one change; the actor step and the target update are
    the plain ones.  self.last always holds what keep=True leaves, plus td_abs and the loss gradients dq1 / dq2."""

    def update(self, batch, step, shifts_obs, shifts_next, noise_critic, noise_actor, weights=None, aug_base=None,
               aug_override=None, enc_in_override=None, keep=True, relu_masks=None, critic_relu_masks=None):
        if step % self.update_every_steps != 0:
            return {}
        dt = self.dtype
        obs_u8, action, reward, discount, next_u8 = batch
        action, reward, discount = action.to(dt), reward.to(dt), discount.to(dt)
        noise_critic, noise_actor = noise_critic.to(dt), noise_actor.to(dt)
        w = torch.ones(obs_u8.shape[0], dtype=dt) if weights is None else weights.to(dt)
        std = O.schedule(self.stddev_schedule, step)
        clip = self.stddev_clip
        metrics = {}

        normalized = enc_in_override is not None
        if normalized:
            obs_a, next_a = (t.to(dt) for t in enc_in_override)
        elif aug_override is not None:
            obs_a, next_a = (t.to(dt) for t in aug_override)
        else:
            base = None if aug_base is None else aug_base.to(dt)
            obs_a = O.random_shifts_aug(obs_u8.to(dt), shifts_obs, 4, base)
            next_a = O.random_shifts_aug(next_u8.to(dt), shifts_next, 4, base)

        req = lambda d: OrderedDict((k, v.detach().requires_grad_(True)) for k, v in d.items())
        enc, critic = req(self.enc), req(self.critic)
        feat, acts = O.encoder_forward(enc, obs_a, return_acts=True, normalized=normalized, relu_masks=relu_masks)
        with torch.no_grad():
            feat_next = O.encoder_forward(self.enc, next_a, normalized=normalized)
        metrics["batch_reward"] = reward.mean().item()

        # ---- critic step with the weighted loss
        with torch.no_grad():
            mu_n = O.actor_mu(self.actor, feat_next)
            a_next = O.trunc_normal_sample(mu_n, noise_critic, std, clip)
            tq1, tq2 = O.critic_q(self.critic_target, feat_next, a_next)
            target_q = reward + discount * torch.minimum(tq1, tq2)
        crit_rec = {"Q1": [], "Q2": []}
        q1, q2 = O.critic_q(critic, feat, action, critic_relu_masks, crit_rec)
        critic_loss, td_abs = weighted_td(q1, q2, target_q, w)
        metrics["critic_target_q"] = target_q.mean().item()
        metrics["critic_q1"] = q1.mean().item()
        metrics["critic_q2"] = q2.mean().item()
        metrics["critic_loss"] = critic_loss.item()
        gl = torch.autograd.grad(critic_loss, list(enc.values()) + list(critic.values()) + [q1, q2])
        g_enc = OrderedDict(zip(list(enc), gl[:len(enc)]))
        g_critic = OrderedDict(zip(list(critic), gl[len(enc):len(enc) + len(critic)]))
        self._adam("critic", self.critic, g_critic)
        self._adam("enc", self.enc, g_enc)

        # ---- actor step (unweighted)
        featd = feat.detach()
        actor = req(self.actor)
        mu = O.actor_mu(actor, featd)
        a = O.trunc_normal_sample(mu, noise_actor, std, clip)
        logp = O.normal_log_prob(a, mu, std).sum(-1, keepdim=True)
        aq1, aq2 = O.critic_q(self.critic, featd, a)
        actor_loss = -torch.minimum(aq1, aq2).mean()
        ga = torch.autograd.grad(actor_loss, list(actor.values()))
        g_actor = OrderedDict(zip(list(actor), ga))
        self._adam("actor", self.actor, g_actor)
        metrics["actor_loss"] = actor_loss.item()
        metrics["actor_logprob"] = logp.mean().item()
        metrics["actor_ent"] = float(O.normal_entropy(std) * a.shape[-1])

        for k in self.critic:
            O.polyak(self.critic[k], self.critic_target[k], self.tau)

        self.last = dict(obs_a=obs_a, next_a=next_a, feat=featd, feat_next=feat_next, acts=[t.detach() for t in acts],
                         mu_next=mu_n, a_next=a_next, target_q=target_q, q1=q1.detach(), q2=q2.detach(), g_enc=g_enc,
                         g_critic=g_critic, g_actor=g_actor, mu=mu.detach(), a=a.detach(), aq1=aq1.detach(),
                         aq2=aq2.detach(), critic_pre=crit_rec, td_abs=td_abs, dq1=gl[-2], dq2=gl[-1], weights=w)
        return metrics
