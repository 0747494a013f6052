"""Same-process comparison at cheetah_run, batch 256 (A=6, feature_dim=50, hidden_dim=1024): the reference's update
algorithm written with autograd over the agent's modules (drqv2_amd/autograd.py; opt.zero_grad / loss.backward /
opt.step on the arenas) against the fused DrQV2Agent.update().  Both read the same GPU-resident batch; every update
is followed by a device synchronisation and timed on the host clock; the median over --updates updates is reported.
Also times the conv1 input-gradient kernel (drq_conv1_dgrad) at batch 256 against its HBM estimate.

  python tools/autograd_bench.py [--updates 300] [--warmup 20] [--only autograd|fused]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2  # noqa: E402
import utils  # noqa: E402
from drqv2_amd import ops, synth  # noqa: E402


def autograd_update(ag, batch, step):
    """drqv2.py:177-262 of the reference (metrics left on the device: no .item() waits)."""
    obs, action, reward, discount, next_obs = batch
    obs = ag.aug(obs.float())
    next_obs = ag.aug(next_obs.float())
    obs = ag.encoder(obs)
    with torch.no_grad():
        next_obs = ag.encoder(next_obs)
    std = utils.schedule(ag.stddev_schedule, step)
    with torch.no_grad():
        next_action = ag.actor(next_obs, std).sample(clip=ag.stddev_clip)
        tq1, tq2 = ag.critic_target(next_obs, next_action)
        target_q = reward + discount * torch.min(tq1, tq2)
    q1, q2 = ag.critic(obs, action)
    critic_loss = F.mse_loss(q1, target_q) + F.mse_loss(q2, target_q)
    ag.encoder_opt.zero_grad(set_to_none=True)
    ag.critic_opt.zero_grad(set_to_none=True)
    critic_loss.backward()
    ag.critic_opt.step()
    ag.encoder_opt.step()
    obs = obs.detach()
    dist = ag.actor(obs, std)
    a = dist.sample(clip=ag.stddev_clip)
    aq1, aq2 = ag.critic(obs, a)
    actor_loss = -torch.min(aq1, aq2).mean()
    ag.actor_opt.zero_grad(set_to_none=True)
    actor_loss.backward()
    ag.actor_opt.step()
    utils.soft_update_params(ag.critic, ag.critic_target, ag.critic_target_tau)


def timed(fn, n, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(n):
        t0 = time.perf_counter()
        fn(warmup + i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def conv1_dgrad_us(B, reps=200):
    g = torch.Generator(device="cuda").manual_seed(0)
    dy = ops.relu_mask_pad(torch.randn((B, 32, 41, 41), device="cuda", generator=g), None)
    w = torch.randn((32, 9, 3, 3), device="cuda", generator=g)
    for _ in range(10):
        ops.conv1_dgrad(dy, w)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for i in range(reps):
        ev[2 * i].record()
        ops.conv1_dgrad(dy, w)
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    us = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) * 1e3 for i in range(reps))
    return us[reps // 2], us[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", choices=("autograd", "fused"), default=None)
    args = ap.parse_args()
    B, A, Fd, H = 256, 6, 50, 1024
    torch.manual_seed(0)
    ag = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-4, Fd, H, 0.01, 2000, 1, "linear(1.0,0.1,500000)", 0.3, False)
    enc, actor, critic = synth.make_weights(9, A, Fd, H, 0)
    ag.encoder.load_state_dict(enc)
    ag.actor.load_state_dict(actor)
    ag.critic.load_state_dict(critic)
    ag.critic_target.load_state_dict(critic)
    batch = tuple(t.cuda() for t in synth.make_batch(B, A, 9, seed=0))
    res = {}
    if args.only in (None, "autograd"):
        res["autograd"] = timed(lambda i: autograd_update(ag, batch, i), args.updates, args.warmup)
    if args.only in (None, "fused"):
        res["fused"] = timed(lambda i: ag.update(iter([batch]), i), args.updates, args.warmup)
    for k, (med, lo, hi) in res.items():
        print(f"{k:9s} update: {med:7.3f} ms median  (min {lo:.3f}, max {hi:.3f}) over {args.updates} updates, B={B}",
              flush=True)
    if len(res) == 2:
        print(f"autograd / fused: {res['autograd'][0] / res['fused'][0]:.2f}x", flush=True)
    if args.only is None:
        med, lo = conv1_dgrad_us(B)
        # dy [B,32,41,41] read (the padded buffer's interior) + dx [B,9,84,84] written, fp32, at 6.3 TB/s
        est = (B * 32 * 41 * 41 + B * 9 * 84 * 84) * 4 / 6.3e12 * 1e6
        print(f"drq_conv1_dgrad B={B}: {med:.1f} us median (min {lo:.1f}); HBM estimate {est:.1f} us", flush=True)


if __name__ == "__main__":
    main()
