"""DrQ+BC at cheetah_run, batch 256 (A=6, feature_dim=50, hidden_dim=1024), one process, one agent, the three paths
alternated inside every repeat after a warm-up of each (as tools/act_bench.py does):

  plain      DrQV2Agent.update()                                   the yardstick
  bc         the same after set_behavior_cloning(alpha)            the fused BC update
  autograd   the BC update written through the differentiable modules (tools/autograd_bench.py's loop with the BC
             actor loss): what an offline user had to write before

Two figures per path: device-event time = median over the updates of an event pair around ONE update; host wall = a
perf_counter window over all updates of a repeat that ends in a synchronise, per update.  --repeats repeats; min / median
/ max of the repeats are printed.  All three read the same GPU-resident batch; metrics are off (use_tb=False).

  python tools/bc_bench.py [--updates 200] [--repeats 5] [--alpha 2.5]
  python tools/bc_bench.py --only plain|bc --updates 50      one path alone, for a kernel trace:
      rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bc_bench.py --only bc --updates 50
  (the per-kernel call counts of the two traces, divided by warm-up + updates, are the launches per update)
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2  # noqa: E402
import utils  # noqa: E402
from drqv2_amd import synth  # noqa: E402


def autograd_bc_update(ag, batch, step, alpha):
    """tools/autograd_bench.py's update with the DrQ+BC actor loss (DrQV2Agent.set_behavior_cloning's definitions)."""
    obs, action, reward, discount, next_obs = batch
    obs = ag.encoder(ag.aug(obs.float()))
    with torch.no_grad():
        next_obs = ag.encoder(ag.aug(next_obs.float()))
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
    a = ag.actor(obs, std).sample(clip=ag.stddev_clip)
    qmin = torch.min(*ag.critic(obs, a))
    lam = alpha / qmin.abs().mean().detach()
    actor_loss = -lam * qmin.mean() + F.mse_loss(a, action)
    ag.actor_opt.zero_grad(set_to_none=True)
    actor_loss.backward()
    ag.actor_opt.step()
    utils.soft_update_params(ag.critic, ag.critic_target, ag.critic_target_tau)


def measure(fn, n, step0):
    """(median device-event us of one update, host wall us per update) over n updates."""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, (e0, e1) in enumerate(pairs):
        e0.record()
        fn(step0 + i)
        e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / n
    dev = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)[n // 2]
    return 1e3 * dev, 1e6 * wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=2.5)
    ap.add_argument("--only", choices=("plain", "bc"), default=None)
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

    def fused(alpha):
        def run(i):
            ag.set_behavior_cloning(alpha)
            ag.update(iter([batch]), i)
        return run

    paths = {"plain": fused(None), "bc": fused(args.alpha),
             "autograd": lambda i: (ag.set_behavior_cloning(None), autograd_bc_update(ag, batch, i, args.alpha))}
    if args.only:
        paths = {args.only: paths[args.only]}
    step = 0
    for fn in paths.values():
        for _ in range(args.warmup):
            fn(step)
            step += 1
    torch.cuda.synchronize()
    if args.only:
        for _ in range(args.updates):
            paths[args.only](step)
            step += 1
        torch.cuda.synchronize()
        print(f"{args.only}: {args.warmup + args.updates} updates issued (B={B})", flush=True)
        return
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():                # alternate the paths inside every repeat
            res[k].append(measure(fn, args.updates, step))
            step += args.updates
    mid = args.repeats // 2
    print(f"cheetah_run B={B}, alpha={args.alpha}, {args.repeats} repeats of {args.updates} updates per path, alternated",
          flush=True)
    for k, v in res.items():
        d, w = sorted(x[0] for x in v), sorted(x[1] for x in v)
        print(f"{k:9s} update: device-event {d[mid]:8.1f} us [{d[0]:.1f} .. {d[-1]:.1f}]   "
              f"host wall {w[mid]:8.1f} us [{w[0]:.1f} .. {w[-1]:.1f}]", flush=True)
    med = {k: sorted(x[1] for x in v)[mid] for k, v in res.items()}
    print(f"bc / plain (host wall): {med['bc'] / med['plain']:.4f}   autograd / bc: {med['autograd'] / med['bc']:.2f}x",
          flush=True)


if __name__ == "__main__":
    main()
