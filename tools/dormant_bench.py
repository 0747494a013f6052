"""Times DrQV2Agent.dormant_ratio() and DrQV2Agent.perturb() against one DrQV2Agent.update() in the same process.

  python tools/dormant_bench.py [--batch 256] [--action-dim 6] [--feature-dim 50] [--hidden-dim 1024] [--rounds 20]
                                [--out profiles/dormant_bench.txt]

The three calls are run in interleaved rounds (update, dormant_ratio on the actor, dormant_ratio on actor + critic, perturb)
and timed with device events around each call; perturb() also builds fresh weights on the host, so its wall time (host
clock, device drained before and after) is reported beside the device time of its launches.  Median and minimum over the
rounds, on synthetic frames (drqv2_amd.synth).  There is no target: the numbers say what the two calls cost next to the
update they accompany every few thousand steps."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2  # noqa: E402
from drqv2_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--action-dim", type=int, default=6)
    ap.add_argument("--feature-dim", type=int, default=50)
    ap.add_argument("--hidden-dim", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dormant_bench.py runs on the GPU: no device found")
    B, A = args.batch, args.action_dim
    torch.manual_seed(0)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-4, args.feature_dim, args.hidden_dim, 0.01, 2000, 2,
                             "linear(1.0,0.1,500000)", 0.3, False)
    agent.metrics_on_device = True
    batch = tuple(t.cuda() for t in synth.make_batch(B, A, 9, seed=0, smooth=False))
    obs, action = batch[0], batch[1]

    def update():
        agent.update(iter([batch]), 10000)

    calls = {"update()": update,
             "dormant_ratio(actor)": lambda: agent.dormant_ratio(obs),
             "dormant_ratio(actor, critic)": lambda: agent.dormant_ratio(obs, action, nets=("actor", "critic")),
             "perturb(0.9)": lambda: agent.perturb(0.9)}
    dev_us = {k: [] for k in calls}
    wall_us = {k: [] for k in calls}
    for r in range(args.warmup + args.rounds):
        for name, fn in calls.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if r >= args.warmup:
                dev_us[name].append(e0.elapsed_time(e1) * 1e3)
                wall_us[name].append((t1 - t0) * 1e6)
    lines = [f"dormant_bench: batch {B}, action_dim {A}, feature_dim {args.feature_dim}, hidden_dim {args.hidden_dim}, "
             f"{args.rounds} interleaved rounds after {args.warmup}; {torch.cuda.get_device_name(0)}",
             "device us = between two events around the call (includes host gaps between its launches); wall us = host "
             "clock around the call with the device drained before and after",
             f"{'call':32s} {'device us median':>17s} {'min':>9s} {'wall us median':>15s} {'min':>9s}"]
    for name in calls:
        d, w = dev_us[name], wall_us[name]
        lines.append(f"{name:32s} {statistics.median(d):17.1f} {min(d):9.1f} {statistics.median(w):15.1f} {min(w):9.1f}")
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
