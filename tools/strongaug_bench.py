"""Device time of the strong augmentations (drqv2_amd.augment: drq_aug_overlay, drq_aug_random_conv) beside the copy floor.

  python tools/strongaug_bench.py [--batch 256] [--channels 9] [--launches 200] [--rounds 5]

One process: per round the three paths in turn -- obs.clone() (one read and one write of the same bytes: the floor of a
kernel that reads and writes the batch once), the overlay entry and the convolution entry, both raw through the library
with fixed indices / weights, so that no host work of the classes and no generator draw is in the figure -- each as
`launches` launches back to back between two device events after a warm-up.  Prints microseconds per launch, the median
over the rounds [smallest .. largest], and the bytes each moves."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drqv2_amd import _lib  # noqa: E402
from drqv2_amd._lib import launch, ptr  # noqa: E402
from drqv2_amd.augment import noise_bank  # noqa: E402


def timed(fn, launches):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--channels", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("strongaug_bench.py runs on the GPU: no device found")
    _lib.load()
    B, C, M = args.batch, args.channels, 64
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    obs = torch.randint(0, 256, (B, C, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty_like(obs)
    bank = noise_bank(M, seed=0, device="cuda")
    idx = torch.randint(M, (B,), dtype=torch.int32, device="cuda", generator=g)
    w = torch.randn((B, 3, 3, 3, 3), device="cuda", generator=g)
    paths = {
        "obs.clone()": lambda: obs.clone(),
        "drq_aug_overlay": lambda: launch("drq_aug_overlay", ptr(obs), ptr(bank), ptr(idx), ptr(out), B, C, M, 128),
        "drq_aug_random_conv": lambda: launch("drq_aug_random_conv", ptr(obs), ptr(w), ptr(out), B, C),
    }
    times = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            times[k].append(timed(fn, args.launches))
    nbytes = obs.numel()
    print(f"B = {B}, C = {C}: {nbytes / 1e6:.2f} MB read and {nbytes / 1e6:.2f} MB written per launch; {args.rounds} rounds of "
          f"{args.launches} launches, device-event microseconds per launch, median [smallest .. largest]")
    floor = statistics.median(times["obs.clone()"])
    for k, v in times.items():
        med = statistics.median(v)
        print(f"  {k:22s} {med:8.1f} [{min(v):.1f} .. {max(v):.1f}]   {2 * nbytes / med / 1e6:6.2f} TB/s   {med / floor:5.2f} x the copy")


if __name__ == "__main__":
    main()
