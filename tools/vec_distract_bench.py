"""Device time of the distraction launch (drq_vec_distract) beside drq_vec_reach_render, which writes the same number of
bytes with the same launch shape, in one process, alternated.

  python tools/vec_distract_bench.py [--envs 16,1024] [--calls 300] [--repeats 5]

Per N and path: `calls` launches, each between a pair of events of its own (the device-event time of ONE launch: the
kernel and what the queue adds around a lone short launch), and the same `calls` launches back to back between ONE pair
(device time per launch when the queue never drains; at small N this is bounded by how fast the host enqueues).  The
paths are alternated inside every repeat; the table gives the median over the repeats and [smallest .. largest].  The
frames are those of a reset VecReach, keyed by its background, so most pixels are background -- the expensive side in
noise mode.  Strengths: camera 4, colour 32, alpha 256, dynamic; the bank is 4 clips of 8 random frames.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drqv2_amd.distract import FrameDistractor  # noqa: E402
from drqv2_amd.envs import VecReach  # noqa: E402


def lone(fn, calls):
    """median device-event microseconds of one call, each call between its own pair of events"""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in pairs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(1e3 * a.elapsed_time(b) for a, b in pairs)


def stream(fn, calls):
    """device-event microseconds per call of `calls` calls back to back"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="16,1024")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vec_distract_bench.py runs on the GPU: no device found")
    print(f"{torch.cuda.get_device_name(0)}; {args.calls} calls per path and repeat, {args.repeats} repeats, paths alternated; "
          "microseconds, median [smallest .. largest]")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    bank = torch.randint(0, 256, (4, 8, 3, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    for N in (int(n) for n in args.envs.split(",")):
        env = VecReach(N, "cuda", seed=0)
        frame = env.reset().clone()
        first = torch.zeros(N, dtype=torch.uint8, device="cuda")
        key = env.background_key()
        paths = {"drq_vec_reach_render": env.render}
        for name, kw in (("identity (strengths 0)", dict(key=key)),
                         ("mode 0 (camera, colour)", dict(camera=4, color=32, key=key)),
                         ("mode 1 (noise)", dict(camera=4, color=32, background="noise", key=key)),
                         ("mode 2 (bank)", dict(camera=4, color=32, background=bank, key=key))):
            d = FrameDistractor(N, "cuda", seed=1, **kw)
            paths["drq_vec_distract, " + name] = (lambda d=d: d.apply(frame, first))
        for fn in paths.values():            # warm up: code objects, the output buffers
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        got = {k: ([], []) for k in paths}
        for _ in range(args.repeats):
            for k, fn in paths.items():
                got[k][0].append(lone(fn, args.calls))
            for k, fn in paths.items():
                got[k][1].append(stream(fn, args.calls))
        mb = 2 * N * 21168 / 1e6
        print(f"\nN = {N}: {mb:.2f} MB read + written per launch (the render launch writes half of it and reads none)")
        print(f"{'path':48s} {'one launch, own event pair':>30s} {'back to back, per launch':>30s}")
        for k, (one, many) in got.items():
            fmt = lambda v: f"{statistics.median(v):7.2f} [{min(v):6.2f} .. {max(v):6.2f}]"
            print(f"{k:48s} {fmt(one):>30s} {fmt(many):>30s}")


if __name__ == "__main__":
    main()
