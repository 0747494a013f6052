"""Prioritized replay at cheetah_run, batch 256 (A=6, feature_dim=50, hidden_dim=1024), one process, one agent, the two
ways of feeding update() alternated inside every repeat after a warm-up of each (as tools/bc_bench.py does):

  uniform      DeviceReplay(indexed=True)                        the yardstick: uniform draws, unweighted loss
  prioritized  DeviceReplay(indexed=True, priority_alpha=0.6)    draw on the sum tree, weighted loss, priorities renewed

Both stores hold the same episodes and feed update() through their look-ahead iterators.  Two figures per path: device-
event time = median over the updates of an event pair around ONE update() call (with the draw of the next batch and, for
the prioritized path, the priority launch, which the call issues); host wall = a perf_counter window over all updates
of a repeat that ends in a synchronise, per update.  Then the three launches of csrc/per.hip alone: device-event
median of one launch on the same store (fill: one 500-step episode's drawable range).

  python tools/per_bench.py [--updates 200] [--repeats 5] [--capacity 100000]
  python tools/per_bench.py --only uniform|prioritized --updates 50      one path alone, for a kernel trace:
      rocprofv3 --kernel-trace --stats -d <dir> -- python tools/per_bench.py --only prioritized --updates 50
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2  # noqa: E402
from drqv2_amd import _lib, synth  # noqa: E402
from drqv2_amd._lib import check, ptr  # noqa: E402
from drqv2_amd.replay import DeviceReplay  # noqa: E402

OBS = (9, 84, 84)


def episode(T, A, seed):
    r = np.random.RandomState(seed)
    return {"observation": r.randint(0, 256, (T + 1,) + OBS).astype(np.uint8),
            "action": r.uniform(-1, 1, (T + 1, A)).astype(np.float32),
            "reward": r.rand(T + 1, 1).astype(np.float32), "discount": np.ones((T + 1, 1), np.float32)}


def measure(fn, n, step0):
    """(median device-event us of one call, host wall us per call) over n calls."""
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
    ap.add_argument("--capacity", type=int, default=100000)
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--only", choices=("uniform", "prioritized"), default=None)
    args = ap.parse_args()
    B, A, Fd, H, nstep = 256, 6, 50, 1024, 3
    torch.manual_seed(0)
    ag = drqv2.DrQV2Agent(OBS, (A,), "cuda", 1e-4, Fd, H, 0.01, 2000, 1, "linear(1.0,0.1,500000)", 0.3, False)
    enc, actor, critic = synth.make_weights(9, A, Fd, H, 0)
    ag.encoder.load_state_dict(enc)
    ag.actor.load_state_dict(actor)
    ag.critic.load_state_dict(critic)
    ag.critic_target.load_state_dict(critic)
    stores = {"uniform": DeviceReplay(args.capacity, OBS, A, nstep, 0.99, "cuda", seed=1, indexed=True),
              "prioritized": DeviceReplay(args.capacity, OBS, A, nstep, 0.99, "cuda", seed=1, indexed=True,
                                          priority_alpha=0.6)}
    for e in range(args.episodes):
        ep = episode(500, A, e)
        for s in stores.values():
            s.add_episode(ep)
    its = {}
    for k, s in stores.items():
        s.batch_size = B
        its[k] = iter(s)
    paths = {k: (lambda i, it=it: ag.update(it, i)) for k, it in its.items()}
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
    rp = stores["prioritized"]
    print(f"cheetah_run B={B}, store of {args.capacity} slots (tree of {rp.tree_leaves} leaves), {args.repeats} repeats of "
          f"{args.updates} updates per path, alternated", flush=True)
    for k, v in res.items():
        d, w = sorted(x[0] for x in v), sorted(x[1] for x in v)
        print(f"{k:11s} update: device-event {d[mid]:8.1f} us [{d[0]:.1f} .. {d[-1]:.1f}]   "
              f"host wall {w[mid]:8.1f} us [{w[0]:.1f} .. {w[-1]:.1f}]", flush=True)
    med = {k: sorted(x[1] for x in v)[mid] for k, v in res.items()}
    print(f"prioritized / uniform (host wall): {med['prioritized'] / med['uniform']:.4f}", flush=True)

    # the three launches alone
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    L = rp.tree_leaves
    u = torch.rand(B, dtype=torch.float64, device="cuda")
    idx = torch.empty((3, B), dtype=torch.int64, device="cuda")
    w = torch.empty(B, dtype=torch.float32, device="cuda")
    td = torch.rand(B, device="cuda")
    s0, n0 = rp.episodes[0]
    launches = {
        "drq_per_sample": lambda i: check(lib.drq_per_sample(ptr(rp.tree), L, ptr(u), B, nstep, rp.n_valid, 0.4, ptr(idx),
                                                             ptr(w), st), "drq_per_sample"),
        "drq_per_update": lambda i: check(lib.drq_per_update(ptr(rp.tree), L, ptr(idx[2]), ptr(td), B, 0.6, 1e-6, st),
                                          "drq_per_update"),
        "drq_per_fill": lambda i: check(lib.drq_per_fill(ptr(rp.tree), L, s0 + 1, s0 + n0 - nstep + 1, 1, st), "drq_per_fill"),
    }
    for k, fn in launches.items():
        measure(fn, 20, 0)
        d = sorted(measure(fn, 200, 0)[0] for _ in range(3))
        print(f"{k:15s} one launch: device-event {d[1]:6.1f} us [{d[0]:.1f} .. {d[-1]:.1f}]", flush=True)


if __name__ == "__main__":
    main()
