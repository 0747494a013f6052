"""Latency of acting (encoder + actor forward, drqv2.py:164-175) -- dev tool.
First the two historical lines (act() host wall).  Then, in this one process, alternating after a warm-up of every
shape: act() against act_batch() on one numpy frame, and on device tensors at n = 1, 4, 16, 64 engine.act_forward (the
parent path: the training kernels) against act_batch (csrc/act.hip).  Two figures per path: device-event time = median
over the calls of an event pair around ONE call; host wall = a perf_counter window over all calls that ends in a
synchronise, per call.  Three repeats; min / median / max of the repeats are printed."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2
CALLS = 300
ag = drqv2.DrQV2Agent((9, 84, 84), (6,), "cuda", 1e-4, 50, 1024, 0.01, 2000, 2, "linear(1.0,0.1,500000)", 0.3, True)
obs = np.random.RandomState(0).randint(0, 256, (9, 84, 84)).astype(np.uint8)
for mode in (True, False):
    for _ in range(20):
        ag.act(obs, 5000, mode)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 300
    for _ in range(n):
        a = ag.act(obs, 5000, mode)      # returns a numpy action: includes the device->host copy and sync
    dt = (time.perf_counter() - t0) / n
    print(f"act(eval_mode={mode}): {1e6*dt:7.1f} us per call (host wall, action returned as numpy)", flush=True)


def measure(fn):
    """(median device-event us of one call, host wall us per call) over CALLS calls."""
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for e0, e1 in pairs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / CALLS
    dev = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)[CALLS // 2]
    return 1e3 * dev, 1e6 * wall


def compare(label, paths):
    for fn in paths.values():
        for _ in range(30):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in paths}
    for _ in range(3):
        for k, fn in paths.items():           # alternate the paths inside every repeat
            res[k].append(measure(fn))
    for k, v in res.items():
        d, w = sorted(x[0] for x in v), sorted(x[1] for x in v)
        print(f"{label:28s} {k:24s} device-event {d[1]:7.1f} us [{d[0]:.1f} .. {d[2]:.1f}]   "
              f"host wall {w[1]:7.1f} us [{w[0]:.1f} .. {w[2]:.1f}]", flush=True)


frames = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (64, 9, 84, 84)).astype(np.uint8)).cuda()
eng = ag._engine
for mode in (True, False):
    compare(f"numpy frame, eval_mode={mode}", {"act()": lambda: ag.act(obs, 5000, mode),
                                              "act_batch(n=1)": lambda: ag.act_batch(obs[None], 5000, mode)})
shipped = eng.ACT_FUSED_MAX_ROWS
eng.ACT_FUSED_MAX_ROWS = 64                # every n below on the fused launches: this is where the crossover is read
for n in (1, 4, 16, 64):
    x = frames[:n].contiguous()
    compare(f"device tensor, n={n}", {"engine.act_forward": lambda: eng.act_forward(x),
                                      "act_batch fused (eval)": lambda: ag.act_batch(x, 5000, True),
                                      "act_batch fused (sample)": lambda: ag.act_batch(x, 5000, False)})
print(f"as shipped the engine routes n > {shipped} through act_forward's kernels", flush=True)
