"""Host-side cost of feeding the update from the device replay (dev tool): time inside DeviceReplay.sample() and inside
update() per iteration, and a cProfile of the sampling.

--single-frames measures the single-frame episode store (DeviceReplay(single_frames=True)) against the stacked one
instead, alternated inside every repeat of one process: add_episode() of a 501-step stacked episode (stacked store;
single-frame store with the frame-stack check; without it) and update() at batch 256 fed by each store's look-ahead
iterator.  Two figures per line: device-event time = median over the iterations of an event pair around ONE iteration;
host wall = a perf_counter window over all iterations of a repeat that ends in a synchronise, per iteration; each as
the median over the repeats with [min .. max].

  python tools/replay_host_prof.py --single-frames [--adds 8] [--updates 200] [--repeats 3]
"""
import cProfile, os, pstats, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2
from drqv2_amd import synth
from drqv2_amd.replay import DeviceReplay
dev = torch.device("cuda", 0)
torch.manual_seed(1)
B, A = 256, 6
agent = drqv2.DrQV2Agent((9, 84, 84), (A,), dev, 1e-4, 50, 1024, 0.01, 2000, 2, "linear(1.0,0.1,100000)", 0.3, True)


def single_frames_mode():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--single-frames", action="store_true")
    ap.add_argument("--adds", type=int, default=8)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    T1, cap = 501, 16 * 501
    r = np.random.RandomState(0)

    def episode():
        f = r.randint(0, 256, (T1, 3, 84, 84)).astype(np.uint8)
        t = np.arange(T1)
        obs = np.concatenate([f[np.maximum(t - 2, 0)], f[np.maximum(t - 1, 0)], f], axis=1)     # dmc.py:98-109
        return {"observation": obs, "action": r.uniform(-1, 1, (T1, A)).astype(np.float32),
                "reward": r.uniform(0, 1, (T1, 1)).astype(np.float32), "discount": np.ones((T1, 1), np.float32)}

    pool = [episode() for _ in range(2)]
    mk = lambda **kw: DeviceReplay(cap, (9, 84, 84), A, 3, 0.99, dev, seed=0, indexed=True, **kw)
    stores = {"stacked": mk(), "single": mk(single_frames=True), "single, check_stacks=False": mk(single_frames=True,
                                                                                                   check_stacks=False)}
    its = {}
    for k, st in stores.items():
        st.batch_size = B
        for e in range(8):
            st.add_episode(pool[e & 1])
        its[k] = iter(st)
        print(f"{k:28s}: {st.frame_bytes} bytes per slot, {st.frames.numel() / 1e6:.1f} MB of frames for {cap} slots; "
              f"add_episode uploads {T1 * st.frame_bytes / 1e6:.1f} MB", flush=True)

    def timed(fn, n):
        pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, (e0, e1) in enumerate(pairs):
            e0.record()
            fn(i)
            e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n
        return 1e3 * sorted(e0.elapsed_time(e1) for e0, e1 in pairs)[n // 2], 1e6 * wall

    def spread(v):
        v = sorted(v)
        return f"{v[len(v) // 2]:10.1f} us [{v[0]:.1f} .. {v[-1]:.1f}]"

    add = lambda k: (lambda i: stores[k].add_episode(pool[i & 1]))
    upd = lambda k: (lambda i: agent.update(its[k], 2 * i))
    fed = [k for k in stores if "check" not in k]
    for k in fed:
        for i in range(20):
            upd(k)(i)
    res = {}
    for _ in range(args.repeats):
        for k in stores:
            res.setdefault(("add_episode(501 steps)", k), []).append(timed(add(k), args.adds))
        for k in fed:
            res.setdefault((f"update B={B}", k), []).append(timed(upd(k), args.updates))
    for (what, k), v in res.items():
        n = args.adds if what.startswith("add") else args.updates
        print(f"{what:24s} {k:28s}: device-event {spread([x[0] for x in v])}   host wall {spread([x[1] for x in v])}   "
              f"({n} x {args.repeats}, alternated)", flush=True)


if "--single-frames" in sys.argv:
    single_frames_mode()
    sys.exit(0)
batch = synth.make_batch(B, A, 9, seed=0, smooth=True)
store = DeviceReplay(4096, (9, 84, 84), A, 3, 0.99, dev, seed=0, indexed=True)
obs_pool = batch[0].numpy()
r = np.random.RandomState(0)
for e in range(16):
    T1 = 201
    store.add_episode({"observation": obs_pool[r.randint(0, obs_pool.shape[0], T1)],
                       "action": r.uniform(-1, 1, (T1, A)).astype(np.float32),
                       "reward": r.uniform(0, 1, (T1, 1)).astype(np.float32),
                       "discount": np.ones((T1, 1), np.float32)})
store.batch_size = B


class Timed:
    def __init__(self):
        self.t = 0.0
    def __iter__(self):
        return self
    def __next__(self):
        t0 = time.perf_counter()
        b = store.sample(B)
        self.t += time.perf_counter() - t0
        return b


it = Timed()
for s in range(20):
    agent.update(it, 2 * s)
torch.cuda.synchronize()
it.t = 0.0
n = 300
t0 = time.perf_counter(); host = 0.0
for s in range(n):
    h0 = time.perf_counter()
    agent.update(it, 2 * s)
    host += time.perf_counter() - h0
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"indexed device replay: {1e6*dt/n:8.1f} us/update wall, {1e6*host/n:8.1f} us inside update(), of which {1e6*it.t/n:6.1f} us in sample()")
pr = cProfile.Profile()
pr.enable()
for s in range(300):
    store.sample(B)
pr.disable()
torch.cuda.synchronize()
pstats.Stats(pr).sort_stats("tottime").print_stats(14)
