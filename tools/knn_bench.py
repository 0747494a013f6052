"""Device time of the k-NN bonus's entry (drq_explore_knn, csrc/knn.hip) beside what a user would otherwise write.

  python tools/knn_bench.py [--batch 256] [--dim 50] [--k 3] [--rounds 5] [--launches 50]

One process: per case and round the two paths in turn -- the raw entry on fixed slots (no host work of KnnBonus, no draw),
and torch.cdist(q, table).kthvalue(k + 1) on the same tensors (k + 1: the row itself is among the candidates there at
distance 0; it materialises the B x M matrix) -- each as `launches` calls back to back between two device events after a
warm-up.  Cases: live = 65,536 and 1,048,576 rows with stride 1, and 1,048,576 with stride 16 (the torch path then
indexes the lattice rows first, outside the timed span).  Prints microseconds per call, the median over the rounds
[smallest .. largest], and the count-based floor: B x M x d x 3 single float32 operations at the chip's unpacked vector
issue rate (1,024 SIMDs x 32 lanes per clock x 2.4 GHz; a packed float32 instruction occupies a SIMD as long as two plain
ones, so packing does not move it)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drqv2_amd import _lib  # noqa: E402
from drqv2_amd._lib import launch, ptr  # noqa: E402

LANE_OPS_PER_SECOND = 1024 * 32 * 2.4e9


def timed(fn, launches):
    for _ in range(3):
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
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench.py runs on the GPU: no device found")
    lib = _lib.load()
    B, d, k = args.batch, args.dim, args.k
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    print(f"B = {B}, d = {d}, k = {k}: {args.rounds} rounds of back-to-back calls between two device events, microseconds per "
          f"call, median [smallest .. largest]")
    for live, stride in ((65536, 1), (1048576, 1), (1048576, 16)):
        table = torch.randn((live, d), device="cuda", generator=g)
        slots = torch.randint(0, live, (B,), device="cuda", generator=g)
        dist = torch.empty(B, device="cuda")
        need = lib.drq_explore_knn_ws_bytes(B, live, stride)
        ws = torch.empty(max(1, need // 4), device="cuda")
        q, cand = table[slots], table[::stride].contiguous()
        M = cand.shape[0]
        launches = max(5, args.launches * 65536 // M)
        paths = {
            "drq_explore_knn": lambda: launch("drq_explore_knn", ptr(table), live, d, live, ptr(slots), B, k, stride, 0, ptr(dist),
                                              ptr(ws), need),
            "torch.cdist(q, table).kthvalue(k + 1)": lambda: torch.cdist(q, cand).kthvalue(k + 1, dim=1),
        }
        times = {name: [] for name in paths}
        for _ in range(args.rounds):
            for name, fn in paths.items():
                times[name].append(timed(fn, launches))
        ops = 3.0 * B * M * d
        floor = 1e6 * ops / LANE_OPS_PER_SECOND
        # the two agree where float32 leaves them room to: cdist takes another route to the same distance
        ref = torch.cdist(q.double(), cand.double()).kthvalue(k + 1 if stride == 1 else k, dim=1).values
        on = (slots % stride) == 0
        if stride > 1:
            ref = torch.where(on, torch.cdist(q.double(), cand.double()).kthvalue(k + 1, dim=1).values, ref)
        err = float(((dist.double() - ref).abs() / ref).max())
        print(f"live = {live}, stride = {stride}: {M} candidates, {launches} calls per round; {ops / 1e9:.2f} G operations, floor "
              f"{floor:.1f} us; largest relative difference from float64 cdist {err:.1e}")
        for name, v in times.items():
            med = statistics.median(v)
            print(f"  {name:40s} {med:9.1f} [{min(v):.1f} .. {max(v):.1f}]   {med / floor:6.2f} x the floor")


if __name__ == "__main__":
    main()
