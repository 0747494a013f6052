#!/usr/bin/env python3
"""Reads the kernel trace (rocprofv3 --kernel-trace, csv) of `tools/ab_overlap.py --trace` and prints, per configuration,
medians over its updates of: the three Winograd input gradients' times, the wall of the actor chain (start of the
critic's Adam launch to the end of the actor trunk's weight gradient), how long before the END of the last input
gradient that chain STARTED (positive = it ran beside them), and the update's wall (aug launch to aug launch).

  tools/overlap_trace_summary.py kernel_trace.csv [updates per configuration]      (AB_CONFIGS as for the traced run)"""
import csv
import os
import statistics
import sys

DEFAULT = "serial,512,480,448,416,384,320,256,224,192"          # tools/ab_overlap.py's


def configs():
    return [c.strip() for c in os.environ.get("AB_CONFIGS", DEFAULT).split(",") if c.strip()]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in rows))
    starts = [i for i, k in enumerate(ks) if "conv1_aug_kernel" in k[2]]
    cfgs = configs()
    need = n * len(cfgs)
    starts = starts[-(need + 1):]            # the traced updates are the last ones of the process; one more closes the last
    if len(starts) < need + 1:
        sys.exit(f"{len(starts) - 1} updates in the trace, {need} wanted")
    print(f"# medians over the last {n - 4} of {n} updates per configuration, microseconds")
    print(f"# {'slots':>8} {'igrad39':>8} {'igrad41':>8} {'igrad43':>8} {'actor chain':>12} {'started before igrads end':>26} "
          f"{'update wall':>12}")
    for ci, c in enumerate(cfgs):
        acc = []
        for u in range(4, n):
            a, b = starts[ci * n + u], starts[ci * n + u + 1]
            seg = ks[a:b]
            ig = [k for k in seg if "conv3x3_wino_kernel<" in k[2] and ", true, false" in k[2]]
            adam = [k for k in seg if "adam_kernel" in k[2]]
            tw = [k for k in seg if "trunk_wgrad_kernel" in k[2]]
            if len(ig) != 3 or not adam or len(tw) < 2:
                sys.exit(f"update {ci * n + u}: {len(ig)} input gradients, {len(adam)} adam, {len(tw)} trunk wgrads")
            ig_end = max(k[1] for k in ig)
            acc.append([(k[1] - k[0]) / 1e3 for k in ig] + [(tw[-1][1] - adam[0][0]) / 1e3, (ig_end - adam[0][0]) / 1e3,
                                                           (ks[b][0] - ks[a][0]) / 1e3])
        med = [statistics.median(col) for col in zip(*acc)]
        print(f"  {c:>8} {med[0]:8.1f} {med[1]:8.1f} {med[2]:8.1f} {med[3]:12.1f} {med[4]:26.1f} {med[5]:12.1f}")


if __name__ == "__main__":
    main()
