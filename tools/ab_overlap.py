#!/usr/bin/env python3
"""Same-process, interleaved A/B of the update's overlapped schedule (DrqStep.flags bit 16: the actor update on a second
stream beside the encoder backward) over the slot budgets of its input gradients.

  tools/ab_overlap.py [task] [batch] [rounds]        timed: median / best / worst updates/s per configuration
  tools/ab_overlap.py --trace [task] [batch] [n]     n untimed updates per configuration, one after the other, for a
                                                     kernel trace (tools/overlap_trace_summary.py reads it with the
                                                     same AB_CONFIGS)

AB_CONFIGS: comma-separated; `serial` = the serial schedule, a number = the overlapped schedule with that many workgroup
slots for each input gradient (a multiple of 16 up to 512 on a 256-CU device)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

DEFAULT = "serial,512,480,448,416,384,320,256,224,192"


def configs():
    return [c.strip() for c in os.environ.get("AB_CONFIGS", DEFAULT).split(",") if c.strip()]


def apply(engine, cfg, cus):
    engine.overlap_actor = cfg != "serial"
    # the library takes the budget in thirty-seconds of the chip's 2 x CUs slots
    engine.overlap_budget32 = 0 if cfg == "serial" else max(1, int(cfg) * 32 // (2 * cus))


def main():
    args = [a for a in sys.argv[1:] if a != "--trace"]
    trace = "--trace" in sys.argv[1:]
    task = args[0] if len(args) > 0 else "cheetah_run"
    B = int(args[1]) if len(args) > 1 else 256
    n = int(args[2]) if len(args) > 2 else (12 if trace else 6)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = bench.Runner(task, B, B, torch.device("cuda", 0), 0, 1, False)
    eng = r.agent._engine
    cfgs = configs()
    r.run(30, 10)
    if trace:
        for c in cfgs:
            apply(eng, c, cus)
            r.run(n - 2, 2)
        apply(eng, "serial", cus)
        r.run(1, 0)                          # one more aug launch closes the last traced update
        return
    res = {c: [] for c in cfgs}
    for _ in range(n):
        for c in cfgs:
            apply(eng, c, cus)
            res[c].append(1e3 / r.run(100, 5)["ms_per_step"])
    print(f"# {task} B={B}, {n} rounds of 100 updates per configuration, alternating in one process; updates/s")
    print(f"# {'slots':>8} {'median':>9} {'worst':>9} {'best':>9}")
    for c in cfgs:
        v = sorted(res[c])
        print(f"  {c:>8} {v[len(v) // 2]:9.1f} {v[0]:9.1f} {v[-1]:9.1f}", flush=True)


if __name__ == "__main__":
    main()
