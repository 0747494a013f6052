"""Workload for a kernel trace of DrQV2Agent.act_batch -- dev tool.  `rocprofv3 --kernel-trace --stats -- python
tools/act_batch_trace.py N [CALLS]` runs CALLS (default 100) eval-mode calls on N device-resident frames through the
fused path; launches per call = kernel dispatches in the trace / CALLS (no warm-up calls are made, so the count is
exact)."""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 100
ag = drqv2.DrQV2Agent((9, 84, 84), (6,), "cuda", 1e-4, 50, 1024, 0.01, 2000, 2, "linear(1.0,0.1,500000)", 0.3, True)
ag._engine.ACT_FUSED_MAX_ROWS = max(n, ag._engine.ACT_FUSED_MAX_ROWS)
x = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (n, 9, 84, 84)).astype(np.uint8)).cuda()
torch.cuda.synchronize()
for _ in range(calls):
    a = ag.act_batch(x, 5000, True)
torch.cuda.synchronize()
print(f"act_batch n={n}: {calls} calls", flush=True)
