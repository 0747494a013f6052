"""Episode files and the step-major ring, measured ("Episode files"; the raw output of one run is
profiles/episodes_bench.txt):

  prefill   VecFrameReplay.add_episodes() of --episodes episodes of --length steps into a ring of --rows x --envs, against
            the same planned rows through a loop of add() calls (host rows, staged: what the store offered before), in the
            same process, alternating, wall time around a device synchronise
  export    VecFrameReplay.export_episodes() of that ring: wall time, and the share spent inside replay_buffer.save_episode
            (np.savez_compressed) measured by wrapping it
  kernels   drq_vec_fill and drq_vec_export_rows alone, device events over --reps launches, as bytes read + bytes written
            per second, beside a device-to-device copy (Tensor.copy_: hipMemcpyAsync) of as many bytes in the same run

  python tools/episodes_bench.py [--envs 16] [--rows 4096] [--episodes 64] [--length 250] [--reps 10] [--dir DIR]

The frames are low-entropy images (random 21 x 21 blocks, 4 x 4 pixels each) so that compression has something to do;
the copies do not care what the bytes are."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import replay_buffer as RB  # noqa: E402
from drqv2_amd import episodes as E  # noqa: E402
from drqv2_amd import ops  # noqa: E402
from drqv2_amd.replay import VecFrameReplay  # noqa: E402

FB = 3 * 84 * 84


def make_episodes(count, length, A, seed):
    r = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        small = r.randint(0, 256, (length + 1, 3, 21, 21)).astype(np.uint8)
        frame = np.ascontiguousarray(np.repeat(np.repeat(small, 4, axis=2), 4, axis=3))
        out.append({"observation": frame, "action": r.uniform(-1, 1, (length + 1, A)).astype(np.float32),
                    "reward": r.uniform(size=(length + 1, 1)).astype(np.float32),
                    "discount": np.ones((length + 1, 1), np.float32)})
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def events(fn, reps):
    """seconds per call of fn over reps calls, device events, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--length", type=int, default=250)
    ap.add_argument("--action-dim", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the exported files go (default: a temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episodes_bench.py measures on the GPU: no device found")
    N, R, A = args.envs, args.rows, args.action_dim
    new = lambda: VecFrameReplay(R, N, A, 3, 0.99, "cuda", seed=0)
    eps = make_episodes(args.episodes, args.length, A, 0)
    prepared = [{"frame": ep["observation"], "action": ep["action"], "reward": ep["reward"], "discount": ep["discount"]}
                for ep in eps]
    plan = E.plan_fill([args.length] * args.episodes, N)
    L = plan.L
    rows = E.planned_rows(plan, prepared, 0, L)
    row_bytes = N * (FB + 4 * A + 9)
    print(f"{torch.cuda.get_device_name(0)}; ring {R} rows x {N} environments, {args.episodes} episodes of {args.length} steps: "
          f"L = {L} rows, {plan.pad_rows} pad rows, {L * row_bytes / 1e6:.1f} MB of rows", flush=True)

    # ---- prefill: one call against the loop ------------------------------------------------------------------------
    def loop(store):
        for r in range(L):
            store.add(rows[0][r], rows[1][r], rows[2][r], rows[3][r], rows[4][r])

    wall(lambda: new().add_episodes(eps, check=False))              # warm-up: code objects, the pinned allocator
    wall(lambda: loop(new()))
    fills, loops = [], []
    for _ in range(args.rounds):
        a, b = new(), new()
        fills.append(wall(lambda: a.add_episodes(eps, check=False)))
        loops.append(wall(lambda: loop(b)))
        torch.cuda.synchronize()
        same = all(torch.equal(getattr(a, n)[:L * N], getattr(b, n)[:L * N]) for n in a._RING) and a.T == b.T
        del a, b
    print(f"prefill   add_episodes   {min(fills) * 1e3:9.1f} ms (best of {args.rounds}: " + " ".join(f"{t * 1e3:.1f}" for t in fills)
          + f")   {L * row_bytes / min(fills) / 1e9:6.2f} GB/s of rows", flush=True)
    print(f"prefill   add() loop     {min(loops) * 1e3:9.1f} ms (best of {args.rounds}: " + " ".join(f"{t * 1e3:.1f}" for t in loops)
          + f")   {L * row_bytes / min(loops) / 1e9:6.2f} GB/s of rows   x{min(loops) / min(fills):.2f}   rings equal: {same}",
          flush=True)

    # ---- export: the whole call, and the share of compression -----------------------------------------------------------
    store = new()
    store.add_episodes(eps, check=False)
    spent = [0.0]
    save = RB.save_episode

    def timed_save(episode, fn):
        t = time.perf_counter()
        save(episode, fn)
        spent[0] += time.perf_counter() - t

    with tempfile.TemporaryDirectory() as tmp:
        d = args.dir or tmp
        RB.save_episode = timed_save
        try:
            rep = []
            t = wall(lambda: rep.append(store.export_episodes(d, include_open=True)))
        finally:
            RB.save_episode = save
        rep = rep[0]
        size = sum(os.path.getsize(f) for f in rep.files)
    raw = (rep.transitions + rep.episodes) * (3 * FB + 4 * A + 8)
    print(f"export    export_episodes {t * 1e3:9.1f} ms: {rep.episodes} episodes, {rep.transitions} transitions, {raw / 1e6:.1f} MB "
          f"of steps -> {size / 1e6:.1f} MB of files; save_episode (compression, file writes) {spent[0] * 1e3:.1f} ms, "
          f"everything else {(t - spent[0]) * 1e3:.1f} ms", flush=True)

    # ---- the kernels alone ----------------------------------------------------------------------------------------------
    d_rows = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rows]
    d_rows[0] = d_rows[0].view(L, N, FB)
    ring = (store.frames, store.action, store.reward, store.discount, store.first)
    t_fill = events(lambda: ops.vec_fill(*ring, R, N, 0, *d_rows), args.reps)
    moved = 2 * L * row_bytes
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    t_copy = events(lambda: dst.copy_(src), args.reps)
    print(f"kernel    drq_vec_fill         {L} rows: {t_fill * 1e6:9.1f} us  {moved / t_fill / 1e9:8.1f} GB/s (read + written)   "
          f"device copy of {moved / 2e6:.1f} MB: {t_copy * 1e6:9.1f} us  {moved / t_copy / 1e9:8.1f} GB/s", flush=True)
    table = torch.from_numpy(E.export_table([(e, t0, n) for e, t0, n in E.plan_export(
        store.first.cpu().numpy(), store.T, R, N, include_open=True).episodes])).cuda()
    M = min(int(table.shape[0]), 4096)
    table = table[:M].contiguous()
    t_exp = events(lambda: ops.vec_export_rows(store.frames, store.action, store.reward, store.discount, R, N, table, 3), args.reps)
    # the bytes the launch must move: every output byte is written once, but a source frame is part of up to three
    # stacks and is read that often, the second and third time from cache.  Only the DISTINCT source frames are counted
    # as read, so the rate is the one the comparison copy's (distinct bytes in, as many out) can be held against
    tab = table.cpu().numpy().astype(np.int64)
    src_rows = np.stack([np.maximum(tab[:, 0] - k, tab[:, 2]) for k in (2, 1, 0)], axis=1)
    distinct = len(set((src_rows * N + tab[:, 1:2]).reshape(-1).tolist()))
    written = M * (3 * FB + 4 * A + 8)
    moved = distinct * FB + M * (4 * A + 8) + written
    del src, dst
    src, dst = torch.empty(written, dtype=torch.uint8, device="cuda"), torch.empty(written, dtype=torch.uint8, device="cuda")
    t_copy = events(lambda: dst.copy_(src), args.reps)
    print(f"kernel    drq_vec_export_rows  {M} steps: {t_exp * 1e6:9.1f} us  {moved / t_exp / 1e9:8.1f} GB/s ({distinct} distinct "
          f"source frames = {distinct * FB / 1e6:.1f} MB read, each up to three times and re-read across the {args.reps} "
          f"launches, + {written / 1e6:.1f} MB written; the output is allocated per call)   device copy of "
          f"{written / 1e6:.1f} MB: {t_copy * 1e6:9.1f} us  {2 * written / t_copy / 1e9:8.1f} GB/s", flush=True)


if __name__ == "__main__":
    main()
