"""Collection cost of N lockstep environments at cheetah_run shapes (frames 9x84x84, A=6, nstep 3, batch 256), one process:

  vec       VecDeviceReplay: store.add(<device tensors of one step of all N>) + store.sample(256) per environment step
  episode   the same rows through the episode store, as a user of a batched GPU simulator has to feed it today: every
            step's tensors are copied to the host (.cpu(): one synchronisation per step), kept in per-environment lists,
            and every --episode-len steps the N finished episodes go in through DeviceReplay.add_episode (host arrays ->
            four blocking copies each); DeviceReplay.sample(256) per environment step

for N = 16 / 256 / 1024, then update() at batch 256 (feature_dim 50, hidden_dim 1024) fed by each store's look-ahead
iterator, alternated inside every repeat: the ring with one add() of N = 16 rows in front of every update, the episode
store as tools/per_bench.py's uniform path feeds it.

Two figures per line (measuring-on-mi355x, section 4): device-event time = median over the iterations of an event pair
around ONE iteration; host wall = a perf_counter window over all iterations of a repeat that ends in a synchronise,
per iteration.  The episode path synchronises by itself, so only its host wall is meaningful; it is reported alone.
The inputs of a step come from a pool of four pre-generated device rows; nothing is allocated inside a timed window
except what the stores allocate themselves.

  python tools/vec_replay_bench.py [--steps 2000] [--repeats 3] [--episode-len 16] [--episodes 3] [--envs 16,256,1024] [--updates 200]

--priority-alpha 0.6 measures prioritized sampling on the ring instead (VecDeviceReplay(priority_alpha=...)): for every N
two rings of the same shape, uniform and prioritized, alternated inside every repeat of the same process -- add() +
sample(256) per environment step (prioritized: drq_vec_add + drq_vec_per_advance, then drq_vec_per_sample in place of
drq_vec_sample), and update() with one add() of N rows in front of it (prioritized: the weighted loss and one
drq_vec_per_update more).  Same steps, updates, repeats and the same two figures per line as above.  No environment is
ever reset here, so every drawable slot carries a priority.

  python tools/vec_replay_bench.py --priority-alpha 0.6 [--steps 2000] [--repeats 3] [--envs 16,256,1024] [--updates 200]

--single-frames measures the single-frame ring (VecFrameReplay: one 3x84x84 frame per slot, the stacks gathered by the
consumer) against the stacked ring of the same shape, alternated in the same way: add() + sample(256) per environment
step -- the single-frame add() moves a third of the bytes --, update() with one add() in front of it (the fused
aug+conv1 launch gathers the stacks from three slots), and observation(), the gather that feeds act_batch().

  python tools/vec_replay_bench.py --single-frames [--steps 2000] [--repeats 3] [--envs 16,256,1024] [--updates 200]

--episode-stats measures the episode statistics (VecEpisodeStats: drq_vec_stats_step, one launch per environment step) next
to the ring: add() + sample(256) per environment step alone, with stats.step(reward, first) behind the add(), and with the
same book-keeping written in torch ops (TorchStats below: running return and length, episode count, length and return
sums, min and max -- without the record log, which has no short torch form), the three alternated inside every repeat of
one process; then stats.step(), the torch form and publish() + poll() on their own.  One environment in 64 is reset in
every row, so episodes do end.  Same steps, repeats and the same two figures per line as above.

  python tools/vec_replay_bench.py --episode-stats [--steps 2000] [--repeats 3] [--envs 16,256,1024]

--render measures VecFrameReplay.add_render() -- the renderer's uint8 [N, S, S, 4] image resized into the ring by one launch
(drq_vec_add_render) -- against what a user writes in front of add() today, in torch ops (torch_chain below: permute, float,
avg_pool2d where 84 divides S and interpolate(mode="area") elsewhere, round, uint8, contiguous; at S = 84 the permute and
the copy alone), and add() of a ready frame as the baseline, the three alternated inside every repeat of one process on one
ring, for S = 84, 128, 168.  The images come from a pool of four per size.  Per line the same two figures as above, and
for add_render() the bytes it moves (image read + frames written) over its device-event time.  The torch chain rounds
float32 means half to even, so its frames are not add_render()'s everywhere; the tool counts the bytes that differ.

  python tools/vec_replay_bench.py --render [--steps 2000] [--repeats 3] [--envs 16,256,1024] [--sizes 84,128,168]

--env reach | pointmass | cartpole | reacher | maze | catch | walker | finger measures the built-in environment (drqv2_amd.envs.VecReach / VecPointMass:
drq_vec_task_step; VecCartpole, swing-up: drq_vec_cartpole_step; VecReacher, sparse: drq_vec_reacher_step; VecMaze, size 6, sparse, a fresh maze per episode: drq_vec_maze_step; VecCatch, cup_width 0.3, sparse: drq_vec_catch_step; VecWalker, the walk speed: drq_vec_walker_step; VecFinger, spin, sparse: drq_vec_finger_step; one launch per step of all N; --action-repeat K sub-steps
inside it, 1 by default)
next to the single-frame ring it feeds: env.step(), ring.add() of one step's outputs, and the two together, alternated
inside every repeat of one process.  Same steps, repeats and the same two figures per line as above.

  python tools/vec_replay_bench.py --env reach|pointmass|cartpole|reacher|maze|catch|walker|finger [--action-repeat 1] [--steps 2000] [--repeats 3] [--envs 16,256,1024]

--eval-stack measures the evaluation pieces (drqv2_amd.evaluate): VecFrameStack.push() -- drq_vec_stack_push, one launch --
beside what an evaluation loop used before it, VecFrameReplay.add() + observation() (two launches), and add() alone, the
three alternated inside every repeat of one process; then VecVideo.record() at its defaults (16 environments, 4 x 4 tiles,
scale 2) and the host wall of VecVideo.save() for a 102-image clip of a VecReach rollout, as .png and as .npy.  Same
steps, repeats and the same two figures per line as above.

  python tools/vec_replay_bench.py --eval-stack [--steps 2000] [--repeats 3] [--envs 16,256,1024]

--explore measures the exploration bonus (drqv2_amd.explore.SimHashBonus: drq_explore_simhash_step, two launches per step
of all N) on the frames of VecReach: env.step(), bonus.step(frame, reward), bonus.step(frame, update=False), and the
collection step with the bonus in it -- env.step() + bonus.step() + ring.add() --, the four alternated inside every
repeat of one process.  Same steps, repeats and the same two figures per line as above, and for the bonus the frame
bytes it reads over its device-event time.

  python tools/vec_replay_bench.py --explore [--explore-bits 16] [--steps 2000] [--repeats 3] [--envs 16,256]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2  # noqa: E402
from drqv2_amd import synth  # noqa: E402
from drqv2_amd.replay import DeviceReplay, VecDeviceReplay, VecEpisodeStats, VecFrameReplay  # noqa: E402

OBS = (9, 84, 84)
A, NSTEP, B = 6, 3, 256
SLOTS = 65536                       # both stores hold this many steps: 4.2 GB of frames each


def pool_rows(N, n=4):
    g = torch.Generator(device="cuda")
    g.manual_seed(N)
    return [(torch.randint(0, 256, (N,) + OBS, dtype=torch.uint8, device="cuda", generator=g),
             torch.rand(N, A, device="cuda", generator=g) * 2 - 1, torch.rand(N, device="cuda", generator=g),
             torch.ones(N, device="cuda")) for _ in range(n)]


def timed(fn, n):
    """(median device-event us of one call, host wall us per call) over n calls"""
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
    return f"{v[len(v) // 2]:9.1f} us [{v[0]:.1f} .. {v[-1]:.1f}]"


def collection(N, args):
    rows = pool_rows(N)
    vec = VecDeviceReplay(max(32, SLOTS // N), N, OBS, A, NSTEP, 0.99, "cuda", seed=1)
    epi = DeviceReplay(SLOTS, OBS, A, NSTEP, 0.99, "cuda", seed=1, indexed=True)
    first = torch.zeros(N, dtype=torch.bool, device="cuda")
    L = args.episode_len
    held = []

    def vec_step(i):
        vec.add(*rows[i & 3], first)
        vec.sample(B)

    def epi_step(i):
        held.append(tuple(t.cpu().numpy() for t in rows[i & 3]))          # the per-step trip to the host
        if len(held) == L + 1:
            cols = [np.stack(c) for c in zip(*held)]                      # [L+1][N]...
            for e in range(N):
                epi.add_episode({"observation": cols[0][:, e], "action": cols[1][:, e], "reward": cols[2][:, e],
                                 "discount": cols[3][:, e]})
            del held[:]
        if epi.episodes:
            epi.sample(B)

    for i in range(NSTEP + 1):                                            # warm-up: both stores become drawable
        vec.add(*rows[i & 3], first)
    for i in range(20):
        vec_step(i)
    for i in range(L + 2):
        epi_step(i)
    del held[:]
    n_epi = args.episodes * (L + 1)                                       # whole episodes: every add_episode is inside
    res = {"vec_dev": [], "vec_wall": [], "epi_wall": []}
    for _ in range(args.repeats):
        d, w = timed(vec_step, args.steps)
        res["vec_dev"].append(d)
        res["vec_wall"].append(w)
        res["epi_wall"].append(timed(epi_step, n_epi)[1])
    print(f"N={N:5d}  vec     add()+sample({B}) per environment step: device-event {spread(res['vec_dev'])}   host wall "
          f"{spread(res['vec_wall'])}   ({args.steps} steps x {args.repeats})", flush=True)
    print(f"N={N:5d}  episode .cpu() + add_episode every {L} steps + sample({B}), per environment step: host wall "
          f"{spread(res['epi_wall'])}   ({n_epi} steps x {args.repeats})", flush=True)
    mid = args.repeats // 2
    print(f"N={N:5d}  episode / vec (host wall): {sorted(res['epi_wall'])[mid] / sorted(res['vec_wall'])[mid]:.1f}", flush=True)


def make_agent():
    Fd, H = 50, 1024
    torch.manual_seed(0)
    ag = drqv2.DrQV2Agent(OBS, (A,), "cuda", 1e-4, Fd, H, 0.01, 2000, 1, "linear(1.0,0.1,500000)", 0.3, False)
    enc, actor, critic = synth.make_weights(9, A, Fd, H, 0)
    ag.encoder.load_state_dict(enc)
    ag.actor.load_state_dict(actor)
    ag.critic.load_state_dict(critic)
    ag.critic_target.load_state_dict(critic)
    return ag


def prioritized(N, args, ag):
    """uniform ring against prioritized ring at N environments: collection steps, then updates, alternated per repeat"""
    rows = pool_rows(N)
    mk = lambda alpha: VecDeviceReplay(max(32, SLOTS // N), N, OBS, A, NSTEP, 0.99, "cuda", seed=1, priority_alpha=alpha)
    two_rings(N, args, ag, {"uniform": (mk(None), rows), "prioritized": (mk(args.priority_alpha), rows)})


def single_frames(N, args, ag):
    """stacked ring against single-frame ring at N environments, same rows and slots; then observation()"""
    rows = pool_rows(N)
    newest = [(r[0][:, 6:9].contiguous(),) + r[1:] for r in rows]      # the frame a renderer hands out
    R = max(32, SLOTS // N)
    single = VecFrameReplay(R, N, A, NSTEP, 0.99, "cuda", seed=1)
    stacked = VecDeviceReplay(R, N, OBS, A, NSTEP, 0.99, "cuda", seed=1)
    print(f"N={N:5d}  bytes per slot: stacked {stacked.frame_bytes}, single {single.frame_bytes}; per add(): "
          f"{N * stacked.frame_bytes / 1e6:.1f} MB against {N * single.frame_bytes / 1e6:.1f} MB", flush=True)
    two_rings(N, args, ag, {"stacked": (stacked, rows), "single": (single, newest)})
    v = [timed(lambda i: single.observation(), args.steps) for _ in range(args.repeats)]
    print(f"N={N:5d}  single      ring  observation(): device-event {spread([x[0] for x in v])}   host wall "
          f"{spread([x[1] for x in v])}   ({args.steps} x {args.repeats})", flush=True)


class TorchStats:
    """the totals of VecEpisodeStats.step() in torch ops, for the comparison only: no record log, no per-environment limit"""

    def __init__(self, N):
        z = lambda dt: torch.zeros((), dtype=dt, device="cuda")
        self.ret, self.len = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
        self.episodes, self.length_sum, self.return_sum = z(torch.int64), z(torch.int64), z(torch.float64)
        self.min_return, self.max_return = z(torch.float32) + float("inf"), z(torch.float32) - float("inf")
        self.inf = z(torch.float32) + float("inf")

    def step(self, reward, first):
        closed = first & (self.len > 0)
        self.episodes += closed.sum()
        self.length_sum += (self.len * closed).sum()
        self.return_sum += (self.ret * closed).sum(dtype=torch.float64)
        self.min_return = torch.minimum(self.min_return, torch.where(closed, self.ret, self.inf).min())
        self.max_return = torch.maximum(self.max_return, torch.where(closed, self.ret, -self.inf).max())
        self.ret = torch.where(first, 0.0, self.ret + reward)
        self.len = torch.where(first, 0, self.len + 1)


def episode_stats(N, args):
    """the ring alone, with stats.step() and with the torch book-keeping, alternated per repeat; then each on its own"""
    rows = pool_rows(N)
    e = torch.arange(N, device="cuda")
    firsts = [(e + 16 * k) % 64 == 0 for k in range(4)]                   # one environment in 64 is reset in each row
    ring = VecDeviceReplay(max(32, SLOTS // N), N, OBS, A, NSTEP, 0.99, "cuda", seed=1)
    stats, tstats = VecEpisodeStats(N, "cuda"), TorchStats(N)

    def ring_step(i):
        ring.add(*rows[i & 3], firsts[i & 3])
        ring.sample(B)

    def stats_step(i):
        ring.add(*rows[i & 3], firsts[i & 3])
        stats.step(rows[i & 3][2], firsts[i & 3])
        ring.sample(B)

    def torch_step(i):
        ring.add(*rows[i & 3], firsts[i & 3])
        tstats.step(rows[i & 3][2], firsts[i & 3])
        ring.sample(B)

    def publish(i):
        stats.publish()
        stats.poll()

    paths = {f"ring: add()+sample({B})": ring_step, "ring + stats.step()": stats_step, "ring + torch book-keeping": torch_step,
             "stats.step() alone": lambda i: stats.step(rows[i & 3][2], firsts[i & 3]),
             "torch book-keeping alone": lambda i: tstats.step(rows[i & 3][2], firsts[i & 3]),
             "stats.publish() + poll()": publish}
    for i in range(NSTEP + 1):
        ring.add(*rows[i & 3], firsts[i & 3])
    stats.step(rows[0][2])                                                # call 0: a reset row for every environment
    tstats.step(rows[0][2], torch.ones(N, dtype=torch.bool, device="cuda"))
    for fn in paths.values():
        for i in range(20):
            fn(i)
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            res[k].append(timed(fn, args.steps))
    for k, v in res.items():
        print(f"N={N:5d}  {k:28s} per environment step: device-event {spread([x[0] for x in v])}   host wall "
              f"{spread([x[1] for x in v])}   ({args.steps} x {args.repeats}, alternated)", flush=True)
    snap = stats.read()
    print(f"N={N:5d}  statistics after {snap.rows} steps: {snap.episodes} episodes, mean length {snap.mean_length:.1f}; the "
          f"torch form counted {int(tstats.episodes)}", flush=True)


def torch_chain(image):
    """what stands in front of add() without add_render(), for the comparison only: RGBA [N, S, S, 4] -> uint8 [N, 3, 84, 84]"""
    S = image.shape[1]
    x = image[..., :3].permute(0, 3, 1, 2)
    if S == 84:
        return x.contiguous()
    x = x.float()
    x = torch.nn.functional.avg_pool2d(x, S // 84) if S % 84 == 0 else torch.nn.functional.interpolate(x, size=(84, 84), mode="area")
    return x.round().to(torch.uint8).contiguous()


def render(N, S, args):
    """add() of a ready frame, add_render() of the image and the torch chain + add(), alternated per repeat on one ring"""
    g = torch.Generator(device="cuda")
    g.manual_seed(N + S)
    rows = [(torch.randint(0, 256, (N, S, S, 4), dtype=torch.uint8, device="cuda", generator=g),
             torch.rand(N, A, device="cuda", generator=g) * 2 - 1, torch.rand(N, device="cuda", generator=g),
             torch.ones(N, device="cuda")) for _ in range(4)]
    frames = [torch_chain(r[0]) for r in rows]
    first = torch.zeros(N, dtype=torch.bool, device="cuda")
    ring = VecFrameReplay(max(32, SLOTS // N), N, A, NSTEP, 0.99, "cuda", seed=1)
    paths = {"add() of a ready frame": lambda i: ring.add(frames[i & 3], *rows[i & 3][1:], first),
             "add_render()": lambda i: ring.add_render(*rows[i & 3], first),
             "torch chain + add()": lambda i: ring.add(torch_chain(rows[i & 3][0]), *rows[i & 3][1:], first)}
    ring.add_render(*rows[0], first)
    mine = ring.frames[:N].view(N, 3, 84, 84).clone()
    diff = int((mine != frames[0]).sum())
    for fn in paths.values():
        for i in range(20):
            fn(i)
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            res[k].append(timed(fn, args.steps))
    for k, v in res.items():
        print(f"N={N:5d} S={S:3d}  {k:24s}: device-event {spread([x[0] for x in v])}   host wall "
              f"{spread([x[1] for x in v])}   ({args.steps} x {args.repeats}, alternated)", flush=True)
    moved = N * (S * S * 4 + ring.frame_bytes)
    dev = sorted(x[0] for x in res["add_render()"])[args.repeats // 2]
    print(f"N={N:5d} S={S:3d}  add_render() moves {moved / 1e6:.1f} MB: {moved / dev / 1e3:.1f} GB/s over its device-event time; "
          f"the torch chain's frames differ in {diff} of {mine.numel()} bytes", flush=True)


def device_env(N, args):
    """step() of the built-in environment (--env reach | pointmass | cartpole | reacher | maze | catch | walker | finger at --action-repeat K), VecFrameReplay.add() of one
    step's outputs, and both, alternated per repeat"""
    from drqv2_amd.envs import VecCartpole, VecCatch, VecFinger, VecMaze, VecPointMass, VecReach, VecReacher, VecWalker
    cls = {"reach": VecReach, "pointmass": VecPointMass, "cartpole": VecCartpole, "reacher": VecReacher, "maze": VecMaze,
           "catch": VecCatch, "walker": VecWalker, "finger": VecFinger}[args.env]
    env = cls(N, "cuda", action_dim=A, episode_length=250, seed=1, action_repeat=args.action_repeat)
    ring = VecFrameReplay(max(32, SLOTS // N), N, A, NSTEP, 0.99, "cuda", seed=1)
    g = torch.Generator(device="cuda")
    g.manual_seed(N)
    actions = [torch.rand(N, A, device="cuda", generator=g) * 2 - 1 for _ in range(4)]
    env.reset()
    held = tuple(t.clone() for t in env.step(actions[0]))

    def both(i):
        frame, reward, discount, first = env.step(actions[i & 3])
        ring.add(frame, actions[i & 3], reward, discount, first)

    paths = {"env.step()": lambda i: env.step(actions[i & 3]),
             "ring.add() of a step's outputs": lambda i: ring.add(held[0], actions[i & 3], *held[1:]),
             "env.step() + ring.add()": both}
    for fn in paths.values():
        for i in range(20):
            fn(i)
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            res[k].append(timed(fn, args.steps))
    what = "" if (args.env, args.action_repeat) == ("reach", 1) else f"{args.env} x{args.action_repeat}  "
    for k, v in res.items():
        print(f"N={N:5d}  {what}{k:31s}: device-event {spread([x[0] for x in v])}   host wall {spread([x[1] for x in v])}   "
              f"({args.steps} x {args.repeats}, alternated)", flush=True)


def explore(N, args):
    """SimHashBonus.step(frame, reward) of VecReach's frames, env.step(), and the two with ring.add() of reward + bonus,
    alternated per repeat; the bonus reads 21,168 bytes per environment, its rate over the device-event time is printed"""
    from drqv2_amd.envs import VecReach
    from drqv2_amd.explore import SimHashBonus
    env = VecReach(N, "cuda", action_dim=A, episode_length=250, seed=1)
    ring = VecFrameReplay(max(32, SLOTS // N), N, A, NSTEP, 0.99, "cuda", seed=1)
    bonus = SimHashBonus(N, "cuda", bits=args.explore_bits, beta=0.1, seed=1)
    g = torch.Generator(device="cuda")
    g.manual_seed(N)
    actions = [torch.rand(N, A, device="cuda", generator=g) * 2 - 1 for _ in range(4)]
    env.reset()
    held = tuple(t.clone() for t in env.step(actions[0]))

    def loop(i):
        frame, reward, discount, first = env.step(actions[i & 3])
        ring.add(frame, actions[i & 3], bonus.step(frame, reward), discount, first)

    paths = {"env.step()": lambda i: env.step(actions[i & 3]),
             "bonus.step(frame, reward)": lambda i: bonus.step(held[0], held[1]),
             "bonus.step(frame, update=False)": lambda i: bonus.step(held[0], update=False),
             "env.step() + bonus.step() + ring.add()": loop}
    for fn in paths.values():
        for i in range(20):
            fn(i)
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            res[k].append(timed(fn, args.steps))
    for k, v in res.items():
        dev = sorted(x[0] for x in v)[len(v) // 2]
        rate = f"   {N * 21168 / dev / 1e3:6.2f} GB/s of frames" if k.startswith("bonus") else ""
        print(f"N={N:5d}  bits={args.explore_bits:2d}  {k:38s}: device-event {spread([x[0] for x in v])}   host wall "
              f"{spread([x[1] for x in v])}   ({args.steps} x {args.repeats}, alternated){rate}", flush=True)


def eval_stack(N, args):
    """VecFrameStack.push() beside what stood in for it, VecFrameReplay.add() + observation(), alternated per repeat"""
    from drqv2_amd.evaluate import VecFrameStack
    rows = pool_rows(N)
    newest = [(r[0][:, 6:9].contiguous(),) + r[1:] for r in rows]      # the frame a renderer hands out
    first = torch.zeros(N, dtype=torch.bool, device="cuda")
    ring = VecFrameReplay(max(32, SLOTS // N), N, A, NSTEP, 0.99, "cuda", seed=1)
    stack = VecFrameStack(N, "cuda")

    def ring_pair(i):
        ring.add(*newest[i & 3], first)
        ring.observation()

    paths = {"stack.push()": lambda i: stack.push(newest[i & 3][0], first),
             "ring.add() + observation()": ring_pair,
             "ring.add() alone": lambda i: ring.add(*newest[i & 3], first)}
    for fn in paths.values():
        for i in range(20):
            fn(i)
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            res[k].append(timed(fn, args.steps))
    for k, v in res.items():
        print(f"N={N:5d}  {k:27s}: device-event {spread([x[0] for x in v])}   host wall {spread([x[1] for x in v])}   "
              f"({args.steps} x {args.repeats}, alternated)", flush=True)


def eval_video(args):
    """VecVideo.record() at its defaults (the first 16 environments, 4 x 4 tiles, scale 2), then save() of a clip as the
    demo records it: 102 images of a VecReach rollout under uniform-random actions"""
    import tempfile
    from drqv2_amd.envs import VecReach
    from drqv2_amd.evaluate import VecVideo
    N = 16
    env = VecReach(N, "cuda", action_dim=A, episode_length=50, seed=1)
    video = VecVideo(N, "cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(N)
    actions = [torch.rand(N, A, device="cuda", generator=g) * 2 - 1 for _ in range(4)]
    frame = env.reset().clone()
    done = torch.zeros(N, dtype=torch.int32, device="cuda")
    done[::3] = 1                                                         # a third of the tiles dimmed

    def record(i):
        if len(video) == video.max_frames:
            video.clear()
        video.record(frame, done, 1)

    for i in range(20):
        record(i)
    v = [timed(record, args.steps) for _ in range(args.repeats)]
    nbytes = video.buffer[0].numel()
    print(f"N={N:5d}  video.record() ({video.grid[0]} x {video.grid[1]} tiles, scale {video.scale}, {nbytes / 1e6:.2f} MB per "
          f"image): device-event {spread([x[0] for x in v])}   host wall {spread([x[1] for x in v])}   "
          f"({args.steps} x {args.repeats})", flush=True)
    video.clear()
    video.record(frame)
    for i in range(101):
        video.record(env.step(actions[i & 3])[0])
    with tempfile.TemporaryDirectory() as d:
        for ext in (".png", ".npy"):
            path, t = os.path.join(d, "clip" + ext), []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                size = video.save(path)
                t.append(time.perf_counter() - t0)
            print(f"N={N:5d}  video.save({ext}) of {len(video)} images ({len(video) * nbytes / 1e6:.1f} MB raw -> "
                  f"{size / 1e6:.2f} MB): host wall {sorted(t)[len(t) // 2]:.3f} s [{min(t):.3f} .. {max(t):.3f}]", flush=True)
        t0 = time.perf_counter()
        host = video.clip().cpu().numpy()
        t1 = time.perf_counter()
        print(f"N={N:5d}  of which the copy of the clip to the host: {t1 - t0:.3f} s ({host.nbytes / 1e6:.1f} MB); the rest is "
              f"zlib and the file", flush=True)


def two_rings(N, args, ag, rings):
    """rings: name -> (store, its pool of rows); collection steps, then updates, alternated per repeat"""
    first = torch.zeros(N, dtype=torch.bool, device="cuda")
    rows = {k: r for k, (_, r) in rings.items()}
    rings = {k: ring for k, (ring, _) in rings.items()}
    its = {}
    for k, ring in rings.items():
        ring.batch_size = B
        for i in range(NSTEP + 1 + 20):
            ring.add(*rows[k][i & 3], first)
        its[k] = iter(ring)

    def step(k):
        def fn(i):
            rings[k].add(*rows[k][i & 3], first)
            rings[k].sample(B)
        return fn

    def update(k):
        def fn(i):
            rings[k].add(*rows[k][i & 3], first)
            ag.update(its[k], i)
        return fn

    for k in rings:
        for i in range(20):
            step(k)(i)
            update(k)(i)
    res = {(what, k): [] for what in ("step", "update") for k in rings}
    for _ in range(args.repeats):
        for k in rings:
            res["step", k].append(timed(step(k), args.steps))
        for k in rings:
            res["update", k].append(timed(update(k), args.updates))
    for (what, k), v in res.items():
        label = f"add()+sample({B}) per environment step" if what == "step" else f"add() + update B={B}"
        n = args.steps if what == "step" else args.updates
        print(f"N={N:5d}  {k:11s} ring  {label}: device-event {spread([x[0] for x in v])}   host wall "
              f"{spread([x[1] for x in v])}   ({n} x {args.repeats}, alternated)", flush=True)


def updates(args):
    N = 16
    ag = make_agent()
    rows = pool_rows(N)
    first = torch.zeros(N, dtype=torch.bool, device="cuda")
    vec = VecDeviceReplay(SLOTS // N, N, OBS, A, NSTEP, 0.99, "cuda", seed=1)
    epi = DeviceReplay(SLOTS, OBS, A, NSTEP, 0.99, "cuda", seed=1, indexed=True)
    for i in range(200):
        vec.add(*rows[i & 3], first)
    r = np.random.RandomState(0)
    for e in range(8):
        epi.add_episode({"observation": r.randint(0, 256, (501,) + OBS).astype(np.uint8),
                         "action": r.uniform(-1, 1, (501, A)).astype(np.float32),
                         "reward": r.rand(501, 1).astype(np.float32), "discount": np.ones((501, 1), np.float32)})
    vec.batch_size = epi.batch_size = B
    it_vec, it_epi = iter(vec), iter(epi)

    def vec_update(i):
        vec.add(*rows[i & 3], first)
        ag.update(it_vec, i)

    paths = {"vec (add + update)": vec_update, "episode (update)": lambda i: ag.update(it_epi, i)}
    for fn in paths.values():
        for i in range(20):
            fn(i)
    res = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            res[k].append(timed(fn, args.updates))
    for k, v in res.items():
        print(f"update B={B} fed by {k:20s}: device-event {spread([x[0] for x in v])}   host wall "
              f"{spread([x[1] for x in v])}   ({args.updates} updates x {args.repeats}, alternated)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--episodes", type=int, default=3, help="episode lengths per repeat of the episode path")
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--episode-len", type=int, default=16)
    ap.add_argument("--envs", default="16,256,1024")
    ap.add_argument("--priority-alpha", type=float, default=None,
                    help="measure the uniform ring against the prioritized one instead of against the episode store")
    ap.add_argument("--single-frames", action="store_true",
                    help="measure the stacked ring against the single-frame ring (VecFrameReplay) instead")
    ap.add_argument("--episode-stats", action="store_true",
                    help="measure the ring with and without VecEpisodeStats.step(), and the same book-keeping in torch ops")
    ap.add_argument("--render", action="store_true",
                    help="measure add_render() against the torch resize chain in front of add(), and add() alone")
    ap.add_argument("--sizes", default="84,128,168", help="image sizes of --render")
    ap.add_argument("--env", choices=["reach", "pointmass", "cartpole", "reacher", "maze", "catch", "walker", "finger"], default=None,
                    help="measure the built-in environment's step() next to the single-frame ring's add()")
    ap.add_argument("--action-repeat", type=int, default=1, metavar="K", help="simulator steps per step() of --env, 1 .. 16")
    ap.add_argument("--eval-stack", action="store_true",
                    help="measure VecFrameStack.push() beside VecFrameReplay.add() + observation(), and VecVideo.record() / save()")
    ap.add_argument("--explore", action="store_true",
                    help="measure SimHashBonus.step() next to the built-in environment's step() and the ring's add()")
    ap.add_argument("--explore-bits", type=int, default=16, metavar="K", help="bits of the SimHash code of --explore, 1 .. 24")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vec_replay_bench.py measures on the GPU: no device found")
    if args.explore:
        for N in (int(x) for x in args.envs.split(",")):
            explore(N, args)
            torch.cuda.empty_cache()
        return
    if args.eval_stack:
        for N in (int(x) for x in args.envs.split(",")):
            eval_stack(N, args)
            torch.cuda.empty_cache()
        eval_video(args)
        return
    if args.env:
        for N in (int(x) for x in args.envs.split(",")):
            device_env(N, args)
            torch.cuda.empty_cache()
        return
    if args.render:
        for N in (int(x) for x in args.envs.split(",")):
            for S in (int(x) for x in args.sizes.split(",")):
                render(N, S, args)
                torch.cuda.empty_cache()
        return
    if args.episode_stats:
        for N in (int(x) for x in args.envs.split(",")):
            episode_stats(N, args)
            torch.cuda.empty_cache()
        return
    if args.priority_alpha is not None or args.single_frames:
        ag = make_agent()
        for N in (int(x) for x in args.envs.split(",")):
            (single_frames if args.single_frames else prioritized)(N, args, ag)
            torch.cuda.empty_cache()
        return
    for N in (int(x) for x in args.envs.split(",")):
        collection(N, args)
        torch.cuda.empty_cache()
    updates(args)


if __name__ == "__main__":
    main()
