"""The "Vectorised collection" loop of INTEGRATION.md, run as written, on the built-in environment:

  VecReach, VecPointMass, VecCartpole, VecReacher, VecMaze, VecCatch or VecWalker (N environments stepped by one launch) -> VecFrameReplay.add() -> VecEpisodeStats.step()
  VecFrameReplay.observation() -> DrQV2Agent.act_batch() -> the next step; one DrQV2Agent.update() per step after a warm-up

Nothing in the loop waits for the GPU but the statistics read-out once per reporting interval.  It prints the mean episode
return (and length) of the episodes that finished in every interval, from VecEpisodeStats, and afterwards the mean return of
uniform-random actions over the SAME number of episodes on a second environment of the same seed, measured in the same
process: that is the baseline the training curve is read against, not a constant written down in advance.

  python tools/vec_train_demo.py [--task reach|pointmass|cartpole_balance|cartpole_swingup|reacher_easy|reacher_hard|maze|maze_small|catch|catch_hard|walker_stand|walker_walk|walker_run|finger_spin|finger_turn_easy|finger_turn_hard]
                                 [--reward sparse|dense] [--action-repeat 1]
                                 [--maze-layouts K] [--maze-loops Q] [--maze-eval-layout-seed S]
                                 [--steps 20000] [--envs 16] [--episode-length 50] [--warmup 1000] [--report 2000]
                                 [--batch 256] [--lr 3e-4] [--feature-dim 50] [--hidden-dim 256] [--seed 0]
                                 [--checkpoint PATH [--checkpoint-every STEPS] [--resume]]
                                 [--dormant-every K] [--perturb-every K [--perturb-k 2.0]]
                                 [--export-dir DIR] [--prefill-dir DIR]
                                 [--eval-every STEPS [--eval-episodes K] [--video DIR]]
                                 [--explore-beta B [--explore-bits K]]
                                 [--explore-knn-beta B [--explore-knn-k 3] [--explore-knn-candidates M]]
                                 [--demos DIR [--demo-fraction 0.5] [--demo-rows D]]
                                 [--distract SPEC [--distract-on train|eval|both]]
                                 [--svea overlay|conv [--svea-alpha 0.5] [--svea-bank 64]]

--task pointmass trains on the point mass, whose velocity is in no single frame (the frame stack is what shows it);
--task cartpole_balance and cartpole_swingup train on VecCartpole (swing_up False / True), whose step reads one action column
(--action-dim 1 fits it; the reference configures action repeat 2 and episodes of 1,000 simulator steps for its cartpoles);
--task reacher_easy and reacher_hard train on VecReacher (target_radius 0.15 / 0.05), the one task here whose reward is
sparse: 1 for every simulator step with the fingertip inside the target's disc, else 0 (the reference configures episodes of
1,000 simulator steps for its reachers); --reward dense swaps in VecReacher's dense shaping of the same distance, the
comparison arm;
--task maze and maze_small train on VecMaze (size 6 / 4): walls generated on the device at every reset, 1 for every simulator
step in the goal cell, else 0; --reward dense swaps in the shaping by the geodesic distance.  --maze-layouts K draws every
episode's walls from a pool of K mazes (0, the default: a fresh maze per episode), --maze-loops Q opens every remaining
wall with probability Q / 256.  --maze-eval-layout-seed S builds the evaluation environment with layout_seed=S, another
pool of the same size (the training pool is layout_seed 0): the evaluation lines are then held-out returns, and the
report ends with the mean return of the last training interval beside the last held-out one.  It needs --maze-layouts K
and --eval-every STEPS;
--task catch and catch_hard train on VecCatch (cup_width 0.3 / 0.18): a ball on a tether must be swung up and caught in a
driven cup, 1 for every simulator step with the ball in the cup, else 0 (the reference configures episodes of 1,000
simulator steps for its cup_catch); --reward dense swaps in the shaping by the distance to the cup's interior;
--task finger_spin, finger_turn_easy and finger_turn_hard train on VecFinger: a finger that must spin a hinged rod, or turn
its tip into a target disc of radius 0.1 or 0.04, by contact alone; --reward dense swaps in the shapings of the two modes;
--task walker_stand, walker_walk and walker_run train on VecWalker at speed 0, 0.3 and 0.6: a planar legged runner paid
for standing, and for standing and moving forward at that speed (the reference configures episodes of 1,000 simulator
steps for its walker and cheetah tasks); --action-dim defaults to the columns the task reads, at least 2: 4 there;
--action-repeat K holds every action for up to K simulator steps inside the step launch.  All of these apply to the training
environment, the evaluation environment and the random baseline alike.  --episode-length counts simulator steps; the
lengths that are printed count rows, i.e. agent steps.

--eval-every STEPS evaluates the policy every STEPS steps (drqv2_amd.evaluate.evaluate: the first --eval-episodes episodes of
every environment under act_batch(..., eval_mode=True), on a second environment of its own seed, --seed + 1) and prints the
mean, smallest and largest return; --video DIR records those episodes (VecVideo: a mosaic of the first 16 environments,
one launch per step) and writes DIR/eval_<step>.png, an animated PNG.  An evaluation draws from no generator and touches
neither ring nor optimiser, so the training lines of a run are the same with and without it.  Off by default.

--dormant-every K prints the actor's dormant ratio (DrQV2Agent.dormant_ratio) on the look-ahead batch every K updates;
--perturb-every K pulls the weights toward a fresh initialisation every K updates (DrQV2Agent.perturb) with
alpha = clip(1 - perturb_k * ratio, 0.2, 0.9).  Both are off by default, and the output is then unchanged.

--checkpoint PATH saves the whole loop (drqv2_amd.checkpoint: agent, ring, look-ahead batch, environment, statistics, the
generators) at the end of every --checkpoint-every'th iteration; --resume loads PATH into freshly built objects and goes
on at the saved step, so the report lines that follow are those of the uninterrupted run, digit for digit (the wall
times aside).  The other arguments must be the ones the saved run was given; --steps may grow.

--export-dir DIR writes the episodes that finished since the last report as the reference's episode files at every
reporting interval (VecFrameReplay.export_episodes from the previous report's next_row: each closed episode once; the call
WAITS, like the read-out beside it; --report x --envs steps must fit the ring, or episodes leave it unwritten and are
counted as headless).  --prefill-dir DIR loads such a directory into the ring before the first reset row
(VecFrameReplay.add_episodes), e.g. what an earlier run exported; a resumed run has its ring from the checkpoint and skips
it.  Both are off by default, and the output is then unchanged.

--explore-beta B adds a count-based exploration bonus (drqv2_amd.explore.SimHashBonus: a SimHash of the frame of
--explore-bits K bits, 16 by default, bonus = B / sqrt(count)) to the reward that goes into the ring; the episode
statistics, and so every return that is printed, keep the environment's own reward.  The report line then ends with the
number of distinct codes counted so far, and the count table goes into the checkpoint.  Off by default, and the output is
then unchanged.

--explore-knn-beta B adds RE3's state-entropy bonus (drqv2_amd.explore.KnnBonus, INTEGRATION.md, "k-NN bonus (RE3)") to the
reward of every batch as it is handed to update(): B * log(1 + the distance to the --explore-knn-k'th nearest neighbour,
3 by default, among the rows the ring holds), in the 50 features of a fixed random encoder (RandomFeatures) computed from
the observation after every add().  --explore-knn-candidates M looks at every ceil(live / M)'th row only.  The ring, the
statistics and every printed return keep the environment's reward; the report line then ends with the mean distance of
the newest batch, and the feature table goes into the checkpoint.  Not combined with --explore-beta (one bonus per
checkpoint) or --prefill-dir (prefilled rows have no features).  Off by default, and the output is then unchanged.

--demos DIR keeps the episodes of DIR (episode files, e.g. what --export-dir wrote) as demonstrations for the whole run
and draws --demo-fraction of every batch from them (VecDeviceReplay(demo_rows=D), add_demonstrations(), demo_fraction;
INTEGRATION.md, "Demonstrations").  Demonstrations need a ring of whole observations, so the loop then runs on a
VecDeviceReplay of 9 x 84 x 84 stacks -- three times the bytes per slot -- which a VecFrameStack in front of add() puts
together and act_batch() reads.  --demo-rows D sizes the partition; by default it is what the files need at N lanes.
The fraction is held constant here; a loop that anneals it assigns store.demo_fraction before a draw.  Not combined with
--dormant-every / --perturb-every (they gather a single-frame batch) or with checkpoints (the frame stack in front of
the ring is not saved).  Off by default, and the output is then unchanged.

--distract SPEC puts visual distractions over the frames (drqv2_amd.distract: VecDistract around the environment, one more
launch per step, INTEGRATION.md, "Distractions"): SPEC is easy, medium or hard, or a list such as
camera=4,color=32,background=noise (further: camera_period=K, alpha=A, dynamic=0|1); the key is the built-in tasks' own
background.  --distract-on train applies them to the training environment and the random baseline, eval to the evaluation
environment, both (the default) to all three: train-only and eval-only runs are the two halves of the DMControl-GB
protocol, whose difference from a clean run is the generalisation gap.  The distractor's state goes into the checkpoint
with the environment's.  Off by default, and the output is then unchanged.

--svea overlay|conv trains with a strong augmentation the SVEA way (drqv2_amd.augment, INTEGRATION.md, "Strong
augmentation (SVEA)"): every batch is drawn at half of --batch, materialised, and handed to the unchanged update() as
svea_batch(batch, strong) -- the clean rows and their strongly augmented copies, --batch rows in all.  overlay blends
with weight --svea-alpha an image of a procedurally made bank of --svea-bank images (noise_bank: nothing is shipped), conv
is the random convolution.  The augmenter's state goes into the checkpoint.  With --distract SPEC --distract-on eval this
is the DMControl-GB protocol with a method that is meant to close the gap.  Off by default, and the output is then unchanged.

This is a demonstration that the pieces run together and of what the agent does on this toy task in a few thousand
updates; it is no benchmark and makes no claim about DMC.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import drqv2  # noqa: E402
import utils  # noqa: E402
from drqv2_amd import checkpoint  # noqa: E402
from drqv2_amd.augment import RandomConv, RandomOverlay, noise_bank, svea_batch  # noqa: E402
from drqv2_amd.distract import FrameDistractor, VecDistract, parse_spec  # noqa: E402
from drqv2_amd.envs import VecCartpole, VecCatch, VecFinger, VecMaze, VecPointMass, VecReach, VecReacher, VecWalker  # noqa: E402
from drqv2_amd.evaluate import VecFrameStack, VecVideo, evaluate  # noqa: E402
from drqv2_amd.explore import KnnBonus, RandomFeatures, SimHashBonus  # noqa: E402
from drqv2_amd.replay import VecDeviceReplay, VecEpisodeStats, VecFrameReplay  # noqa: E402


TASKS = {"reach": (VecReach, {}), "pointmass": (VecPointMass, {}), "cartpole_balance": (VecCartpole, {"swing_up": False}),
         "cartpole_swingup": (VecCartpole, {"swing_up": True}), "reacher_easy": (VecReacher, {"target_radius": 0.15}),
         "reacher_hard": (VecReacher, {"target_radius": 0.05}), "maze": (VecMaze, {"size": 6}), "maze_small": (VecMaze, {"size": 4}),
         "catch": (VecCatch, {"cup_width": 0.3}), "catch_hard": (VecCatch, {"cup_width": 0.18}),
         "walker_stand": (VecWalker, {"speed": 0.0}), "walker_walk": (VecWalker, {"speed": VecWalker.WALK_SPEED}),
         "walker_run": (VecWalker, {"speed": VecWalker.RUN_SPEED}),
         "finger_spin": (VecFinger, {"task": "spin"}),
         "finger_turn_easy": (VecFinger, {"task": "turn", "target_radius": VecFinger.TURN_EASY_RADIUS}),
         "finger_turn_hard": (VecFinger, {"task": "turn", "target_radius": VecFinger.TURN_HARD_RADIUS})}
REWARDS = {None: {}, "sparse": {"sparse": True}, "dense": {"sparse": False}}       # --reward: the two forms of VecReacher, VecMaze, VecCatch and VecFinger


def make_env(args, seed, role="train"):
    """the environment of a role ("train": training and the random baseline; "eval"), distracted when --distract-on says so"""
    cls, more = TASKS[args.task]
    if cls is VecMaze:      # the pool of layouts: the evaluation's is another one under --maze-eval-layout-seed
        held_out = role == "eval" and args.maze_eval_layout_seed is not None
        more = dict(more, layouts=args.maze_layouts, loops=args.maze_loops, layout_seed=args.maze_eval_layout_seed if held_out else 0)
    env = cls(args.envs, "cuda", action_dim=args.action_dim, episode_length=args.episode_length, seed=seed,
              action_repeat=args.action_repeat, **more, **REWARDS[args.reward])
    if args.distract and args.distract_on in (role, "both"):
        env = VecDistract(env, FrameDistractor(args.envs, "cuda", seed=seed, key="env", **parse_spec(args.distract)))
    return env


class SveaBatches:
    """The iterator update() draws from under --svea: the store's batches, materialised and doubled by svea_batch().  The
    look-ahead stays the store iterator's own (prefetch), so a checkpoint saves it as it always did."""

    def __init__(self, it, strong):
        self.it, self.strong = it, strong

    def __iter__(self):
        return self

    def __next__(self):
        return svea_batch(next(self.it).materialize((9, 84, 84)), self.strong)

    def prefetch(self):
        self.it.prefetch()


def random_baseline(args, episodes):
    """mean return and length of the first `episodes` episodes under uniform-random actions: the same task, action
    repeat, N, length and seed"""
    N, A = args.envs, args.action_dim
    env = make_env(args, args.seed)
    stats = VecEpisodeStats(N, "cuda", log_size=max(1024, episodes + 64 * N))      # 100 more steps end at most 50 N more
    g = torch.Generator(device="cuda")
    g.manual_seed(args.seed)
    env.reset()
    stats.step(torch.zeros(N, device="cuda"))
    while True:
        for _ in range(100):
            _, reward, _, first = env.step(torch.rand(N, A, device="cuda", generator=g) * 2 - 1)
            stats.step(reward, first)
        snap = stats.read()
        if snap.episodes >= episodes:
            rec = snap.records[:episodes]                  # oldest first: the log is large enough to hold them all
            return float(rec["return"].mean()), float(rec["length"].mean()), snap.rows - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", choices=sorted(TASKS), default="reach")
    ap.add_argument("--reward", choices=("sparse", "dense"), default=None, help="the reward of the reacher, maze, catch and finger tasks (sparse)")
    ap.add_argument("--maze-layouts", type=int, default=0, metavar="K", help="the mazes come from a pool of K layouts (0: a fresh maze per episode)")
    ap.add_argument("--maze-loops", type=int, default=0, metavar="Q", help="open every remaining wall with probability Q / 256, 0 .. 255")
    ap.add_argument("--maze-eval-layout-seed", type=int, default=None, metavar="S",
                    help="evaluate on the pool of layout_seed S (training uses 0): held-out mazes")
    ap.add_argument("--action-repeat", type=int, default=1, metavar="K", help="simulator steps per action, 1 .. 16")
    ap.add_argument("--steps", type=int, default=20000, help="environment steps (each of all N environments)")
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--action-dim", type=int, default=None, help="columns of an action (what the task reads, at least 2)")
    ap.add_argument("--episode-length", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=1000, help="steps of uniform-random actions before the first update")
    ap.add_argument("--report", type=int, default=2000, help="steps per reporting interval")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=4096, help="rows of the ring (x N environments)")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--feature-dim", type=int, default=50)
    ap.add_argument("--hidden-dim", type=int, default=256)
    ap.add_argument("--stddev", default="linear(1.0,0.1,10000)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--checkpoint", default=None, metavar="PATH", help="the checkpoint file")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="STEPS", help="save every STEPS steps (0: never)")
    ap.add_argument("--resume", action="store_true", help="continue from the checkpoint file")
    ap.add_argument("--dormant-every", type=int, default=0, metavar="K",
                    help="print the actor's dormant ratio on the look-ahead batch every K updates (0: never)")
    ap.add_argument("--perturb-every", type=int, default=0, metavar="K",
                    help="every K updates pull the weights toward a fresh initialisation, by the dormant ratio (0: never)")
    ap.add_argument("--perturb-k", type=float, default=2.0, help="alpha = clip(1 - k * ratio, 0.2, 0.9)")
    ap.add_argument("--export-dir", default=None, metavar="DIR",
                    help="write the episodes finished since the last report as episode files at every reporting interval")
    ap.add_argument("--prefill-dir", default=None, metavar="DIR",
                    help="load a directory of episode files into the ring before the first reset row")
    ap.add_argument("--eval-every", type=int, default=0, metavar="STEPS", help="evaluate every STEPS steps (0: never)")
    ap.add_argument("--eval-episodes", type=int, default=1, metavar="K", help="episodes per environment of an evaluation")
    ap.add_argument("--video", default=None, metavar="DIR", help="write every evaluation as DIR/eval_<step>.png")
    ap.add_argument("--explore-beta", type=float, default=0.0, metavar="B",
                    help="add the exploration bonus B / sqrt(count of the frame's SimHash code) to the ring's reward (0: off)")
    ap.add_argument("--explore-bits", type=int, default=None, metavar="K", help="bits of the SimHash code, 1 .. 24 (16)")
    ap.add_argument("--explore-knn-beta", type=float, default=0.0, metavar="B",
                    help="add B * log1p(distance to the k-th nearest neighbour in random features) to every batch's reward (0: off)")
    ap.add_argument("--explore-knn-k", type=int, default=None, metavar="K", help="which neighbour, 1 .. 8 (3)")
    ap.add_argument("--explore-knn-candidates", type=int, default=None, metavar="M", help="look at about M rows of the ring (all)")
    ap.add_argument("--demos", default=None, metavar="DIR", help="episode files kept as demonstrations for the whole run")
    ap.add_argument("--demo-fraction", type=float, default=0.5, metavar="F", help="share of every batch drawn from them")
    ap.add_argument("--demo-rows", type=int, default=None, metavar="D", help="rows of the partition (what DIR needs)")
    ap.add_argument("--distract", default=None, metavar="SPEC",
                    help="visual distractions: easy|medium|hard, or e.g. camera=4,color=32,background=noise")
    ap.add_argument("--distract-on", choices=("train", "eval", "both"), default=None, help="which environments are distracted (both)")
    ap.add_argument("--svea", choices=("overlay", "conv"), default=None, help="train on svea_batch() of a strong augmentation")
    ap.add_argument("--svea-alpha", type=float, default=None, metavar="A", help="weight of the overlaid image, 0 .. 1 (0.5)")
    ap.add_argument("--svea-bank", type=int, default=None, metavar="M", help="images of the procedural overlay bank (64)")
    args = ap.parse_args()
    if args.action_dim is None:
        args.action_dim = max(2, getattr(TASKS[args.task][0], "_MIN_ACTION_DIM", 2))
    if args.reward and TASKS[args.task][0] not in (VecReacher, VecMaze, VecCatch, VecFinger):
        raise SystemExit("--reward needs --task reacher_easy, reacher_hard, maze, maze_small, catch, catch_hard or a finger task")
    if TASKS[args.task][0] is not VecMaze and (args.maze_layouts or args.maze_loops or args.maze_eval_layout_seed is not None):
        raise SystemExit("--maze-layouts, --maze-loops and --maze-eval-layout-seed need --task maze or maze_small")
    if not 0 <= args.maze_layouts <= VecMaze.MAX_LAYOUTS or not 0 <= args.maze_loops <= VecMaze.MAX_LOOPS:
        raise SystemExit(f"--maze-layouts is 0 .. {VecMaze.MAX_LAYOUTS}, --maze-loops 0 .. {VecMaze.MAX_LOOPS}")
    if args.maze_eval_layout_seed is not None and not (args.maze_layouts and args.eval_every):
        raise SystemExit("--maze-eval-layout-seed needs --maze-layouts K and --eval-every STEPS")
    if args.distract_on and not args.distract:
        raise SystemExit("--distract-on needs --distract SPEC")
    if args.distract:
        args.distract_on = args.distract_on or "both"
        try:
            parse_spec(args.distract)
        except ValueError as err:
            raise SystemExit(f"--distract: {err}")
        if args.distract_on == "eval" and not args.eval_every:
            raise SystemExit("--distract-on eval needs --eval-every STEPS")
    if args.svea != "overlay" and (args.svea_alpha is not None or args.svea_bank is not None):
        raise SystemExit("--svea-alpha and --svea-bank need --svea overlay")
    if args.svea and (args.batch < 2 or args.batch % 2):
        raise SystemExit("--svea doubles every batch: --batch must be even")
    if args.demos and (args.dormant_every or args.perturb_every or args.checkpoint):
        raise SystemExit("--demos does not combine with --dormant-every, --perturb-every or --checkpoint")
    if not args.demos and (args.demo_rows is not None or args.demo_fraction != 0.5):
        raise SystemExit("--demo-fraction and --demo-rows need --demos DIR")
    if args.explore_bits is not None and not args.explore_beta:
        raise SystemExit("--explore-bits needs --explore-beta B")
    if not args.explore_knn_beta and (args.explore_knn_k is not None or args.explore_knn_candidates is not None):
        raise SystemExit("--explore-knn-k and --explore-knn-candidates need --explore-knn-beta B")
    if args.explore_knn_beta and (args.explore_beta or args.prefill_dir):
        raise SystemExit("--explore-knn-beta does not combine with --explore-beta or --prefill-dir")
    if args.video and not args.eval_every:
        raise SystemExit("--video needs --eval-every STEPS")
    if (args.checkpoint_every or args.resume) and not args.checkpoint:
        raise SystemExit("--checkpoint-every and --resume need --checkpoint PATH")
    if not torch.cuda.is_available():
        raise SystemExit("vec_train_demo.py runs on the GPU: no device found")
    N, A = args.envs, args.action_dim
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)
    print(f"{args.task}{' (' + args.reward + ' reward)' if args.reward else ''}: N={N} environments, episode_length={args.episode_length}, action_repeat={args.action_repeat}, A={A}; "
          f"{args.steps} steps, warm-up {args.warmup}, "
          f"batch {args.batch}, lr {args.lr}, feature_dim {args.feature_dim}, hidden_dim {args.hidden_dim}, stddev "
          f"{args.stddev}, seed {args.seed}", flush=True)

    if args.distract:
        print(f"distractions on {args.distract_on}: {parse_spec(args.distract)}", flush=True)

    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", args.lr, args.feature_dim, args.hidden_dim, 0.01, args.warmup, 1,
                             args.stddev, 0.3, False)
    env = make_env(args, args.seed)
    if args.demos:
        import replay_buffer
        from drqv2_amd.episodes import plan_fill
        need = plan_fill([n for _, _, n in replay_buffer._episode_files(args.demos)], N).L
        store = VecDeviceReplay(rows=args.rows, num_envs=N, obs_shape=(9, 84, 84), action_dim=A, nstep=3, discount=0.99,
                                device="cuda", seed=args.seed, demo_rows=args.demo_rows or max(need, 5))
        fill = store.add_demonstrations(args.demos)
        store.demo_fraction = args.demo_fraction
        print(f"demonstrations from {args.demos}: {fill.episodes} episodes, {fill.transitions} transitions in {fill.rows} of "
              f"{store.D} rows ({fill.pad_rows} pad rows); {store.demo_count(args.batch)} of every {args.batch} batch rows",
              flush=True)
        # the ring holds whole observations: the stack is put together in front of add(), and act_batch() reads it there
        stack = VecFrameStack(N, "cuda")
        add_row = lambda frame, action, reward, discount, first: store.add(stack.push(frame, first), action, reward, discount, first)
        observe = stack.observation
    else:
        store = VecFrameReplay(rows=args.rows, num_envs=N, action_dim=A, nstep=3, discount=0.99, device="cuda", seed=args.seed)
        add_row, observe = store.add, store.observation
    # under --svea the store draws half a batch: update() sees --batch rows, the clean half and the augmented half
    store.batch_size = args.batch // 2 if args.svea else args.batch
    stats = VecEpisodeStats(N, "cuda", log_size=max(1024, 2 * N * args.report))
    it = iter(store)
    strong, batches = None, it
    if args.svea:
        try:
            strong = RandomConv("cuda", seed=args.seed) if args.svea == "conv" else RandomOverlay(
                noise_bank(64 if args.svea_bank is None else args.svea_bank, seed=args.seed),
                alpha=0.5 if args.svea_alpha is None else args.svea_alpha, device="cuda", seed=args.seed)
        except ValueError as err:
            raise SystemExit(f"--svea: {err}")
        batches = SveaBatches(it, strong)      # (its inner iterator becomes the k-NN bonus's below, when there is one)
        print(f"svea: {args.svea}" + (f", alpha_q8 {strong.alpha_q8}, a bank of {strong.M} images" if args.svea == "overlay" else "")
              + f"; batches of {store.batch_size} drawn, {args.batch} rows per update", flush=True)
    bonus = SimHashBonus(N, "cuda", bits=args.explore_bits or 16, beta=args.explore_beta, seed=args.seed) \
        if args.explore_beta else None
    if bonus is not None:
        print(f"exploration bonus: beta {bonus.beta}, {bonus.bits} bits", flush=True)
    knn = features = None
    if args.explore_knn_beta:
        try:
            knn = KnnBonus(store, dim=50, k=args.explore_knn_k or 3, beta=args.explore_knn_beta,
                           candidates=args.explore_knn_candidates, seed=args.seed)
        except ValueError as err:
            raise SystemExit(f"--explore-knn-beta: {err}")
        features = RandomFeatures((9, 84, 84), 50, "cuda", seed=args.seed)
        # the bonus is applied when a batch is handed out; the look-ahead stays the store iterator's own
        if strong is not None:
            batches.it = knn.batches(it)
        else:
            batches = knn.batches(it)
        print(f"k-NN bonus: beta {knn.beta}, k {knn.k}, candidates {knn.candidates or 'all'}, {knn.dim} random features", flush=True)
        plain_add = add_row

        def add_row(*row):
            plain_add(*row)
            knn.observe(features(observe()))
    zeros_NA, zeros_N, ones_N = torch.zeros(N, A, device="cuda"), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")

    if args.eval_every:
        K = args.eval_episodes
        eval_env = make_env(args, args.seed + 1, "eval")
        eval_stats = VecEpisodeStats(N, "cuda", log_size=max(1024, K * N), max_episodes_per_env=K)
        eval_stack, video = VecFrameStack(N, "cuda"), None
        if args.video:
            os.makedirs(args.video, exist_ok=True)
            video = VecVideo(N, "cuda", max_frames=K * (args.episode_length + 1) + 51)    # evaluate()'s max_steps, and row 0

    start, logged, updates, export_from = 0, 0, 0, None
    last_train = last_eval = None      # the newest interval's mean training return and the newest evaluation's, for the maze's report
    if args.resume:
        extra = checkpoint.load(args.checkpoint, agent=agent, store=store, iterator=it, env=env, stats=stats, bonus=bonus or knn)
        start, logged, updates, export_from = extra["step"], extra["logged"], extra["updates"], extra.get("export_from")
        if strong is not None:
            if not isinstance(extra.get("svea"), dict):
                raise SystemExit(f"--resume: {args.checkpoint} was saved without --svea")
            strong.load_state_dict(extra["svea"])
        print(f"resumed {args.checkpoint} at step {start}", flush=True)
    else:
        if args.prefill_dir:
            fill = store.add_episodes(args.prefill_dir)
            print(f"prefilled from {args.prefill_dir}: {fill.episodes} episodes, {fill.transitions} transitions in "
                  f"{fill.rows} rows ({fill.pad_rows} pad rows)", flush=True)
            # the prefilled episodes are on disk already: exports start behind the reset row below, which closes the
            # last of them (row T; an episode is listed when the row after its end is start_row or later)
            export_from = store.T + 1
        frame = env.reset()
        # the reset row of every environment, flagged as one: only row 0 of an empty ring is a reset row by itself, and
        # after a prefill this row must not continue the prefilled episodes
        add_row(frame, zeros_NA, zeros_N, ones_N, torch.ones(N, dtype=torch.uint8, device="cuda"))
        stats.step(zeros_N)
    t0 = time.perf_counter()
    for step in range(start, args.steps):
        action = agent.act_batch(observe(), step, False)             # [N, A], stays on the device
        frame, reward, discount, first = env.step(action)
        # the ring learns from reward + bonus; the statistics keep the environment's own reward
        add_row(frame, action, reward if bonus is None else bonus.step(frame, reward), discount, first)
        stats.step(reward, first)
        if step >= args.warmup:
            agent.update(batches, step)
            updates += 1
            show = args.dormant_every and updates % args.dormant_every == 0
            pull = args.perturb_every and updates % args.perturb_every == 0
            if show or pull:                                         # DrM's two primitives; these lines WAIT
                batch = it.peek()                                    # the batch the next update trains on
                ratio = float(agent.dormant_ratio(batch.stacks(batch[0]).view(-1, 9, 84, 84)))
                if show:
                    print(f"step {step + 1:6d}  updates {updates:6d}  dormant ratio (actor) {ratio:.4f}", flush=True)
                if pull:
                    alpha = utils.perturb_factor(ratio, args.perturb_k, 0.2, 0.9)
                    agent.perturb(alpha)
                    print(f"step {step + 1:6d}  updates {updates:6d}  perturbed with alpha {alpha:.3f} (dormant ratio "
                          f"{ratio:.4f})", flush=True)
        if (step + 1) % args.report == 0:
            snap = stats.read()                                      # the one wait per interval
            new, missed = snap.since(logged)
            logged = snap.episodes
            mean = f"{new['return'].mean():7.3f}" if len(new) else "    n/a"
            last_train = float(new["return"].mean()) if len(new) else last_train
            length = f"{new['length'].mean():5.1f}" if len(new) else "  n/a"
            print(f"step {step + 1:6d}  updates {updates:6d}  episodes {snap.episodes:6d} (+{len(new) + missed})  mean return "
                  f"{mean}  mean length {length}  return per step "
                  f"{(new['return'].sum() / max(1, new['length'].sum())):.3f}  [{time.perf_counter() - t0:.1f} s]"
                  + ("" if bonus is None else f"  distinct codes {int(bonus.distinct())}")
                  + ("" if knn is None or knn.last_dist is None else f"  mean k-NN distance {float(knn.last_dist.mean()):.4f}"),
                  flush=True)
            if args.export_dir:                                      # this WAITS as well
                rep = store.export_episodes(args.export_dir, start_row=export_from)
                export_from = rep.next_row
                print(f"step {step + 1:6d}  exported {rep.episodes} episodes ({rep.transitions} transitions) to "
                      f"{args.export_dir}; left out: {rep.open} open, {rep.headless} headless, {rep.zero_length} zero-length",
                      flush=True)
        if args.eval_every and (step + 1) % args.eval_every == 0:    # between two training steps: this WAITS, once per 50 steps
            if video is not None:
                video.clear()
            te = time.perf_counter()
            res = evaluate(agent, eval_env, K, step, stats=eval_stats, stack=eval_stack, video=video)
            rec = res.snapshot.records
            last_eval = res.snapshot.mean_return
            print(f"step {step + 1:6d}  eval: {res.snapshot.episodes} episodes ({K} per environment) in {res.steps} steps: mean "
                  f"return {res.snapshot.mean_return:7.3f}  min {res.snapshot.min_return:7.3f}  max "
                  f"{res.snapshot.max_return:7.3f}  mean length {rec['length'].mean():5.1f}  "
                  f"[{time.perf_counter() - te:.2f} s]", flush=True)
            if video is not None:
                path = os.path.join(args.video, f"eval_{step + 1}.png")
                ts = time.perf_counter()
                size = video.save(path)
                print(f"step {step + 1:6d}  eval: {len(video)} images of {video.image_shape[1]} x {video.image_shape[0]} -> {path} "
                      f"({size / 1e6:.2f} MB) [save {time.perf_counter() - ts:.2f} s]", flush=True)
        if args.checkpoint_every and (step + 1) % args.checkpoint_every == 0:    # the end of an iteration: this WAITS
            checkpoint.save(args.checkpoint, agent=agent, store=store, iterator=it, env=env, stats=stats, bonus=bonus or knn,
                            extra=dict({"step": step + 1, "logged": logged, "updates": updates, "export_from": export_from},
                                       **({} if strong is None else {"svea": strong.state_dict()})))
    snap = stats.read()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    print(f"trained: {snap.episodes} episodes in {snap.rows - 1} steps x {N} environments, mean return over all of them "
          f"{snap.mean_return:.3f}, mean length {snap.mean_length:.1f}; {wall:.1f} s, {1e3 * wall / max(1, args.steps - start):.2f} ms per step",
          flush=True)
    if args.maze_eval_layout_seed is not None and last_train is not None and last_eval is not None:
        print(f"maze: {args.maze_layouts} training layouts (layout_seed 0): mean return of the last interval {last_train:.3f}; "
              f"held-out layouts (layout_seed {args.maze_eval_layout_seed}): mean return of the last evaluation {last_eval:.3f}", flush=True)
    b_ret, b_len, b_steps = random_baseline(args, snap.episodes)
    print(f"baseline: uniform-random actions, the first {snap.episodes} episodes ({b_steps} steps): mean return {b_ret:.3f}, "
          f"mean length {b_len:.1f}, return per step {b_ret / b_len:.3f}", flush=True)


if __name__ == "__main__":
    main()
