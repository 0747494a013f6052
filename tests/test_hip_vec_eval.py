"""Evaluation for the vectorised loop on the GPU: drq_vec_stack_push / drq_vec_video_record, VecFrameStack, VecVideo and
evaluate() against the numpy restatement (tests/vec_eval_oracle.py), against the single-frame ring's observation(), and
against the hand-written evaluation loop of INTEGRATION.md ("Episode statistics").

Bounds.  Everything is compared bit for bit: both kernels copy, replicate, transpose and shift bytes, and the runner adds
nothing to what VecReach, act_batch() and VecEpisodeStats compute -- it only fixes their order.

Poison.  The stacks and the clip are allocated through drqv2_amd.ops._alloc, which the autouse fixture turns into
sentinel-filled, guard-banded memory; the C-level calls allocate theirs from tests/poison.py directly.  Random frames
never hold the byte sentinel 0xA5 (it is replaced by 0xA4), a dimmed byte is at most 63 and an empty tile 0, so an
output that equals the oracle has been written in every byte, and check() finds the guard bands untouched.

Shapes.  N = 1 and N = 5 for the stack (one workgroup row, an odd number of them); N = 5 frames and every k = 1 .. 4 for the
mosaic: a tile row of 252 k bytes is a multiple of 16 only for k = 4, and the grids put seams between tiles (2 x 2, 1 x 3),
an empty tile (M = 3 in 2 x 2) and a permuted table inside 16-byte pieces.  The mosaic is also written at addresses that
are 4 and 1 bytes past a 16-byte boundary: the two narrower store widths."""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_env_oracle as E
from tests import vec_eval_oracle as EO
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p, rs_

pytestmark = pytest.mark.gpu
U8 = poison.sentinel_of(torch.uint8)
DONE = np.array([0, 1, 2, 0, 5], np.int32)
CASES = (((1, 1), [0]), ((2, 2), [0, 1, 2]), ((2, 2), [4, 0, 3, 1]), ((1, 3), [0, 1, 2]))       # (grid, envs)


@pytest.fixture(scope="module")
def lib():
    from drqv2_amd import _lib
    assert torch.cuda.is_available()
    assert "drq_vec_stack_push" in _lib.PROTOTYPES and "drq_vec_video_record" in _lib.PROTOTYPES, \
        "the evaluation entries are missing"
    return _lib.load()


def frames_of(seed, N, rows=1):
    """random frames uint8 [rows, N, 3, 84, 84] without the byte sentinel"""
    f = rs_(seed).randint(0, 256, (rows, N, 3, 84, 84)).astype(np.uint8)
    f[f == U8] = U8 - 1
    return f


@pytest.fixture(scope="module")
def five():
    """the N = 5 frames of the mosaic tests, and the mosaics of every (k, case, limit), computed once and never modified"""
    frame = frames_of(21, 5)[0]
    want = {(k, c, limit): EO.mosaic(frame, envs, grid, k, DONE, limit)
            for k in (1, 2, 3, 4) for c, (grid, envs) in enumerate(CASES) for limit in (0, 1, 2)}
    return frame, want


def same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == np.ascontiguousarray(want).tobytes(), what


# ------------------------------------------------------------------------------------------------ push
@pytest.mark.parametrize("N", [1, 5])
def test_push_matches_the_oracle(lib, N):
    """six calls: flags all zero on call 0 (it must reset all the same), none, one environment, the same one again (two
    resets in a row), all, none.  After every call the returned stacks equal the oracle's, the stacks of the call before
    are what they were (two buffers in turn), observation() is the return; then the entry alone into fresh poison"""
    from drqv2_amd.evaluate import VecFrameStack
    fr = frames_of(N, N, 6)
    one = np.zeros(N, np.uint8)
    one[N - 1] = 1
    flags = [np.zeros(N, np.uint8), None, one, one, np.ones(N, np.uint8), None]
    stack, oracle = VecFrameStack(N, "cuda"), EO.StackOracle(N)
    kept, wants = [], []
    for t in range(6):
        first = None if flags[t] is None else torch.from_numpy(flags[t]).cuda()
        out = stack.push(torch.from_numpy(fr[t]).cuda(), first)
        wants.append(oracle.push(fr[t], flags[t]).copy())
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (N, 9, 84, 84)
        same(out, wants[t], (t, "stacks"))
        assert stack.observation() is out
        kept.append(out)
        if t >= 1:
            same(kept[t - 1], wants[t - 1], (t, "the stacks of the call before"))
            assert kept[t - 1].data_ptr() != out.data_ptr()
        if t >= 2:
            assert kept[t - 2].data_ptr() == out.data_ptr()
        poison.check()
    stack.reset()                                                          # the next push resets whatever the flags say
    same(stack.push(torch.from_numpy(fr[0]).cuda(), torch.zeros(N, dtype=torch.bool, device="cuda")),
         EO.stack_push(None, fr[0], reset_all=True), "after reset()")
    # numpy inputs are staged
    same(stack.push(fr[1], flags[2]), EO.stack_push(EO.stack_push(None, fr[0], reset_all=True), fr[1], flags[2]), "host inputs")

    # the entry: prev NULL with reset_all, then flags, then first = NULL
    prev = None
    for t, (first, reset_all) in enumerate(((None, 1), (one, 0), (None, 0))):
        nxt = poison.alloc((N, 9, 84, 84), torch.uint8, "cuda", name="next")
        frame, fl = dev(torch.from_numpy(fr[t]), "frame"), None if first is None else dev(torch.from_numpy(first), "first")
        keep = None if prev is None else prev.clone()
        assert lib.drq_vec_stack_push(p(prev), p(nxt), p(frame), p(fl), N, reset_all, None) == 0
        want = EO.stack_push(None if prev is None else keep.cpu().numpy(), fr[t], first, bool(reset_all))
        same(nxt, want, (t, "entry"))
        assert not (nxt.cpu().numpy() == U8).any()
        if prev is not None:
            assert torch.equal(prev, keep)
        prev = nxt
        poison.check()


def test_push_equals_the_rings_observation():
    """12 steps of a VecReach whose resets stagger, the same frames into a VecFrameReplay and a VecFrameStack: after every
    row observation() == push(), bit for bit"""
    from drqv2_amd.envs import VecReach
    from drqv2_amd.evaluate import VecFrameStack
    from drqv2_amd.replay import VecFrameReplay
    N, A = 3, 2
    env = VecReach(N, "cuda", action_dim=A, episode_length=3, seed=1)
    twin = E.ReachOracle(N, episode_length=3, seed=1)                       # the environment in numpy: it names the actions
    twin.reset()
    ring, stack = VecFrameReplay(16, N, A, 3, 0.99, "cuda", seed=1), VecFrameStack(N, "cuda")
    frame = env.reset()
    ring.add(frame, torch.zeros(N, A, device="cuda"), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"))
    assert torch.equal(ring.observation(), stack.push(frame))
    resets = []
    for s in range(12):
        aim = ((twin.target - twin.pos) / np.float32(0.1)).astype(np.float32)   # every environment heads for its target:
        twin.step(aim)                                                          # those that start near it end early
        action = torch.from_numpy(aim).cuda()
        frame, reward, discount, first = env.step(action)
        ring.add(frame, action, reward, discount, first)
        assert torch.equal(ring.observation(), stack.push(frame, first)), s
        resets.append(first.cpu().numpy().copy())
    resets = np.stack(resets)
    assert resets.any(axis=0).all(), "every environment must have been reset"
    assert len({tuple(np.flatnonzero(resets[:, e])) for e in range(N)}) > 1, "the resets must stagger"


# ------------------------------------------------------------------------------------------------ argument errors
def test_entries_refuse_bad_arguments_and_launch_nothing(lib):
    N = 2
    buf = poison.alloc((3 * N, 9, 84, 84), torch.uint8, "cuda", name="stacks", kind="refused")
    frame = dev(torch.from_numpy(frames_of(1, N)[0]), "frame")
    base = buf.data_ptr()
    assert lib.drq_vec_stack_push(base, base, p(frame), None, N, 0, None) == -1                  # the same buffer
    assert lib.drq_vec_stack_push(base, base + 16, p(frame), None, N, 0, None) == -1             # overlapping
    assert lib.drq_vec_stack_push(base + 63504, base, p(frame), None, N, 0, None) == -1          # by one environment
    assert lib.drq_vec_stack_push(base, p(buf[N:]), p(frame), None, 0, 0, None) == -1            # N = 0
    assert lib.drq_vec_stack_push(None, p(buf[N:]), p(frame), None, N, 0, None) == -1            # no prev, no reset_all
    assert lib.drq_vec_stack_push(base, p(buf[N:]), None, None, N, 0, None) == -1
    assert lib.drq_vec_stack_push(base, None, p(frame), None, N, 0, None) == -1
    out = poison.alloc((2 * 336, 2 * 336, 3), torch.uint8, "cuda", name="image", kind="refused")
    envs = dev(torch.arange(N, dtype=torch.int32), "envs")
    for k in (0, 5):
        assert lib.drq_vec_video_record(p(frame), p(envs), N, None, 0, p(out), 2, 2, k, N, None) == -1
    assert lib.drq_vec_video_record(p(frame), p(envs), 5, None, 0, p(out), 2, 2, 1, N, None) == -1   # M > GH GW
    assert lib.drq_vec_video_record(p(frame), p(envs), 0, None, 0, p(out), 2, 2, 1, N, None) == -1   # M < 1
    for args in ((None, p(envs), p(out)), (p(frame), None, p(out)), (p(frame), p(envs), None)):
        assert lib.drq_vec_video_record(args[0], args[1], N, None, 0, args[2], 2, 2, 1, N, None) == -1
    poison.check()                                                          # "refused": every byte is still poison


# ------------------------------------------------------------------------------------------------ record
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_record_matches_the_oracle_on_a_poisoned_clip(five, k):
    """VecVideo.record() for the four grids and limit 0, 1, 2 with done = [0, 1, 2, 0, 5]: image 0 equals the oracle, image 1
    still holds the sentinel"""
    from drqv2_amd.evaluate import VecVideo
    frame, want = five
    dframe, done = torch.from_numpy(frame).cuda(), torch.from_numpy(DONE).cuda()
    for c, (grid, envs) in enumerate(CASES):
        video = VecVideo(5, "cuda", envs=envs, grid=grid, scale=k, max_frames=2)
        for limit in (0, 1, 2):
            video.clear()
            video.record(dframe, done, limit)
            assert len(video) == 1 and video.dropped == 0 and tuple(video.clip().shape) == (1,) + want[k, c, limit].shape
            same(video.clip()[0], want[k, c, limit], (k, grid, envs, limit))
            assert bool((video.buffer[1] == U8).all()), "the image after the recorded one was written"
        if c == 1:
            assert not want[k, c, 0][84 * k:, 84 * k:].any()               # the empty tile of M = 3 in 2 x 2
            assert (want[k, c, 2] != want[k, c, 0]).any() and (want[k, c, 1] != want[k, c, 2]).any()
        video.clear()
        video.record(dframe)                                                # no counters: never dimmed
        same(video.clip()[0], want[k, c, 0], (k, grid, envs, "done=None"))
        poison.check()


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_record_chooses_the_store_width_from_the_address(lib, five, k):
    """the entry into an image that starts 0, 4 and 1 bytes behind a 16-byte boundary: pieces of 16, 4 and 1 bytes.  The
    bytes in front of and behind the image keep the sentinel"""
    frame, want = five
    grid, envs = CASES[1]
    w = want[k, 1, 2]
    dframe, done = dev(torch.from_numpy(frame), "frame"), dev(torch.from_numpy(DONE), "done")
    table = dev(torch.tensor(envs, dtype=torch.int32), "envs")
    for off in (0, 4, 1):
        flat = poison.alloc(w.size + 32, torch.uint8, "cuda", name=f"image+{off}")
        out = flat[off:off + w.size]
        assert out.data_ptr() % 16 == off
        assert lib.drq_vec_video_record(p(dframe), p(table), len(envs), p(done), 2, p(out), grid[0], grid[1], k, 5, None) == 0
        same(out.view(w.shape), w, (k, off))
        host = flat.cpu().numpy()
        assert (host[:off] == U8).all() and (host[off + w.size:] == U8).all(), (k, off)
    poison.check()


def test_a_full_clip_drops_frames_and_launches_nothing(five):
    from drqv2_amd.evaluate import VecVideo
    frame, want = five
    grid, envs = CASES[2]
    video = VecVideo(5, "cuda", envs=envs, grid=grid, scale=1, max_frames=2)
    other = frame[:, :, ::-1].copy()
    for f in (frame, other, frame):
        video.record(torch.from_numpy(f).cuda())
    assert len(video) == 2 and video.dropped == 1 and tuple(video.clip().shape) == (2, 168, 168, 3)
    same(video.clip()[0], want[1, 2, 0], "image 0")
    same(video.clip()[1], EO.mosaic(other, envs, grid, 1), "image 1")
    poison.check()                                                          # a third image would lie in the guard band
    video.clear()
    assert len(video) == 0 and video.dropped == 0


def test_save_writes_npy_and_an_animated_png(five, tmp_path):
    from drqv2_amd import _lib
    from drqv2_amd.evaluate import VecVideo, read_apng
    frame, want = five
    grid, envs = CASES[3]
    video = VecVideo(5, "cuda", envs=envs, grid=grid, scale=2, max_frames=4)
    with pytest.raises(_lib.DrqError):
        video.save(str(tmp_path / "empty.png"))
    done = torch.from_numpy(DONE).cuda()
    for limit in (0, 1, 2):
        video.record(torch.from_numpy(frame).cuda(), done, limit)
    clip = np.stack([want[2, 3, limit] for limit in (0, 1, 2)])
    video.save(str(tmp_path / "clip.png"), fps=10)
    video.save(str(tmp_path / "clip.npy"))
    back, fps = read_apng(str(tmp_path / "clip.png"))
    assert fps == 10
    same(back, clip, "png")
    same(np.load(str(tmp_path / "clip.npy")), clip, "npy")


# ------------------------------------------------------------------------------------------------ evaluate()
def small_agent(A=2):
    import drqv2
    return drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)


def test_evaluate_equals_the_hand_written_loop():
    """evaluate() on VecReach(3, episode_length 5, seed 7), two episodes per environment, polled every 4 steps, against the
    eval_store loop of INTEGRATION.md on a second environment of the same seed with the same agent: the same records,
    and the clip is the mosaic oracle of that loop's frames and closed-episode counters"""
    from drqv2_amd import _lib
    from drqv2_amd.envs import VecReach
    from drqv2_amd.evaluate import VecVideo, evaluate
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    N, A, K, POLL, STEP = 3, 2, 2, 4, 100
    torch.manual_seed(3)
    agent = small_agent(A)
    video = VecVideo(N, "cuda", scale=1, max_frames=64)
    res = evaluate(agent, VecReach(N, "cuda", action_dim=A, episode_length=5, seed=7), episodes_per_env=K, step=STEP,
                   video=video, poll_every=POLL)
    assert res.snapshot.complete and res.snapshot.episodes == K * N
    assert res.steps % POLL == 0 and res.frames == res.steps + 1 == len(video) and video.dropped == 0

    sim = VecReach(N, "cuda", action_dim=A, episode_length=5, seed=7)
    stats = VecEpisodeStats(num_envs=N, device="cuda", max_episodes_per_env=K)
    eval_store = VecFrameReplay(16, N, A, 3, 0.99, "cuda", seed=1)
    order = EO.EvalOrder(N, video.envs, video.grid, 1, K)
    zeros_N = torch.zeros(N, device="cuda")
    frame = sim.reset()
    eval_store.add(frame, torch.zeros(N, A, device="cuda"), zeros_N, torch.ones(N, device="cuda"))
    stats.step(zeros_N)
    order.row(frame.cpu().numpy())
    steps = 0
    while True:
        for _ in range(POLL):
            action = agent.act_batch(eval_store.observation(), STEP, eval_mode=True)
            frame, reward, discount, first = sim.step(action)
            eval_store.add(frame, action, reward, discount, first)
            stats.step(reward, first)
            order.row(frame.cpu().numpy(), first.cpu().numpy())
            steps += 1
        snap = stats.read()
        if snap.complete:
            break
        assert steps < 64
    assert steps == res.steps
    assert res.snapshot.records.tobytes() == snap.records.tobytes() and len(snap.records) == K * N
    assert res.snapshot.return_sum == snap.return_sum and res.snapshot.length_sum == snap.length_sum
    same(stats.episodes_done, order.done, "the closed-episode counters")
    assert (order.dones[-1] >= K).all() and (order.dones[0] == 0).all()
    same(video.clip(), np.stack(order.clip), "the clip")
    # the last frame of a counted episode is recorded as it is, the first frame of the next one dimmed
    row = next(t for t in range(len(order.dones)) if (order.dones[t] >= K).any())
    e = int(np.flatnonzero(order.dones[row] >= K)[0])
    gy, gx = divmod(e, video.grid[1])
    tile = lambda t: video.clip()[t, 84 * gy:84 * (gy + 1), 84 * gx:84 * (gx + 1)].permute(2, 0, 1).cpu().numpy()
    assert np.array_equal(tile(row), order.frames[row][e] >> 2) and np.array_equal(tile(row - 1), order.frames[row - 1][e])

    with pytest.raises(_lib.DrqError):
        evaluate(agent, VecReach(N, "cuda", action_dim=A, episode_length=5, seed=7), episodes_per_env=K, poll_every=POLL,
                 max_steps=3)
    # objects kept around serve the next evaluation: the statistics are reset, the stack starts over
    again = evaluate(agent, VecReach(N, "cuda", action_dim=A, episode_length=5, seed=7), episodes_per_env=K, step=STEP,
                     stats=stats, poll_every=POLL)
    assert again.snapshot.records.tobytes() == snap.records.tobytes() and again.frames == 0


def training_run(with_eval):
    """the 24-step loop of tests/test_hip_vec_env.py at its shapes; with_eval: evaluate() on a separate VecReach after
    steps 8 and 16.  Returns everything an evaluation could have disturbed, as host bytes"""
    import drqv2
    from drqv2_amd.envs import VecReach
    from drqv2_amd.evaluate import VecVideo, evaluate
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    N, A, EL, ROWS, T, B = 8, 2, 6, 32, 24, 16
    torch.manual_seed(5)
    torch.cuda.manual_seed_all(5)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 20, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = VecReach(N, "cuda", action_dim=A, episode_length=EL, seed=3)
    store = VecFrameReplay(ROWS, N, A, 3, 0.99, "cuda", seed=2)
    store.batch_size = B
    stats = VecEpisodeStats(N, "cuda")
    it = iter(store)
    zeros = torch.zeros(N, device="cuda")
    store.add(env.reset(), torch.zeros(N, A, device="cuda"), zeros, torch.ones(N, device="cuda"))
    stats.step(zeros)
    evals = []
    for step in range(T):
        action = agent.act_batch(store.observation(), step, False)
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, reward, discount, first)
        stats.step(reward, first)
        lo, hi = store.bounds()
        if hi >= lo:
            agent.update(it, step)
        if with_eval and step + 1 in (8, 16):
            evals.append(evaluate(agent, VecReach(3, "cuda", action_dim=A, episode_length=5, seed=7), episodes_per_env=1,
                                  step=step, video=VecVideo(3, "cuda", scale=1, max_frames=16), poll_every=4))
    torch.cuda.synchronize()
    out = {"rng_cpu": torch.get_rng_state().numpy().tobytes(), "rng_cuda": torch.cuda.get_rng_state().numpy().tobytes(),
           "T": store.T, "episodes": stats.read().records.tobytes()}
    for name in ("encoder", "actor", "critic", "critic_target"):
        for key, v in getattr(agent, name).state_dict().items():
            out[f"{name}.{key}"] = v.detach().cpu().numpy().tobytes()
    for name in ("frames", "action", "reward", "discount", "first"):
        out[f"ring.{name}"] = getattr(store, name).cpu().numpy().tobytes()
    for key, v in env.state().items():
        out[f"env.{key}"] = v.tobytes()
    return out, evals


def test_training_is_undisturbed_by_evaluations_in_between():
    plain, _ = training_run(False)
    mixed, evals = training_run(True)
    assert len(evals) == 2 and all(r.snapshot.complete and r.snapshot.episodes == 3 for r in evals)
    assert plain.keys() == mixed.keys()
    for key in plain:
        assert plain[key] == mixed[key], key
