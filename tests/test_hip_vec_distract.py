"""Distractions on the GPU: drq_vec_distract raw on poisoned, guard-banded memory, and drqv2_amd.distract (FrameDistractor,
VecDistract) against the numpy restatement tests/vec_distract_oracle.py, through render(), image(), state dicts, a
checkpoint file, evaluate() and the collection loop.

Bounds.  Everything is compared bit for bit: the contract is integer arithmetic throughout.

Shapes.  N = 1 and 3 (more than one workgroup; a frame is 441 pieces of 16 pixels over 256 lanes, so every launch runs a
full and a partial round), 40 steps with staggered first flags -- three episodes per lane -- at both ends of every
strength: camera 8 at period 1, colour 128 on frames that hold 0 and 255, noise that drifts below zero on both axes, a
bank of 2 clips of 3 frames that reverses within the run, alpha 0, 77 and 256, dynamic on and off, with and without a
key (vec_distract_oracle.SCENARIOS).  The oracle's runs are made once, shared and never modified; that they take every
branch is asserted without a GPU by tests/test_cpu_vec_distract.py and again here."""
import numpy as np
import pytest
import torch

from tests import poison
from tests import vec_distract_oracle as O
from tests.poison import poisoned_ops  # noqa: F401  (autouse: poisoned allocations, check() after every test)
from tests.test_hip_entries import dev, p
from tests.vec_env_checks import lib_fixture, same_bits, same_state

pytestmark = pytest.mark.gpu
MODES = ("none", "noise", "bank")
lib = lib_fixture("drq_vec_distract", "the distraction entry is missing")


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def scalars(run):
    """the scalar arguments of the entry behind `seed` for a run: reset_all and hold are the caller's"""
    kw = dict(dict(camera=0, camera_period=4, color=0, bg_mode=0, bg_alpha=256, dynamic=True), **run["kwargs"])
    M, F = (0, 0) if run["bank"] is None else run["bank"].shape[:2]
    return lambda reset_all, hold: (O.SEED, int(reset_all), int(hold), kw["camera"], kw["camera_period"], kw["color"],
                                    kw["bg_mode"], kw["bg_alpha"], int(kw["dynamic"]), int(M), int(F))


def distractor_of(run, N=None, seed=O.SEED, key="own", bank="own"):
    """the FrameDistractor of a scenario's configuration"""
    from drqv2_amd.distract import FrameDistractor
    kw = dict(run["kwargs"])
    mode = kw.pop("bg_mode", 0)
    key = run["key"] if isinstance(key, str) else key
    bank = run["bank"] if isinstance(bank, str) else bank
    background = torch.from_numpy(bank).cuda() if mode == 2 else MODES[mode]
    return FrameDistractor(N or run["N"], "cuda", seed=seed, background=background, background_alpha=kw.pop("bg_alpha", 256),
                           key=None if key is None else torch.from_numpy(key).cuda(), **kw)


# ------------------------------------------------------------------------------------------------ the entry on poisoned memory
@pytest.mark.parametrize("name", list(O.SCENARIOS))
def test_entry_matches_the_oracle_bit_for_bit_and_writes_nothing_else(lib, name):
    """40 calls into fresh poisoned outputs from guard-banded inputs: the frame and the two state words equal the oracle's
    after every call; a hold call beside each draws the same frame and leaves the state alone; check() finds every guard
    band untouched"""
    fresh = O.DistractOracle(1)
    with pytest.raises(AssertionError, match="never took"):                # it can fail: nothing has been drawn
        fresh.require_branches()
    run = O.run_of(name)
    N, args = run["N"], scalars(run)
    key = None if run["key"] is None else dev(torch.from_numpy(run["key"]), "key")
    bank = None if run["bank"] is None else dev(torch.from_numpy(run["bank"]), "bank")
    episode, t = dev(torch.zeros(N, dtype=torch.int32), "episode"), dev(torch.zeros(N, dtype=torch.int32), "t")
    for s in range(O.STEPS):
        frame = dev(torch.from_numpy(run["frames"][s]), "frame_in")
        first = None if run["firsts"][s] is None else dev(torch.from_numpy(run["firsts"][s]), "first")
        out = poison.alloc((N,) + O.FRAME, torch.uint8, "cuda", name="frame_out")
        assert lib.drq_vec_distract(p(frame), p(first), p(key), p(bank), p(episode), p(t), N, *args(s == 0, 0), p(out), None) == 0
        same_bits(out.cpu().numpy(), run["outs"][s], (name, s, "frame"))
        same_bits(u32(episode), run["states"][s][0], (name, s, "episode"))
        same_bits(u32(t), run["states"][s][1], (name, s, "t"))
        if s % 4 == 0:
            again = poison.alloc((N,) + O.FRAME, torch.uint8, "cuda", name="held")
            assert lib.drq_vec_distract(p(frame), None, p(key), p(bank), p(episode), p(t), N, *args(0, 1), p(again), None) == 0
            same_bits(again.cpu().numpy(), run["outs"][s], (name, s, "hold"))
            same_bits(u32(t), run["states"][s][1], (name, s, "t after hold"))
            same_bits(u32(episode), run["states"][s][0], (name, s, "episode after hold"))
        poison.check()
    if name in O.IDENTITY:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(run["frames"], run["outs"]))


def test_the_runs_above_take_every_branch():
    total = O.DistractOracle(1)
    with pytest.raises(AssertionError, match="never took"):
        total.require_branches()
    for name in O.SCENARIOS:
        for k, v in O.run_of(name)["oracle"].seen.items():
            total.seen[k] += v
    total.require_branches()


def test_every_argument_error_is_refused_and_nothing_is_written(lib):
    """the DRQ_EARG cases (tests/vec_distract_oracle.refused_calls, all held to return the error without a GPU by
    tests/test_cpu_vec_distract.py) on real allocations full of the sentinel: the error, and check() finds every byte
    still poison.  Then the calls at the edge of what is accepted run"""
    N = 3
    al = lambda nbytes, name, kind="refused": poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind=kind)
    frame_in, frame_out = al(N * 21168, "frame_in"), al(N * 21168, "frame_out")
    first, key, bank, state = al(256, "first"), al(21168, "key"), al(6 * 21168 + 256, "bank"), al(1024, "state")
    calls = O.refused_calls(p(frame_in), p(first), p(key), p(bank), p(state), p(frame_out), N)
    assert len(calls) == 42
    for why, a in calls:
        assert lib.drq_vec_distract(*a, None) == -1, why
    poison.check()
    for t in (frame_in, frame_out, first, key, bank, state):
        poison.forget(t)
    # accepted: the inputs hold anything, first no flag; every byte of the output is written (a uint8 output cannot be
    # checked for that by its value: the comparisons above do it), the guards stay
    bufs = {k: poison.alloc(n, torch.uint8, "cuda", name=k, kind="in") for k, n in
            (("frame_in", N * 21168), ("first", 256), ("key", 21168), ("bank", 6 * 21168 + 256), ("state", 1024))}
    bufs["first"].zero_()
    bufs["state"].zero_()
    out = poison.alloc(N * 21168, torch.uint8, "cuda", name="frame_out")
    for a in O.accepted_calls(p(bufs["frame_in"]), p(bufs["first"]), p(bufs["key"]), p(bufs["bank"]), p(bufs["state"]), p(out), N):
        assert lib.drq_vec_distract(*a, None) == 0, a
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the class
@pytest.mark.parametrize("name", ["noise-alpha77", "bank", "camera8-colour128-unkeyed"])
def test_frame_distractor_follows_the_oracle_with_two_buffers_in_turn(name):
    run = O.run_of(name)
    N = run["N"]
    d = distractor_of(run)
    kept = []
    for s in range(O.STEPS):
        frame = torch.from_numpy(run["frames"][s]).cuda()
        first = None if run["firsts"][s] is None else torch.from_numpy(run["firsts"][s]).cuda()
        if s == 20:
            first = first.bool()                                          # either type of flag
        out = d.apply(frame, first)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (N, 3, 84, 84)
        same_bits(out.cpu().numpy(), run["outs"][s], (s, "apply"))
        kept.append(out)
        if s >= 1:      # two buffers in turn: the one of the step before is intact, the one before that is reused
            same_bits(kept[s - 1].cpu().numpy(), run["outs"][s - 1], (s, "the frame of the step before"))
        if s >= 2:
            assert kept[s - 2].data_ptr() == kept[s].data_ptr() != kept[s - 1].data_ptr()
        same_bits(d.state()["episode"], run["states"][s][0], (s, "episode"))
        same_bits(d.state()["t"], run["states"][s][1], (s, "t"))
    same_bits(d.render(frame).cpu().numpy(), run["outs"][-1], "render() draws the newest frame again")
    same_bits(d.state()["t"], run["states"][-1][1], "render() steps nothing")
    # reset(): the next apply() starts a new episode in every lane, whatever first says
    d.reset()
    d.apply(frame, torch.zeros(N, dtype=torch.uint8, device="cuda"))
    same_bits(d.state()["episode"], run["states"][-1][0] + np.uint32(1), "episode after reset()")
    same_bits(d.state()["t"], np.zeros(N, np.uint32), "t after reset()")
    from drqv2_amd import _lib
    with pytest.raises(_lib.DrqError, match="DRQ_EARG"):                   # the frame given is the buffer the call writes
        d.apply(d._out[d._out[2]])


def make_env(task, N, seed=3):
    from drqv2_amd.envs import VecCartpole, VecReach
    if task == "reach":
        return VecReach(N, "cuda", action_dim=2, episode_length=7, seed=seed, action_repeat=2)
    return VecCartpole(N, "cuda", action_dim=1, episode_length=9, seed=seed, action_repeat=2, swing_up=False)


def make_wrapped(task, N, seed=3, **kw):
    from drqv2_amd.distract import FrameDistractor, VecDistract
    kw = dict(dict(seed=5, camera=8, camera_period=1, color=48, background="noise", background_alpha=200, key="env"), **kw)
    return VecDistract(make_env(task, N, seed), FrameDistractor(N, "cuda", **kw))


def env_oracle(N, **kw):
    return O.DistractOracle(N, **dict(dict(seed=5, camera=8, camera_period=1, color=48, bg_mode=1, bg_alpha=200, key=O.ramp()), **kw))


def actions(task, N, steps, seed=0):
    r = np.random.RandomState(seed)
    return [torch.from_numpy(r.uniform(-1, 1, (N, 2 if task == "reach" else 1)).astype(np.float32)).cuda() for _ in range(steps)]


@pytest.mark.parametrize("task", ["reach", "cartpole"])
def test_wrapped_environment_is_the_plain_one_under_the_oracle(task):
    """30 steps of VecDistract(env) beside the plain environment of the same seed under the same actions: the frame is the
    oracle's distraction of the plain frame (the cartpole's rail is one pixel thin, its pole three), reward, discount, first
    and last_substeps are the plain environment's; image() is the distracted frame replicated"""
    from tests import vec_env_oracle as E
    N = 3
    w, plain, o = make_wrapped(task, N), make_env(task, N), env_oracle(N)
    with pytest.raises(AssertionError, match="never took"):
        o.require_branches("background", "foreground", "reset_row", "step_row")
    same_bits(w.reset().cpu().numpy(), o.apply(plain.reset().cpu().numpy(), reset_all=True), "reset")
    firsts = 0
    for s, a in enumerate(actions(task, N, 30)):
        frame, reward, discount, first = w.step(a)
        pf, pr, pd, pfirst = plain.step(a)
        same_bits(frame.cpu().numpy(), o.apply(pf.cpu().numpy(), pfirst.cpu().numpy()), (s, "frame"))
        for got, want, what in ((reward, pr, "reward"), (discount, pd, "discount"), (first, pfirst, "first"),
                                (w.last_substeps, plain.last_substeps, "substeps")):
            same_bits(got.cpu().numpy(), want.cpu().numpy(), (s, what))
        firsts += int(pfirst.sum())
    assert firsts >= 2 * N                                                 # at least two episodes per lane
    o.require_branches("background", "foreground", "reset_row", "step_row", "tri_rising", "tri_falling")
    same_bits(w.image(168, 4).cpu().numpy(), E.replicate(frame.cpu().numpy(), 168, 4), "image()")
    same_bits(w.render().cpu().numpy(), frame.cpu().numpy(), "render() draws the current frame again")
    assert (w.N, w.A, w.episode_length, w.action_repeat) == (plain.N, plain.A, plain.episode_length, 2)


def test_checkpoint_round_trip_continues_bit_for_bit(tmp_path):
    """save at step 11, inside an episode of every lane or not; fresh objects loaded from the file render the frame of step
    11 and take the next 12 steps to the bit"""
    from drqv2_amd import checkpoint
    N, acts = 3, actions("reach", 3, 23)
    w = make_wrapped("reach", N)
    w.reset()
    for a in acts[:11]:
        frame = w.step(a)[0]
    at_k = frame.cpu().numpy().copy()
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=w, extra={"step": 11})
    saved = w.state()
    assert saved["distract_t"].max() > 0 and saved["distract_episode"].max() >= 2
    fresh = make_wrapped("reach", N)
    assert checkpoint.load(path, env=fresh) == {"step": 11}
    same_bits(fresh.render().cpu().numpy(), at_k, "render() after the restore is the frame of step k")
    same_state(fresh.state(), saved, "restored")
    for s, a in enumerate(acts[11:]):
        for got, want in zip(fresh.step(a), w.step(a)):
            same_bits(got.cpu().numpy(), want.cpu().numpy(), (s, "after the restore"))
    with pytest.raises(ValueError, match="camera: saved 8, here 4"):
        checkpoint.load(path, env=make_wrapped("reach", N, camera=4))


def test_evaluate_and_video_take_the_wrapper_and_draw_from_no_generator():
    import drqv2
    from drqv2_amd.evaluate import VecVideo, evaluate
    torch.manual_seed(3)
    agent = drqv2.DrQV2Agent((9, 84, 84), (2,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = make_wrapped("reach", 3)
    video = VecVideo(3, "cuda", scale=1, max_frames=32)
    torch.cuda.synchronize()
    before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())
    res = evaluate(agent, env, 1, poll_every=4, video=video)
    assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(), before[1])
    snap = res.snapshot
    assert snap.complete and snap.episodes == 3 and sorted(snap.records["env"].tolist()) == [0, 1, 2]
    assert (snap.records["length"] <= 4).all() and len(video) >= 2 and np.isfinite(snap.mean_return)
    # the clip shows distracted frames: its first image is not the plain environment's first frame
    plain = make_env("reach", 3).reset().cpu().numpy()
    shown = video.clip()[0].cpu().numpy()[:84, :84].transpose(2, 0, 1)
    assert shown.tobytes() != plain[0].tobytes()


def collect(wrapped, steps=12):
    """the collection loop of tools/vec_train_demo.py without its updates: the ring's frames, actions and flags"""
    import drqv2
    from drqv2_amd.replay import VecEpisodeStats, VecFrameReplay
    N, A = 3, 2
    torch.manual_seed(4)
    torch.cuda.manual_seed_all(4)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    env = make_wrapped("reach", N, camera=0, color=0, background="none") if wrapped else make_env("reach", N)
    store = VecFrameReplay(32, N, A, 3, 0.99, "cuda", seed=1)
    stats = VecEpisodeStats(N, "cuda", log_size=64)
    store.add(env.reset(), torch.zeros(N, A, device="cuda"), torch.zeros(N, device="cuda"), torch.ones(N, device="cuda"),
              torch.ones(N, dtype=torch.uint8, device="cuda"))
    stats.step(torch.zeros(N, device="cuda"))
    for step in range(steps):
        action = agent.act_batch(store.observation(), step, False)
        frame, reward, discount, first = env.step(action)
        store.add(frame, action, reward, discount, first)
        stats.step(reward, first)
    torch.cuda.synchronize()
    return {k: getattr(store, k).cpu().numpy() for k in ("frames", "action", "reward", "discount", "first")}


def test_with_strengths_zero_the_wrapped_loop_collects_what_the_plain_one_does():
    a, b = collect(True), collect(False)
    for k in a:
        same_bits(a[k], b[k], k)
    assert a["first"].sum() > 3                                            # more than the reset row: episodes ended
