"""What the GPU tests of the device-environment family share (a helper module like tests/poison.py: not collected, not a
conftest): the bit-for-bit comparisons, the `lib` fixture, the poisoned output set of a step entry, the loop that holds a
step entry to its oracle on poisoned, guarded memory, and the bodies of the tests every task's file has
(tests/test_hip_vec_{cartpole,reacher,maze,catch}.py).  Such a body takes the task's description T, a namespace built in
the task's file, and never asks which task it is:
  T.O          the oracle module: O.run(cfg), O.STEPS, O.EPISODE_LENGTH
  T.kind       the name of the class of drqv2_amd.envs;  T.make(cfg, **kw) constructs it
  T.words      the task's state words: (name, trailing shape, torch dtype), in the order of the step entry's arguments
  T.staggered  the words the start of a run writes through load_state_dict()
  T.step(lib, cfg, state, action, reset_all, outs), T.render(lib, cfg, state, frame)     the entries over pointers (state:
               {name: pointer} in the entry's order; outs: pointers)
  T.also(env, run, s)     what else the task compares of an environment that stands after step s of the run, or None"""
import numpy as np
import pytest
import torch

from tests import poison
from tests.test_hip_entries import dev, p
from tests.test_hip_vec_replay import raw
from tests.vec_env_oracle import replicate
from tests.vec_skeleton_oracle import run_of, same_bits  # noqa: F401  (same_bits: the tests take it from here)

OUT = ("frame", "reward", "discount", "first", "substeps")
U8 = poison.sentinel_of(torch.uint8)


def lib_fixture(entry, missing):
    """the module's `lib` fixture: the loaded library, on a machine with a GPU, whose prototypes hold `entry`"""
    @pytest.fixture(scope="module")
    def lib():
        from drqv2_amd import _lib
        assert torch.cuda.is_available()
        assert entry in _lib.PROTOTYPES, missing
        return _lib.load()
    return lib


def same_state(got, want, what="state", keys=None):
    """every word of `want` in `got`, and no other (keys: these words only)"""
    if keys is None:
        assert got.keys() == want.keys(), what
    for k in keys or want:
        same_bits(got[k], want[k], (what, k))


def alloc_outs(N, substeps=True):
    """a fresh output set of a step entry, full of the sentinel between guard bands"""
    outs = [poison.alloc((N, 3, 84, 84), torch.uint8, "cuda", name="frame"),
            poison.alloc(N, torch.float32, "cuda", name="reward"), poison.alloc(N, torch.float32, "cuda", name="discount"),
            poison.alloc(N, torch.uint8, "cuda", name="first")]
    return outs + [poison.alloc(N, torch.int32, "cuda", name="substeps")] if substeps else outs


def state_words(state, names):
    """the host copy of the state arrays `names`, episode as the uint32 it is"""
    got = {n: state[n].cpu().numpy() for n in names}
    got["episode"] = got["episode"].view(np.uint32)
    return got


def entry_on_poisoned_memory(step, run, N, steps=12, substeps=True, state=None, compared=(), after_reset=None, beside=None):
    """A step entry on guarded allocations full of the sentinel: the reset of all with a NULL action, then `steps` steps
    into fresh poisoned outputs each.  The outputs equal the oracle's, which never holds the byte sentinel 0xA5 (a frame
    is 32 .. 73, 64 or 255, a flag 0 or 1) nor the 4-byte one, so every byte was written; check() finds the guard bands
    of outputs, state and action untouched; the words `compared` of `state` equal the oracle's after every call.
    step(action, reset_all, outs) calls the entry on pointers and returns its status; after_reset() runs once behind
    the reset; beside(s, want) runs in front of every check()."""
    for s in range(-1, steps):
        outs = alloc_outs(N, substeps)
        action = None if s < 0 else dev(torch.from_numpy(run["actions"][s]), "action")
        assert step(p(action), int(s < 0), [p(t) for t in outs]) == 0
        if s < 0 and after_reset:
            after_reset()
        want = (run["frame0"], np.zeros(N, np.float32), np.ones(N, np.float32), np.ones(N, np.uint8),
                np.zeros(N, np.int32)) if s < 0 else run["out"][s]
        for name, t, w in zip(OUT, outs, want):
            got = t.cpu().numpy()
            same_bits(got, w, (s, name))
            if got.dtype == np.uint8:
                assert not (got == U8).any(), (s, name)
        if beside:
            beside(s, want)
        poison.check()
        if compared:
            same_state(state_words(state, compared), run["state0"] if s < 0 else run["states"][s], s)


def refused_on_poisoned_memory(state_bytes, cases):
    """the DRQ_EARG cases on real allocations full of the sentinel: cases(S0, ACT, FR, SC) -> (entry, argument lists, how
    many) per entry, over the addresses of the state, the action, the frame and the scalar outputs.  Every call returns the
    error, and check() finds every byte still poison"""
    al = lambda nbytes, name: poison.alloc(nbytes, torch.uint8, "cuda", name=name, kind="refused")
    state, action, frame, scalars = al(state_bytes, "state"), al(0x100, "action"), al(5 * 3 * 84 * 84, "frame"), al(0x400, "scalars")
    for entry, calls, count in cases(p(state), p(action), p(frame), p(scalars)):
        for a in calls:
            assert entry(*a, None) == -1, a
        assert len(calls) == count, (len(calls), count)
    poison.check()


# ---- an environment of a task's class along a run of its oracle ----------------------------------------------------------
def stagger(T, env, run):
    """the state the oracle's run starts from (its staggered t, hand-set states) into an environment that has just been
    reset, through load_state_dict(), as a user of the class would write it"""
    sd = env.state_dict()
    for k in T.staggered:
        sd[k] = torch.from_numpy(run["state0"][k])
    env.load_state_dict(sd)


def start(T, env, run):
    env.reset()
    stagger(T, env, run)


def follow(T, env, run, first, last):
    for s in range(first, last):
        out = env.step(torch.from_numpy(run["actions"][s]).cuda())
        assert len(out) == 4 and [t.dtype for t in out] == [torch.uint8, torch.float32, torch.float32, torch.uint8]
        for name, t, want in zip(OUT, out + (env.last_substeps,), run["out"][s]):
            same_bits(t.cpu().numpy(), want, (s, name))
        same_state(env.state(), run["states"][s], s)
        if T.also:
            T.also(env, run, s)


# ---- the bodies of the tests every task's file has -----------------------------------------------------------------------
def env_matches_the_oracle(T, cfg, before_steps=None):
    """reset(), the stagger, then O.STEPS macro steps: frame, reward, discount, first, last_substeps and state() after
    every step; the two output sets are used in turn.  before_steps(env, run): the task's own look at the first state"""
    run = run_of(T.O, cfg)
    N = cfg[0]
    env = T.make(cfg)
    frame = env.reset()
    same_bits(frame.cpu().numpy(), run["frame0"], "first frame")
    same_bits(env.last_substeps.cpu().numpy(), np.zeros(N, np.int32), "substeps of the reset")
    stagger(T, env, run)
    same_state(env.state(), run["state0"], "reset")
    same_bits(env.render().cpu().numpy(), run["frame0"], "the frame does not depend on t")
    if before_steps:
        before_steps(env, run)
    kept = []
    for s in range(T.O.STEPS):
        follow(T, env, run, s, s + 1)
        kept.append(env.last_substeps)
        if s >= 1:      # two output sets in turn: the set of the step before is intact, the one before that is reused
            same_bits(kept[s - 1].cpu().numpy(), run["out"][s - 1][4], (s, "the substeps of the step before"))
        if s >= 2:
            assert kept[s - 2].data_ptr() == kept[s].data_ptr() != kept[s - 1].data_ptr()


def step_entry_on_poisoned_memory(T, lib, cfg, beside=None):
    """T.step on guarded allocations full of the sentinel (entry_on_poisoned_memory), from the staggered t of the oracle's
    run; T.render beside every call, into a poisoned frame of its own; beside(state, s, run): what else the task calls
    there"""
    run = run_of(T.O, cfg)
    N = cfg[0]
    z = lambda shape, dt, name: dev(torch.zeros(shape, dtype=dt), name)
    state = {name: z((N,) + shape, dt, name) for name, shape, dt in T.words}
    state.update(t=z(N, torch.int32, "t"), episode=z(N, torch.int32, "episode"), over=z(N, torch.uint8, "over"))
    pointers = {name: p(t) for name, t in state.items()}

    def render_beside(s, want):
        again = poison.alloc((N, 3, 84, 84), torch.uint8, "cuda", name="rendered")
        assert T.render(lib, cfg, pointers, p(again)) == 0
        same_bits(again.cpu().numpy(), want[0], (s, "render"))
        if beside:
            beside(pointers, s, run)

    entry_on_poisoned_memory(lambda action, reset_all, outs: T.step(lib, cfg, pointers, action, reset_all, outs), run, N,
                             state=state, compared=tuple(state), beside=render_beside,
                             after_reset=lambda: state["t"].copy_(torch.from_numpy(run["state0"]["t"])))     # the run's stagger


def state_dict_image_and_ring(T, cfg):
    """9 steps, state_dict(); a fresh environment given the dict renders the saved frame and takes the next 5 steps to the
    bit.  image() of it at 168 x 168 x 4 is the oracle's frame with every pixel twice in both directions.  One
    VecFrameReplay.add() of the reset row and one of a step, then observation(): the stack a frame stacker would hold.
    Returns the dict, for the task's own assertions on it"""
    from drqv2_amd.replay import VecFrameReplay
    run = run_of(T.O, cfg)
    N, A = cfg[:2]
    env = T.make(cfg)
    start(T, env, run)
    follow(T, env, run, 0, 9)
    want = run["out"][8][0]
    sd = env.state_dict()
    assert sd["kind"] == T.kind
    for name, shape, dt in T.words:
        assert tuple(sd[name].shape) == (N,) + shape and sd[name].dtype == dt, name
    fresh = T.make(cfg)
    fresh.load_state_dict(sd)
    same_bits(fresh.render().cpu().numpy(), want, "the frame of the restored state")
    same_state(fresh.state(), run["states"][8], "restored")
    if T.also:
        T.also(fresh, run, 8)
    same_bits(fresh.image(168, 4).cpu().numpy(), replicate(want, 168, 4), "image()")
    ring = VecFrameReplay(16, N, A, 3, 0.99, "cuda", seed=1)
    zeros, ones = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    ring.add(fresh.render(), torch.zeros(N, A, device="cuda"), zeros, ones, torch.ones(N, dtype=torch.uint8, device="cuda"))
    action = torch.from_numpy(run["actions"][9]).cuda()
    frame, reward, discount, first = fresh.step(action)
    ring.add(frame, torch.nan_to_num(action).clamp(-1, 1), reward, discount, first)
    newest, reset_row = run["out"][9][0], run["out"][9][3].astype(bool)[:, None, None, None]
    stack = np.concatenate([np.where(reset_row, newest, want)] * 2 + [newest], axis=1)      # a reset row fills the stack
    same_bits(ring.observation().cpu().numpy(), stack, "observation()")
    same_state(fresh.state(), run["states"][9], "after the step")
    follow(T, fresh, run, 10, 14)
    return sd


def checkpoint_round_trip(T, cfg, tmp_path, cut, more, between, **kw):
    """`cut` macro steps, checkpoint.save(), `more` further steps; a fresh environment loaded from the file takes the same
    steps to the bit, outputs and state.  between(path, saved): the task's own assertions on the state that was saved --
    that the save falls where the test's name says -- and on the file.  kw: what T.make takes beside cfg"""
    from drqv2_amd import checkpoint
    run = run_of(T.O, cfg)
    env = T.make(cfg, **kw)
    start(T, env, run)
    follow(T, env, run, 0, cut)
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=env, extra={"step": cut})
    between(path, env.state())
    fresh = T.make(cfg, **kw)
    assert checkpoint.load(path, env=fresh) == {"step": cut}
    same_state(fresh.state(), run["states"][cut - 1], "restored")
    assert raw(fresh.render()).tobytes() == run["out"][cut - 1][0].tobytes()
    follow(T, fresh, run, cut, cut + more)
    follow(T, env, run, cut, cut + more)
    same_state(fresh.state(), env.state(), f"after {more} steps")


def distractions_and_the_exploration_bonus(T, cfg):
    """reset() and one step of VecDistract(env, distractor) against the distraction oracle applied to the task oracle's
    frames -- no shape pixel is the background key -- and SimHashBonus of the plain frames and the reward against its own
    oracle"""
    from drqv2_amd.distract import FrameDistractor, VecDistract
    from drqv2_amd.explore import SimHashBonus
    from tests import simhash_oracle as S
    from tests import vec_distract_oracle as D
    run = run_of(T.O, cfg)
    N = cfg[0]
    kw = dict(seed=5, camera=8, camera_period=1, color=48)
    wrapped = VecDistract(T.make(cfg), FrameDistractor(N, "cuda", background="noise", background_alpha=200, key="env", **kw))
    o = D.DistractOracle(N, bg_mode=1, bg_alpha=200, key=D.ramp(), **kw)
    same_bits(wrapped.reset().cpu().numpy(), o.apply(run["frame0"], reset_all=True), "reset")
    stagger(T, wrapped.env, run)
    frame, reward, discount, first = wrapped.step(torch.from_numpy(run["actions"][0]).cuda())
    want = run["out"][0]
    same_bits(frame.cpu().numpy(), o.apply(want[0], want[3]), "the distracted frame")
    for got, w, what in ((reward, want[1], "reward"), (discount, want[2], "discount"), (first, want[3], "first"),
                         (wrapped.last_substeps, want[4], "substeps")):
        same_bits(got.cpu().numpy(), w, what)
    o.require_branches("background", "foreground")
    bonus, so = SimHashBonus(N, "cuda", bits=16, beta=0.5, seed=4), S.SimHashOracle(16, 0.5, 4)
    plain = T.make(cfg)
    start(T, plain, run)
    for s in range(2):
        frame, reward = plain.step(torch.from_numpy(run["actions"][s]).cuda())[:2]
        ret = bonus.step(frame, reward)
        code, count, extra, total = so.step(run["out"][s][0], run["out"][s][1])[:4]
        for got, w, what in ((bonus.codes, code, "codes"), (bonus.counts, count, "counts"), (bonus.last_bonus, extra, "bonus"),
                             (ret, total, "reward + bonus")):
            same_bits(got.cpu().numpy(), w, (s, what))


def evaluate_and_video(T, cfg):
    """evaluate() runs one episode of each of N = 3 environments of O.EPISODE_LENGTH simulator steps at the repeat of cfg
    with a VecVideo beside it; returns the snapshot, for what the task says of its returns"""
    import drqv2
    from drqv2_amd.evaluate import VecVideo, evaluate
    N, A, k = cfg[:3]
    torch.manual_seed(3)
    agent = drqv2.DrQV2Agent((9, 84, 84), (A,), "cuda", 1e-3, 50, 64, 0.01, 8, 1, "0.5", 0.3, True)
    video = VecVideo(N, "cuda", max_frames=64)
    res = evaluate(agent, T.make(cfg), 1, poll_every=4, video=video)
    snap = res.snapshot
    assert snap.complete and snap.episodes == N and sorted(snap.records["env"].tolist()) == list(range(N))
    assert (snap.records["length"] == -(-T.O.EPISODE_LENGTH // k)).all() and len(video) >= 5
    return snap
