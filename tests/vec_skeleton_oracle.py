"""numpy restatement of the skeleton of a device environment (a helper module: not collected): vec_env_step_kernel of
drqv2_amd/csrc/vecenv_task.h, as the comment of include/drqv2_hip.h ("device environment", "Tasks and action repeat")
states it -- what a task does not decide, written once for every task oracle.  A task oracle (tests/vec_tasks_oracle.py,
vec_cartpole_oracle.py, vec_reacher_oracle.py, vec_maze_oracle.py, vec_catch_oracle.py) is a subclass that supplies what
`Task` supplies in C: its state words, new_episode(), sanitise(), substep() and frame(), and its own coverage counters.
tests/vec_env_oracle.ReachOracle stays written out on its own: tests/test_cpu_vec_tasks.py holds this skeleton to it, at
repeat 1 bit for bit and at repeat k folded by the wrapper rule.

  macro step of e   reset row (over[e], or reset()): episode += 1 mod 2^32, t = 0, over = 0, the task's new episode;
                    first = 1, reward = 0, discount = 1, substeps = 0; the action is not read
                    otherwise: reward = 0, discount = 1, the action row sanitised once; for i < repeat: (r, d, ended) =
                    the task's sub-step; t += 1; over on ended or t == episode_length; reward = reward + r * discount;
                    discount = discount * d; stop after the sub-step that set over.  first = 0, substeps = the sub-steps
                    executed
  frame             the task's, of the state after the last executed sub-step

Beside the skeleton, one copy each of what the runs of every task share: wild_actions(), the stagger, the recorder, the
cache of runs, the bit-for-bit comparison; the builder of the argument lists an entry must refuse; and the part of the
constructor test that no task decides."""
import numpy as np
import pytest

from tests.vec_env_oracle import F, M32, clamp1


def sanitise(v):
    """an action component as every task reads it"""
    return F(0) if np.isnan(v) else clamp1(v)


class SkeletonOracle:
    WORDS = ()          # the task's state words: (name, trailing shape, dtype), in the order of state()

    def __init__(self, num_envs, episode_length, seed, repeat, frames=True):
        """frames=False: reset(), step() and frames() return None for the frames, which are most of a run's time"""
        assert 1 <= int(repeat) <= 16
        self.N, self.episode_length, self.seed = int(num_envs), int(episode_length), int(seed) & M32
        self.repeat, self.with_frames = int(repeat), bool(frames)
        for name, shape, dtype in self.WORDS:
            setattr(self, name, np.zeros((self.N,) + shape, dtype))
        self.t = np.zeros(self.N, np.int32)
        self.episode = np.zeros(self.N, np.uint32)
        self.over = np.zeros(self.N, np.uint8)
        # what a run met: full rows, rows cut short by the task and by the time limit, reset rows; episodes the time limit ended
        self.full = self.cut_by_task = self.cut_by_limit = self.reset_rows = self.timed_out = 0

    # ---- what a task supplies
    def new_episode(self, e, ep):
        """the state words of episode ep of environment e"""
        raise NotImplementedError

    def sanitise(self, row):
        """what a sub-step reads of an action row"""
        raise NotImplementedError

    def substep(self, e, act):
        """one simulator step of environment e -> (r, d, ended): float32 reward and discount, whether the task ended the episode"""
        raise NotImplementedError

    def frame(self, e):
        raise NotImplementedError

    # ---- the skeleton
    def _reset_one(self, e):
        ep = (int(self.episode[e]) + 1) & M32
        self.episode[e], self.t[e], self.over[e] = ep, 0, 0
        self.new_episode(e, ep)

    def frames(self):
        return np.stack([self.frame(e) for e in range(self.N)]) if self.with_frames else None

    def reset(self):
        for e in range(self.N):
            self._reset_one(e)
        return self.frames()

    def step(self, action):
        """action: float32 [N, A] -> (frame, reward, discount, first, substeps)"""
        action = np.asarray(action, F)
        reward, discount, first = np.zeros(self.N, F), np.ones(self.N, F), np.zeros(self.N, np.uint8)
        substeps = np.zeros(self.N, np.int32)
        for e in range(self.N):
            if self.over[e]:
                self._reset_one(e)
                first[e] = 1
                self.reset_rows += 1
                continue
            act = self.sanitise(action[e])
            ended = False
            while substeps[e] < self.repeat and not self.over[e]:
                r, d, ended = self.substep(e, act)
                self.t[e] += 1
                if ended or self.t[e] == self.episode_length:
                    self.over[e] = 1
                    self.timed_out += not ended
                reward[e] = F(reward[e] + F(r * discount[e]))
                discount[e] = F(discount[e] * d)
                substeps[e] += 1
            if substeps[e] == self.repeat:
                self.full += 1
            elif ended:
                self.cut_by_task += 1
            else:
                self.cut_by_limit += 1
        return self.frames(), reward, discount, first, substeps

    def state(self):
        return {name: getattr(self, name).copy() for name in [w[0] for w in self.WORDS] + ["t", "episode", "over"]}


# ---- the runs the CPU and the GPU tests share --------------------------------------------------------------------------
def wild_actions(r, N, A):
    """a row of actions from RandomState r: uniform in [-2, 2], so the clamp is hit; one component in sixteen NaN, one in
    eight +-inf"""
    a = r.uniform(-2, 2, (N, A)).astype(F)
    kind = r.randint(0, 16, (N, A))
    a[kind == 0] = np.nan
    a[kind == 1] = np.inf
    a[kind == 2] = -np.inf
    return a


def stagger(o):
    """Only the time limit ends an episode of most tasks, so environments reset together would stay in step for ever: after
    the reset, t of environment e is set to e mod episode_length (a run's "state0" holds it; a user of the class does the
    same through load_state_dict()), and the resets stagger from then on"""
    o.t[:] = np.arange(o.N) % o.episode_length


def record(o, steps, actions, seen):
    """the oracle o, reset and prepared by the caller, driven for `steps` macro steps by actions(s): the first frames and
    state, the actions it was given, everything it returned, the state after every step, and the counters `seen`"""
    run = {"frame0": o.frames(), "state0": o.state(), "actions": [], "out": [], "states": []}
    for s in range(steps):
        a = actions(s)
        run["actions"].append(a)
        run["out"].append(o.step(a))
        run["states"].append(o.state())
    for k in seen:
        run[k] = getattr(o, k)
    return run


_RUNS = {}


def run_of(O, cfg, frames=True):
    """the run O.run(cfg, frames) of a configuration of the oracle module O: computed once, on first use, shared, never modified"""
    key = (O.__name__, cfg, frames)
    if key not in _RUNS:
        _RUNS[key] = O.run(cfg, frames)
    return _RUNS[key]


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        where = f", first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}" if len(bad) else ""
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ{where}")


# ---- the argument lists an entry must refuse ---------------------------------------------------------------------------
# The role of a position of the well-formed list `ok`: w a pointer to 4-byte words, w8 to 8-byte words, b to bytes, frame,
# action, N, A (ok holds the fewest columns the task reads), L, repeat, reset, - none.  `own`: {position: bad values}.
_BAD = {"N": (0, -1, 2 ** 31), "L": (0, -5), "repeat": (0, -1, 17, 2 ** 31 - 1), "reset": (2, -1)}
_POINTERS = ("w", "w8", "b", "frame", "action")


def sub(ok, k, v):
    return ok[:k] + [v] + ok[k + 1:]


def _bad_values(ok, role, k, own):
    if k in own:
        return own[k]
    return tuple(range(ok[k] - 1, -1, -1)) + (-2,) if role == "A" else _BAD.get(role, ())


def refused_steps(ok, roles, own):
    """what a step entry must refuse around `ok`: every pointer null (the action: without reset_all); every bad scalar, the
    task's own among them, in the order of the positions; the frame not 16-byte aligned; an array of 8-byte words not
    8-byte aligned; an array of words, the action among them, not 4-byte aligned"""
    roles = roles.split()
    assert len(roles) == len(ok)
    bad = [sub(ok, k, None) for k, role in enumerate(roles) if role in _POINTERS]
    bad += [sub(ok, k, v) for k, role in enumerate(roles) for v in _bad_values(ok, role, k, own)]
    bad += [sub(ok, k, ok[k] + m) for k, role in enumerate(roles) if role == "frame" for m in (1, 4, 8)]
    bad += [sub(ok, k, ok[k] + 4) for k, role in enumerate(roles) if role == "w8"]
    bad += [sub(ok, k, ok[k] + 2) for k, role in enumerate(roles) if role in ("w", "w8", "action")]
    return bad


def refused_reads(ok, roles, own):
    """what an entry that only reads the state (a render, a measure) must refuse around `ok`: every pointer null, N, the frame
    not 16-byte aligned, every array not aligned to its words, then the task's own bad scalars"""
    roles = roles.split()
    assert len(roles) == len(ok)
    bad = [sub(ok, k, None) for k, role in enumerate(roles) if role in _POINTERS]
    bad += [sub(ok, k, v) for k, role in enumerate(roles) if role == "N" for v in _BAD["N"]]
    bad += [sub(ok, k, ok[k] + m) for k, role in enumerate(roles) if role == "frame" for m in (4, 8)]
    bad += [sub(ok, k, ok[k] + {"w": 2, "w8": 4}[role]) for k, role in enumerate(roles) if role in ("w", "w8")]
    bad += [sub(ok, k, v) for k in sorted(own) for v in own[k]]
    return bad


def all_refused(entries_and_calls):
    """every (entry, argument lists) pair: the entry returns DRQ_EARG for every list"""
    for entry, calls in entries_and_calls:
        for a in calls:
            assert entry(*a, None) == -1, a


# ---- the class without a device: what no task decides ---------------------------------------------------------------------
def class_without_a_device(cls, env, tmp_path, word, methods=(), bad_repeats=(0, 17, True)):
    """cls refuses the bad action_repeat values; env, an instance on "cpu", has the methods of the family, no substeps yet
    and no CPU fallback; its t / episode / over have the skeleton's dtypes; drqv2_amd.checkpoint takes the class with no
    special case: after one element of the state word `word` was written, the file holds the dict as it is.  Returns the
    checkpoint's content"""
    import torch
    from drqv2_amd import _lib, checkpoint
    for bad in bad_repeats:
        with pytest.raises(ValueError, match="action_repeat"):
            cls(3, "cpu", action_repeat=bad)
    for method in ("reset", "step", "render", "image", "state", "state_dict", "load_state_dict") + tuple(methods):
        assert callable(getattr(env, method)), method
    assert env.last_substeps is None
    with pytest.raises(_lib.DrqError, match="no CPU fallback"):
        env.reset()
    s = env.state()
    assert s["episode"].dtype == np.uint32 and s["over"].dtype == np.uint8 and s["t"].dtype == np.int32
    getattr(env, word[0])[word[1]] = word[2]
    path = str(tmp_path / "env.pt")
    checkpoint.save(path, env=env, extra={"step": 4})
    ck = torch.load(path, weights_only=True)
    assert ck["env"]["kind"] == cls.__name__ and ck["env"]["config"] == env.state_dict()["config"]
    assert torch.equal(ck["env"][word[0]], getattr(env, word[0])) and ck["extra"] == {"step": 4}
    return ck
