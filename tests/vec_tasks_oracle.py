"""numpy restatement of the device environment's task family with action repeat (a helper module: not collected).  The
contract is the comment of include/drqv2_hip.h ("device environment", "Tasks and action repeat"), stated here once more
with float32 scalars, one rounding per operation in the written order.  The hash, the draws and the frame rule are those
of tests/vec_env_oracle.py and are imported from it; the step is written out again, so that at repeat 1 the two
restatements can be held against each other.

  macro step of e   reset row (over[e], or reset()): episode += 1, t = 0, over = 0, the four draws, vel = 0;
                    first = 1, reward = 0, discount = 1, substeps = 0; the action is not read
                    otherwise: reward = 0, discount = 1, a = action[e, 0:2] sanitised once (NaN -> 0, clamp to [-1, 1]);
                    for i < repeat: (r, d, over) = sub-step; reward = reward + r * discount; discount = discount * d;
                    stop after the sub-step that set over.  first = 0, substeps = the sub-steps executed
  reach             pos = clamp(pos + a * 0.1, -1, 1); t += 1; d2 = dx dx + dy dy; r = max(0, 1 - d2); d2 <= 0.01: d = 0, over;
                    else t == episode_length: d = 1, over; else d = 1
  pointmass         per axis v = v * 0.9; v = v + a * 0.02; p = pos + v; p < -1: pos = -1, v = 0; p > 1: pos = 1, v = 0; else
                    pos = p.  t += 1; r as in reach; d = 1 always; over only at t == episode_length
  frame             of the state after the last executed sub-step, by vec_env_oracle.render: velocity is in no frame
"""
import numpy as np

from tests.vec_env_oracle import F, M32, clamp1, draw, render

TASKS = ("reach", "pointmass")


class TaskOracle:
    def __init__(self, task, num_envs, episode_length=250, seed=0, repeat=1):
        assert task in TASKS and 1 <= int(repeat) <= 16
        self.task, self.N, self.episode_length = task, int(num_envs), int(episode_length)
        self.seed, self.repeat = int(seed) & M32, int(repeat)
        self.pos = np.zeros((self.N, 2), F)
        self.target = np.zeros((self.N, 2), F)
        self.vel = np.zeros((self.N, 2), F)
        self.t = np.zeros(self.N, np.int32)
        self.episode = np.zeros(self.N, np.uint32)
        self.over = np.zeros(self.N, np.uint8)
        self.reached = self.timed_out = 0       # terminations of either kind so far
        self.cut_by_target = self.cut_by_limit = self.full = 0      # rows of fewer than `repeat` sub-steps, and of all

    def _reset_one(self, e):
        ep = (int(self.episode[e]) + 1) & M32
        self.episode[e], self.t[e], self.over[e] = ep, 0, 0
        v = [draw(self.seed, e, ep, k) for k in range(4)]
        self.pos[e], self.target[e] = v[:2], v[2:]
        self.vel[e] = 0

    def frames(self):
        return np.stack([render(self.pos[e], self.target[e]) for e in range(self.N)])

    def reset(self):
        for e in range(self.N):
            self._reset_one(e)
        return self.frames()

    def _substep(self, e, a):
        """one simulator step of environment e under the sanitised action a -> (r, d)"""
        for k in range(2):
            if self.task == "reach":
                self.pos[e, k] = clamp1(F(self.pos[e, k] + F(a[k] * F(0.1))))
            else:
                v = F(self.vel[e, k] * F(0.9))
                v = F(v + F(a[k] * F(0.02)))
                p = F(self.pos[e, k] + v)
                if p < F(-1):
                    p, v = F(-1), F(0)
                elif p > F(1):
                    p, v = F(1), F(0)
                self.pos[e, k], self.vel[e, k] = p, v
        self.t[e] += 1
        dx, dy = F(self.pos[e, 0] - self.target[e, 0]), F(self.pos[e, 1] - self.target[e, 1])
        d2 = F(F(dx * dx) + F(dy * dy))
        r = F(F(1) - d2)
        r = r if r > 0 else F(0)
        d = F(1)
        if self.task == "reach" and d2 <= F(0.01):
            d, self.over[e] = F(0), 1
            self.reached += 1
        elif self.t[e] == self.episode_length:
            self.over[e] = 1
            self.timed_out += 1
        return r, d

    def step(self, action):
        """action: float32 [N, A], A >= 2 -> (frame, reward, discount, first, substeps)"""
        action = np.asarray(action, F)
        reward, discount, first = np.zeros(self.N, F), np.ones(self.N, F), np.zeros(self.N, np.uint8)
        substeps = np.zeros(self.N, np.int32)
        for e in range(self.N):
            if self.over[e]:
                self._reset_one(e)
                first[e] = 1
                continue
            a = [F(0) if np.isnan(action[e, k]) else clamp1(action[e, k]) for k in range(2)]
            for _ in range(self.repeat):
                r, d = self._substep(e, a)
                reward[e] = F(reward[e] + F(r * discount[e]))
                discount[e] = F(discount[e] * d)
                substeps[e] += 1
                if self.over[e]:
                    break
            if substeps[e] == self.repeat:
                self.full += 1
            elif discount[e] == 0:
                self.cut_by_target += 1
            else:
                self.cut_by_limit += 1
        return self.frames(), reward, discount, first, substeps

    def state(self):
        s = {"pos": self.pos.copy(), "target": self.target.copy(), "t": self.t.copy(), "episode": self.episode.copy(),
             "over": self.over.copy()}
        if self.task == "pointmass":
            s["vel"] = self.vel.copy()
        return s


def wild_actions(r, o, A, s):
    """row s of actions for oracle o from RandomState r: uniform in [-2, 2], so the clamp is hit; environments 0, 3, 6,
    ... "home" -- clip((target - pos) / 0.1) from the oracle's state, so that reach hits its target, inside a repeat too
    -- on three rows of four (with N = 1 every environment homes, and would never see an out-of-range action); then one
    component in sixteen is NaN and one in eight +-inf"""
    a = r.uniform(-2, 2, (o.N, A)).astype(F)
    if s % 4 != 3:
        a[::3, :2] = np.clip((o.target[::3] - o.pos[::3]) / F(0.1), -1, 1)
    kind = r.randint(0, 16, (o.N, A))
    a[kind == 0] = np.nan
    a[kind == 1] = np.inf
    a[kind == 2] = -np.inf
    return a


def driven_run(task, N, A, repeat, seed, steps, episode_length, frames=True):
    """the oracle driven for `steps` macro steps by wild_actions: the actions it was given, everything it returned (the
    frames only if asked for: they are most of the time) and the state after every step"""
    r = np.random.RandomState(seed * 100003 + TASKS.index(task) * 10007 + N * 101 + A * 17 + repeat)
    o = TaskOracle(task, N, episode_length=episode_length, seed=seed, repeat=repeat)
    if not frames:
        o.frames = lambda: None
    run = {"frame0": o.reset(), "state0": o.state(), "actions": [], "out": [], "states": []}
    for s in range(steps):
        a = wild_actions(r, o, A, s)
        run["actions"].append(a)
        run["out"].append(o.step(a))
        run["states"].append(o.state())
    for k in ("reached", "timed_out", "cut_by_target", "cut_by_limit", "full"):
        run[k] = getattr(o, k)
    return run


def covers(run, task, repeat):
    """the condition on the inputs of a driven run: a row cut short by the target (reach), one cut short by the time
    limit, a full-length row -- with repeat 1 no row can be cut short, and the terminations themselves stand in -- and a
    NaN, an infinite and an out-of-range component among the two columns that are read"""
    acts = np.stack(run["actions"])[:, :, :2]
    wild = bool(np.isnan(acts).any() and np.isinf(acts).any() and (np.abs(np.nan_to_num(acts, posinf=0, neginf=0)) > 1).any())
    if repeat == 1:
        ends = run["timed_out"] >= 1 and (task != "reach" or run["reached"] >= 1)
    else:
        ends = run["cut_by_limit"] >= 1 and (task != "reach" or run["cut_by_target"] >= 1)
    return wild and ends and run["full"] >= 1


# ---- the argument lists drq_vec_task_step refuses: shared by the CPU and the GPU test ---------------------------------
def refused_calls(S0, ACT, FR, SC):
    """the argument lists drq_vec_task_step must refuse, around one well-formed list over the four given base addresses
    (state arrays 0x100 apart from S0, the action, the frame, the scalar outputs 0x100 apart from SC)"""
    #     task pos target      vel         t           episode     over        N  A  action seed L repeat reset frame
    ok = [1, S0, S0 + 0x100, S0 + 0x200, S0 + 0x300, S0 + 0x400, S0 + 0x500, 5, 2, ACT, 7, 9, 2, 0, FR,
          SC, SC + 0x100, SC + 0x200, SC + 0x300]                         # reward discount first substeps
    sub = lambda k, v, base=ok: base[:k] + [v] + base[k + 1:]
    reach = sub(0, 0)
    bad = [sub(k, None) for k in (1, 2, 3, 4, 5, 6, 9, 14, 15, 16, 17, 18)]  # every pointer; vel: task 1; action: no reset_all
    bad += [sub(k, None, reach) for k in (1, 2, 4, 5, 6, 9, 14, 15, 16, 17, 18)]      # reach: every pointer but vel
    bad += [sub(0, v) for v in (-1, 2, 7)]                                 # task
    bad += [sub(12, v) for v in (0, -1, 17, 2 ** 31 - 1)]                  # repeat
    bad += [sub(12, v, reach) for v in (0, 17)]
    for k, vals in ((7, (0, -1, 2 ** 31)), (8, (1, 0, -2)), (11, (0, -5)), (13, (2, -1))):     # N, A, episode_length, reset_all
        bad += [sub(k, v) for v in vals]
    bad += [sub(14, FR + m) for m in (1, 4, 8)]                            # frame not 16-byte aligned
    bad += [sub(k, ok[k] + 2) for k in (1, 2, 3, 4, 5, 9, 15, 16, 18)]     # a float / int array not 4-byte aligned
    assert len(bad) == 12 + 11 + 3 + 4 + 2 + 10 + 3 + 9
    return bad
