"""numpy restatement of the device environment's task family with action repeat (a helper module: not collected).  The
contract is the comment of include/drqv2_hip.h ("device environment", "Tasks and action repeat"), stated here once more
with float32 scalars, one rounding per operation in the written order.  The hash, the draws and the frame rule are those
of tests/vec_env_oracle.py and are imported from it.  The macro step -- the reset row, the repeat, the time limit, the
fold of reward and discount -- is the skeleton's, written once for every task in tests/vec_skeleton_oracle.py; here are
the two rules alone.  tests/vec_env_oracle.ReachOracle writes the step of reach out on its own, so that at repeat 1 the two
restatements can be held against each other, and at repeat k the skeleton's fold against the single step folded by hand.

  reset             the four draws -> pos, target; vel = 0
  action            a = action[e, 0:2], NaN -> 0, clamp to [-1, 1]
  reach             pos = clamp(pos + a * 0.1, -1, 1); d2 = dx dx + dy dy; r = max(0, 1 - d2); d2 <= 0.01: d = 0, ended; else d = 1
  pointmass         per axis v = v * 0.9; v = v + a * 0.02; p = pos + v; p < -1: pos = -1, v = 0; p > 1: pos = 1, v = 0; else
                    pos = p.  r as in reach; d = 1 always; never ended: over only at t == episode_length
  frame             by vec_env_oracle.render: velocity is in no frame
"""
import numpy as np

from tests import vec_skeleton_oracle as S
from tests.vec_env_oracle import F, clamp1, draw, render

TASKS = ("reach", "pointmass")
_SEEN = ("reached", "timed_out", "cut_by_target", "cut_by_limit", "full")


class TaskOracle(S.SkeletonOracle):
    def __init__(self, task, num_envs, episode_length=250, seed=0, repeat=1, frames=True):
        assert task in TASKS
        self.task = task
        self.WORDS = (("pos", (2,), F), ("target", (2,), F)) + ((("vel", (2,), F),) if task == "pointmass" else ())
        super().__init__(num_envs, episode_length, seed, repeat, frames)
        self.reached = 0        # sub-steps that ended an episode on the target (reach)

    cut_by_target = property(lambda self: self.cut_by_task)      # rows of fewer than `repeat` sub-steps that the target ended

    def new_episode(self, e, ep):
        v = [draw(self.seed, e, ep, k) for k in range(4)]
        self.pos[e], self.target[e] = v[:2], v[2:]
        if self.task == "pointmass":
            self.vel[e] = 0

    def sanitise(self, row):
        return [S.sanitise(row[k]) for k in range(2)]

    def frame(self, e):
        return render(self.pos[e], self.target[e])

    def substep(self, e, a):
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
        dx, dy = F(self.pos[e, 0] - self.target[e, 0]), F(self.pos[e, 1] - self.target[e, 1])
        d2 = F(F(dx * dx) + F(dy * dy))
        r = F(F(1) - d2)
        r = r if r > 0 else F(0)
        if self.task == "reach" and d2 <= F(0.01):
            self.reached += 1
            return r, F(0), True
        return r, F(1), False


def wild_actions(r, o, A, s):
    """row s of actions for oracle o from RandomState r: S.wild_actions -- uniform in [-2, 2], so the clamp is hit, one
    component in sixteen NaN and one in eight +-inf -- where environments 0, 3, 6, ... "home" on three rows of four:
    clip((target - pos) / 0.1) from the oracle's state in place of the uniform components, so that reach hits its target,
    inside a repeat too (with N = 1 every environment homes, and would never see an out-of-range action)"""
    a = S.wild_actions(r, o.N, A)
    if s % 4 != 3:
        home = np.clip((o.target[::3] - o.pos[::3]) / F(0.1), -1, 1)
        a[::3, :2] = np.where(np.isfinite(a[::3, :2]), home, a[::3, :2])
    return a


def driven_run(task, N, A, repeat, seed, steps, episode_length, frames=True):
    """the oracle driven for `steps` macro steps by wild_actions: the actions it was given, everything it returned (the
    frames only if asked for: they are most of the time) and the state after every step"""
    r = np.random.RandomState(seed * 100003 + TASKS.index(task) * 10007 + N * 101 + A * 17 + repeat)
    o = TaskOracle(task, N, episode_length=episode_length, seed=seed, repeat=repeat, frames=frames)
    o.reset()
    return S.record(o, steps, lambda s: wild_actions(r, o, A, s), _SEEN)


def run(cfg, frames=True):
    """cfg: (task, N, A, repeat, seed, steps, episode_length)"""
    return driven_run(*cfg, frames=frames)


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
    sub = lambda k, v, base=ok: S.sub(base, k, v)     # two well-formed lists, reach's without vel: written out, not a table
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
