"""Host planning for episode files and the step-major ring (new; pure numpy, no GPU, no torch).

The ring of VecDeviceReplay / VecFrameReplay is step-major: slot (t mod R) N + e holds row t of environment e, and an
episode is whatever lies between two `first` flags of one environment.  An episode file (replay_buffer.py:22-34 of the
reference) is episode-major: arrays [len + 1, ...] whose index 0 is the dummy reset transition.  Two plans connect them:

  plan_export   reads the flags of a ring and lists the episodes it holds whole, as (environment, reset row, length),
                with a count of everything it leaves out and why
  plan_fill     lays episodes of different lengths out as lockstep rows of N lanes, padded with reset rows
  planned_rows  the rows of such a layout as the arrays add() takes, step-major: what VecDeviceReplay.add_episodes()
                stages for drq_vec_fill, and what a loop of add() calls would be fed to reach the same ring

The kernels that move the frames are csrc/vecepisodes.hip; the public interface is VecDeviceReplay.export_episodes() and
add_episodes() (drqv2_amd/replay.py)."""
from collections import namedtuple

import numpy as np

ExportPlan = namedtuple("ExportPlan", "episodes next_row zero_length headless open short")
ExportPlan.__doc__ = """episodes: [(e, t0, length)] ordered by (t0 + length, e): rows t0 .. t0 + length of environment e, row
t0 the reset row, `length` transitions.  next_row = T: the start_row of the next periodic call.  zero_length, headless,
open, short: how many runs were left out under each name (plan_export)."""

FillPlan = namedtuple("FillPlan", "L episode index pad_rows")
FillPlan.__doc__ = """L: rows per lane.  episode, index: int64 [N, L]; lane e, row r holds index[e, r] of episode
episode[e, r], or is a pad row where episode[e, r] == PAD (then index is PAD too).  pad_rows: how many such rows."""

PAD = -1


def plan_export(first, T, R, N, start_row=None, include_open=False, min_length=1):
    """The episodes a ring holds whole.  first: the ring's uint8 [R N] flags (slot (t mod R) N + e holds row t); rows
    max(0, T - R) .. T - 1 are live.  Row 0 counts as a reset row whatever its flag holds: the store's own rule.

    For environment e an episode is a maximal run t0 .. t1: row t0 a reset row, rows t0 + 1 .. t1 none, and row t1 + 1
    either a live reset row (the episode is closed) or row T (it is open).  Its length is t1 - t0 transitions.  Left out,
    and counted:
      zero_length   a reset row followed at once by another (length 0; also an open episode of length 0 that
                    include_open asked for: there is nothing to write)
      headless      the rows of an environment before its first live reset row: the reset row has left the ring
      open          episodes not closed yet, unless include_open
      short         episodes of fewer than min_length transitions
    start_row: only runs with t1 + 1 >= start_row are looked at at all (neither listed nor counted).  With
    start_row = the previous plan's next_row every closed episode is listed by exactly one of a series of calls, as long
    as no reset row leaves the ring between two of them."""
    T, R, N, min_length = int(T), int(R), int(N), int(min_length)
    first = np.asarray(first)
    if R < 1 or N < 1 or T < 0 or first.shape != (R * N,):
        raise ValueError(f"plan_export: flags of shape ({R * N},) required for a ring of {R} rows x {N}, got {first.shape}")
    if min_length < 1:
        raise ValueError("plan_export: min_length must be >= 1")
    start = 0 if start_row is None else int(start_row)
    lo = max(0, T - R)
    rows = np.arange(lo, T)
    flags = first.reshape(R, N)[rows % R] != 0 if T > lo else np.zeros((0, N), bool)
    if lo == 0 and T > 0:
        flags = flags.copy()
        flags[0] = True
    found, counts = [], {"zero_length": 0, "headless": 0, "open": 0, "short": 0}
    for e in range(N):
        resets = lo + np.flatnonzero(flags[:, e])
        # the run before the first live reset row (or the whole column): its reset row is gone
        head_end = int(resets[0]) if resets.size else T            # = t1 + 1
        if head_end > lo and head_end >= start:
            counts["headless"] += 1
        for k, t0 in enumerate(resets.tolist()):
            closed = k + 1 < resets.size
            end = int(resets[k + 1]) if closed else T               # = t1 + 1
            length = end - 1 - t0
            if end < start:
                continue
            if not closed and not include_open:
                counts["open"] += 1
            elif length == 0:
                counts["zero_length"] += 1
            elif length < min_length:
                counts["short"] += 1
            else:
                found.append((end - 1, e, t0, length))
    found.sort()
    return ExportPlan([(e, t0, length) for _, e, t0, length in found], T, **counts)


def export_table(episodes):
    """int32 [M, 3]: one (t, e, t0) per step of the listed episodes (e, t0, length), in their order, rows t0 .. t0 + length
    of each -- the table drq_vec_export_rows reads"""
    parts = [np.stack([np.arange(t0, t0 + n + 1), np.full(n + 1, e), np.full(n + 1, t0)], axis=1) for e, t0, n in episodes]
    if not parts:
        return np.zeros((0, 3), np.int32)
    tab = np.concatenate(parts)
    if tab.max() > np.iinfo(np.int32).max:
        raise ValueError("export_table: row numbers beyond int32")
    return np.ascontiguousarray(tab, dtype=np.int32)


def plan_fill(lengths, N):
    """Episodes of lengths[i] transitions (lengths[i] + 1 rows each) placed into N lanes.  They go in the given order,
    each to the lane with the fewest rows so far, ties to the lowest lane.  L is the longest lane; shorter ones are padded
    at their end with reset rows (planned_rows says what they hold).  A run of reset rows is legal input to add(): the
    sampler never draws one as a transition and every window ends at one, so padding loses no data."""
    N = int(N)
    if N < 1:
        raise ValueError("plan_fill: N must be >= 1")
    lengths = [int(n) for n in lengths]
    if any(n < 1 for n in lengths):
        raise ValueError("plan_fill: every episode needs at least one transition")
    fill = [0] * N
    placed = []
    for i, n in enumerate(lengths):
        e = min(range(N), key=lambda k: (fill[k], k))
        placed.append((i, e, fill[e], n + 1))
        fill[e] += n + 1
    L = max(fill) if lengths else 0
    episode = np.full((N, L), PAD, np.int64)
    index = np.full((N, L), PAD, np.int64)
    for i, e, r0, rows in placed:
        episode[e, r0:r0 + rows] = i
        index[e, r0:r0 + rows] = np.arange(rows)
    return FillPlan(L, episode, index, N * L - sum(fill))


def planned_rows(plan, episodes, r0, r1, out=None):
    """Rows r0 .. r1 - 1 of a plan_fill layout as add() takes them, step-major: (frame uint8 [n, N, *slot_shape], action
    float32 [n, N, A], reward float32 [n, N], discount float32 [n, N], first uint8 [n, N]).  episodes[i] holds "frame"
    [len + 1, *slot_shape], "action" [len + 1, A], "reward" and "discount" [len + 1] or [len + 1, 1] of episode i.  A row
    with index 0 is the episode's reset row: first = 1, the other fields what the file holds there.  A pad row: first = 1,
    action 0, reward 0, discount 1, frame = the last frame written to its lane, zeros for a lane that received no episode.
    out: five arrays to write into (their first n rows), e.g. pinned staging."""
    N, L = plan.episode.shape
    r0, r1 = int(r0), int(r1)
    if not 0 <= r0 <= r1 <= L:
        raise ValueError(f"planned_rows: rows {r0} .. {r1} of a plan of {L}")
    n = r1 - r0
    if out is None:
        if not episodes:
            raise ValueError("planned_rows: no episode gives the shapes; pass out")
        slot, A = episodes[0]["frame"].shape[1:], episodes[0]["action"].shape[1]
        out = (np.empty((n, N) + tuple(slot), np.uint8), np.empty((n, N, A), np.float32), np.empty((n, N), np.float32),
               np.empty((n, N), np.float32), np.empty((n, N), np.uint8))
    frame, action, reward, discount, first = (a[:n] for a in out)
    for e in range(N):
        ep = plan.episode[e, r0:r1]
        r = 0
        while r < n:
            i = int(ep[r])
            stop = r + 1
            while stop < n and ep[stop] == i:
                stop += 1
            if i == PAD:
                used = int(np.count_nonzero(plan.episode[e] != PAD))
                frame[r:stop, e] = episodes[int(plan.episode[e, used - 1])]["frame"][-1] if used else 0
                action[r:stop, e] = 0
                reward[r:stop, e] = 0
                discount[r:stop, e] = 1
                first[r:stop, e] = 1
            else:
                # two episodes of one lane are never the same episode, so a run of equal entries is consecutive indices
                k0 = int(plan.index[e, r0 + r])
                src = episodes[i]
                frame[r:stop, e] = src["frame"][k0:k0 + stop - r]
                action[r:stop, e] = src["action"][k0:k0 + stop - r]
                reward[r:stop, e] = np.reshape(src["reward"], -1)[k0:k0 + stop - r]
                discount[r:stop, e] = np.reshape(src["discount"], -1)[k0:k0 + stop - r]
                first[r:stop, e] = plan.index[e, r0 + r:r0 + stop] == 0
            r = stop
    return frame, action, reward, discount, first
